"""Per-point labels (rh_assign_points, rh_cloud_assign, include/ransac_hip.h) without a device: the numpy twin of
tests/assign_reference.py against hand-made cases with known answers and against the oracle's own refit, the facts the
GPU tests rely on about their scene, and the ABI -- symbols, version, every RH_E_INVALID case (all of them are decided
before the first device call), the Python wrappers' argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc
import assign_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_shape(kind, outwards, v):
    s = L.Shape()
    s.kind, s.outwards = kind, int(bool(outwards))
    for i, x in enumerate(v):
        s.v[i] = float(x)
    R.lib().rh_shape_finalize(C.byref(s))
    return s


def params(eps=0.1, alpha=0.35):
    p = L.Params()
    R.lib().rh_default_params(C.byref(p))
    for k in range(4):
        p.eps[k], p.alpha[k] = eps, alpha
    R.lib().rh_params_finalize(C.byref(p))
    return p


_SCENE = {}


def the_scene():
    if not _SCENE:
        xyz, nrm, shapes = A.scene(make_shape)
        p = A.scene_params(params())
        _SCENE.update(xyz=xyz, nrm=nrm, shapes=shapes, p=p, values=A.compat_values(xyz, nrm, shapes))
    return _SCENE


# ------------------------------------------------------------------------------------- the twin ----
def test_midway_between_two_parallel_planes_goes_to_the_lower_index():
    up = [0.0, 0.0, 1.0]
    lo, hi = make_shape(L.PLANE, True, [0.0, 0.0, 0.0] + up), make_shape(L.PLANE, True, [0.0, 0.0, 0.125] + up)
    xyz = np.array([[1.0, 2.0, 0.0625], [3.0, -1.0, 0.0], [0.5, 0.5, 0.125], [0.0, 0.0, 9.0]])
    nrm = np.tile(up, (4, 1))
    r = A.ref_assign(xyz, nrm, [lo, hi], params())
    assert r["labels"].tolist() == [1, 1, 2, 0] and r["dist"].tolist() == [0.0625, 0.0, 0.0, -1.0]
    r = A.ref_assign(xyz, nrm, [hi, lo], params())
    assert r["labels"].tolist() == [1, 2, 1, 0] and r["dist"].tolist() == [0.0625, 0.0, 0.0, -1.0]
    assert r["counts"].tolist() == [1, 2, 1] and r["offsets"].tolist() == [0, 1, 3, 4] and r["idx"].tolist() == [4, 1, 3, 2]


def test_identical_shapes_all_points_go_to_the_first():
    s = [make_shape(L.SPHERE, True, [1.0, 2.0, 3.0, 2.0]) for _ in range(2)]
    rng = np.random.default_rng(3)
    d = rng.normal(size=(50, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = np.array([1.0, 2.0, 3.0]) + 2.0 * d + rng.normal(0, 0.01, size=d.shape)
    r = A.ref_assign(xyz, d, s, params())
    assert (r["labels"] == 1).all() and r["counts"].tolist() == [0, 50, 0]


def test_wrong_normal_is_unlabelled_until_normals_are_off_and_nan_is_never_labelled():
    pl = make_shape(L.PLANE, True, [0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    xyz = np.array([[1.0, 1.0, 0.01], [2.0, 2.0, 0.02], [np.nan, 0.0, 0.0]])
    nrm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    r = A.ref_assign(xyz, nrm, [pl], params())
    assert r["labels"].tolist() == [1, 0, 0] and r["dist"].tolist() == [0.01, -1.0, -1.0]
    r = A.ref_assign(xyz, None, [pl], params())
    assert r["labels"].tolist() == [1, 1, 0] and r["dist"].tolist() == [0.01, 0.02, -1.0]
    r = A.ref_assign(xyz, None, [pl], params(), enabled=[False, True, True])
    assert r["labels"].tolist() == [0, 1, 0]
    r = A.ref_assign(xyz, nrm, [], params())
    assert r["labels"].tolist() == [0, 0, 0] and r["counts"].tolist() == [3] and r["offsets"].tolist() == [0, 3]


def test_claim_sets_equal_the_oracles_refit():
    """the twin's predicate is the reference's compatibles*: per shape, its claim set is what orc_refit returns"""
    S = the_scene()
    D, T = S["values"]
    c = A.claims(D, T, S["shapes"], S["p"])
    oc = orc.Cloud(S["xyz"], S["nrm"], np.arange(1, 11, dtype=np.int64))
    op = orc.Params.from_buffer_copy(bytes(S["p"]))
    sizes = []
    for j, s in enumerate(S["shapes"]):
        got = oc.refit(orc.Shape.from_buffer_copy(bytes(s)), op)
        assert np.array_equal(got, np.flatnonzero(c[:, j]) + 1), j
        sizes.append(len(got))
    assert sum(1 for x in sizes if x > 0) == 10


def test_the_scene_has_every_case():
    """what the GPU tests take for granted: doubly claimed points, unclaimed points, exact ties, and every label in use but
    those of the three shapes that claim nothing and of the exact duplicate, which comes later than its twin and so loses
    every tie (rule 3)"""
    S = the_scene()
    D, T = S["values"]
    n = len(S["xyz"])
    for nrm in (S["nrm"], None):
        c = A.claims(D, T, S["shapes"], S["p"], nrm is not None)
        r = A.ref_assign(S["xyz"], nrm, S["shapes"], S["p"], values=S["values"])
        assert (c.sum(axis=1) >= 2).sum() > n // 2
        Dm = np.where(c, D, np.inf)
        best = Dm.min(axis=1)
        ties = ((Dm == best[:, None]) & c).sum(axis=1) >= 2
        assert ties.sum() >= 100
        empty = sorted(np.flatnonzero(r["counts"][1:] == 0).tolist())
        assert empty == sorted(A.I_NOTHING + (A.I_SPHERE_DUP,)), empty
        if nrm is not None:
            assert r["counts"][0] > 100
        assert not c[:, list(A.I_NOTHING)].any()
        assert np.array_equal(c[:, A.I_SPHERE], c[:, A.I_SPHERE_DUP])
    kinds = [s.kind for s in S["shapes"]]
    assert kinds != sorted(kinds)


def test_lists_are_the_stable_partition():
    S = the_scene()
    r = A.ref_assign(S["xyz"], S["nrm"], S["shapes"], S["p"], values=S["values"])
    lists = R.lists_from_assignment(r["offsets"], r["idx"])
    assert len(lists) == 14 and sum(len(x) for x in lists) == len(S["xyz"])
    for k, l in enumerate(lists):
        assert np.array_equal(l, np.flatnonzero(r["labels"] == k) + 1)
    with pytest.raises(ValueError):
        R.lists_from_assignment(r["offsets"][:-1], r["idx"])


# ------------------------------------------------------------------------------------- the ABI ----
def test_symbols_and_version():
    lib = R.lib()
    for name in ("rh_assign_points", "rh_assign_points_f32", "rh_cloud_assign", "rh_cloud_assign_dev"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", hdr).group(1)) >= 114
    assert lib.rh_version() >= 114
    assert int(re.search(r"#define\s+RH_ASSIGN_MAX_SHAPES\s+(\d+)", hdr).group(1)) == L.ASSIGN_MAX_SHAPES == 1024
    assert re.search(r"RH_ASSIGN_NO_NORMALS\s*=\s*1\s*,\s*RH_ASSIGN_ENABLED_ONLY\s*=\s*2", hdr)
    assert (L.ASSIGN_NO_NORMALS, L.ASSIGN_ENABLED_ONLY) == (1, 2)


def _raw_call(fn=None, xyz=True, nrm=True, n=4, shapes=True, b=2, p=True, flags=0, labels=True, dist=False, counts=False,
              offsets=False, idx=False, kind=None, ct=C.c_double, t=np.float64):
    lib = R.lib()
    fn = fn or lib.rh_assign_points
    m = max(1, min(n, 16))
    a = np.zeros((m, 3), dtype=t)
    arr = (L.Shape * max(1, min(max(b, 1), 1025)))()
    for s in arr:
        s.kind = L.SPHERE
        s.v[3] = 1.0
    if kind is not None:
        arr[min(b, len(arr)) - 1].kind = kind
    lab, di = np.zeros(m, dtype=np.int32), np.zeros(m)
    cn, of, ix = np.zeros(1030, dtype=np.int64), np.zeros(1030, dtype=np.int64), np.zeros(m, dtype=np.int64)
    pp = params()
    return fn(a.ctypes.data_as(C.POINTER(ct)) if xyz else None, a.ctypes.data_as(C.POINTER(ct)) if nrm else None, n,
              arr if shapes else None, b, C.byref(pp) if p else None, flags, 0,
              lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None, di.ctypes.data_as(C.POINTER(C.c_double)) if dist else None,
              cn.ctypes.data_as(C.POINTER(C.c_int64)) if counts else None, of.ctypes.data_as(C.POINTER(C.c_int64)) if offsets else None,
              ix.ctypes.data_as(C.POINTER(C.c_int64)) if idx else None)


INVALID = [dict(b=-1), dict(b=1025), dict(kind=4), dict(kind=-1), dict(n=-1), dict(n=1 << 31), dict(xyz=False), dict(labels=False),
           dict(p=False), dict(shapes=False), dict(offsets=True), dict(idx=True), dict(flags=4), dict(flags=8 | 1),
           dict(flags=L.ASSIGN_ENABLED_ONLY)]


@pytest.mark.parametrize("case", INVALID, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_raw_entries_reject_bad_arguments_without_a_device(case):
    lib = R.lib()
    assert _raw_call(**case) == L.RH_E_INVALID
    assert lib.rh_last_error()
    assert _raw_call(fn=lib.rh_assign_points_f32, ct=C.c_float, t=np.float32, **case) == L.RH_E_INVALID


def test_cloud_entries_reject_a_null_cloud():
    lib = R.lib()
    arr, p, lab = (L.Shape * 1)(), params(), np.zeros(4, dtype=np.int32)
    assert lib.rh_cloud_assign(None, arr, 1, C.byref(p), 0, lab.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None) == L.RH_E_INVALID
    assert lib.rh_cloud_assign_dev(None, None, 1, C.byref(p), 0, None, None, None, None, None) == L.RH_E_INVALID


def test_no_shapes_and_no_points_need_no_device():
    xyz = np.arange(15, dtype=np.float64).reshape(5, 3)
    lab, dist, counts, off, idx = R.assign_points(xyz, None, [], params(), return_dist=True, return_counts=True, return_lists=True)
    assert lab.tolist() == [0] * 5 and dist.tolist() == [-1.0] * 5 and counts.tolist() == [5]
    assert off.tolist() == [0, 5] and idx.tolist() == [1, 2, 3, 4, 5]
    s = make_shape(L.SPHERE, True, [0.0, 0.0, 0.0, 1.0])
    lab, counts, off, idx = R.assign_points(np.zeros((0, 3)), None, [s, s], params(), return_counts=True, return_lists=True)
    assert lab.size == 0 and counts.tolist() == [0, 0, 0] and off.tolist() == [0, 0, 0, 0] and idx.size == 0


def test_python_wrappers_check_their_arguments():
    s = make_shape(L.SPHERE, True, [0.0, 0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        R.assign_points(np.zeros((5, 3)), np.zeros((4, 3)), [s], params())
    with pytest.raises(ValueError):
        R.assign_points(np.zeros((5, 3)), None, [s] * 1025, params())
    with pytest.raises(R.RansacHipError) as e:
        bad = L.Shape.from_buffer_copy(bytes(s))
        bad.kind = 9
        R.assign_points(np.zeros((5, 3)), None, [bad], params())
    assert e.value.code == L.RH_E_INVALID
    assert R.assign_cloud and R.lists_from_assignment
