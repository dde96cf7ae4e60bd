"""Per-point labels on the device against the twin of tests/assign_reference.py: labels, dist (as bytes), counts, offsets
and idx of every entry -- rh_assign_points, rh_assign_points_f32, rh_cloud_assign on a Float64 and on a Float32 cloud,
rh_cloud_assign_dev through rh_dev_* -- compared for equality, nothing left out, no tolerance.  The scene and what it is
known to contain: assign_reference.scene, tests/test_assign_host.py::test_the_scene_has_every_case (asserted again here)."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
import assign_reference as A
from test_assign_host import make_shape, params, the_scene

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 17]
S = the_scene()
XYZ, NRM, SHAPES, P = S["xyz"], S["nrm"], S["shapes"], S["p"]
XYZ32, NRM32 = XYZ.astype(np.float32), NRM.astype(np.float32)
_VALUES = {}


def values(f32):
    """the (D, T) matrices of the whole scene against the 13 shapes, computed once per element type"""
    if f32 not in _VALUES:
        _VALUES[f32] = A.compat_values(XYZ32, NRM32, SHAPES) if f32 else S["values"]
    return _VALUES[f32]


def rows_of(n):
    return np.arange(n) % len(XYZ)      # prefixes of the scene, cycled when longer


def twin(rows, shapes_idx, f32, use_normals=True, enabled=None):
    D, T = values(f32)
    sub = np.ix_(rows, shapes_idx)
    shapes = [SHAPES[j] for j in shapes_idx]
    return A.ref_assign(None, NRM if use_normals else None, shapes, P, enabled=enabled, values=(D[sub], T[sub]))


def same(got, ref, what):
    lab, dist, counts, off, idx = got
    assert np.array_equal(lab, ref["labels"]), what
    assert lab.dtype == np.int32 and counts.dtype == np.int64
    assert dist.tobytes() == ref["dist"].tobytes(), what
    assert np.array_equal(counts, ref["counts"]), what
    assert np.array_equal(off, ref["offsets"]), what
    assert np.array_equal(idx, ref["idx"]), what


ALL = dict(return_dist=True, return_counts=True, return_lists=True)


def dev_assign(pc, shapes, flags):
    """rh_cloud_assign_dev with every buffer made by rh_dev_alloc; one rh_cloud_sync, then the downloads"""
    lib, n, b = R.lib(), pc.size, len(shapes)
    arr = (L.Shape * max(1, b))(*shapes)
    sizes = {"shapes": C.sizeof(L.Shape) * max(1, b), "lab": 4 * n, "dist": 8 * n, "counts": 8 * (b + 1), "off": 8 * (b + 2), "idx": 8 * n}
    d = {}
    for k, sz in sizes.items():
        h = C.c_void_p()
        R._lib.check(lib.rh_dev_alloc(pc._h, sz, C.byref(h)))
        d[k] = h
    try:
        R._lib.check(lib.rh_dev_upload(pc._h, d["shapes"], C.cast(arr, C.c_void_p), sizes["shapes"]))
        R._lib.check(lib.rh_cloud_assign_dev(pc._h, d["shapes"], b, C.byref(P), flags, d["lab"], d["dist"], d["counts"], d["off"], d["idx"]))
        R._lib.check(lib.rh_cloud_sync(pc._h))
        out = (np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(b + 1, dtype=np.int64), np.zeros(b + 2, dtype=np.int64),
               np.zeros(n, dtype=np.int64))
        for a, k in zip(out, ("lab", "dist", "counts", "off", "idx")):
            R._lib.check(lib.rh_dev_download(pc._h, a.ctypes.data_as(C.c_void_p), d[k], a.nbytes))
        return out
    finally:
        for h in d.values():
            lib.rh_dev_free(pc._h, h)


def test_the_scene_is_what_the_checks_need():
    D, T = values(False)
    r = twin(rows_of(len(XYZ)), list(range(13)), False)
    c = A.claims(D, T, SHAPES, P)
    assert (c.sum(axis=1) >= 2).sum() > len(XYZ) // 2 and r["counts"][0] > 100
    Dm = np.where(c, D, np.inf)
    assert (((Dm == Dm.min(axis=1)[:, None]) & c).sum(axis=1) >= 2).sum() >= 100
    assert sorted(np.flatnonzero(r["counts"][1:] == 0).tolist()) == sorted(A.I_NOTHING + (A.I_SPHERE_DUP,))
    assert [s.kind for s in SHAPES] != sorted(s.kind for s in SHAPES)


@pytest.mark.parametrize("n", SIZES)
def test_every_entry_equals_the_twin(n):
    rows = rows_of(n)
    subs = [np.arange(1, n + 1, dtype=np.int64)]
    clouds = {False: R.RANSACCloud(XYZ[rows], NRM[rows], subs), True: R.RANSACCloud(XYZ32[rows], NRM32[rows], subs, force_eltype=np.float32)}
    third = np.arange(0, n, 3)                           # the points rh_invalidate switches off for the last leg
    enabled = np.ones(n, dtype=bool)
    enabled[third] = False
    for bsel in ([], [0], list(range(13))):
        shapes = [SHAPES[j] for j in bsel]
        for use_n in (True, False):
            tag = (n, len(bsel), use_n)
            ref64, ref32 = twin(rows, bsel, False, use_n), twin(rows, bsel, True, use_n)
            same(R.assign_points(XYZ[rows], NRM[rows], shapes, P, use_normals=use_n, **ALL), ref64, ("raw64",) + tag)
            same(R.assign_points(XYZ32[rows], NRM32[rows], shapes, P, use_normals=use_n, **ALL), ref32, ("raw32",) + tag)
            if not use_n:                                # no normals at all: the same as normals switched off
                same(R.assign_points(XYZ[rows], None, shapes, P, **ALL), ref64, ("raw64 nrm=None",) + tag)
            flags = 0 if use_n else L.ASSIGN_NO_NORMALS
            for f32, ref in ((False, ref64), (True, ref32)):
                same(R.assign_cloud(clouds[f32], shapes, P, use_normals=use_n, **ALL), ref, ("cloud", f32) + tag)
                same(dev_assign(clouds[f32], shapes, flags), ref, ("dev", f32) + tag)
    # labels alone (no counts, no lists: the label kernel on its own), counts without lists
    ref = twin(rows, list(range(13)), False)
    assert np.array_equal(R.assign_cloud(clouds[False], SHAPES, P), ref["labels"])
    lab, counts = R.assign_points(XYZ[rows], NRM[rows], SHAPES, P, return_counts=True)
    assert np.array_equal(lab, ref["labels"]) and np.array_equal(counts, ref["counts"])
    # ENABLED_ONLY after rh_invalidate of a known third; without the flag the bits do not matter
    for f32 in (False, True):
        pc = clouds[f32]
        R.invalidate_indexes(pc, third + 1)
        before = pc.enabled_chunks().copy()
        for bsel in ([], [0], list(range(13))):
            shapes = [SHAPES[j] for j in bsel]
            same(R.assign_cloud(pc, shapes, P, enabled_only=True, **ALL), twin(rows, bsel, f32, True, enabled), ("enabled", f32, n, len(bsel)))
            same(dev_assign(pc, shapes, L.ASSIGN_ENABLED_ONLY | L.ASSIGN_NO_NORMALS), twin(rows, bsel, f32, False, enabled),
                 ("enabled dev", f32, n, len(bsel)))
            same(R.assign_cloud(pc, shapes, P, **ALL), twin(rows, bsel, f32), ("not enabled_only", f32, n, len(bsel)))
        assert np.array_equal(pc.enabled_chunks(), before)


def test_1024_shapes():
    """the largest key count: LDS rows and the count matrix hold b + 1 = 1025 columns"""
    n, b = 4097, 1024
    rows = rows_of(n)
    rng = np.random.default_rng(5)
    bsel = np.concatenate([rng.permutation(13), rng.integers(0, 13, size=b - 13)]).tolist()
    shapes = [SHAPES[j] for j in bsel]
    ref = twin(rows, bsel, False)
    assert (ref["counts"][1:] > 0).sum() == 9 and ref["labels"].max() <= 13   # the first copy of a shape wins its ties
    same(R.assign_points(XYZ[rows], NRM[rows], shapes, P, **ALL), ref, "raw64 b=1024")
    pc = R.RANSACCloud(XYZ32[rows], NRM32[rows], [np.arange(1, n + 1, dtype=np.int64)], force_eltype=np.float32)
    same(R.assign_cloud(pc, shapes, P, **ALL), twin(rows, bsel, True), "cloud32 b=1024")
    # the last key of the range: 1023 copies of a shape that claims nothing, then the true sphere
    bsel2 = [A.I_NOTHING[0]] * 1023 + [A.I_SPHERE]
    ref2 = twin(rows, bsel2, False)
    assert ref2["counts"][1024] > 0 and ref2["counts"][1:1024].sum() == 0
    same(R.assign_points(XYZ[rows], NRM[rows], [SHAPES[j] for j in bsel2], P, **ALL), ref2, "raw64 b=1024, last key")
    lab = np.zeros(n, dtype=np.int32)
    rc = R.lib().rh_cloud_assign(pc._h, (L.Shape * 1025)(), 1025, C.byref(P), 0, lab.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None)
    assert rc == L.RH_E_INVALID


def test_consistent_with_refit_and_extents():
    """on a Float64 cloud with every point enabled: a shape's label set lies inside its rh_refit set, the union of the
    refit sets is the labelled points, and the lists feed rh_shape_extents as they are"""
    n = len(XYZ)
    pc = R.RANSACCloud(XYZ, NRM, synth.make_subsets(n, 2, seed=1))
    lab, counts, off, idx = R.assign_cloud(pc, SHAPES, P, return_counts=True, return_lists=True)
    lists = R.lists_from_assignment(off, idx)
    union = np.zeros(n, dtype=bool)
    for j, s in enumerate(SHAPES):
        mine = np.flatnonzero(lab == j + 1) + 1
        assert np.array_equal(lists[j + 1], mine)
        ref = R.refit(s, pc, P).inpoints
        assert np.isin(mine, ref).all(), j
        union[ref - 1] = True
    assert np.array_equal(union, lab > 0)
    ok = [j for j in range(13) if j != A.I_NOTHING[2]]          # (the zero-axis cone is invalid input to rh_shape_extents)
    ext = R.shape_extents(pc, [(SHAPES[j], lists[j + 1]) for j in ok])
    assert [e.n for e in ext] == [int(counts[j + 1]) for j in ok]


def test_same_bits_twice_and_a_point_alone():
    n = 4097
    rows = rows_of(n)
    a = R.assign_points(XYZ[rows], NRM[rows], SHAPES, P, **ALL)
    b = R.assign_points(XYZ[rows], NRM[rows], SHAPES, P, **ALL)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for i in (0, 63, 64, 1000, 4096):
        lab, dist = R.assign_points(XYZ[rows[i:i + 1]], NRM[rows[i:i + 1]], SHAPES, P, return_dist=True)
        assert lab[0] == a[0][i] and dist.tobytes() == a[1][i:i + 1].tobytes()


def test_nan_point_and_fitted_shapes():
    """a non-finite point claims nothing (raw entry: a cloud is not built over such points); the wrappers take
    FittedShapes and ExtractedShapes as well as C records"""
    rows = rows_of(65)
    xyz = XYZ[rows].copy()
    xyz[3] = [np.nan, 1.0, 2.0]
    xyz[64] = [np.inf, 0.0, 0.0]
    ref = A.ref_assign(xyz, NRM[rows], SHAPES, P)
    assert ref["labels"][3] == 0 and ref["labels"][64] == 0
    same(R.assign_points(xyz, NRM[rows], SHAPES, P, **ALL), ref, "nan")
    refn = A.ref_assign(xyz, None, SHAPES, P)
    same(R.assign_points(xyz, NRM[rows], SHAPES, P, use_normals=False, **ALL), refn, "nan, no normals")
    fs = [R.shape_from_c(SHAPES[A.I_SPHERE]), R.ExtractedShape(R.shape_from_c(SHAPES[A.I_PLANE]), np.zeros(0, dtype=np.int64))]
    got = R.assign_points(XYZ[rows], NRM[rows], fs, P)
    assert np.array_equal(got, twin(rows, [A.I_SPHERE, A.I_PLANE], False)["labels"])
