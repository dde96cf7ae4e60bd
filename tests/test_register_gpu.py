"""Rigid registration (rh_register) on the GPU, held to the numpy twin of tests/register_reference.py for EQUALITY: the bytes
of the transform, the iterations, the status and the histories n_valid_it and rms_it.  The definition fixes every
operation and its order, so nothing here has a tolerance.

The number of queries m spans the cuts of the reduction tree -- a lane's four, a wave, a block of L.OUT_BLOCK_POINTS, the
level-2 fold over the block partials and a ragged last block.  A level-3 tree (m > 1024^2) is beyond what a brute-force
twin can check in seconds; the fold kernel is the same code at every level."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
import register_reference as RR
from register_reference import ref_register

pytestmark = pytest.mark.gpu

B = L.OUT_BLOCK_POINTS
MS = [1, 5, 6, 63, 64, 65, B - 1, B, B + 1, 2 * B + 300]
PRIMS = ["plane", "plane", "plane", "sphere", "cylinder"]
REF, NRM, _ = synth.make_cloud(3000, PRIMS, seed=0)
SPACING = synth.median_nn_distance(REF)
MOTION = RR.rigid(2.0, 0.5, 0, REF.mean(axis=0))
HIST = ("n_valid", "rms")


def _queries(m, seed=0, noise=0.02, motion=MOTION):
    """m points of the reference, displaced a little and moved"""
    rng = np.random.default_rng(300 + seed)
    pick = rng.choice(len(REF), m, replace=False)
    return np.ascontiguousarray(RR.apply(motion, REF[pick] + rng.normal(0.0, noise, size=(m, 3))))


def _check(ref, qry, nrm, metric, **kw):
    kw.setdefault("max_iter", 30)
    exp = ref_register(ref, qry, normals=nrm if metric == "plane" else None, metric=metric, **kw)
    T, info = R.register(ref, qry, normals=nrm if metric == "plane" else None, metric=metric, return_info=True, **kw)
    it = exp["iterations"]
    print("m=%d %s %r: %s after %d, n_valid %s, rms %s (twin: %s after %d)" % (
        len(qry), metric, {k: v for k, v in kw.items() if k != "init"}, info["status"], info["iterations"],
        info["history"]["n_valid"].tolist()[:3], info["history"]["rms"].tolist()[:3], RR.STATUS[exp["status"]], it))
    assert T.dtype == np.float64 and T.shape == (4, 4) and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert info["status"] == RR.STATUS[exp["status"]] and info["iterations"] == it
    assert np.array_equal(info["history"]["n_valid"], exp["n_valid_it"][:it])
    assert info["history"]["rms"].tobytes() == exp["rms_it"][:it].tobytes()
    assert T[:3].tobytes() == exp["transform"].tobytes(), np.abs(T[:3] - exp["transform"]).max()
    assert info["n_valid"] == exp["n_valid"] and np.float64(info["rms"]).tobytes() == np.float64(exp["rms"]).tobytes()
    return exp


# ------------------------------------------------------------------------ 1. the tree's cuts ----
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_register_equals_the_twin(m, metric):
    exp = _check(REF, _queries(m), NRM, metric)
    if m < 6:
        assert exp["status"] == RR.TOO_FEW
    if m >= 63:
        assert exp["status"] == RR.CONVERGED and exp["iterations"] > 2


# ------------------------------------------------------------------------------- 2. radius ----
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_a_radius_leaves_some_queries_out_at_first(metric):
    qry = np.concatenate([_queries(B + 200), RR.apply(MOTION, REF[:40] + 25.0 * SPACING)])    # 40 that never find a partner
    exp = _check(REF, np.ascontiguousarray(qry), NRM, metric, radius=1.5 * SPACING)
    nv, it = exp["n_valid_it"], exp["iterations"]
    assert 6 <= nv[0] < nv[it - 1] < len(qry)                              # fewer are left out in the last iteration


# --------------------------------------------------------------------------------- 3. init ----
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_an_init_starts_the_iteration_where_it_says(metric):
    big = RR.rigid(25.0, 8.0, 3, REF.mean(axis=0))
    qry = _queries(700, seed=1, motion=big)
    inv = np.hstack([big[:, :3].T, -(big[:, :3].T @ big[:, 3])[:, None]])
    near = RR.rigid(1.0, 0.3, 4, REF.mean(axis=0))                         # the start: the inverse, a degree and 0.3 off
    init = np.hstack([near[:, :3] @ inv[:, :3], (near[:, :3] @ inv[:, 3] + near[:, 3])[:, None]])
    exp = _check(REF, qry, NRM, metric, init=init)
    assert exp["status"] == RR.CONVERGED
    back = RR.apply(exp["transform"], qry)
    assert np.abs(RR.apply(inv, qry) - back).max() < 0.1                   # (it ends at the inverse, up to the noise)
    T4 = R.register(REF, qry, normals=NRM if metric == "plane" else None, metric=metric, max_iter=30,
                    init=np.vstack([init, [0.0, 0.0, 0.0, 1.0]]))
    assert T4[:3].tobytes() == exp["transform"].tobytes()                  # a 4x4 init is its first three rows


# ------------------------------------------------------------------------------ 4. float32 ----
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_float32_is_the_widened_double_call(metric):
    r32, n32, q32 = REF.astype(np.float32), NRM.astype(np.float32), _queries(B + 7, seed=2).astype(np.float32)
    exp = ref_register(r32.astype(np.float64), q32.astype(np.float64), normals=n32.astype(np.float64) if metric == "plane" else None,
                       metric=metric, max_iter=30)
    T, info = R.register(r32, q32, normals=n32 if metric == "plane" else None, metric=metric, max_iter=30, return_info=True)
    it = exp["iterations"]
    assert T.dtype == np.float64 and T[:3].tobytes() == exp["transform"].tobytes()
    assert (info["status"], info["iterations"]) == (RR.STATUS[exp["status"]], it)
    assert np.array_equal(info["history"]["n_valid"], exp["n_valid_it"][:it])
    assert info["history"]["rms"].tobytes() == exp["rms_it"][:it].tobytes()
    mixed = R.register(r32, q32.astype(np.float64), normals=n32 if metric == "plane" else None, metric=metric, max_iter=30)
    assert mixed.tobytes() == T.tobytes()                                  # a mixed pair is widened in Python


# -------------------------------------------------------------------- 5. far from the origin ----
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_both_clouds_a_million_away(metric):
    """The centring keeps the normal equations at the clouds' own scale, and the search margin covers the magnitude."""
    far = np.array([1e6, 1e6, 1e6])
    exp = _check(np.ascontiguousarray(REF + far), np.ascontiguousarray(_queries(B + 50, seed=3) + far), NRM, metric)
    assert exp["status"] == RR.CONVERGED


# ------------------------------------------------------------------------------- 6. status ----
def test_the_three_other_ways_to_end():
    rng = np.random.default_rng(1)
    flat = np.zeros((400, 3))
    flat[:, :2] = rng.uniform(0.0, 20.0, size=(400, 2))
    up = np.tile([0.0, 0.0, 1.0], (400, 1))
    exp = _check(flat, np.ascontiguousarray(flat[:150] + np.array([0.01, -0.02, 0.3])), up, "plane")
    assert (exp["status"], exp["iterations"]) == (RR.DEGENERATE, 1)
    qry = _queries(200, seed=4)
    exp = _check(REF, np.ascontiguousarray(np.concatenate([qry[:5], qry[5:] + 40.0 * SPACING])), NRM, "plane", radius=3.0 * SPACING)
    assert (exp["status"], exp["n_valid"]) == (RR.TOO_FEW, 5)
    exp = _check(REF, np.ascontiguousarray(qry + 1e4), NRM, "point", radius=SPACING)
    assert (exp["status"], exp["n_valid"], exp["rms"]) == (RR.TOO_FEW, 0, 0.0)
    for metric in ("plane", "point"):
        exp = _check(REF, qry, NRM, metric, max_iter=2)
        assert (exp["status"], exp["iterations"]) == (RR.MAX_ITER, 2)
        exp = _check(REF, qry, NRM, metric, max_iter=1)
        assert (exp["status"], exp["iterations"]) == (RR.MAX_ITER, 1)


# -------------------------------------------------------------------------- 7. permutation ----
def test_a_permutation_of_the_queries_changes_the_last_bits_at_most():
    """The trees run over the query index order: another order rounds the sums differently, and nothing else.  Both runs
    stop at steps below 1e-9 of an iteration that converges quadratically here (plane metric, rms of the steps 1e-2,
    1e-4, 1e-8, ..), so their transforms agree far within 1e-9 * the coordinates' 100."""
    qry = _queries(B + 333, seed=5)
    perm = np.random.default_rng(7).permutation(len(qry))
    a = _check(REF, qry, NRM, "plane")
    b = _check(REF, np.ascontiguousarray(qry[perm]), NRM, "plane")         # the twin on the permuted input, to the byte
    assert a["iterations"] == b["iterations"] and np.abs(a["transform"] - b["transform"]).max() <= 1e-7


# -------------------------------------------------------------- 8. device pointers, two runs ----
def _dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_device_pointers_and_two_runs_give_the_same_bytes(metric):
    qry = _queries(B + 100, seed=6)
    kw = dict(normals=NRM if metric == "plane" else None, metric=metric, max_iter=20, return_info=True)
    T, info = R.register(REF, qry, **kw)
    T2, info2 = R.register(REF, qry, **kw)
    assert T.tobytes() == T2.tobytes() and info["iterations"] == info2["iterations"]
    assert info["history"]["rms"].tobytes() == info2["history"]["rms"].tobytes()
    d_ref, d_nrm, d_qry = (torch.from_numpy(np.array(x)).cuda() for x in (REF, NRM, qry))
    prm = L.RegisterParams(radius=0.0, rot_tol=1e-9, trans_tol=1e-9, metric=L.DIST_PLANE if metric == "plane" else L.DIST_POINT,
                           max_iter=20)
    out, res = np.zeros((3, 4)), L.RegisterResult()
    nv, rms = np.full(20, -1, dtype=np.int32), np.full(20, -1.0)
    dp = C.POINTER(C.c_double)
    L.check(R.lib().rh_register(_dptr(d_ref, C.c_double), _dptr(d_nrm, C.c_double) if metric == "plane" else None, len(REF),
                                _dptr(d_qry, C.c_double), len(qry), C.byref(prm), None, 0, out.ctypes.data_as(dp), C.byref(res),
                                nv.ctypes.data_as(C.POINTER(C.c_int32)), rms.ctypes.data_as(dp)))
    torch.cuda.synchronize()
    it = info["iterations"]
    assert out.tobytes() == T[:3].tobytes() and (res.iterations, res.n_valid) == (it, info["n_valid"])
    assert L.REG_STATUS_NAMES[res.status] == info["status"]
    assert np.array_equal(nv[:it], info["history"]["n_valid"]) and not nv[it:].any()       # 0 behind `iterations`
    assert rms[:it].tobytes() == info["history"]["rms"].tobytes() and not rms[it:].any()
    # every output but the transform is optional
    out2 = np.zeros((3, 4))
    L.check(R.lib().rh_register(_dptr(d_ref, C.c_double), _dptr(d_nrm, C.c_double) if metric == "plane" else None, len(REF),
                                _dptr(d_qry, C.c_double), len(qry), C.byref(prm), None, 0, out2.ctypes.data_as(dp), None, None, None))
    assert out2.tobytes() == out.tobytes()


def test_a_coordinate_that_is_not_finite():
    ref, qry = REF[:300].copy(), _queries(257, seed=8)
    bad_ref, bad_qry = ref.copy(), qry.copy()
    bad_ref[37, 1] = np.nan
    bad_qry[256, 2] = np.inf
    for r, q in ((bad_ref, qry), (ref, bad_qry)):
        with pytest.raises(R.RansacHipError) as e:
            R.register(r, q)
        assert e.value.code == L.RH_E_INVALID


# ------------------------------------------------------------------- 9. what it is there for ----
def test_cloud_distance_after_registration_measures_the_deviation():
    qry = _queries(1500, seed=9, noise=0.0)
    before = R.cloud_distance(REF, qry, return_stats=True)[1]
    T = R.register(REF, qry, normals=NRM)
    after = R.cloud_distance(REF, R.transform_points(T, qry), return_stats=True)[1]
    assert before["rms"] > 0.3 * SPACING and after["max"] < 1e-9           # the queries are reference points, moved
