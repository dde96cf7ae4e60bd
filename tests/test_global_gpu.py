"""Global registration (rh_describe, rh_match_features, rh_register_global) on the GPU, held to the numpy twins of
tests/global_reference.py for EQUALITY of bytes: descriptors, neighbour counts, match indices and distances, the counts
of every trial, the transform and the result.  The definitions fix every operation and its order, and everything summed
is an integer, so nothing here has a tolerance but the last test's, which is the clouds' own noise."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
import global_reference as G
import global_scene as GS
from test_normals_host import ref_neighbours

pytestmark = pytest.mark.gpu

SCENE = GS.make()
NB = {}


def _cloud(n, far=0.0):
    """the first n points of the scene's reference sample (a mix of the four surfaces), with their normals"""
    return np.ascontiguousarray(SCENE["ref"][:n] + far), np.ascontiguousarray(SCENE["ref_nrm"][:n])


def _nb(n):
    if n not in NB:
        NB[n] = ref_neighbours(_cloud(n)[0], 64)
    return NB[n]


def _dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


# ------------------------------------------------------------------------------ 1. describe ----
@pytest.mark.parametrize("n", [1, 2, 17, 64, 65, 1025, 2048])
def test_describe_equals_the_twin(n):
    xyz, nrm = _cloud(n)
    for k in (1, 16, 63):
        exp, ecount, _ = G.ref_describe(xyz, nrm, k, nb=_nb(n))
        got, count = R.describe(xyz, nrm, k=k, return_count=True)
        assert got.dtype == np.uint16 and got.shape == (n, 33)
        assert np.array_equal(count, ecount) and got.tobytes() == exp.tobytes(), (n, k, int((got != exp).sum()))
    assert n == 1 or got.any()


def test_a_radius_empties_some_lists():
    xyz, nrm = _cloud(1025)
    radius = 0.6 * synth.median_nn_distance(xyz)
    exp, ecount, _ = G.ref_describe(xyz, nrm, 16, radius, nb=_nb(1025))
    got, count = R.describe(xyz, nrm, k=16, radius=radius, return_count=True)
    assert (ecount == 0).sum() > 50 and (ecount > 0).sum() > 50
    assert np.array_equal(count, ecount) and got.tobytes() == exp.tobytes()
    assert not got[ecount == 0].any()


def test_duplicates_and_a_zero_normal_are_degenerate_pairs():
    xyz, nrm = _cloud(300)
    xyz[100:120] = xyz[50:70]                                       # d2 == 0 between the copies
    nrm[7] = 0.0                                                    # v2 == 0 for its own pairs, g == 0 as a neighbour
    nrm[8] *= 2.0                                                   # features beyond [-1, 1]: clamped
    exp, ecount, S = G.ref_describe(xyz, nrm, 16)
    got, count = R.describe(xyz, nrm, k=16, return_count=True)
    assert not S[7].any() and S[50, :11].sum() < 16
    assert np.array_equal(count, ecount) and got.tobytes() == exp.tobytes()


def test_describe_float32_is_the_widened_double_call():
    xyz, nrm = _cloud(1025)
    x32, n32 = xyz.astype(np.float32), nrm.astype(np.float32)
    exp, ecount, _ = G.ref_describe(x32.astype(np.float64), n32.astype(np.float64), 16)
    got, count = R.describe(x32, n32, k=16, return_count=True)
    assert np.array_equal(count, ecount) and got.tobytes() == exp.tobytes()
    assert R.describe(x32.astype(np.float64), n32, k=16).tobytes() == got.tobytes()     # a mixed pair is widened in Python


def test_describe_a_million_from_the_origin():
    xyz, nrm = _cloud(1025, far=float(2 ** 20))
    exp, ecount, _ = G.ref_describe(xyz, nrm, 16)
    got, count = R.describe(xyz, nrm, k=16, return_count=True)
    assert np.array_equal(count, ecount) and got.tobytes() == exp.tobytes()


def test_describe_device_pointers_and_two_runs():
    xyz, nrm = _cloud(2048)
    a, ca = R.describe(xyz, nrm, k=32, return_count=True)
    b = R.describe(xyz, nrm, k=32)
    assert a.tobytes() == b.tobytes()
    d_xyz, d_nrm = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    d_desc = torch.zeros((2048, 33), dtype=torch.int16, device="cuda")
    d_cnt = torch.zeros(2048, dtype=torch.int32, device="cuda")
    L.check(R.lib().rh_describe(_dptr(d_xyz, C.c_double), _dptr(d_nrm, C.c_double), 2048, 32, 0.0, 0, _dptr(d_desc, C.c_uint16),
                                _dptr(d_cnt, C.c_int32)))
    torch.cuda.synchronize()
    assert d_desc.cpu().numpy().view(np.uint16).tobytes() == a.tobytes() and np.array_equal(d_cnt.cpu().numpy(), ca)


def test_a_normal_or_coordinate_that_is_not_finite_writes_nothing():
    xyz, nrm = _cloud(300)
    dp = C.POINTER(C.c_double)
    for which, val in (("nrm", np.nan), ("nrm", np.inf), ("xyz", np.nan)):
        x, nr = xyz.copy(), nrm.copy()
        (nr if which == "nrm" else x)[211, 1] = val
        desc = np.full((300, 33), 9999, dtype=np.uint16)
        cnt = np.full(300, -7, dtype=np.int32)
        rc = R.lib().rh_describe(x.ctypes.data_as(dp), nr.ctypes.data_as(dp), 300, 16, 0.0, 0, desc.ctypes.data_as(C.POINTER(C.c_uint16)),
                                 cnt.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == L.RH_E_INVALID and (desc == 9999).all() and (cnt == -7).all()


# ------------------------------------------------------------------------------ 2. matching ----
def _descs(rows, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, G.DESC_MAX + 1, size=(rows, 33)).astype(np.uint16)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 65), (63, 64), (1025, 2348), (4096, 4096)])
def test_match_equals_the_twin(n, m):
    ref, qry = _descs(n, 10 + n), _descs(m, 20 + m)
    ref[0], qry[0] = 0, G.DESC_MAX                                   # rows at both extremes: 33 * 7938^2 is reached when n = 1
    if n > 1:
        ref[n - 1] = G.DESC_MAX
        qry[m - 1] = 0
    if n >= 63 and m >= 64:                                          # planted exact ties: equal rows far apart in the reference
        ref[n - 2], ref[3] = ref[1], ref[1]
        qry[5], qry[6] = ref[1], ref[1]
    for mutual in (False, True):
        eidx, edist = G.ref_match(ref, qry, mutual)
        idx, dist = R.match_features(ref, qry, mutual=mutual, return_dist=True)
        assert idx.dtype == np.int32 and dist.dtype == np.uint32
        assert np.array_equal(idx, eidx) and np.array_equal(dist, edist), (n, m, mutual, int((idx != eidx).sum()))
    if n == 1:
        assert int(edist[0]) == 33 * G.DESC_MAX ** 2
    if n >= 63 and m >= 64:
        plain = G.ref_match(ref, qry)[0]
        assert plain[5] == 2 and plain[6] == 2 and (eidx[5], eidx[6]) == (2, 0)     # the tie goes to row 2, and row 2 to query 6
        assert (eidx == 0).sum() > 0 and (eidx > 0).sum() > 0


def test_match_on_real_descriptors_and_device_pointers():
    ref = R.describe(SCENE["ref"], SCENE["ref_nrm"], k=32)
    qry = R.describe(SCENE["qry"], SCENE["qry_nrm"], k=32)
    eidx, edist = G.ref_match(ref, qry, True)
    d_ref, d_qry = torch.from_numpy(ref.view(np.int16)).cuda(), torch.from_numpy(qry.view(np.int16)).cuda()
    d_idx = torch.zeros(len(qry), dtype=torch.int32, device="cuda")
    L.check(R.lib().rh_match_features(_dptr(d_ref, C.c_uint16), len(ref), _dptr(d_qry, C.c_uint16), len(qry), L.MATCH_MUTUAL, 0,
                                      _dptr(d_idx, C.c_int32), None))
    torch.cuda.synchronize()
    assert np.array_equal(d_idx.cpu().numpy(), eidx)


def test_a_value_above_the_range_is_refused():
    ref, qry = _descs(200, 1), _descs(300, 2)
    for bad_ref, at in ((True, (199, 32)), (False, (0, 0)), (False, (299, 31))):
        r, q = ref.copy(), qry.copy()
        (r if bad_ref else q)[at] = G.DESC_MAX + 1
        idx = np.full(300, -7, dtype=np.int32)
        rc = R.lib().rh_match_features(r.ctypes.data_as(C.POINTER(C.c_uint16)), 200, q.ctypes.data_as(C.POINTER(C.c_uint16)), 300, 0, 0,
                                       idx.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == L.RH_E_INVALID and (idx == -7).all()


# ------------------------------------------------------------------------ 3. register_global ----
def _pairs(c, seed=0, outliers=0.5):
    """c correspondences between two clouds of 1500 and 1300 points: a part of them true (up to the scene's noise)"""
    rng = np.random.default_rng(seed)
    ref, qry = SCENE["ref"][:1500], SCENE["qry"][:1300]
    cq = rng.integers(1, 1301, size=c).astype(np.int32) if c > 3 else np.array([1, 2, 3], dtype=np.int32)
    truth = SCENE["truth"][cq - 1]
    d = ((truth[:, None, :] - ref[None, :, :]) ** 2).sum(axis=2)
    cr = (np.argmin(d, axis=1) + 1).astype(np.int32)
    wrong = rng.random(c) < outliers
    cr[wrong] = rng.integers(1, 1501, size=int(wrong.sum()))
    return np.ascontiguousarray(ref), np.ascontiguousarray(qry), cq, cr


def _call(ref, qry, cq, cr, tau, trials=None, seed=0, edge_ratio=0.9, min_edge=0.0, triples=None, f32=False):
    trials = len(triples) if triples is not None else trials
    prm = L.GlobalParams(trials=trials, seed=seed, tau=tau, edge_ratio=edge_ratio, min_edge=min_edge)
    out, res, counts = np.full((3, 4), -5.0), L.GlobalResult(), np.full(trials, -9, dtype=np.int32)
    ct = C.c_float if f32 else C.c_double
    tri = None if triples is None else np.ascontiguousarray(triples, dtype=np.int32)
    fn = R.lib().rh_register_global_f32 if f32 else R.lib().rh_register_global
    L.check(fn(ref.ctypes.data_as(C.POINTER(ct)), len(ref), qry.ctypes.data_as(C.POINTER(ct)), len(qry),
               cq.ctypes.data_as(C.POINTER(C.c_int32)), cr.ctypes.data_as(C.POINTER(C.c_int32)), len(cq), C.byref(prm),
               None if tri is None else tri.ctypes.data_as(C.POINTER(C.c_int32)), 0, out.ctypes.data_as(C.POINTER(C.c_double)),
               C.byref(res), counts.ctypes.data_as(C.POINTER(C.c_int32))))
    return out, res, counts


def _same(got, exp):
    out, res, counts = got
    assert np.array_equal(counts, exp["counts"]), int((counts != exp["counts"]).sum())
    assert out.tobytes() == np.ascontiguousarray(exp["transform"], dtype=np.float64).tobytes()
    assert (res.status, res.best_trial, res.best_count, res.n_valid_trials) == (
        exp["status"], exp["best_trial"], exp["best_count"], exp["n_valid_trials"])


@pytest.mark.parametrize("c,trials", [(3, 1), (64, 64), (65, 65), (2048, 4096)])
def test_given_triples_equal_the_twin(c, trials):
    ref, qry, cq, cr = _pairs(c, seed=c, outliers=0.0 if c == 3 else 0.5)
    rng = np.random.default_rng(c)
    tri = rng.integers(0, c, size=(trials, 3)).astype(np.int32)
    if c == 3:
        tri[0] = [2, 0, 1]
    else:
        tri[1] = [4, 4, 9]                                           # a repeated index among them
    kw = dict(edge_ratio=0.8, min_edge=0.05)
    exp = G.ref_global(ref, qry, cq, cr, GS.TAU, triples=tri, **kw)
    _same(_call(ref, qry, cq, cr, GS.TAU, triples=tri, **kw), exp)
    assert exp["n_valid_trials"] >= 1 and (c == 3 or (exp["counts"] == -1).sum() >= 1)
    if c == 2048:
        assert exp["best_count"] > 500 and GS.rotation_error_deg(exp["transform"], SCENE["inverse"]) < 10.0


@pytest.mark.parametrize("seed", [1, 77])
def test_the_drawn_path_equals_the_twin_and_the_replayed_draws(seed):
    ref, qry, cq, cr = _pairs(300, seed=5)
    exp = G.ref_global(ref, qry, cq, cr, GS.TAU, 2000, seed, 0.85)
    got = _call(ref, qry, cq, cr, GS.TAU, trials=2000, seed=seed, edge_ratio=0.85)
    _same(got, exp)
    rng = L.Rng()                                                    # the triples the call used, replayed from the host generator
    R.lib().rh_rng_seed(C.byref(rng), seed)
    tri = np.array([R.lib().rh_rng_range(C.byref(rng), 300) - 1 for _ in range(6000)], dtype=np.int32).reshape(2000, 3)
    again = _call(ref, qry, cq, cr, GS.TAU, triples=tri, edge_ratio=0.85)
    assert np.array_equal(again[2], got[2]) and again[0].tobytes() == got[0].tobytes()
    assert exp["n_valid_trials"] > 10


def test_no_valid_trial_gives_the_identity():
    ref, qry, cq, cr = _pairs(64, seed=3)
    tri = np.array([[1, 1, 2], [5, 6, 5], [7, 7, 7]], dtype=np.int32)
    out, res, counts = _call(ref, qry, cq, cr, GS.TAU, triples=tri)
    assert counts.tolist() == [-1, -1, -1] and np.array_equal(out, np.eye(4)[:3])
    assert (res.status, res.best_trial, res.best_count, res.n_valid_trials) == (L.GLOB_NO_TRIAL, -1, -1, 0)
    _same((out, res, counts), G.ref_global(ref, qry, cq, cr, GS.TAU, triples=tri))
    # every edge refused: a min_edge beyond the scene
    exp = G.ref_global(ref, qry, cq, cr, GS.TAU, 500, 2, min_edge=50.0)
    _same(_call(ref, qry, cq, cr, GS.TAU, trials=500, seed=2, min_edge=50.0), exp)
    assert exp["status"] == G.NO_TRIAL


def test_register_global_float32_is_the_widened_double_call():
    ref, qry, cq, cr = _pairs(500, seed=8)
    r32, q32 = ref.astype(np.float32), qry.astype(np.float32)
    exp = G.ref_global(r32.astype(np.float64), q32.astype(np.float64), cq, cr, GS.TAU, 1000, 4)
    _same(_call(r32, q32, cq, cr, GS.TAU, trials=1000, seed=4, f32=True), exp)
    assert exp["n_valid_trials"] > 5


def test_bad_correspondences_and_triples_write_nothing():
    ref, qry, cq, cr = _pairs(64, seed=3)
    for bq, br, tri in ((1301, 1, None), (0, 1, None), (1, 1501, None), (1, 1, [[0, 1, 64]]), (1, 1, [[-1, 1, 2]])):
        q2, r2 = cq.copy(), cr.copy()
        q2[10], r2[11] = bq, br
        with pytest.raises(R.RansacHipError) as e:
            _call(ref, qry, q2, r2, GS.TAU, trials=10, triples=tri)
        assert e.value.code == L.RH_E_INVALID
    bad = qry.copy()
    bad[3, 0] = np.nan
    with pytest.raises(R.RansacHipError) as e:
        _call(ref, bad, cq, cr, GS.TAU, trials=10)
    assert e.value.code == L.RH_E_INVALID


# ------------------------------------------------------------------------------ 4. end to end ----
def test_the_whole_chain_on_the_scene_equals_the_twin_chain():
    s = SCENE
    exp = G.ref_register_global(s["ref"], s["qry"], s["ref_nrm"], s["qry_nrm"], GS.TAU, k=GS.K, trials=GS.TRIALS,
                                edge_ratio=GS.EDGE_RATIO, seed=1)
    T, info = R.register_global(s["ref"], s["qry"], s["ref_nrm"], s["qry_nrm"], GS.TAU, k=GS.K, trials=GS.TRIALS,
                                edge_ratio=GS.EDGE_RATIO, seed=1, return_info=True)
    assert np.array_equal(info["corr_qry"], exp["corr_qry"]) and np.array_equal(info["corr_ref"], exp["corr_ref"])
    assert np.array_equal(info["counts"], exp["counts"])
    assert info["coarse"][:3].tobytes() == exp["transform"].tobytes()
    assert (info["status"], info["best_trial"], info["best_count"], info["n_valid_trials"]) == (
        "ok", exp["best_trial"], exp["best_count"], exp["n_valid_trials"])
    assert T[:3].tobytes() == exp["T"].tobytes() and info["register"]["iterations"] == exp["register"]["iterations"]
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    print("coarse %.2f deg, refined point error %.5f" % (GS.rotation_error_deg(info["coarse"], s["inverse"]), GS.point_error(T, s)))
    # what it is there for: the clouds in one frame, as far apart as their own noise
    stats = R.cloud_distance(s["ref"], R.transform_points(T, s["qry"]), normals=s["ref_nrm"], return_stats=True)[1]
    assert stats["rms"] < 2.0 * GS.SIGMA * math.sqrt(3.0)
    coarse_only = R.register_global(s["ref"], s["qry"], s["ref_nrm"], s["qry_nrm"], GS.TAU, k=GS.K, trials=GS.TRIALS,
                                    edge_ratio=GS.EDGE_RATIO, seed=1, refine=False)
    assert coarse_only.tobytes() == info["coarse"].tobytes()
