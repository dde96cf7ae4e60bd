"""Nearest neighbours of query points in another cloud and cloud distances (rh_knn_query, rh_cloud_distance) on the GPU,
held to the numpy twin of tests/query_reference.py for EQUALITY: indices, counts, and the bytes of every double -- d2, the
distances, mean, rms, max, median.  The definition fixes every operation and its order, so nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from query_reference import ref_cloud_distance, ref_knn_query, ref_query_order
from test_knn_gpu import _datasets

pytestmark = pytest.mark.gpu

KS = [1, 8, 16, 63]
B = L.OUT_BLOCK_POINTS                 # points per block of the reduction tree
NAMES = ["cylinder", "lattice", "plane", "sphere", "uniform"]
DATA = _datasets()                     # the five clouds of tests/test_knn_gpu.py: 2000 - 3000 points each
FAR_DIRS = [(1, 0, 0), (0, -1, 0), (1, 1, 0), (0, -1, 1), (1, 1, 1), (-1, -1, -1)]   # off a face, an edge, a corner


def _same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _spacing(ref):
    """the median distance to the nearest OTHER reference point (1 where duplicates make it 0: the lattice)"""
    d2 = ref_query_order(ref, ref, 2)[1][:, 1]
    s = float(np.sqrt(np.median(d2)))
    return s if s > 0.0 else 1.0


def _query_set(ref, seed):
    """Reference points themselves; reference points displaced by about a point spacing; uniform points in the box
    inflated by 25 % on every side; points 5 and 1000 box lengths outside.  Returns (queries, rows of the far ones)."""
    rng = np.random.default_rng(seed)
    n = len(ref)
    lo, hi = ref.min(axis=0), ref.max(axis=0)
    ext = hi - lo
    side = float(ext.max())
    own = ref[rng.choice(n, 300, replace=False)]
    near = ref[rng.choice(n, 400)] + rng.normal(0.0, _spacing(ref), size=(400, 3))
    pad = 0.25 * np.maximum(ext, 1e-3 * side)
    box = rng.uniform(lo - pad, hi + pad, size=(600, 3))
    far = []
    for mult in (5.0, 1000.0):
        for d in FAR_DIRS:
            d = np.array(d, dtype=np.float64)
            base = 0.5 * (lo + hi) + d * (0.5 * ext + mult * side)
            far.append(base + rng.uniform(-0.3, 0.3, size=(3, 3)) * ext * (d == 0))   # (jitter along the box, not towards it)
    far = np.concatenate(far)
    q = np.ascontiguousarray(np.concatenate([own, near, box, far]))
    return q, np.arange(len(q) - len(far), len(q))


_SETS, _NB = {}, {}


def _set(name):
    if name not in _SETS:
        _SETS[name] = _query_set(DATA[name], 40 + NAMES.index(name))
    return _SETS[name]


def _nb(name):
    """one brute-force search per cloud, shared by every k and radius"""
    if name not in _NB:
        _NB[name] = ref_query_order(DATA[name], _set(name)[0], 64)
    return _NB[name]


def _check(ref, qry, k, radius=0.0, nb=None):
    idx, d2, count = R.knn_query(ref, qry, k, radius=radius, return_count=True)
    eidx, ed2, ecount = ref_knn_query(ref, qry, k, radius, nb=nb)
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and count.dtype == np.int32
    assert idx.shape == (len(qry), k) and d2.shape == (len(qry), k) and count.shape == (len(qry),)
    assert np.array_equal(count, ecount), np.flatnonzero(count != ecount)[:10]
    assert np.array_equal(idx, eidx), np.argwhere(idx != eidx)[:10]
    assert _same_bytes(d2, ed2)
    return eidx, ed2, ecount


# ------------------------------------------------------------------------- 1. the five clouds ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("with_radius", [False, True])
def test_query_equals_the_twin(name, k, with_radius):
    ref, (qry, _) = DATA[name], _set(name)
    radius = 0.0
    if with_radius:
        radius = float(np.sqrt(np.median(_nb(name)[1][:, k - 1])))        # the median k-th distance
        radius = radius if radius > 0.0 else 1.0                          # (the lattice at k = 1: a median of 0 is "no limit")
    _, _, ecount = _check(ref, qry, k, radius, nb=_nb(name))
    if not with_radius:
        assert (ecount == k).all()
    elif name != "lattice":                                               # (on the lattice whole shells tie at the median)
        assert 0 < (ecount < k).sum() < len(qry)                          # the radius cuts some lists and not all


# --------------------------------------------------------------------------------- 2. margin ----
@pytest.mark.parametrize("shift", [(1e6, 0.0, 0.0), (1e6, 1e6, 1e6)])
@pytest.mark.parametrize("moved", ["queries", "reference"])
def test_clouds_a_million_apart(shift, moved):
    """The distance bounds of the search are rounded at the magnitude of the farther cloud: its margin has to cover that."""
    ref, (qry, _) = DATA["uniform"][:2000], _set("uniform")
    if moved == "queries":
        qry = np.ascontiguousarray(qry + np.array(shift))
    else:
        ref = np.ascontiguousarray(ref + np.array(shift))
    _check(ref, qry, 8)


# ------------------------------------------------------------------------ 3. table-scan path ----
@pytest.mark.parametrize("k", [1, 16])
def test_two_blobs_far_apart(k):
    rng = np.random.default_rng(3)
    a, b = rng.normal(0.0, 0.1, size=(1000, 3)), rng.normal(0.0, 0.1, size=(1000, 3))
    diam = float(np.linalg.norm(a.max(axis=0) - a.min(axis=0)))
    gap = 1000.0 * diam
    ref = np.ascontiguousarray(np.concatenate([a, b + [gap, 0.0, 0.0]]))
    t = np.linspace(0.0, 1.0, 41)                                         # t = 0.5, the midpoint, among them
    line = np.stack([t * gap, np.zeros_like(t), np.zeros_like(t)], axis=1)
    qry = np.ascontiguousarray(np.concatenate([line, line[18:23] + rng.normal(0.0, 0.05, size=(5, 3))]))
    eidx, _, ecount = _check(ref, qry, k)
    assert (ecount == k).all()
    if k > 1:                                                             # some lists reach across: both blobs in one list
        assert ((eidx <= 1000).any(axis=1) & (eidx > 1000).any(axis=1)).any()
    else:                                                                 # ... and the single neighbours come from both sides
        assert (eidx <= 1000).any() and (eidx > 1000).any()


# ---------------------------------------------------------------------- 4. radius early-out ----
@pytest.mark.parametrize("name", NAMES)
def test_far_queries_end_empty_within_a_point_spacing(name):
    ref, (qry, far) = DATA[name], _set(name)
    radius = _spacing(ref)
    idx, d2, count = R.knn_query(ref, qry, 8, radius=radius, return_count=True)
    assert not count[far].any() and not idx[far].any() and np.isposinf(d2[far]).all()
    _, _, ecount = _check(ref, qry, 8, radius, nb=_nb(name))              # the near ones are unaffected
    assert 0 < (ecount > 0).sum() < len(qry)


# ---------------------------------------------------------------------- 5. degenerate shapes ----
def test_degenerate_shapes():
    rng = np.random.default_rng(5)
    qry = rng.uniform(-2.0, 12.0, size=(37, 3))
    one = np.array([[1.0, 2.0, 3.0]])
    _, _, c = _check(one, np.concatenate([qry, one]), 4)                  # n = 1
    assert (c == 1).all()
    _check(one, qry, 1, radius=9.0)
    copies = np.ascontiguousarray(np.repeat(one, 500, axis=0))            # an extent of 0 along every axis
    eidx, ed2, _ = _check(copies, np.concatenate([qry, one]), 8)
    assert (eidx == np.arange(1, 9)).all() and (ed2[-1] == 0.0).all()     # all tie: the index order
    flat = rng.uniform(0.0, 10.0, size=(2000, 3))
    flat[:, 2] = 3.0                                                      # a planar reference, queries off the plane
    _check(flat, np.ascontiguousarray(qry), 8)
    _check(flat, np.ascontiguousarray(qry), 8, radius=2.0)
    for m in (1, 3, 4, 5):                                                # a partial block of query waves
        _check(DATA["uniform"], np.ascontiguousarray(qry[:m]), 8)
    few = rng.uniform(0.0, 10.0, size=(5, 3))                             # k > n
    eidx, ed2, c = _check(few, qry, 16)
    assert (c == 5).all() and not eidx[:, 5:].any() and np.isposinf(ed2[:, 5:]).all()


# ----------------------------------------------------------------------------------- 6. ties ----
@pytest.mark.parametrize("k", [1, 8, 27])
def test_ties_follow_the_index_order(k):
    g = np.arange(8, dtype=np.float64)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ref = np.ascontiguousarray(sites[np.random.default_rng(6).permutation(len(sites))])
    c = np.arange(7, dtype=np.float64) + 0.5
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    qry = np.ascontiguousarray(np.concatenate([centres, sites]))
    eidx, ed2, _ = _check(ref, qry, k)
    assert (ed2[:len(centres), :min(k, 8)] == 0.75).all()                 # eight reference points at equal d^2 ...
    if k >= 8:
        assert (np.diff(eidx[:len(centres), :8], axis=1) > 0).all()       # ... in index order


# ---------------------------------------------------------------- 7. against the existing call ----
@pytest.mark.parametrize("k", [1, 16, 62])
def test_self_query_is_knn_with_the_point_in_front(k):
    x = DATA["uniform"]
    assert len(np.unique(x, axis=0)) == len(x)                            # duplicate-free: d^2 = 0 only for the point itself
    idx, d2 = R.knn_query(x, x, k + 1)
    sidx, sd2 = R.knn(x, k)
    assert np.array_equal(idx[:, 0], np.arange(1, len(x) + 1)) and not d2[:, 0].any()
    assert idx[:, 1:].tobytes() == sidx.tobytes() and d2[:, 1:].tobytes() == sd2.tobytes()


# ------------------------------------------------------------------------------ 8. row order ----
def test_row_order_two_runs_and_optional_outputs():
    ref, (qry, _) = DATA["cylinder"], _set("cylinder")
    a = R.knn_query(ref, qry, 8, return_count=True)
    b = R.knn_query(ref, qry, 8, return_count=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    perm = np.random.default_rng(8).permutation(len(qry))
    p = R.knn_query(ref, np.ascontiguousarray(qry[perm]), 8, return_count=True)
    for u, v in zip(a, p):
        assert u[perm].tobytes() == v.tobytes()                           # permuting the queries permutes the rows
    only_idx = R.knn_query(ref, qry, 8, return_dist=False)
    assert isinstance(only_idx, np.ndarray) and only_idx.tobytes() == a[0].tobytes()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cnt, d2 = np.zeros(len(qry), dtype=np.int32), np.zeros((len(qry), 8))
    fn = R.lib().rh_knn_query
    L.check(fn(ref.ctypes.data_as(dp), len(ref), qry.ctypes.data_as(dp), len(qry), 8, 0.5, 0, None, None, cnt.ctypes.data_as(i32p)))
    assert np.array_equal(cnt, ref_knn_query(ref, qry, 8, 0.5, nb=_nb("cylinder"))[2])
    L.check(fn(ref.ctypes.data_as(dp), len(ref), qry.ctypes.data_as(dp), len(qry), 8, 0.0, 0, None, d2.ctypes.data_as(dp), None))
    assert d2.tobytes() == a[1].tobytes()
    L.check(fn(ref.ctypes.data_as(dp), len(ref), qry.ctypes.data_as(dp), len(qry), 8, 0.0, 0, None, None, None))


def test_a_coordinate_of_either_cloud_that_is_not_finite():
    ref, qry = DATA["uniform"][:300].copy(), _set("uniform")[0][:257].copy()
    bad_ref, bad_qry = ref.copy(), qry.copy()
    bad_ref[37, 1] = np.nan
    bad_qry[256, 2] = np.inf                                              # the last row of the second block
    for r, q in ((bad_ref, qry), (ref, bad_qry)):
        for call in (lambda: R.knn_query(r, q, 4), lambda: R.cloud_distance(r, q)):
            with pytest.raises(R.RansacHipError) as e:
                call()
            assert e.value.code == L.RH_E_INVALID


# --------------------------------------------------------------------------------- 9. float32 ----
def test_float32_is_the_widened_double_call():
    for name in ("uniform", "lattice", "cylinder"):
        r32, q32 = DATA[name].astype(np.float32), _set(name)[0].astype(np.float32)
        a = R.knn_query(r32, q32, 16, return_count=True)
        b = R.knn_query(r32.astype(np.float64), q32.astype(np.float64), 16, return_count=True)
        assert a[1].dtype == np.float64
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
        # a mixed pair is widened in Python: the float64 call on the widened array
        for mixed in (R.knn_query(r32, q32.astype(np.float64), 16, return_count=True),
                      R.knn_query(r32.astype(np.float64), q32, 16, return_count=True)):
            for u, v in zip(mixed, b):
                assert u.tobytes() == v.tobytes()
    e = ref_knn_query(r32.astype(np.float64), q32.astype(np.float64), 16)
    assert np.array_equal(a[0], e[0]) and _same_bytes(a[1], e[1]) and np.array_equal(a[2], e[2])
    d32 = R.cloud_distance(r32, q32, return_index=True, return_stats=True)
    d64 = R.cloud_distance(r32.astype(np.float64), q32.astype(np.float64), return_index=True, return_stats=True)
    assert d32[0].dtype == np.float64 and d32[0].tobytes() == d64[0].tobytes() and np.array_equal(d32[1], d64[1])
    assert d32[2] == d64[2]


# ---------------------------------------------------------------------------- 10. distances ----
def _sphere_pair(m, seed=10):
    """a sphere of 2500 points with its normals, and m points of the same sphere displaced by a tenth of its radius"""
    rng = np.random.default_rng(seed)
    ref, nrm, _ = synth.sphere(2500, rng, radius=8.0)
    pick = rng.choice(len(ref), m)
    qry = ref[pick] + rng.normal(0.0, 0.8, size=(m, 3))
    return np.ascontiguousarray(ref), np.ascontiguousarray(nrm), np.ascontiguousarray(qry)


STAT_FIELDS = ("n_valid", "n_within", "argmax", "mean", "rms", "max", "median")
_SUMS_DIFFER = []


def _check_distance(ref, qry, normals, metric, radius, threshold):
    exp = ref_cloud_distance(ref, qry, normals=normals, radius=radius, threshold=threshold, metric=metric)
    dist, nn, st = R.cloud_distance(ref, qry, normals=normals, radius=radius, threshold=threshold, metric=metric,
                                    return_index=True, return_stats=True)
    print("m=%d %s radius %r: %r (twin %r)" % (len(qry), metric, radius, st, {f: exp[f] for f in STAT_FIELDS}))
    assert dist.dtype == np.float64 and nn.dtype == np.int32
    assert np.array_equal(nn, exp["nn_idx"]), np.flatnonzero(nn != exp["nn_idx"])[:10]
    assert _same_bytes(dist, exp["dist"])
    for f in STAT_FIELDS[:3]:
        assert st[f] == exp[f], (f, st[f], exp[f])
    for f in STAT_FIELDS[3:]:
        assert _same_bytes(st[f], exp[f]), (f, st[f], exp[f])
    only = R.cloud_distance(ref, qry, normals=normals, radius=radius, metric=metric)      # the distances alone
    assert isinstance(only, np.ndarray) and only.tobytes() == dist.tobytes()
    if exp["n_valid"]:
        valid = exp["nn_idx"] > 0
        _SUMS_DIFFER.append(float(np.sum(exp["dist"][valid]) / exp["n_valid"]) != exp["mean"])
    return exp


@pytest.mark.parametrize("m", [B - 1, B, B + 1, 2 * B + 3])
@pytest.mark.parametrize("metric", ["point", "plane"])
def test_cloud_distance_equals_the_twin(m, metric):
    """m around the boundaries of the reduction tree's blocks; with and without a radius that invalidates some queries."""
    ref, nrm, qry = _sphere_pair(m)
    normals = nrm if metric == "plane" else None
    free = _check_distance(ref, qry, normals, metric, 0.0, 0.5)
    assert free["n_valid"] == m and 0 < free["n_within"] < m
    radius = float(np.median(ref_cloud_distance(ref, qry)["dist"]))       # about half of the queries have a point within it
    cut = _check_distance(ref, qry, normals, metric, radius, np.inf)
    assert 0 < cut["n_valid"] < m and cut["n_within"] == cut["n_valid"]
    if metric == "plane":                                                 # normals that are not unit vectors are used as given
        _check_distance(ref, qry, np.ascontiguousarray(nrm * np.linspace(0.5, 3.0, len(nrm))[:, None]), metric, 0.0, 0.5)


def test_cloud_distance_the_summation_order_shows_in_the_last_bit():
    """np.sum adds in another order than T(): on at least one of the inputs above its mean differs from the tree's in the
    last bits, so the byte comparison of `mean` tests the tree and not luck."""
    if not _SUMS_DIFFER:                                                  # (run alone: the inputs of the test above)
        for m in (B - 1, B, B + 1, 2 * B + 3):
            ref, _, qry = _sphere_pair(m)
            exp = ref_cloud_distance(ref, qry)
            _SUMS_DIFFER.append(float(np.sum(exp["dist"]) / m) != exp["mean"])
    assert any(_SUMS_DIFFER)


def test_cloud_distance_no_valid_query_and_a_single_one():
    ref, nrm, qry = _sphere_pair(B + 1)
    away = np.ascontiguousarray(qry + 1e4)
    exp = _check_distance(ref, away, None, "point", 1.0, np.inf)
    assert exp["n_valid"] == 0 and exp["argmax"] == 0 and np.isposinf(exp["dist"]).all()
    one = np.ascontiguousarray(np.concatenate([away[:700], ref[5:6], away[700:]]))        # the only valid query, at 0
    exp = _check_distance(ref, one, nrm, "plane", 1.0, 0.0)
    assert (exp["n_valid"], exp["n_within"], exp["argmax"], exp["max"]) == (1, 1, 701, 0.0)
    # several queries reach the maximum: the smallest index
    dup = np.ascontiguousarray(np.concatenate([qry[:50], qry[7:8], qry[50:], qry[7:8]]))
    far7 = ref_cloud_distance(ref, dup)
    dup[[7, 50, len(dup) - 1]] += 3.0 * (dup[7] - ref.mean(axis=0)) / np.linalg.norm(dup[7] - ref.mean(axis=0))
    exp = _check_distance(ref, dup, None, "point", 0.0, 1.0)
    assert exp["argmax"] == 8 and exp["max"] > far7["max"] and (exp["dist"] == exp["max"]).sum() == 3


# ----------------------------------------------------------------------- 11. transfer_labels ----
def test_labels_of_a_thinned_cloud_reach_the_full_cloud():
    rng = np.random.default_rng(12)
    pl, pl_n, tp = synth.plane_patch(1500, rng, size=20.0)
    sp, sp_n, ts = synth.sphere(1500, rng, radius=8.0)
    stray = rng.uniform(0.0, 100.0, size=(40, 3))
    order = rng.permutation(3040)
    full = np.ascontiguousarray(np.concatenate([pl, sp, stray])[order])
    full_n = np.ascontiguousarray(np.concatenate([pl_n, sp_n, np.tile([0.0, 0.0, 1.0], (40, 1))])[order])
    thin, thin_n = R.voxeldownsample(full, 1.0, normals=full_n)
    shapes = [R.FittedPlane(tp["point"], tp["normal"]), R.FittedSphere(ts["center"], ts["radius"], True)]
    labels = R.assign_points(thin, thin_n, shapes, R.ransacparameters([R.FittedPlane, R.FittedSphere]))
    assert len(thin) < len(full) and len(np.unique(labels)) >= 2          # something to carry: more than one label
    nb = ref_query_order(thin, full, 1)
    for radius, fill in ((0.0, 0), (0.6, -1)):
        eidx, _, ecount = ref_knn_query(thin, full, 1, radius, nb=nb)
        exp = np.where(ecount > 0, labels[np.maximum(eidx[:, 0], 1) - 1], fill).astype(labels.dtype)
        got = R.transfer_labels(thin, labels, full, radius=radius, fill=fill)
        assert got.dtype == labels.dtype and np.array_equal(got, exp)
        assert (ecount == 0).any() == (radius > 0.0)                      # the radius excludes some, and only the radius
    # any per-point attribute rides the same way: the thinned normals, row by row
    got_n = R.transfer_labels(thin, thin_n, full)
    assert got_n.shape == full.shape and got_n.tobytes() == thin_n[ref_knn_query(thin, full, 1, nb=nb)[0][:, 0] - 1].tobytes()
