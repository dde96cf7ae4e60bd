"""Exact k nearest neighbours and outlier removal (rh_knn, rh_remove_outliers) on the GPU, held to the numpy twin of
tests/test_knn_host.py for EQUALITY: indices, counts, kept sets, and the bytes of every double -- d2, the mean distances,
mu, sigma, tau, the median.  The definition fixes every operation and its order, so nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from test_knn_host import outlier_cloud, ref_knn, ref_outliers
from test_normals_host import ref_neighbours

pytestmark = pytest.mark.gpu

KS = [1, 8, 16, 63]
B = L.OUT_BLOCK_POINTS                 # points per block of the reduction tree


def _datasets():
    """The five clouds of tests/test_normals_gpu.py."""
    rng = np.random.default_rng(11)
    out = {"uniform": rng.uniform(0, 10, size=(3000, 3)),
           "lattice": rng.integers(0, 8, size=(2000, 3)).astype(np.float64)}   # 512 sites: duplicates and ties
    out["plane"] = synth.plane_patch(3000, rng, size=20.0)[0]
    out["sphere"] = synth.sphere(3000, rng, radius=8.0)[0]
    out["cylinder"] = synth.cylinder(3000, rng)[0]
    return out


DATA = _datasets()
DATA["outliers"] = outlier_cloud()
_NB = {}


def _nb(name):
    if name not in _NB:
        _NB[name] = ref_neighbours(DATA[name], 64)
    return _NB[name]


def _same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _radius(name, k):
    r = float(np.sqrt(np.median(_nb(name)[1][:, k])))         # about half of the points keep all k
    return r if r > 0.0 else 1.0                              # (the lattice's duplicates: a median of 0 would mean "no limit")


@pytest.mark.parametrize("name", ["cylinder", "lattice", "plane", "sphere", "uniform"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("with_radius", [False, True])
def test_knn_equals_the_twin(name, k, with_radius):
    xyz = DATA[name]
    radius = _radius(name, k) if with_radius else 0.0
    idx, d2, count = R.knn(xyz, k, radius=radius, return_count=True)
    eidx, ed2, ecount = ref_knn(xyz, k, radius, nb=_nb(name))
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and count.dtype == np.int32
    assert np.array_equal(count, ecount), np.flatnonzero(count != ecount)[:10]
    assert np.array_equal(idx, eidx), np.argwhere(idx != eidx)[:10]
    assert _same_bytes(d2, ed2)
    if not with_radius:
        assert (count == k).all()
    elif name != "lattice":                                   # (on the lattice whole shells tie at the median)
        assert 0 < (ecount < k).sum() < len(xyz)              # the radius cuts some lists and not all


def test_knn_float32_is_the_widened_double_call():
    for name in ("uniform", "lattice", "cylinder"):
        x32 = DATA[name].astype(np.float32)
        a = R.knn(x32, 16, radius=0.0, return_count=True)
        b = R.knn(x32.astype(np.float64), 16, radius=0.0, return_count=True)
        assert a[1].dtype == np.float64
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
        e = ref_knn(x32.astype(np.float64), 16)
        assert np.array_equal(a[0], e[0]) and _same_bytes(a[1], e[1])


def test_knn_two_runs_give_the_same_bytes_and_outputs_are_optional():
    xyz = DATA["lattice"]
    a = R.knn(xyz, 8, return_count=True)
    b = R.knn(xyz, 8, return_count=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    only_idx = R.knn(xyz, 8, return_dist=False)
    assert isinstance(only_idx, np.ndarray) and only_idx.tobytes() == a[0].tobytes()
    cnt = np.zeros(len(xyz), dtype=np.int32)
    L.check(R.lib().rh_knn(xyz.ctypes.data_as(C.POINTER(C.c_double)), len(xyz), 8, 1.0, 0, None, None,
                           cnt.ctypes.data_as(C.POINTER(C.c_int32))))
    assert np.array_equal(cnt, ref_knn(xyz, 8, 1.0, nb=_nb("lattice"))[2])


def _check_outliers(xyz, k, mode, nb, **kw):
    exp = ref_outliers(xyz, k, mode, nb=nb, **kw)
    pts, idx, st, mean = R.removeoutliers(xyz, k=k, mode=mode, return_index=True, return_stats=True, return_mean_dist=True, **kw)
    print("k=%d %s %r: dropped %d, mu %r sigma %r tau %r median %r (twin %r %r %r %r)"
          % (k, mode, kw, len(xyz) - st["n_kept"], st["mu"], st["sigma"], st["tau"], st["nn_median"],
             exp["mu"], exp["sigma"], exp["tau"], exp["nn_median"]))
    assert st["n_valid"] == exp["n_valid"] and st["n_kept"] == exp["n_kept"] == len(idx)
    assert idx.dtype == np.int32 and np.array_equal(idx, exp["kept_idx"])
    assert _same_bytes(mean, exp["mean_dist"])
    for f in ("mu", "sigma", "tau", "nn_median"):
        assert _same_bytes(st[f], exp[f]), (f, st[f], exp[f])
    assert pts.tobytes() == xyz[exp["kept_idx"] - 1].tobytes()
    return exp, idx


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("std_mul", [1.0, 2.0])
def test_outliers_all_modes_equal_the_twin(k, std_mul):
    xyz, nb = DATA["outliers"], _nb("outliers")
    exp, _ = _check_outliers(xyz, k, "statistical", nb, std_mul=std_mul)
    assert 46 <= len(xyz) - exp["n_kept"] <= 56
    # the raw entry's keep flags (the wrapper returns the list)
    keep, nk = np.zeros(len(xyz), dtype=np.uint8), C.c_int64()
    prm = L.OutlierParams(k=k, mode=L.OUT_STATISTICAL, std_mul=std_mul)
    L.check(R.lib().rh_remove_outliers(xyz.ctypes.data_as(C.POINTER(C.c_double)), len(xyz), C.byref(prm), 0,
                                       keep.ctypes.data_as(C.POINTER(C.c_uint8)), None, 0, C.byref(nk), None, None))
    assert np.array_equal(keep, exp["keep"]) and nk.value == exp["n_kept"]
    # absolute: a threshold of std_mul times twice the median mean distance; radius: std_mul times the median k-th distance
    thr = std_mul * 2.0 * float(np.median(exp["mean_dist"]))
    ea, _ = _check_outliers(xyz, k, "absolute", nb, threshold=thr)
    assert 0 < len(xyz) - ea["n_kept"] < len(xyz)
    er, _ = _check_outliers(xyz, k, "radius", nb, radius=std_mul * _radius("outliers", k))
    assert 0 < er["n_kept"] < len(xyz)


def test_outliers_a_shuffled_copy_keeps_the_same_points():
    xyz = DATA["outliers"]
    perm = np.random.default_rng(8).permutation(len(xyz))
    for k in (8, 63):
        _, idx = R.removeoutliers(xyz, k=k, return_index=True)
        _, idx2 = R.removeoutliers(np.ascontiguousarray(xyz[perm]), k=k, return_index=True)
        assert np.array_equal(np.sort(perm[idx2 - 1]), idx - 1)


def test_outliers_float32_and_normals_ride_along():
    x32 = DATA["outliers"].astype(np.float32)
    nrm = np.arange(3 * len(x32), dtype=np.float32).reshape(-1, 3)
    p32, n32, i32, s32 = R.removeoutliers(x32, k=16, normals=nrm, return_index=True, return_stats=True)
    _, i64, s64 = R.removeoutliers(x32.astype(np.float64), k=16, return_index=True, return_stats=True)
    assert p32.dtype == np.float32 and np.array_equal(i32, i64) and s32 == s64
    assert np.array_equal(p32, x32[i32 - 1]) and np.array_equal(n32, nrm[i32 - 1])
    exp = ref_outliers(x32.astype(np.float64), 16)
    assert np.array_equal(i32, exp["kept_idx"]) and _same_bytes(s32["mu"], exp["mu"])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, B - 1, B, B + 1, 3 * B + 5])
def test_tree_boundaries(n):
    """Sizes around the lane, wave and block boundaries of the reduction: mu and sigma to the byte."""
    rng = np.random.default_rng(100 + n)
    xyz = rng.uniform(0, 10, size=(n, 3)) * [1.0, 1.0, 0.05]
    exp = ref_outliers(xyz, 8, "statistical", std_mul=1.5)
    _, idx, st, mean = R.removeoutliers(xyz, k=8, std_mul=1.5, return_index=True, return_stats=True, return_mean_dist=True)
    print("n=%d mu %r sigma %r (twin %r %r)" % (n, st["mu"], st["sigma"], exp["mu"], exp["sigma"]))
    assert _same_bytes(mean, exp["mean_dist"])
    for f in ("mu", "sigma", "tau", "nn_median"):
        assert _same_bytes(st[f], exp[f]), (f, st[f], exp[f])
    assert st["n_valid"] == exp["n_valid"] == (n if n > 1 else 0)
    assert np.array_equal(idx, exp["kept_idx"])


def test_errors_and_capacity():
    one = np.array([[1.0, 2.0, 3.0]])
    idx, d2, count = R.knn(one, 4, return_count=True)                    # n = 1: no neighbour, return code 0
    assert count.tolist() == [0] and not idx.any() and np.isinf(d2).all()
    pts, kept, st, mean = R.removeoutliers(one, k=4, return_index=True, return_stats=True, return_mean_dist=True)
    assert len(pts) == 0 and len(kept) == 0 and st["n_valid"] == 0 and st["n_kept"] == 0 and np.isinf(mean).all()
    assert (st["mu"], st["sigma"], st["nn_median"]) == (0.0, 0.0, 0.0)
    # cap too small: RH_E_CAPACITY, the needed size, and keep still written in full
    xyz = DATA["outliers"]
    exp = ref_outliers(xyz, 8, nb=_nb("outliers"))
    keep, small, nk, st = np.zeros(len(xyz), dtype=np.uint8), np.zeros(10, dtype=np.int32), C.c_int64(), L.OutlierStats()
    prm = L.OutlierParams(k=8, mode=L.OUT_STATISTICAL, std_mul=2.0)
    rc = R.lib().rh_remove_outliers(xyz.ctypes.data_as(C.POINTER(C.c_double)), len(xyz), C.byref(prm), 0,
                                    keep.ctypes.data_as(C.POINTER(C.c_uint8)), small.ctypes.data_as(C.POINTER(C.c_int32)), 10,
                                    C.byref(nk), None, C.byref(st))
    assert rc == L.RH_E_CAPACITY and nk.value == exp["n_kept"] and st.n_kept == exp["n_kept"]
    assert np.array_equal(keep, exp["keep"]) and not small.any()
    # a coordinate that is not finite
    bad = xyz[:200].copy()
    bad[37, 1] = np.nan
    for call in (lambda: R.knn(bad, 4), lambda: R.removeoutliers(bad, k=4)):
        with pytest.raises(R.RansacHipError) as e:
            call()
        assert e.value.code == L.RH_E_INVALID
    # isolated points far from a dense cluster end, and end exact
    rng = np.random.default_rng(2)
    far = np.concatenate([rng.normal(size=(3000, 3)) * 0.1, [[1e3, 0, 0], [0, -2e3, 5e2], [1e3, 1.0, 0.5]]])
    got = R.knn(far, 8)
    e = ref_knn(far, 8)
    assert np.array_equal(got[0], e[0]) and _same_bytes(got[1], e[1])


@pytest.mark.parametrize("offset", [0.0, -3.0])
def test_bounding_box_minimum_reached_by_both_zeros(offset):
    """The box comes from the order-preserving integers of cell_grid.h, where -0.0 sorts below +0.0: the minimum of x is
    reached by both (with the offset, by two equal negative numbers), either first."""
    rng = np.random.default_rng(31)
    xyz = rng.uniform(0.0, 2.0, size=(200, 3))
    for zeros in ([0.0, -0.0], [-0.0, 0.0]):
        pts = xyz.copy()
        pts[[17, 150], 0] = zeros
        if offset != 0.0:
            pts[:, 0] += offset                                # (adding 0.0 would turn -0.0 into +0.0)
        else:
            assert (pts[[17, 150], 0] == 0.0).all() and np.signbit(pts[17, 0]) != np.signbit(pts[150, 0])
        idx, d2, count = R.knn(pts, 8, return_count=True)
        eidx, ed2, ecount = ref_knn(pts, 8)
        assert np.array_equal(count, ecount) and np.array_equal(idx, eidx) and _same_bytes(d2, ed2)


def test_a_nan_in_the_last_row_of_the_second_block_is_seen():
    bad = np.random.default_rng(32).uniform(0, 1, size=(257, 3))
    bad[256, 2] = np.nan
    for call in (lambda: R.knn(bad, 8), lambda: R.removeoutliers(bad, k=8), lambda: R.estimatenormals(bad, k=8)):
        with pytest.raises(R.RansacHipError) as e:
            call()
        assert e.value.code == L.RH_E_INVALID
