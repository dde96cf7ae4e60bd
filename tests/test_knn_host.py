"""Exact k nearest neighbours and outlier removal (rh_knn, rh_remove_outliers, include/ransac_hip.h), CPU side: the numpy
twin of the definition -- built on ref_neighbours of tests/test_normals_host.py, the order the search is defined by --
pinned by hand-derived cases, and the ABI declarations.  tests/test_knn_gpu.py holds the library to the twin, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from test_normals_host import ref_neighbours

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_knn(xyz, k, radius=0.0, nb=None):
    """rh_knn: (idx [n, k] int32 1-based, 0 past count; d2 [n, k], +inf past count; count [n] int32).
    nb: ref_neighbours(xyz, >= k + 1), to share one search between calls."""
    xyz = np.asarray(xyz, dtype=np.float64)
    idx, d2 = nb if nb is not None else ref_neighbours(xyz, k + 1)
    idx, d2 = idx[:, 1:k + 1], d2[:, 1:k + 1]          # column 0 is the point itself, left out by its index
    use = idx >= 0
    if radius > 0:
        use &= d2 <= radius * radius
    return (np.where(use, idx + 1, 0).astype(np.int32), np.where(use, d2, np.inf), use.sum(axis=1).astype(np.int32))


def ref_tree(a):
    """T(a): the root of the perfect binary tree over adjacent pairs, padded with +0.0 to the next power of two.  Works on
    the last axis."""
    b = np.asarray(a, dtype=np.float64)
    size = 1
    while size < b.shape[-1]:
        size *= 2
    b = np.concatenate([b, np.zeros(b.shape[:-1] + (size - b.shape[-1],))], axis=-1)
    while b.shape[-1] > 1:
        b = b[..., 0::2] + b[..., 1::2]
    return b[..., 0]


def ref_outliers(xyz, k, mode="statistical", std_mul=2.0, radius=0.0, threshold=0.0, nb=None):
    """rh_remove_outliers, step by step.  Returns a dict: keep (uint8), kept_idx (int32, 1-based), mean_dist, n_valid,
    n_kept, mu, sigma, tau, nn_median."""
    _, d2, count = ref_knn(xyz, k, radius, nb)
    n = len(count)
    dist = np.zeros((n, 64))
    dist[:, :k] = np.where(np.isfinite(d2), np.sqrt(np.where(np.isfinite(d2), d2, 0.0)), 0.0)
    valid = count >= 1
    nv = int(valid.sum())
    m = np.full(n, np.inf)
    m[valid] = ref_tree(dist)[valid] / count[valid]
    mv = np.where(valid, m, 0.0)
    mu = float(ref_tree(mv) / nv) if nv else 0.0
    dev = np.where(valid, mv - mu, 0.0)
    sigma = float(np.sqrt(ref_tree(dev * dev) / (nv - 1))) if nv >= 2 else 0.0
    if mode == "statistical":
        w = std_mul * sigma
        tau = mu + w
        keep = valid & (m <= tau)
    elif mode == "absolute":
        tau = float(threshold)
        keep = valid & (m <= tau)
    else:
        tau = float(radius)
        keep = count == k
    nn = np.sort(dist[valid, 0])
    med = float(nn[(nv - 1) // 2]) if nv else 0.0
    return dict(keep=keep.astype(np.uint8), kept_idx=(np.flatnonzero(keep) + 1).astype(np.int32), mean_dist=m, n_valid=nv,
                n_kept=int(keep.sum()), mu=mu, sigma=sigma, tau=float(tau), nn_median=med)


def outlier_cloud():
    """A 3000-point plane patch (uniform in [0, 20]^2, z ~ N(0, 0.02)) and 60 points uniform in [0, 20]^2 x [-10, 10],
    shuffled."""
    rng = np.random.default_rng(5)
    plane = np.concatenate([rng.uniform(0, 20, size=(3000, 2)), rng.normal(0, 0.02, size=(3000, 1))], axis=1)
    stray = rng.uniform([0, 0, -10], [20, 20, 10], size=(60, 3))
    pts = np.concatenate([plane, stray])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_tree_is_adjacent_pairs_with_zero_padding():
    assert ref_tree([1.0, 2.0, 3.0]) == (1.0 + 2.0) + (3.0 + 0.0)
    assert ref_tree([5.0]) == 5.0
    e = 2.0 ** -53
    # (1 + e) + (e + e) = 1 + 2^-52, while left to right ((1 + e) + e) + e stays 1: the order is part of the definition
    a = np.array([1.0, e, e, e])
    assert ref_tree(a) == 1.0 + 2.0 ** -52
    left_to_right = 0.0
    for x in a:
        left_to_right += x
    assert left_to_right == 1.0 and left_to_right != ref_tree(a)
    assert np.array_equal(ref_tree(np.array([[1.0, 2.0, 3.0, 4.0, 5.0], [1.0, 0.0, 0.0, 0.0, 0.0]])), [15.0, 1.0])


def test_collinear_points_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [10, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn(pts, 1)
    assert idx[:, 0].tolist() == [2, 1, 2, 3]                 # point 1 is equally far from 0 and 2: the smaller index
    assert d2[:, 0].tolist() == [1.0, 1.0, 1.0, 64.0] and count.tolist() == [1, 1, 1, 1]
    r = ref_outliers(pts, 1, "statistical", std_mul=1.0)
    assert r["mean_dist"].tolist() == [1.0, 1.0, 1.0, 8.0]
    # mu = ((1 + 1) + (1 + 8)) / 4 = 2.75; deviations -1.75 (x 3) and 5.25; squares 3.0625 (x 3) and 27.5625, sum 36.75;
    # sigma = sqrt(36.75 / 3) = sqrt(12.25) = 3.5; tau = 2.75 + 1 * 3.5 = 6.25: the point at 10 (m = 8) goes
    assert (r["mu"], r["sigma"], r["tau"], r["n_valid"]) == (2.75, 3.5, 6.25, 4)
    assert r["keep"].tolist() == [1, 1, 1, 0] and r["kept_idx"].tolist() == [1, 2, 3] and r["n_kept"] == 3
    assert r["nn_median"] == 1.0                              # sorted 1, 1, 1, 8: position (4 - 1) // 2 = 1
    r2 = ref_outliers(pts, 1, "statistical", std_mul=2.0)     # tau = 2.75 + 7 = 9.75: everything stays
    assert r2["tau"] == 9.75 and r2["keep"].tolist() == [1, 1, 1, 1]
    ra = ref_outliers(pts, 1, "absolute", threshold=1.0)      # m <= tau, not <
    assert ra["tau"] == 1.0 and ra["keep"].tolist() == [1, 1, 1, 0] and (ra["mu"], ra["sigma"]) == (2.75, 3.5)
    rr = ref_outliers(pts, 2, "radius", radius=2.0)           # two others within 2: the points at 0, 1 and 2
    assert rr["keep"].tolist() == [1, 1, 1, 0] and rr["tau"] == 2.0
    assert rr["mean_dist"].tolist() == [1.5, 1.0, 1.5, np.inf] and rr["n_valid"] == 3


def test_a_duplicate_is_a_neighbour():
    pts = np.array([[0, 0, 0], [0, 0, 0], [3, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn(pts, 2)
    assert idx.tolist() == [[2, 3], [1, 3], [1, 2]]           # the copy at d^2 = 0 first; ties to the smaller index
    assert d2.tolist() == [[0.0, 9.0], [0.0, 9.0], [9.0, 9.0]] and count.tolist() == [2, 2, 2]
    r = ref_outliers(pts, 1, "statistical", std_mul=1.0)
    assert r["mean_dist"].tolist() == [0.0, 0.0, 3.0] and r["mu"] == 1.0 and r["nn_median"] == 0.0
    assert r["sigma"] == np.sqrt(3.0) and r["keep"].tolist() == [1, 1, 0]      # ((1 + 1) + (4 + 0)) / 2 = 3; 3 > 1 + sqrt(3)


def test_a_point_without_neighbours_is_dropped():
    pts = np.array([[0, 0, 0], [1, 0, 0], [10, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn(pts, 2, radius=2.0)
    assert count.tolist() == [1, 1, 0] and idx.tolist() == [[2, 0], [1, 0], [0, 0]]
    assert d2[2].tolist() == [np.inf, np.inf] and d2[0].tolist() == [1.0, np.inf]
    for std_mul in (1.0, 100.0):
        r = ref_outliers(pts, 2, "statistical", std_mul=std_mul, radius=2.0)
        assert r["mean_dist"].tolist() == [1.0, 1.0, np.inf] and r["n_valid"] == 2
        assert (r["mu"], r["sigma"], r["tau"]) == (1.0, 0.0, 1.0) and r["keep"].tolist() == [1, 1, 0]
    lone = ref_outliers(pts[:1], 4)                            # one point: nothing valid, nothing kept
    assert (lone["n_valid"], lone["n_kept"], lone["mu"], lone["sigma"], lone["nn_median"]) == (0, 0, 0.0, 0.0, 0.0)
    assert lone["mean_dist"].tolist() == [np.inf]


def test_the_summation_order_shows_in_the_last_bit():
    """On the outlier cloud of the GPU tests, mu by the tree and by numpy's own summation differ in the last bits for some
    k: a device that summed in another order would keep the same points and still miss the bytes of mu."""
    pts = outlier_cloud()
    nb = ref_neighbours(pts, 64)
    differ = {}
    for k in (1, 8, 16, 63):
        for std_mul in (1.0, 2.0):
            r = ref_outliers(pts, k, std_mul=std_mul, nb=nb)
            assert r["n_valid"] == len(pts) and 46 <= len(pts) - r["n_kept"] <= 56
            # ... while the kept set is far from depending on it: no m_i within 0.28 % of tau
            assert np.abs(r["mean_dist"] - r["tau"]).min() >= 0.0028 * r["tau"]
        differ[k] = float(np.sum(r["mean_dist"]) / len(pts)) - r["mu"]
    assert differ[1] == 0.0 and differ[16] == 0.0
    assert abs(differ[8]) == 2.0 ** -54 and abs(differ[63]) == 2.0 ** -52      # 5.6e-17 and 2.2e-16: one ulp of mu each


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_knn", "rh_knn_f32", "rh_remove_outliers", "rh_remove_outliers_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_outlier_params\s*;", src) and re.search(r"}\s*rh_outlier_stats\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 115
    assert R.lib().rh_version() >= 115
    assert int(re.search(r"#define\s+RH_KNN_MAX_K\s+(\d+)", src).group(1)) == L.KNN_MAX_K == 63
    assert int(re.search(r"#define\s+RH_OUT_BLOCK_POINTS\s+(\d+)", src).group(1)) == L.OUT_BLOCK_POINTS
    assert re.search(r"RH_OUT_STATISTICAL\s*=\s*0\s*,\s*RH_OUT_ABSOLUTE\s*=\s*1\s*,\s*RH_OUT_RADIUS\s*=\s*2", src)


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["k", "mode", "std_mul", "radius", "threshold"]
    sf = ["n_valid", "n_kept", "mu", "sigma", "tau", "nn_median"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_outlier_params), sizeof(rh_outlier_stats));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_outlier_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_outlier_stats, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.OutlierParams), C.sizeof(L.OutlierStats)]
    mine += [getattr(L.OutlierParams, f).offset for f in pf] + [getattr(L.OutlierStats, f).offset for f in sf]
    assert got == mine


def test_python_entries_are_exported():
    for name in ("knn", "removeoutliers"):
        assert callable(getattr(R, name)) and name in R.__all__
    with pytest.raises(ValueError):
        R.removeoutliers(np.zeros((8, 3)), mode="median")
    with pytest.raises(ValueError):
        R.removeoutliers(np.zeros((8, 3)), mode="absolute")
    with pytest.raises(ValueError):
        R.removeoutliers(np.zeros((8, 3)), normals=np.zeros((7, 3)))


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    xyz = np.zeros((8, 3))
    for dt in (np.float64, np.float32):
        x = xyz.astype(dt)
        for kw in (dict(k=0), dict(k=64), dict(k=-3), dict(k=4, radius=-1.0), dict(k=4, radius=float("inf")),
                   dict(k=4, radius=float("nan"))):
            with pytest.raises(R.RansacHipError) as e:
                R.knn(x, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        for kw in (dict(k=0), dict(k=64), dict(radius=-1.0), dict(radius=float("nan")), dict(mode=3), dict(mode=-1),
                   dict(mode="radius"), dict(mode="radius", radius=0.0), dict(std_mul=float("inf")), dict(std_mul=float("nan")),
                   dict(mode="absolute", threshold=float("nan"))):
            with pytest.raises(R.RansacHipError) as e:
                R.removeoutliers(x, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        with pytest.raises(R.RansacHipError) as e:
            R.knn(x[:0], 4)
        assert e.value.code == L.RH_E_INVALID
        with pytest.raises(R.RansacHipError) as e:
            R.removeoutliers(x[:0])
        assert e.value.code == L.RH_E_INVALID
    lib = R.lib()
    dp, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    px = xyz.ctypes.data_as(dp)
    cnt = np.zeros(8, dtype=np.int32)
    assert lib.rh_knn(None, 8, 4, 0.0, 0, None, None, cnt.ctypes.data_as(i32p)) == L.RH_E_INVALID
    for n in (0, -1, 2 ** 31 - 1, 2 ** 40):                    # (n is refused before anything is read through xyz)
        assert lib.rh_knn(px, n, 4, 0.0, 0, None, None, None) == L.RH_E_INVALID, n
    keep, idx, nk = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int32), C.c_int64(-7)
    prm = L.OutlierParams(k=4, mode=L.OUT_STATISTICAL, std_mul=2.0)
    pk, pi = keep.ctypes.data_as(u8p), idx.ctypes.data_as(i32p)
    fn = lib.rh_remove_outliers
    assert fn(None, 8, C.byref(prm), 0, pk, pi, 8, C.byref(nk), None, None) == L.RH_E_INVALID
    assert fn(px, 8, None, 0, pk, pi, 8, C.byref(nk), None, None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, None, pi, 8, C.byref(nk), None, None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, pk, pi, 8, None, None, None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, pk, pi, -1, C.byref(nk), None, None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, pk, None, 8, C.byref(nk), None, None) == L.RH_E_INVALID    # cap without a list
    for n in (0, 2 ** 31 - 1):
        assert fn(px, n, C.byref(prm), 0, pk, pi, 8, C.byref(nk), None, None) == L.RH_E_INVALID
    assert nk.value == -7 and not keep.any()                   # nothing was written
    assert b"rh_remove_outliers" in lib.rh_last_error()
