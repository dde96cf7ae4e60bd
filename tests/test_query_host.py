"""Nearest neighbours of query points in another cloud and cloud distances (rh_knn_query, rh_cloud_distance,
include/ransac_hip.h), CPU side: the numpy twin of tests/query_reference.py pinned by hand-derived cases, and the ABI
declarations.  tests/test_query_gpu.py holds the library to the twin, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from query_reference import ref_cloud_distance, ref_knn_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_collinear_reference_queries_between_and_beyond_its_ends():
    ref = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [10, 0, 0]], dtype=np.float64)
    qry = np.array([[-3, 0, 0], [0.25, 0, 0], [1.75, 0, 0], [7, 0, 0], [14, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn_query(ref, qry, 2)
    assert idx.tolist() == [[1, 2], [1, 2], [3, 2], [4, 3], [4, 3]]
    assert d2.tolist() == [[9.0, 16.0], [0.0625, 0.5625], [0.0625, 0.5625], [9.0, 25.0], [16.0, 144.0]]
    assert count.tolist() == [2, 2, 2, 2, 2] and idx.dtype == np.int32 and count.dtype == np.int32


def test_a_query_equal_to_a_reference_point_is_its_own_first_neighbour():
    ref = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [5, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn_query(ref, ref[[1, 3]], 3)
    assert idx.tolist() == [[2, 3, 1], [4, 2, 3]]             # nothing is left out; the two copies in index order
    assert d2.tolist() == [[0.0, 0.0, 1.0], [0.0, 16.0, 16.0]] and count.tolist() == [3, 3]


def test_equidistant_reference_points_the_smaller_index():
    ref = np.array([[2, 0, 0], [0, 0, 0], [1, 1, 0], [1, -1, 0]], dtype=np.float64)
    idx, d2, _ = ref_knn_query(ref, np.array([[1.0, 0.0, 0.0]]), 4)
    assert idx.tolist() == [[1, 2, 3, 4]] and d2.tolist() == [[1.0, 1.0, 1.0, 1.0]]
    idx, _, _ = ref_knn_query(ref[::-1], np.array([[1.0, 0.0, 0.0]]), 1)
    assert idx.tolist() == [[1]]


def test_the_radius_boundary_is_included_and_short_lists_are_padded():
    ref = np.array([[0, 0, 0], [3, 0, 0], [4, 0, 0]], dtype=np.float64)
    qry = np.array([[0, 0, 0], [0, 4, 0], [100, 0, 0]], dtype=np.float64)
    idx, d2, count = ref_knn_query(ref, qry, 2, radius=5.0)
    # query 1: d^2 = 16, 25, 32 -- 25 = radius^2 stays, 32 goes
    assert idx.tolist() == [[1, 2], [1, 2], [0, 0]] and count.tolist() == [2, 2, 0]
    assert d2.tolist() == [[0.0, 9.0], [16.0, 25.0], [INF, INF]]
    idx, d2, count = ref_knn_query(ref, qry, 3, radius=5.0)
    assert idx.tolist() == [[1, 2, 3], [1, 2, 0], [0, 0, 0]] and count.tolist() == [3, 2, 0]
    # n < k: count = n, 0 / +inf behind
    idx, d2, count = ref_knn_query(ref, qry[:2], 5)
    assert idx.tolist() == [[1, 2, 3, 0, 0], [1, 2, 3, 0, 0]] and count.tolist() == [3, 3]
    assert d2.tolist() == [[0.0, 9.0, 16.0, INF, INF], [16.0, 25.0, 32.0, INF, INF]]


def test_point_and_plane_metric_by_hand():
    ref = np.array([[0, 0, 0], [10, 0, 0]], dtype=np.float64)
    nrm = np.array([[0, 0, 2], [3, 0, 4]], dtype=np.float64)               # not normalised: used as given
    qry = np.array([[1, 2, 2], [9, 0, -1], [4, 3, 0], [0, 0, 0]], dtype=np.float64)
    r = ref_cloud_distance(ref, qry)
    assert r["dist"].tolist() == [3.0, np.sqrt(2.0), 5.0, 0.0] and r["nn_idx"].tolist() == [1, 2, 1, 1]
    # mean = ((3 + sqrt2) + (5 + 0)) / 4; rms = sqrt(((9 + 2.0000000000000004) + (25 + 0)) / 4)
    s2 = np.sqrt(2.0)
    assert r["mean"] == ((3.0 + s2) + (5.0 + 0.0)) / 4 and r["rms"] == np.sqrt(((9.0 + s2 * s2) + (25.0 + 0.0)) / 4)
    assert (r["n_valid"], r["max"], r["argmax"], r["n_within"]) == (4, 5.0, 3, 4)
    assert r["median"] == s2                                               # sorted 0, sqrt2, 3, 5: position (4 - 1) // 2 = 1
    p = ref_cloud_distance(ref, qry, normals=nrm)                          # plane is the default with normals
    # e = q - r: (1, 2, 2).(0, 0, 2) = 4; (-1, 0, -1).(3, 0, 4) = -7; (4, 3, 0).(0, 0, 2) = 0; 0
    assert p["dist"].tolist() == [4.0, 7.0, 0.0, 0.0] and p["nn_idx"].tolist() == [1, 2, 1, 1]
    assert (p["mean"], p["rms"], p["max"], p["argmax"], p["median"]) == (2.75, np.sqrt(65.0 / 4), 7.0, 2, 0.0)
    assert ref_cloud_distance(ref, qry, normals=nrm, metric="point")["dist"].tolist() == r["dist"].tolist()
    w = ref_cloud_distance(ref, qry, threshold=3.0)                        # d <= threshold, not <
    assert w["n_within"] == 3


def test_no_valid_query_gives_zero_stats():
    ref = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float64)
    r = ref_cloud_distance(ref, np.array([[50.0, 0, 0], [0, 60.0, 0]]), radius=2.0)
    assert r["dist"].tolist() == [INF, INF] and r["nn_idx"].tolist() == [0, 0]
    assert [r[f] for f in ("n_valid", "n_within", "argmax", "mean", "rms", "max", "median")] == [0, 0, 0, 0.0, 0.0, 0.0, 0.0]
    # some valid: the others count nowhere
    r = ref_cloud_distance(ref, np.array([[50.0, 0, 0], [0, 1.0, 0], [1, 0, 1.5]]), radius=2.0)
    assert r["dist"].tolist() == [INF, 1.0, 1.5] and (r["n_valid"], r["n_within"], r["argmax"]) == (2, 2, 3)
    assert (r["mean"], r["rms"], r["max"], r["median"]) == (1.25, np.sqrt(3.25 / 2), 1.5, 1.0)


def test_argmax_is_the_smallest_index_and_the_median_the_lower_one():
    ref = np.zeros((1, 3))
    qry = np.array([[1, 0, 0], [0, 4, 0], [0, 0, 2], [0, 0, -4], [3, 0, 0], [4, 0, 0]], dtype=np.float64)
    r = ref_cloud_distance(ref, qry)
    assert r["max"] == 4.0 and r["argmax"] == 2                            # 4 is reached by queries 2, 4 and 6
    assert r["median"] == 3.0                                              # sorted 1 2 3 4 4 4: position (6 - 1) // 2 = 2
    assert ref_cloud_distance(ref, qry[:4])["median"] == 2.0               # sorted 1 2 4 4: position 1, the lower one


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_knn_query", "rh_knn_query_f32", "rh_cloud_distance", "rh_cloud_distance_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_distance_params\s*;", src) and re.search(r"}\s*rh_distance_stats\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 117
    assert R.lib().rh_version() >= 117
    assert re.search(r"RH_DIST_POINT\s*=\s*0\s*,\s*RH_DIST_PLANE\s*=\s*1", src)
    assert (L.DIST_POINT, L.DIST_PLANE) == (0, 1)


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["radius", "threshold", "metric", "reserved"]
    sf = ["n_valid", "n_within", "argmax", "mean", "rms", "max", "median"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_distance_params), sizeof(rh_distance_stats));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_distance_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_distance_stats, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.DistanceParams), C.sizeof(L.DistanceStats)]
    mine += [getattr(L.DistanceParams, f).offset for f in pf] + [getattr(L.DistanceStats, f).offset for f in sf]
    assert got == mine
    assert [f for f, _ in L.DistanceParams._fields_] == pf and [f for f, _ in L.DistanceStats._fields_] == sf


def test_python_entries_are_exported():
    for name in ("knn_query", "cloud_distance", "transfer_labels"):
        assert callable(getattr(R, name)) and name in R.__all__
    with pytest.raises(ValueError):
        R.cloud_distance(np.zeros((8, 3)), np.zeros((4, 3)), metric="chamfer")
    with pytest.raises(ValueError):
        R.cloud_distance(np.zeros((8, 3)), np.zeros((4, 3)), normals=np.zeros((7, 3)))
    with pytest.raises(ValueError):
        R.transfer_labels(np.zeros((8, 3)), np.zeros(7, dtype=np.int32), np.zeros((4, 3)))


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    ref, qry = np.zeros((8, 3)), np.ones((5, 3))
    for dt in (np.float64, np.float32):
        r, q = ref.astype(dt), qry.astype(dt)
        for kw in (dict(k=0), dict(k=64), dict(k=-3), dict(k=4, radius=-1.0), dict(k=4, radius=float("inf")),
                   dict(k=4, radius=float("nan"))):
            with pytest.raises(R.RansacHipError) as e:
                R.knn_query(r, q, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        for a, b in ((r[:0], q), (r, q[:0])):
            with pytest.raises(R.RansacHipError) as e:
                R.knn_query(a, b, 4)
            assert e.value.code == L.RH_E_INVALID
            with pytest.raises(R.RansacHipError) as e:
                R.cloud_distance(a, b)
            assert e.value.code == L.RH_E_INVALID
        for kw in (dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(threshold=float("nan")),
                   dict(metric=2), dict(metric=-1), dict(metric="plane")):                 # (the plane metric without normals)
            with pytest.raises(R.RansacHipError) as e:
                R.cloud_distance(r, q, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
    lib = R.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pr, pq = ref.ctypes.data_as(dp), qry.ctypes.data_as(dp)
    cnt = np.full(5, -7, dtype=np.int32)
    pc = cnt.ctypes.data_as(i32p)
    assert lib.rh_knn_query(None, 8, pq, 5, 4, 0.0, 0, None, None, pc) == L.RH_E_INVALID
    assert lib.rh_knn_query(pr, 8, None, 5, 4, 0.0, 0, None, None, pc) == L.RH_E_INVALID
    for n in (0, -1, 2 ** 31 - 1, 2 ** 40):                    # (n and m are refused before anything is read through the arrays)
        assert lib.rh_knn_query(pr, n, pq, 5, 4, 0.0, 0, None, None, pc) == L.RH_E_INVALID, n
    for m in (0, -1, 2 ** 31, 2 ** 40):
        assert lib.rh_knn_query(pr, 8, pq, m, 4, 0.0, 0, None, None, pc) == L.RH_E_INVALID, m
    assert b"rh_knn_query" in lib.rh_last_error()
    dist, nn, st = np.full(5, -7.0), np.full(5, -7, dtype=np.int32), L.DistanceStats(n_valid=-7)
    pd, pn = dist.ctypes.data_as(dp), nn.ctypes.data_as(i32p)
    prm = L.DistanceParams(radius=0.0, threshold=1.0, metric=L.DIST_POINT)
    fn = lib.rh_cloud_distance
    assert fn(None, None, 8, pq, 5, C.byref(prm), 0, pd, pn, C.byref(st)) == L.RH_E_INVALID
    assert fn(pr, None, 8, None, 5, C.byref(prm), 0, pd, pn, C.byref(st)) == L.RH_E_INVALID
    assert fn(pr, None, 8, pq, 5, None, 0, pd, pn, C.byref(st)) == L.RH_E_INVALID
    assert fn(pr, None, 8, pq, 5, C.byref(prm), 0, None, pn, C.byref(st)) == L.RH_E_INVALID
    for n, m in ((0, 5), (2 ** 31 - 1, 5), (8, 0), (8, 2 ** 31)):
        assert fn(pr, None, n, pq, m, C.byref(prm), 0, pd, pn, C.byref(st)) == L.RH_E_INVALID, (n, m)
    plane = L.DistanceParams(radius=0.0, threshold=1.0, metric=L.DIST_PLANE)
    assert fn(pr, None, 8, pq, 5, C.byref(plane), 0, pd, pn, C.byref(st)) == L.RH_E_INVALID
    assert b"rh_cloud_distance" in lib.rh_last_error()
    assert (cnt == -7).all() and (dist == -7.0).all() and (nn == -7).all() and st.n_valid == -7      # nothing was written
