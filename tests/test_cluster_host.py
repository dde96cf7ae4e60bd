"""Density-based clustering (rh_cluster, include/ransac_hip.h), CPU side: the numpy twin of tests/cluster_reference.py pinned
by hand-derived cases with the expected labels written out, the ABI declarations, the argument checks that come before
the device is opened, and the index mapping of cluster_inpoints.  tests/test_cluster_gpu.py holds the library to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from cluster_reference import BORDER, CORE, NOISE, ref_cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(*xs):
    """points on the x axis"""
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float64)


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_three_collinear_points_at_exactly_eps():
    """0, 0.5 and 1: d2 = 0.25 = eps2, the boundary counts."""
    pts = line(0.0, 0.5, 1.0)
    r = ref_cluster(pts, 0.5, min_pts=2)                       # every point has a neighbour: three core points, one chain
    assert r["labels"].tolist() == [1, 1, 1] and r["kind"].tolist() == [CORE, CORE, CORE] and r["n_clusters"] == 1
    r = ref_cluster(pts, 0.5, min_pts=3)                       # only the middle one has two: the ends are its border
    assert r["labels"].tolist() == [1, 1, 1] and r["kind"].tolist() == [BORDER, CORE, BORDER]
    assert (r["n_core"], r["n_border"], r["n_noise"], r["n_small"], r["largest"]) == (1, 2, 0, 0, 3)
    assert r["counts"].tolist() == [0, 3] and r["offsets"].tolist() == [0, 0, 3] and r["idx"].tolist() == [1, 2, 3]
    r = ref_cluster(pts, 0.4999999999999999, min_pts=2)        # one ulp below: nobody has a neighbour
    assert r["labels"].tolist() == [0, 0, 0] and r["kind"].tolist() == [NOISE] * 3 and r["n_clusters"] == 0
    assert r["counts"].tolist() == [3] and r["offsets"].tolist() == [0, 3]


def test_a_border_point_between_two_clusters_goes_to_the_smaller_index():
    """b = +1 and a = -1 are core points (min_pts 4: two supporters at +-1.5 and x = 0 within eps = 1 of each); the
    supporters see b (or a) and each other only, x sees a and b only: 3 < 4, no core points.  x is at d2 = 1 from both."""
    pts = line(1.0, 1.5, 1.5, 0.0, -1.0, -1.5, -1.5)           # b s s x a s s
    r = ref_cluster(pts, 1.0, min_pts=4)
    assert r["kind"].tolist() == [CORE, BORDER, BORDER, BORDER, CORE, BORDER, BORDER]
    assert r["labels"].tolist() == [1, 1, 1, 1, 2, 2, 2]       # b has index 0 < 4: x is b's
    assert r["counts"].tolist() == [0, 4, 3] and r["lists"][1].tolist() == [1, 2, 3, 4] and r["lists"][2].tolist() == [5, 6, 7]
    pts = line(-1.0, 1.5, 1.5, 0.0, 1.0, -1.5, -1.5)           # a and b swapped: now a has the smaller index
    r = ref_cluster(pts, 1.0, min_pts=4)
    assert r["labels"].tolist() == [1, 2, 2, 1, 2, 1, 1]
    # a nearer core point wins whatever its index: a = -0.75 (index 0) is at d2 = 1 from x = 0.25, b = 1 at d2 = 0.5625
    r = ref_cluster(line(-0.75, -1.25, -1.25, 0.25, 1.0, 1.5, 1.5), 1.0, min_pts=4)
    assert r["kind"].tolist() == [CORE, BORDER, BORDER, BORDER, CORE, BORDER, BORDER]
    assert r["labels"].tolist() == [1, 1, 1, 2, 2, 2, 2]


def test_a_bridge_point_that_is_no_core_point_does_not_join_two_clusters():
    """Two chains of spacing 0.5, eps = 1, min_pts = 4; the bridge at 1 sees the chain ends 0 (d2 = 1, the boundary) and
    1.75 (d2 = 0.5625) only: no core point.  Both ends are core points, and the clusters stay two."""
    pts = line(0.0, -0.5, -1.0, -1.5, 1.0, 1.75, 2.25, 2.75, 3.25)
    r = ref_cluster(pts, 1.0, min_pts=4)
    assert r["kind"].tolist() == [CORE, CORE, CORE, BORDER, BORDER, CORE, CORE, CORE, BORDER]
    assert r["labels"].tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 2]  # the bridge goes to the nearer end
    assert r["n_clusters"] == 2 and r["counts"].tolist() == [0, 4, 5]
    # with min_pts = 3 the bridge is a core point (itself and two neighbours) and the chains are one cluster
    r = ref_cluster(pts, 1.0, min_pts=3)
    assert r["n_clusters"] == 1 and r["labels"].tolist() == [1] * 9


def test_duplicates_are_neighbours_at_distance_zero():
    pts = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [9, 9, 9]], dtype=np.float64)
    r = ref_cluster(pts, 0.1, min_pts=3)
    assert r["labels"].tolist() == [1, 1, 1, 0] and r["kind"].tolist() == [CORE, CORE, CORE, NOISE]
    r = ref_cluster(pts, 0.1, min_pts=4)
    assert r["labels"].tolist() == [0, 0, 0, 0]


def test_min_pts_one_is_euclidean_cluster_extraction():
    r = ref_cluster(line(0.0, 0.5, 5.0), 1.0, min_pts=1)
    assert r["labels"].tolist() == [1, 1, 2] and r["kind"].tolist() == [CORE] * 3
    assert r["counts"].tolist() == [0, 2, 1] and r["offsets"].tolist() == [0, 0, 2, 3]


def test_min_pts_above_every_neighbourhood():
    r = ref_cluster(line(0.0, 0.5, 1.0, 1.5), 10.0, min_pts=5)
    assert r["n_clusters"] == 0 and r["labels"].tolist() == [0] * 4 and r["kind"].tolist() == [NOISE] * 4
    assert r["counts"].tolist() == [4] and r["offsets"].tolist() == [0, 4] and r["idx"].tolist() == [1, 2, 3, 4]
    assert (r["n_core"], r["n_border"], r["n_noise"], r["n_small"], r["largest"]) == (0, 0, 4, 0, 0)


def test_one_point():
    r = ref_cluster(line(3.0), 1.0, min_pts=1)
    assert r["labels"].tolist() == [1] and r["kind"].tolist() == [CORE] and r["counts"].tolist() == [0, 1]
    r = ref_cluster(line(3.0), 1.0, min_pts=2)
    assert r["labels"].tolist() == [0] and r["kind"].tolist() == [NOISE] and r["n_clusters"] == 0


def test_min_size_drops_a_cluster_and_renumbers_the_rest():
    pts = line(0.0, 5.0, 5.5, 10.0, 10.5, 10.9)
    r = ref_cluster(pts, 0.6, min_pts=1)
    assert r["labels"].tolist() == [1, 2, 2, 3, 3, 3] and r["n_small"] == 0
    r = ref_cluster(pts, 0.6, min_pts=1, min_size=2)
    assert r["labels"].tolist() == [0, 1, 1, 2, 2, 2] and r["n_clusters"] == 2
    assert r["kind"].tolist() == [CORE] * 6                     # the kind is what it was before the drop
    assert (r["n_core"], r["n_noise"], r["n_small"], r["largest"]) == (6, 0, 1, 3) and r["counts"].tolist() == [1, 2, 3]
    r = ref_cluster(pts, 0.6, min_pts=1, min_size=3)
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1] and r["n_small"] == 3


def test_by_size_with_two_clusters_of_equal_size():
    pts = line(0.0, 0.5, 5.0, 10.0, 10.5, 20.0, 20.5, 21.0)     # sizes 2, 1, 2, 3
    assert ref_cluster(pts, 0.6, min_pts=1)["labels"].tolist() == [1, 1, 2, 3, 3, 4, 4, 4]
    r = ref_cluster(pts, 0.6, min_pts=1, order="size")
    assert r["labels"].tolist() == [2, 2, 4, 3, 3, 1, 1, 1]     # 3 first; the two of size 2 by their smallest index
    assert r["counts"].tolist() == [0, 3, 2, 2, 1] and r["lists"][1].tolist() == [6, 7, 8]


def test_component_count_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    csg = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.normal(c, 0.3, size=(150, 3)) for c in rng.uniform(1, 9, size=(4, 3))] + [rng.uniform(0, 10, size=(200, 3))])
    r = ref_cluster(pts, 0.3, min_pts=5, return_graph=True)
    core = np.flatnonzero(r["kind"] == CORE)
    assert 100 < len(core) < len(pts)
    ei, ej = r["edges"]
    g = sp.coo_matrix((np.ones(len(ei)), (ei, ej)), shape=(len(pts), len(pts))).tocsr()
    ncomp, lab = csg.connected_components(g[core][:, core], directed=False)
    assert ncomp == r["n_core_components"] == r["n_clusters"] > 1
    # the same partition of the core points, not only the same number
    pairs = set(zip(lab.tolist(), r["labels"][core].tolist()))
    assert len(pairs) == ncomp


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_cluster", "rh_cluster_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_cluster_params\s*;", src) and re.search(r"}\s*rh_cluster_stats\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 116
    assert R.lib().rh_version() >= 116
    assert re.search(r"RH_CLUSTER_BY_INDEX\s*=\s*0\s*,\s*RH_CLUSTER_BY_SIZE\s*=\s*1", src)
    assert re.search(r"RH_PT_NOISE\s*=\s*0\s*,\s*RH_PT_BORDER\s*=\s*1\s*,\s*RH_PT_CORE\s*=\s*2", src)
    assert (L.CLUSTER_BY_INDEX, L.CLUSTER_BY_SIZE) == (0, 1)
    assert (L.PT_NOISE, L.PT_BORDER, L.PT_CORE) == (NOISE, BORDER, CORE) == (0, 1, 2)


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["eps", "min_pts", "min_size", "order", "reserved"]
    sf = ["n_clusters", "n_core", "n_border", "n_noise", "n_small", "largest"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_cluster_params), sizeof(rh_cluster_stats));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_cluster_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_cluster_stats, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.ClusterParams), C.sizeof(L.ClusterStats)]
    mine += [getattr(L.ClusterParams, f).offset for f in pf] + [getattr(L.ClusterStats, f).offset for f in sf]
    assert got == mine and got[:2] == [24, 48]


def test_python_entries_are_exported():
    for name in ("cluster", "cluster_inpoints"):
        assert callable(getattr(R, name)) and name in R.__all__
    with pytest.raises(ValueError):
        R.cluster(np.zeros((8, 3)), 0.1, order="volume")
    with pytest.raises(ValueError):
        R.cluster_inpoints(np.zeros((8, 3)), [0, 1], 0.1)
    with pytest.raises(ValueError):
        R.cluster_inpoints(np.zeros((8, 3)), [9], 0.1)
    assert R.cluster_inpoints(np.zeros((8, 3)), [], 0.1) == []


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    xyz = np.zeros((8, 3))
    for dt in (np.float64, np.float32):
        x = xyz.astype(dt)
        for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=1.0, min_pts=0),
                   dict(eps=1.0, min_pts=-2), dict(eps=1.0, min_size=0), dict(eps=1.0, order=2), dict(eps=1.0, order=-1)):
            with pytest.raises(R.RansacHipError) as e:
                R.cluster(x, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        with pytest.raises(R.RansacHipError) as e:
            R.cluster(x[:0], 1.0)
        assert e.value.code == L.RH_E_INVALID
    lib = R.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    px = xyz.ctypes.data_as(dp)
    labels, m = np.full(8, -7, dtype=np.int32), C.c_int64(-7)
    pl = labels.ctypes.data_as(i32p)
    prm = L.ClusterParams(eps=1.0, min_pts=2, min_size=1, order=L.CLUSTER_BY_INDEX)
    fn = lib.rh_cluster
    assert fn(None, 8, C.byref(prm), 0, pl, None, 0, None, None, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, 8, None, 0, pl, None, 0, None, None, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, None, None, 0, None, None, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, pl, None, 0, None, None, None, None, None) == L.RH_E_INVALID
    assert fn(px, 8, C.byref(prm), 0, pl, None, -1, None, None, None, C.byref(m), None) == L.RH_E_INVALID
    for n in (0, -1, 2 ** 31, 2 ** 40):                        # (n is refused before anything is read through xyz)
        assert fn(px, n, C.byref(prm), 0, pl, None, 0, None, None, None, C.byref(m), None) == L.RH_E_INVALID, n
    assert m.value == -7 and (labels == -7).all()              # nothing was written
    assert b"rh_cluster" in lib.rh_last_error()


def test_a_valid_call_fails_loudly_without_gpu():
    n = C.c_int()
    if R.lib().rh_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    for dt in (np.float64, np.float32):
        with pytest.raises(R.RansacHipError) as e:
            R.cluster(np.zeros((8, 3), dtype=dt), 1.0)
        assert e.value.code == L.RH_E_NODEVICE


# ------------------------------------------------------------------------ cluster_inpoints ----
def test_cluster_inpoints_maps_back_to_the_callers_indices(monkeypatch):
    """The library call replaced by the twin: what is tested is the selection and the way back."""
    seen = {}

    def twin(vertices, eps, min_pts=8, min_size=1, order="index", device=0, return_lists=False):
        seen["vertices"] = np.array(vertices)
        r = ref_cluster(vertices, eps, min_pts, min_size, order)
        return r["labels"], r["offsets"], r["idx"]

    monkeypatch.setattr(R.api, "cluster", twin)
    #            1     2    3     4    5     6    7     8
    pts = line(10.0, 0.0, 10.5, 50.0, 0.5, 99.0, 0.9, 10.9)
    inpoints = np.array([8, 2, 5, 4, 7, 1, 3])                  # not 6; in no order
    parts = R.cluster_inpoints(pts, inpoints, 0.6, min_pts=1)
    assert np.array_equal(seen["vertices"], pts[inpoints - 1])
    # the selection is 10.9 0 0.5 50 0.9 10 10.5: clusters by first index {10.9, 10, 10.5}, {0, 0.5, 0.9}, {50}
    assert [p.tolist() for p in parts] == [[8, 1, 3], [2, 5, 7], [4]]
    assert all(p.dtype == np.int64 for p in parts)
    parts = R.cluster_inpoints(pts, inpoints, 0.6, min_pts=1, min_size=2, order="size")
    assert [p.tolist() for p in parts] == [[8, 1, 3], [2, 5, 7]]  # noise (the point at 50) is left out
    parts = R.cluster_inpoints(pts, inpoints, 0.6, min_pts=3)     # the core points: 0.5 (third of the selection), 10.5 (last)
    assert [p.tolist() for p in parts] == [[2, 5, 7], [8, 1, 3]]
    with pytest.raises(TypeError):
        R.cluster_inpoints(pts, inpoints, 0.6, return_kind=True)
