"""Region growing by smoothness (rh_segment_smooth, include/ransac_hip.h), CPU side: the numpy twin of
tests/segment_reference.py pinned by hand-derived cases with the expected labels written out, its components computed a
second way, the conditions the scenes of tests/segment_scenes.py are meant to meet, the ABI declarations, the argument
checks that come before the device is opened, and the index mapping of segment_inpoints.  tests/test_segment_gpu.py holds
the library to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from segment_reference import BORDER, CORE, NOISE, UNSIGNED, components_propagate, knn_lists, ref_segment
from segment_scenes import STEP_EXTRA, scene, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = [0.0, 0.0, 1.0]


def line(*xs):
    """points on the x axis"""
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float64)


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_a_line_with_one_point_that_is_no_seed_in_the_middle():
    """0 .. 6 on a line, equal normals, k = 2: every point lists its two nearest.  Point 3 is no seed (its curvature is
    above curv_max); its seeds 2 and 4 are both at d2 = 1, so it goes with 2 -- and does not join the two halves."""
    curv = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    r = ref_segment(line(0, 1, 2, 3, 4, 5, 6), np.tile(UP, (7, 1)), curv, k=2, cos_angle=0.9, curv_max=0.5)
    assert r["labels"].tolist() == [1, 1, 1, 1, 2, 2, 2]       # BY_SIZE: the half that got the border point is larger
    assert r["kind"].tolist() == [CORE] * 3 + [BORDER] + [CORE] * 3
    assert (r["n_regions"], r["n_seed"], r["n_border"], r["n_unassigned"], r["n_invalid"], r["n_small"], r["largest"]) == (2, 6, 1, 0, 0, 0, 4)
    assert r["counts"].tolist() == [0, 4, 3] and r["offsets"].tolist() == [0, 0, 4, 7] and r["idx"].tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert r["contested"] == 1 and r["border_tie"] == 1 and r["reverse_only"] == 0
    # without curvature every point is a seed and the line is one region
    assert ref_segment(line(0, 1, 2, 3, 4, 5, 6), np.tile(UP, (7, 1)), None, k=2, cos_angle=0.9)["labels"].tolist() == [1] * 7


def test_a_dot_product_of_exactly_cos_angle_passes():
    """(1, 0, 0) . (0.6, 0.8, 0) = (1 * 0.6 + 0 * 0.8) + 0 * 0 = 0.6 with no rounding anywhere"""
    nrm = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]])
    assert ref_segment(line(0, 1), nrm, None, k=1, cos_angle=0.6)["labels"].tolist() == [1, 1]
    assert ref_segment(line(0, 1), nrm, None, k=1, cos_angle=np.nextafter(0.6, 1.0))["labels"].tolist() == [1, 2]
    # the sign: -0.6 fails, |-0.6| passes with the flag
    nrm[1] = -nrm[1]
    assert ref_segment(line(0, 1), nrm, None, k=1, cos_angle=0.6)["n_regions"] == 2
    assert ref_segment(line(0, 1), nrm, None, k=1, cos_angle=0.6, flags=UNSIGNED)["n_regions"] == 1


def test_a_border_tie_on_d2_goes_to_the_smaller_index():
    """Seeds at -1 and +1 with normals 0.8 apart (no smooth pair at cos_angle 0.85), between them a point that is no seed
    with a normal at 0.9 from both: d2 = 1 either way."""
    n_a, n_b, n_x = [0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.0, 0.3, 0.9]
    kw = dict(k=2, cos_angle=0.85, curv_max=0.5, order="index")
    r = ref_segment(line(1, 0, -1), np.array([n_a, n_x, n_b]), np.array([0.0, 1.0, 0.0]), **kw)
    assert r["labels"].tolist() == [1, 1, 2] and r["kind"].tolist() == [CORE, BORDER, CORE] and r["border_tie"] == 1
    r = ref_segment(line(-1, 1, 0), np.array([n_b, n_a, n_x]), np.array([0.0, 0.0, 1.0]), **kw)
    assert r["labels"].tolist() == [1, 2, 1]                   # the same cloud in another order: now b has the smaller index
    # no tie: the nearer seed wins whatever its index
    r = ref_segment(line(-1, 1, 0.25), np.array([n_b, n_a, n_x]), np.array([0.0, 0.0, 1.0]), **kw)
    assert r["labels"].tolist() == [1, 2, 2] and r["border_tie"] == 0


def test_a_point_outside_v_between_two_seeds_joins_nothing():
    """k = 1: the ends list the middle point, whose normal is (0, 0, 0); nothing is bridged across it"""
    nrm = np.array([UP, [0.0, 0.0, 0.0], UP])
    r = ref_segment(line(0, 1, 2), nrm, None, k=1, cos_angle=0.9, order="index")
    assert r["labels"].tolist() == [1, 0, 2] and r["kind"].tolist() == [CORE, NOISE, CORE]
    assert (r["n_invalid"], r["n_unassigned"], r["n_seed"]) == (1, 0, 2) and r["counts"].tolist() == [1, 1, 1]
    # a point of V that is no seed and has no smooth seed: unassigned
    nrm[1] = [1.0, 0.0, 0.0]
    r = ref_segment(line(0, 1, 2), nrm, np.array([0.0, np.nan, 0.0]), k=1, cos_angle=0.9, order="index")
    assert r["labels"].tolist() == [1, 0, 2] and (r["n_invalid"], r["n_unassigned"]) == (0, 1)


def test_a_seed_that_lists_a_point_counts_for_that_point():
    """k = 1: 0 and 1 list each other, 3 lists 1; 3 is no seed and nobody lists it, yet 1 is its seed (i ~ j either way)"""
    r = ref_segment(line(0, 1, 3), np.tile(UP, (3, 1)), np.array([0.0, 0.0, 1.0]), k=1, cos_angle=0.9, curv_max=0.5)
    assert r["labels"].tolist() == [1, 1, 1] and r["kind"].tolist() == [CORE, CORE, BORDER] and r["reverse_only"] == 0
    r = ref_segment(line(0, 1, 3), np.tile(UP, (3, 1)), np.array([0.0, 1.0, 0.0]), k=1, cos_angle=0.9, curv_max=0.5)
    assert r["kind"].tolist() == [CORE, BORDER, CORE] and r["labels"].tolist() == [1, 1, 2]
    assert r["reverse_only"] == 0                              # 1 lists 0 itself; 3 lists 1 but is farther
    r = ref_segment(line(0, 1, 3), np.tile(UP, (3, 1)), np.array([1.0, 1.0, 0.0]), k=1, cos_angle=0.9, curv_max=0.5)
    assert r["kind"].tolist() == [NOISE, BORDER, CORE] and r["reverse_only"] == 1   # 1 lists only 0; its seed 3 lists it


def test_the_distance_test_at_exactly_dist_max():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25]])
    nrm = np.tile(UP, (2, 1))
    assert ref_segment(pts, nrm, None, k=1, cos_angle=0.9, dist_max=0.25)["n_regions"] == 1
    assert ref_segment(pts, nrm, None, k=1, cos_angle=0.9, dist_max=np.nextafter(0.25, 0.0))["n_regions"] == 2
    assert ref_segment(pts, nrm, None, k=1, cos_angle=0.9, dist_max=0.0)["n_regions"] == 1       # 0: no distance test


def test_min_size_and_the_two_numberings():
    pts = line(0.0, 0.5, 5.0, 10.0, 10.5, 20.0, 20.5, 21.0)     # sizes 2, 1, 2, 3 with a radius of 0.6
    kw = dict(k=3, radius=0.6, cos_angle=0.9)
    nrm = np.tile(UP, (8, 1))
    assert ref_segment(pts, nrm, None, order="index", **kw)["labels"].tolist() == [1, 1, 2, 3, 3, 4, 4, 4]
    assert ref_segment(pts, nrm, None, order="size", **kw)["labels"].tolist() == [2, 2, 4, 3, 3, 1, 1, 1]
    r = ref_segment(pts, nrm, None, order="size", min_size=2, **kw)
    assert r["labels"].tolist() == [2, 2, 0, 3, 3, 1, 1, 1] and r["n_small"] == 1 and r["kind"].tolist() == [CORE] * 8


# ------------------------------------------------------ the components, a second way ----
@pytest.mark.parametrize("name", ["fold", "corner", "lattice4", "flipped_signed", "sparse"])
def test_union_find_against_label_propagation(name):
    p, n, c, kw = scene(name)
    r = ref_segment(p, n, c, return_graph=True, **kw)
    ei, ej = r["edges"]
    assert np.array_equal(r["comp"], components_propagate(len(p), r["seed"], ei, ej))
    assert len(np.unique(r["comp"][r["comp"] >= 0])) >= r["n_regions"] >= 1


# ------------------------------------------------------ the scenes are what they are meant to be ----
def test_scene_conditions():
    t = twin("corner")
    assert t["n_regions"] == 3 and t["n_border"] > 50 and not t["knn_tie"] and t["border_tie"] == 0
    t = twin("fold")
    assert t["n_regions"] == 2 and t["contested"] >= 3 and t["reverse_only"] >= 1 and t["n_unassigned"] >= 1
    off, on = twin("steps_off"), twin("steps_on")
    sheet = slice(0, len(scene("steps_on")[0]) - STEP_EXTRA)
    assert len(np.unique(off["labels"][sheet])) == 1 and len(np.unique(on["labels"][sheet])) == 2
    assert on["labels"][-4] == on["labels"][-3] and on["labels"][-2] != on["labels"][-1]
    assert twin("flipped_unsigned")["n_regions"] == 1 and twin("flipped_signed")["n_regions"] >= 2
    assert twin("ribbon")["largest"] == 5000 and twin("ribbon_permuted")["largest"] == 5000
    t = twin("lattice4")
    assert t["knn_tie"] and t["border_tie"] > 400 and t["contested"] > 300
    t = twin("holes")
    assert t["n_invalid"] > 100 and t["n_regions"] == 3
    p, _, _, kw = scene("sparse")
    assert np.bincount(knn_lists(p, kw["k"], kw["radius"])[0], minlength=len(p)).min() == 0
    for name in ("corner", "fold", "holes", "lattice4"):
        t = twin(name)
        assert t["n_seed"] + t["n_border"] + t["n_unassigned"] + t["n_invalid"] == len(scene(name)[0])


# ------------------------------------------------------------------------------------ ABI ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_segment_smooth", "rh_segment_smooth_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(R.lib(), name)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 125
    assert R.lib().rh_version() >= 125
    assert re.search(r"#define\s+RH_SEG_UNSIGNED\s+1\b", src) and L.SEG_UNSIGNED == UNSIGNED == 1


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["k", "flags", "radius", "cos_angle", "curv_max", "dist_max", "min_size", "order"]
    sf = ["n_regions", "n_seed", "n_border", "n_unassigned", "n_invalid", "n_small", "largest"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_segment_params), sizeof(rh_segment_stats));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_segment_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_segment_stats, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.SegmentParams), C.sizeof(L.SegmentStats)]
    mine += [getattr(L.SegmentParams, f).offset for f in pf] + [getattr(L.SegmentStats, f).offset for f in sf]
    assert got == mine and got[:2] == [48, 56]


def test_python_entries_are_exported():
    for name in ("segment_smooth", "segment_inpoints"):
        assert callable(getattr(R, name)) and name in R.__all__
    z = np.zeros((8, 3))
    with pytest.raises(ValueError):
        R.segment_smooth(z, z, order="volume")
    with pytest.raises(ValueError):
        R.segment_smooth(z, z[:7])
    with pytest.raises(ValueError):
        R.segment_smooth(z, z, np.zeros(7))
    with pytest.raises(ValueError):
        R.segment_inpoints(z, z, [0, 1])
    with pytest.raises(ValueError):
        R.segment_inpoints(z, z, [9])
    assert R.segment_inpoints(z, z, []) == []


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    xyz, nrm = np.zeros((8, 3)), np.tile(UP, (8, 1))
    nan, inf = float("nan"), float("inf")
    for dt in (np.float64, np.float32):
        x, nr = xyz.astype(dt), nrm.astype(dt)
        for kw in (dict(k=0), dict(k=64), dict(k=-3), dict(radius=-1.0), dict(radius=inf), dict(radius=nan), dict(cos_angle=1.5),
                   dict(cos_angle=-1.5), dict(cos_angle=nan), dict(cos_angle=inf), dict(curv_max=nan), dict(dist_max=-0.1),
                   dict(dist_max=inf), dict(dist_max=nan), dict(min_size=0), dict(min_size=-2), dict(order=2), dict(order=-1)):
            with pytest.raises(R.RansacHipError) as e:
                R.segment_smooth(x, nr, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        with pytest.raises(R.RansacHipError) as e:
            R.segment_smooth(x[:0], nr[:0])
        assert e.value.code == L.RH_E_INVALID
    lib = R.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    px, pn = xyz.ctypes.data_as(dp), nrm.ctypes.data_as(dp)
    labels, m = np.full(8, -7, dtype=np.int32), C.c_int64(-7)
    pl = labels.ctypes.data_as(i32p)

    def params(**kw):
        return L.SegmentParams(**dict(dict(k=4, flags=0, radius=0.0, cos_angle=0.9, curv_max=0.05, dist_max=0.0, min_size=1,
                                           order=L.CLUSTER_BY_INDEX), **kw))

    prm = params()
    fn = lib.rh_segment_smooth
    tail = (None, None, None)
    assert fn(None, pn, None, 8, C.byref(prm), 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, None, None, 8, C.byref(prm), 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, pn, None, 8, None, 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, pn, None, 8, C.byref(prm), 0, None, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID
    assert fn(px, pn, None, 8, C.byref(prm), 0, pl, None, 0, *tail, None, None) == L.RH_E_INVALID
    assert fn(px, pn, None, 8, C.byref(prm), 0, pl, None, -1, *tail, C.byref(m), None) == L.RH_E_INVALID
    for flags in (2, 3, -1, 1 << 20):                          # an unknown flag bit
        assert fn(px, pn, None, 8, C.byref(params(flags=flags)), 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID, flags
    for n in (0, -1, 2 ** 31 - 1, 2 ** 31, 2 ** 40):           # (n is refused before anything is read through xyz)
        assert fn(px, pn, None, n, C.byref(prm), 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID, n
    # n * k >= 2^31: the list slots are counted in 31 bits
    assert fn(px, pn, None, 2 ** 27, C.byref(params(k=16)), 0, pl, None, 0, *tail, C.byref(m), None) == L.RH_E_INVALID
    assert m.value == -7 and (labels == -7).all()              # nothing was written
    assert b"rh_segment_smooth" in lib.rh_last_error()


# ------------------------------------------------------------------------ segment_inpoints ----
def test_segment_inpoints_maps_back_to_the_callers_indices(monkeypatch):
    """The library call replaced by the twin: what is tested is the selection and the way back."""
    seen = {}

    def fake(vertices, normals, curvature=None, k=16, radius=0.0, cos_angle=None, curv_max=0.05, min_size=1, order="size",
             return_lists=False):
        seen["vertices"], seen["normals"], seen["curvature"] = np.array(vertices), np.array(normals), curvature
        r = ref_segment(vertices, normals, curvature, k=k, radius=radius, cos_angle=cos_angle, curv_max=curv_max, min_size=min_size,
                        order=order)
        return r["labels"], r["offsets"], r["idx"]

    monkeypatch.setattr(R.api, "segment_smooth", fake)
    #            1     2    3     4    5     6    7     8
    pts = line(10.0, 0.0, 10.5, 50.0, 0.5, 99.0, 0.9, 10.9)
    nrm = np.tile(UP, (8, 1))
    curv = np.arange(8) * 0.001
    inpoints = np.array([8, 2, 5, 4, 7, 1, 3])                  # not 6; in no order
    parts = R.segment_inpoints(pts, nrm, inpoints, curvature=curv, k=3, radius=0.6, cos_angle=0.9, order="index")
    assert np.array_equal(seen["vertices"], pts[inpoints - 1]) and np.array_equal(seen["curvature"], curv[inpoints - 1])
    # the selection is 10.9 0 0.5 50 0.9 10 10.5: regions by first index {10.9, 10, 10.5}, {0, 0.5, 0.9}, {50}
    assert [p.tolist() for p in parts] == [[8, 1, 3], [2, 5, 7], [4]]
    assert all(p.dtype == np.int64 for p in parts)
    parts = R.segment_inpoints(pts, nrm, inpoints, k=3, radius=0.6, cos_angle=0.9, min_size=2)
    assert [p.tolist() for p in parts] == [[8, 1, 3], [2, 5, 7]]  # the point at 50 is left out
    with pytest.raises(TypeError):
        R.segment_inpoints(pts, nrm, inpoints, return_kind=True)
