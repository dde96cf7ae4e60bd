"""rh_segment_smooth on the device against the numpy twin of tests/segment_reference.py: labels, kinds, counts, offsets, idx
and every field of the stats compared for equality -- no output has a tolerance.  The clouds (tests/segment_scenes.py) are
the smallest at which the kernels can go wrong: all three kinds of points, border points between two regions and border
points that only their seed lists, pairs at exactly cos_angle and dist_max, d2 ties in the search and in the border choice,
one chain united across every block, points outside V, n no multiple of 64.  Every test first asserts ON THE TWIN'S RESULT
that its cloud is the mix it is meant to be."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from segment_reference import BORDER, CORE, NOISE, STATS, UNSIGNED, knn_lists, ref_segment
from segment_scenes import STEP_EXTRA, scene, twin

pytestmark = pytest.mark.gpu

ARRAYS = ("labels", "kind", "counts", "offsets", "idx")


def device(p, n, c, k=16, radius=0.0, cos_angle=0.9, curv_max=0.05, dist_max=0.0, flags=0, min_size=1, order="size"):
    """R.segment_smooth with the twin's keyword arguments: both get the same cos_angle double"""
    labels, kind, counts, offsets, idx, stats = R.segment_smooth(
        p, n, c, k=k, radius=radius, cos_angle=cos_angle, curv_max=curv_max, dist_max=dist_max, unsigned=bool(flags & UNSIGNED),
        min_size=min_size, order=order, return_kind=True, return_counts=True, return_lists=True, return_stats=True)
    return dict(labels=labels, kind=kind, counts=counts, offsets=offsets, idx=idx, **stats)


def same(got, exp):
    for f in ARRAYS:
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f], exp[f]), f
    for f in STATS:
        assert got[f] == exp[f], (f, got[f], exp[f])


def check(name, **over):
    exp = twin(name, **over)
    p, n, c, kw = scene(name)
    got = device(p, n, c, **dict(kw, **over))
    print("%s %s: " % (name, over) + " ".join("%s=%d" % (f, exp[f]) for f in STATS + ("contested", "reverse_only", "border_tie")))
    assert exp["n_seed"] + exp["n_border"] + exp["n_unassigned"] + exp["n_invalid"] == len(p)
    same(got, exp)
    return exp


def test_corner_three_patches_with_border_points_along_the_creases():
    exp = check("corner")
    assert len(scene("corner")[0]) % 64 != 0
    assert exp["n_regions"] == 3 and exp["n_border"] > 50 and exp["n_seed"] > 1000
    assert (exp["kind"] == CORE).any() and (exp["kind"] == BORDER).any()


def test_fold_contested_and_reverse_only_border_points():
    """the border points that an implementation walking only a point's own list, or picking "first reached", gets wrong"""
    exp = check("fold")
    assert exp["n_regions"] == 2 and exp["contested"] >= 3 and exp["reverse_only"] >= 1
    assert exp["n_border"] > 50 and exp["n_unassigned"] >= 1 and (exp["kind"] == NOISE).any()


def test_steps_the_distance_test_separates_parallel_sheets():
    off, on = check("steps_off"), check("steps_on")
    sheet = slice(0, len(scene("steps_on")[0]) - STEP_EXTRA)
    assert len(np.unique(off["labels"][sheet])) == 1 and len(np.unique(on["labels"][sheet])) == 2
    a, b, c, d = on["labels"][-STEP_EXTRA:]
    assert a == b and c != d                                   # exactly dist_max passes, the next double does not
    assert on["n_regions"] == 5 and off["n_regions"] == 3


def test_flipped_normals_need_the_unsigned_flag():
    assert check("flipped_unsigned")["n_regions"] == 1
    assert check("flipped_signed")["n_regions"] >= 2


@pytest.mark.parametrize("name", ["ribbon", "ribbon_permuted"])
def test_ribbon_is_one_chain(name):
    exp = check(name)
    assert exp["n_regions"] == 1 and exp["largest"] == 5000


@pytest.mark.parametrize("order", ["index", "size"])
def test_lattice_ties_in_the_search_and_in_the_border_choice(order):
    exp = check("lattice4", order=order)
    assert exp["knn_tie"] and exp["border_tie"] > 400 and exp["contested"] > 300 and exp["n_regions"] > 100
    sizes = exp["counts"][1:]
    assert len(np.unique(sizes)) < len(sizes)                  # equal sizes: the tie rule of BY_SIZE decides
    if order == "size":
        assert (np.diff(sizes) <= 0).all() and sizes[0] == exp["largest"]
    exp = check("lattice8", order=order)
    assert exp["n_regions"] == 1 and exp["border_tie"] > 400


@pytest.mark.parametrize("order", ["index", "size"])
def test_min_size_drops_regions_and_keeps_the_kinds(order):
    a, b = check("lattice4", order=order), check("lattice4", order=order, min_size=3)
    assert 1 <= b["n_regions"] < a["n_regions"] and b["n_small"] > 0 and np.array_equal(a["kind"], b["kind"])
    assert b["counts"][0] == b["n_small"] + b["n_unassigned"] + b["n_invalid"]
    c = check("sparse", min_size=5, order=order)
    assert c["n_small"] > 0 and c["n_regions"] >= 2


def test_zero_normals_and_nan_curvature():
    p, n, c, _ = scene("holes")
    exp = check("holes")
    assert exp["n_invalid"] == len(range(0, len(p), 7)) and (exp["labels"][::7] == 0).all() and (exp["kind"][::7] == NOISE).all()
    nan = np.flatnonzero(np.isnan(c))
    assert len(nan) > 10 and (exp["kind"][nan] != CORE).all()
    assert exp["n_regions"] == 3                               # nothing is bridged across the points outside V


def test_radius_leaves_points_without_neighbours():
    p, n, c, kw = scene("sparse")
    di, _, _, _ = knn_lists(p, kw["k"], kw["radius"])
    assert np.bincount(di, minlength=len(p)).min() == 0
    exp = check("sparse")
    assert exp["n_regions"] > 10 and exp["counts"][1:].min() == 1


@pytest.mark.parametrize("name", ["one", "five", "identical"])
def test_edge_sizes(name):
    exp = check(name)
    assert exp["n_regions"] == 1 and exp["largest"] == len(scene(name)[0])
    if name == "five":
        assert exp["n_border"] == 1


def test_float32_is_the_widened_double_call():
    p, n, c, kw = scene("fold")
    p32, n32, c32 = p.astype(np.float32), n.astype(np.float32), c.astype(np.float32)
    wide = [a.astype(np.float64) for a in (p32, n32, c32)]
    a, b = device(p32, n32, c32, **kw), device(*wide, **kw)
    same(a, b)
    exp = ref_segment(*wide, **kw)
    assert exp["n_regions"] >= 2 and exp["n_border"] > 50
    same(a, exp)


def test_two_runs_give_the_same_bytes():
    p, n, c, kw = scene("fold")
    a, b = device(p, n, c, **kw), device(p, n, c, **kw)
    for f in ARRAYS:
        assert a[f].tobytes() == b[f].tobytes()
    # the outputs are optional
    only = R.segment_smooth(p, n, c, k=kw["k"], cos_angle=kw["cos_angle"], curv_max=kw["curv_max"])
    assert isinstance(only, np.ndarray) and np.array_equal(only, a["labels"])


def test_a_permutation_gives_the_same_partition():
    exp = twin("corner")
    assert not exp["knn_tie"] and exp["border_tie"] == 0       # general position: no d2 tie decides a list or a border
    p, n, c, kw = scene("corner")
    o = np.random.default_rng(41).permutation(len(p))
    got = device(p[o], n[o], c[o], **kw)
    assert np.array_equal(got["kind"], exp["kind"][o])
    assert np.array_equal(got["counts"], exp["counts"])        # BY_SIZE; the three equal sizes may trade their numbers
    pairs = np.unique(np.stack([got["labels"], exp["labels"][o]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(exp["labels"])) == len(np.unique(got["labels"]))   # a bijection of the labels


def _dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


def _params(kw):
    return L.SegmentParams(k=kw["k"], flags=kw.get("flags", 0), radius=kw.get("radius", 0.0), cos_angle=kw["cos_angle"],
                           curv_max=kw.get("curv_max", 0.05), dist_max=kw.get("dist_max", 0.0), min_size=1, order=L.CLUSTER_BY_SIZE)


def test_device_pointers_give_what_host_arrays_give():
    p, nr, c, kw = scene("fold")
    n = len(p)
    exp = twin("fold")
    d_p, d_n, d_c = (torch.from_numpy(np.array(a)).cuda() for a in (p, nr, c))
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_offsets = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    d_idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    prm, st, m = _params(kw), L.SegmentStats(), C.c_int64()
    L.check(R.lib().rh_segment_smooth(_dptr(d_p, C.c_double), _dptr(d_n, C.c_double), _dptr(d_c, C.c_double), n, C.byref(prm), 0,
                                      _dptr(d_labels, C.c_int32), _dptr(d_kind, C.c_uint8), n, _dptr(d_counts, C.c_int64),
                                      _dptr(d_offsets, C.c_int64), _dptr(d_idx, C.c_int64), C.byref(m), C.byref(st)))
    torch.cuda.synchronize()
    M = m.value
    assert M == exp["n_regions"] and [getattr(st, f) for f in STATS] == [exp[f] for f in STATS]
    assert np.array_equal(d_labels.cpu().numpy(), exp["labels"]) and np.array_equal(d_kind.cpu().numpy(), exp["kind"])
    counts, offsets = d_counts.cpu().numpy(), d_offsets.cpu().numpy()
    assert np.array_equal(counts[:M + 1], exp["counts"]) and np.array_equal(offsets[:M + 2], exp["offsets"])
    assert not counts[M + 1:].any() and (offsets[M + 2:] == n).all()      # the labels past M: empty lists
    assert np.array_equal(d_idx.cpu().numpy(), exp["idx"])


def test_capacity_is_reported_and_labels_are_still_written():
    p, nr, c, kw = scene("lattice4")
    n = len(p)
    exp = twin("lattice4", order="size")
    assert exp["n_regions"] > 2
    labels, kind = np.full(n, -1, dtype=np.int32), np.full(n, 255, dtype=np.uint8)
    counts, m, st = np.full(3, -1, dtype=np.int64), C.c_int64(), L.SegmentStats()
    prm = _params(kw)
    dp, i32p, u8p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    args = (p.ctypes.data_as(dp), nr.ctypes.data_as(dp), c.ctypes.data_as(dp), n, C.byref(prm), 0, labels.ctypes.data_as(i32p))
    rc = R.lib().rh_segment_smooth(*args, kind.ctypes.data_as(u8p), 2, counts.ctypes.data_as(i64p), None, None, C.byref(m), C.byref(st))
    assert rc == L.RH_E_CAPACITY and m.value == exp["n_regions"]
    assert np.array_equal(labels, exp["labels"]) and np.array_equal(kind, exp["kind"])
    assert [getattr(st, f) for f in STATS] == [exp[f] for f in STATS]
    assert (counts == -1).all()                                # a list that does not fit is not written in part
    # without counts and offsets no capacity is needed
    rc = R.lib().rh_segment_smooth(*args, None, 0, None, None, None, C.byref(m), None)
    assert rc == L.RH_OK and m.value == exp["n_regions"]


def test_lists_round_trip_and_inpoints():
    p, n, c, kw = scene("fold")
    exp = twin("fold")
    labels, offsets, idx = R.segment_smooth(p, n, c, k=kw["k"], cos_angle=kw["cos_angle"], curv_max=kw["curv_max"], return_lists=True)
    lists = R.lists_from_assignment(offsets, idx)
    assert len(lists) == 3 and all(np.array_equal(x, y) for x, y in zip(lists, exp["lists"]))
    # the regions of an index list in the caller's indexing: one sheet alone is one region
    parts = R.segment_inpoints(p, n, lists[1], curvature=c, k=kw["k"], cos_angle=kw["cos_angle"], curv_max=kw["curv_max"])
    assert len(parts) == 1 and np.array_equal(parts[0], lists[1])


@pytest.mark.parametrize("what", ["coordinate", "normal_nan", "normal_large"])
def test_refused_input_is_an_error_and_nothing_is_written(what):
    p, nr, c, kw = scene("corner")
    p, nr = np.array(p), np.array(nr)
    if what == "coordinate":
        p[1000, 1] = np.inf
    elif what == "normal_nan":
        nr[77, 2] = np.nan
    else:
        nr[1451, 0] = -2.5
    n = len(p)
    labels, kind = np.full(n, -1, dtype=np.int32), np.full(n, 255, dtype=np.uint8)
    m, st, prm = C.c_int64(-7), L.SegmentStats(n_regions=-7), _params(kw)
    dp, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rc = R.lib().rh_segment_smooth(p.ctypes.data_as(dp), nr.ctypes.data_as(dp), c.ctypes.data_as(dp), n, C.byref(prm), 0,
                                   labels.ctypes.data_as(i32p), kind.ctypes.data_as(u8p), 0, None, None, None, C.byref(m), C.byref(st))
    assert rc == L.RH_E_INVALID
    assert "not finite" in R.lib().rh_last_error().decode()
    assert (labels == -1).all() and (kind == 255).all() and m.value == -7 and st.n_regions == -7
