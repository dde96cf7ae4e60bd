"""rh_cluster on the device against the numpy twin of tests/cluster_reference.py: labels, kinds, counts, offsets, idx and every
field of the stats compared for equality -- no output has a tolerance.  The clouds are the smallest at which the kernels
can go wrong: all three kinds of points, borders between nearby clusters, pairs at exactly eps and pairs that pass or fail
by rounding alone, one chain united across every block, one cell holding many 64-point chunks, a zero-extent axis, n no
multiple of 64.  Every test first asserts ON THE TWIN'S RESULT that its cloud is the mix it is meant to be."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from cluster_reference import BORDER, CORE, NOISE, ref_cluster

pytestmark = pytest.mark.gpu

STATS = ("n_clusters", "n_core", "n_border", "n_noise", "n_small", "largest")


def _blobs():
    rng = np.random.default_rng(11)
    centres = rng.uniform(1, 9, size=(6, 3))
    pts = np.concatenate([rng.normal(c, 0.3, size=(400, 3)) for c in centres] + [rng.uniform(0, 10, size=(600, 3))])
    return pts[rng.permutation(len(pts))]


def _tenths(shift):
    k = np.arange(12) * 0.1
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + shift
    return g[np.random.default_rng(12).permutation(len(g))]


def _helix(permuted):
    t = 0.02 * np.arange(5000)
    pts = np.stack([3 * np.cos(t), 3 * np.sin(t), 0.05 * t], axis=1)
    return pts[np.random.default_rng(13).permutation(len(pts))] if permuted else pts


def _clump():
    rng = np.random.default_rng(14)
    return np.concatenate([rng.uniform(4.0, 4.2, size=(700, 3)), rng.uniform(0, 10, size=(1300, 3))])


def _flat():
    rng = np.random.default_rng(15)
    return np.concatenate([rng.uniform(0, 10, size=(3000, 2)), np.zeros((3000, 1))], axis=1)


def _bridge():
    rng = np.random.default_rng(16)
    a, b = rng.uniform(0, 1, size=(300, 3)), rng.uniform(0, 1, size=(300, 3)) + [3.8, 0.0, 0.0]
    mid = np.array([[1.2 + 0.3 * j, 0.5, 0.5] for j in range(9)])      # a chain from cube to cube, 0.2 off either face
    return np.concatenate([a, mid, b])


MAKERS = {"blobs": _blobs, "lattice": lambda: np.random.default_rng(17).integers(0, 8, size=(2000, 3)).astype(np.float64),
          "tenths": lambda: _tenths(0.0), "tenths_far": lambda: _tenths(1000.0), "helix": lambda: _helix(False),
          "helix_permuted": lambda: _helix(True), "clump": _clump, "flat": _flat, "bridge": _bridge,
          "identical": lambda: np.tile([[1.5, -2.0, 0.25]], (500, 1)),
          "one_cell": lambda: np.random.default_rng(18).uniform(0, 1, size=(3000, 3))}
_DATA, _REF = {}, {}


def data(name):
    if name not in _DATA:
        _DATA[name] = np.ascontiguousarray(MAKERS[name](), dtype=np.float64)
        _DATA[name].setflags(write=False)
    return _DATA[name]


def twin(name, eps, min_pts=8, min_size=1, order="index"):
    """the twin's result, computed once per case and shared"""
    key = (name, eps, min_pts, min_size, order)
    if key not in _REF:
        _REF[key] = ref_cluster(data(name), eps, min_pts, min_size, order)
    return _REF[key]


def device(xyz, eps, min_pts=8, min_size=1, order="index"):
    labels, kind, counts, offsets, idx, stats = R.cluster(xyz, eps, min_pts=min_pts, min_size=min_size, order=order, return_kind=True,
                                                          return_counts=True, return_lists=True, return_stats=True)
    return dict(labels=labels, kind=kind, counts=counts, offsets=offsets, idx=idx, **stats)


def same(got, exp):
    for f in ("labels", "kind", "counts", "offsets", "idx"):
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f], exp[f]), f
    for f in STATS:
        assert got[f] == exp[f], (f, got[f], exp[f])


def check(name, eps, **kw):
    exp = twin(name, eps, **kw)
    got = device(data(name), eps, **kw)
    print("%s eps=%g %s: M=%d core=%d border=%d noise=%d small=%d largest=%d" % ((name, eps, kw) + tuple(exp[f] for f in STATS)))
    same(got, exp)
    return exp


def test_blobs_have_all_three_kinds():
    exp = check("blobs", 0.25, min_pts=8)
    assert exp["n_clusters"] >= 3 and exp["n_core"] > 1000 and exp["n_border"] > 100 and exp["n_noise"] > 300
    assert exp["n_clusters"] < 50                              # clusters, not crumbs


@pytest.mark.parametrize("order", ["index", "size"])
def test_blobs_euclidean_mode_and_min_size(order):
    a = check("blobs", 0.25, min_pts=1, min_size=1, order=order)
    b = check("blobs", 0.25, min_pts=1, min_size=5, order=order)
    assert a["n_core"] == len(data("blobs")) and a["n_small"] == 0 and a["n_clusters"] > 100
    assert 1 <= b["n_clusters"] < a["n_clusters"] and b["n_small"] > 0 and b["n_noise"] == 0
    assert (b["kind"] == CORE).all()                           # what they were before the drop
    if order == "size":
        sizes = b["counts"][1:]
        assert (np.diff(sizes) <= 0).all() and sizes[0] == b["largest"]


def test_lattice_pairs_at_exactly_eps_and_duplicates():
    xyz = data("lattice")
    assert len(np.unique(xyz, axis=0)) < len(xyz)              # duplicates
    exp = check("lattice", 1.0, min_pts=8)
    assert exp["n_clusters"] == 1 and exp["n_core"] > 1500     # the axis neighbours at d2 == eps2 hold it together
    assert twin("lattice", 0.999, min_pts=8)["n_clusters"] != 1


@pytest.mark.parametrize("order", ["index", "size"])
def test_lattice_many_tiny_clusters(order):
    exp = check("lattice", 0.999, min_pts=4, order=order)      # only duplicates are neighbours
    sizes = exp["counts"][1:]
    assert exp["n_clusters"] > 100 and exp["n_noise"] > 200
    assert len(np.unique(sizes)) < len(sizes)                  # equal sizes: the tie rule of BY_SIZE decides
    if order == "size":
        assert (np.diff(sizes) <= 0).all()
        firsts = np.array([l[0] for l in exp["lists"][1:]])
        tie = np.diff(sizes) == 0
        assert tie.any() and (np.diff(firsts)[tie] > 0).all()


@pytest.mark.parametrize("name", ["tenths", "tenths_far"])
def test_tenths_pairs_decided_by_rounding_alone(name):
    """Axis neighbours of the grid of k * 0.1 are at eps = 0.1 up to rounding: d2 <= eps2 holds for some and fails for
    others.  A cell of width eps exactly loses some of the pairs that pass."""
    xyz = data(name)
    eps2 = np.float64(0.1) * np.float64(0.1)
    d = xyz[:, None, 0] - xyz[None, :144, 0]
    near = np.abs(np.abs(d) - 0.1) < 1e-9
    d2 = d * d
    assert 0 < (d2[near] <= eps2).sum() < near.sum()           # both outcomes occur
    exp = check(name, 0.1, min_pts=4)
    assert exp["n_clusters"] >= 2 and exp["n_core"] > 0 and 0 < exp["n_noise"] + exp["n_border"] < len(xyz)


@pytest.mark.parametrize("name", ["helix", "helix_permuted"])
@pytest.mark.parametrize("min_pts", [2, 3])
def test_helix_is_one_chain(name, min_pts):
    exp = check(name, 0.1, min_pts=min_pts)
    assert exp["n_clusters"] == 1 and exp["largest"] == 5000 and exp["n_core"] >= 4998


def test_clump_one_cell_of_many_chunks():
    xyz = data("clump")
    assert len(xyz) % 64 != 0
    exp = check("clump", 0.5, min_pts=5)
    assert exp["largest"] >= 700 and exp["n_clusters"] >= 1 and exp["n_noise"] > 500 and exp["n_core"] >= 700


def test_flat_cloud_with_a_zero_extent_axis():
    exp = check("flat", 0.3, min_pts=6)
    assert exp["n_clusters"] >= 2 and exp["n_border"] > 50 and exp["n_core"] > 1000


def test_bridge_points_do_not_join_the_cubes():
    exp = check("bridge", 0.3, min_pts=6)
    assert exp["n_clusters"] == 2 and (exp["kind"][300:309] != CORE).all()
    assert exp["labels"][:300].max() == 1 and exp["labels"][309:].max() == 2
    bridge = exp["kind"][300:309]
    assert (bridge == BORDER).any() and (bridge[1:8] == NOISE).all()      # the ends touch core points, the middle nobody's


def test_all_points_identical():
    exp = check("identical", 0.1, min_pts=8)
    assert exp["n_clusters"] == 1 and exp["n_core"] == 500
    exp = check("identical", 0.1, min_pts=501)
    assert exp["n_clusters"] == 0 and exp["n_noise"] == 500


def test_everything_in_one_cell():
    exp = check("one_cell", 2.0, min_pts=8)                    # eps above the cube's diagonal: 47 chunks of one cell
    assert exp["n_clusters"] == 1 and exp["n_core"] == 3000
    exp = check("one_cell", 2.0, min_pts=3001)
    assert exp["n_clusters"] == 0


def test_float32_is_the_widened_double_call():
    x32 = data("blobs").astype(np.float32)
    wide = x32.astype(np.float64)
    a, b = device(x32, 0.25), device(wide, 0.25)
    same(a, b)
    exp = ref_cluster(wide, 0.25, 8)
    assert exp["n_clusters"] >= 3 and exp["n_border"] > 100
    same(a, exp)


def test_two_runs_give_the_same_bytes():
    a, b = device(data("blobs"), 0.25), device(data("blobs"), 0.25)
    for f in ("labels", "kind", "counts", "offsets", "idx"):
        assert a[f].tobytes() == b[f].tobytes()
    # the outputs are optional
    only = R.cluster(data("blobs"), 0.25)
    assert isinstance(only, np.ndarray) and np.array_equal(only, a["labels"])


def _dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


def test_device_pointers_give_what_host_arrays_give():
    xyz = data("blobs")
    n = len(xyz)
    exp = device(xyz, 0.25)
    d_xyz = torch.from_numpy(np.array(xyz)).cuda()
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_offsets = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    d_idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    prm, st, m = L.ClusterParams(eps=0.25, min_pts=8, min_size=1, order=L.CLUSTER_BY_INDEX), L.ClusterStats(), C.c_int64()
    L.check(R.lib().rh_cluster(_dptr(d_xyz, C.c_double), n, C.byref(prm), 0, _dptr(d_labels, C.c_int32), _dptr(d_kind, C.c_uint8), n,
                               _dptr(d_counts, C.c_int64), _dptr(d_offsets, C.c_int64), _dptr(d_idx, C.c_int64), C.byref(m), C.byref(st)))
    torch.cuda.synchronize()
    M = m.value
    assert M == exp["n_clusters"] and [getattr(st, f) for f in STATS] == [exp[f] for f in STATS]
    assert np.array_equal(d_labels.cpu().numpy(), exp["labels"]) and np.array_equal(d_kind.cpu().numpy(), exp["kind"])
    counts, offsets = d_counts.cpu().numpy(), d_offsets.cpu().numpy()
    assert np.array_equal(counts[:M + 1], exp["counts"]) and np.array_equal(offsets[:M + 2], exp["offsets"])
    assert not counts[M + 1:].any() and (offsets[M + 2:] == n).all()      # the labels past M: empty lists
    assert np.array_equal(d_idx.cpu().numpy(), exp["idx"])


def test_capacity_is_reported_and_labels_are_still_written():
    xyz = data("blobs")
    n = len(xyz)
    exp = twin("blobs", 0.25, min_pts=8)
    assert exp["n_clusters"] > 2
    labels, kind = np.full(n, -1, dtype=np.int32), np.full(n, 255, dtype=np.uint8)
    counts, m, st = np.full(3, -1, dtype=np.int64), C.c_int64(), L.ClusterStats()
    prm = L.ClusterParams(eps=0.25, min_pts=8, min_size=1, order=L.CLUSTER_BY_INDEX)
    i32p, u8p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    rc = R.lib().rh_cluster(xyz.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(prm), 0, labels.ctypes.data_as(i32p),
                            kind.ctypes.data_as(u8p), 2, counts.ctypes.data_as(i64p), None, None, C.byref(m), C.byref(st))
    assert rc == L.RH_E_CAPACITY and m.value == exp["n_clusters"]
    assert np.array_equal(labels, exp["labels"]) and np.array_equal(kind, exp["kind"])
    assert [getattr(st, f) for f in STATS] == [exp[f] for f in STATS]
    assert (counts == -1).all()                                # a list that does not fit is not written in part
    # without counts and offsets no capacity is needed
    rc = R.lib().rh_cluster(xyz.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(prm), 0, labels.ctypes.data_as(i32p), None, 0,
                            None, None, None, C.byref(m), None)
    assert rc == L.RH_OK and m.value == exp["n_clusters"]


def test_a_nan_is_an_error_and_nothing_is_written():
    bad = np.array(data("clump"))
    bad[1999, 1] = np.nan
    with pytest.raises(R.RansacHipError) as e:
        R.cluster(bad, 0.5)
    assert e.value.code == L.RH_E_INVALID and "not finite" in str(e.value)


def test_every_way_out_releases():
    """The pattern of tests/test_call_scope_gpu.py: the device's free memory after 20 rounds of every way out -- a normal
    end, RH_E_CAPACITY, a coordinate that is not finite, a device that is not there -- equals what it was before them;
    the window is repeated, three times at the most, because other processes may share the device."""
    n = 200_000
    rng = np.random.default_rng(21)
    xyz = np.ascontiguousarray(rng.uniform(0, 16, size=(n, 3)))
    bad = xyz.copy()
    bad[n // 2, 0] = np.inf
    ndev = C.c_int()
    L.check(R.lib().rh_device_count(C.byref(ndev)))
    labels, kind = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    counts, offsets, idx = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 2, dtype=np.int64), np.zeros(n, dtype=np.int64)
    prm, m = L.ClusterParams(eps=0.3, min_pts=4, min_size=1, order=L.CLUSTER_BY_SIZE), C.c_int64()
    i32p, u8p, i64p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def call(pts, dev, cap):
        return R.lib().rh_cluster(pts.ctypes.data_as(dp), n, C.byref(prm), dev, labels.ctypes.data_as(i32p), kind.ctypes.data_as(u8p), cap,
                                  counts.ctypes.data_as(i64p), offsets.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), C.byref(m), None)

    def one_round():
        assert call(xyz, 0, n) == L.RH_OK, R.lib().rh_last_error()
        assert m.value > 3
        assert call(xyz, 0, 3) == L.RH_E_CAPACITY
        assert call(bad, 0, n) == L.RH_E_INVALID
        assert call(xyz, ndev.value, n) == L.RH_E_INVALID

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    one_round()
    seen = []
    for _ in range(3):
        warm = free_bytes()
        for _ in range(20):
            one_round()
        seen.append(warm - free_bytes())
        print("cluster: free before the window %d, after its 20 rounds %d bytes less" % (warm, seen[-1]))
        if seen[-1] == 0:
            break
    assert 0 in seen, seen


def test_round_trip_through_the_lists_into_shape_extents():
    """R.cluster's lists split by lists_from_assignment are lists that shape_extents takes: two plane patches of one
    plane come back as two clusters with an extent each."""
    rng = np.random.default_rng(22)
    a = np.concatenate([rng.uniform(0, 1, size=(400, 2)), np.zeros((400, 1))], axis=1)
    b = a + [3.0, 0.0, 0.0]
    xyz = np.ascontiguousarray(np.concatenate([a, b])[rng.permutation(800)])
    nrm = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (800, 1)))
    labels, offsets, idx = R.cluster(xyz, 0.2, min_pts=4, return_lists=True)
    lists = R.lists_from_assignment(offsets, idx)
    assert len(lists) == 3 and len(lists[0]) == 0 and sorted(len(l) for l in lists[1:]) == [400, 400]
    exp = ref_cluster(xyz, 0.2, 4)
    assert np.array_equal(labels, exp["labels"]) and all(np.array_equal(x, y) for x, y in zip(lists, exp["lists"]))
    pc = R.RANSACCloud(xyz, nrm, R.synth.make_subsets(800, 2, seed=1))
    plane = R.FittedPlane([0.0, 0.0, 0.0], [0.0, 0.0, 1.0])
    ext = R.shape_extents(pc, [(plane, l) for l in lists[1:]])
    assert [e.n for e in ext] == [len(l) for l in lists[1:]]
    for e, l in zip(ext, lists[1:]):
        p = xyz[l - 1]
        assert np.all(np.sort(e.size)[1:] <= 1.5) and e.dist_maxabs == 0.0       # one unit patch, not the 4-long pair
        assert np.allclose(e.centroid, p.mean(axis=0), atol=1e-9)
    # the patches of an index list in the caller's indexing
    parts = R.cluster_inpoints(xyz, lists[1], 0.2, min_pts=4)
    assert len(parts) == 1 and np.array_equal(parts[0], lists[1])
    both = np.concatenate([lists[2], lists[1]])
    parts = R.cluster_inpoints(xyz, both, 0.2, min_pts=4)
    assert len(parts) == 2 and np.array_equal(parts[0], lists[2]) and np.array_equal(parts[1], lists[1])
