"""rh_refit_component and the component filter of rh_ransac on the GPU, held EXACTLY (index lists, |I|, number of
components) to the numpy / Python twin of tests/test_component_host.py.  Arbitrary point sets are selected with a plane
through the origin, a huge eps, alpha = pi and every normal equal to the plane's: every enabled point is then an inlier,
and rh_cloud_set_enabled chooses the set."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from test_component_host import ref_component

pytestmark = pytest.mark.gpu

ANY_PLANE = R.FittedPlane([0.0, 0.0, 0.0], [0.0, 0.0, 1.0])
ANY = R.params_to_c(R.ransacparameters([R.FittedPlane], plane={"ϵ": 1e30, "α": math.pi}))


def _cloud(xyz, f32=False):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (len(xyz), 1))
    return R.RANSACCloud(xyz, nrm, [np.arange(1, len(xyz) + 1)], force_eltype=np.float32 if f32 else None)


def _check(pc, beta, conn26, enabled=None, shape=ANY_PLANE, params=ANY):
    """the call against the twin on rh_refit's own list; -> (list, stats)"""
    if enabled is not None:
        pc.set_enabled(enabled)
    before = pc.enabled_chunks().copy()
    refit = R.refit(shape, pc, params).inpoints
    if shape is ANY_PLANE:
        assert np.array_equal(refit, np.flatnonzero(pc.isenabled) + 1)
    exp, ncomp = ref_component(pc.vertices, refit, beta, conn26)
    es, st = R.refit_component(shape, pc, params, beta, conn26, return_stats=True)
    assert st == {"n_refit": refit.size, "n_components": ncomp}, (st, refit.size, ncomp)
    assert np.array_equal(es.inpoints, exp), (es.inpoints[:10], exp[:10], es.inpoints.size, exp.size)
    assert np.array_equal(pc.enabled_chunks(), before)
    return es.inpoints, st


@pytest.mark.parametrize("conn26", [True, False])
def test_degenerate_sets(conn26):
    rng = np.random.default_rng(0)
    xyz = np.concatenate([rng.uniform(-5, 5, size=(100, 3)), np.tile([[1.25, -2.5, 3.0]], (500, 1))])
    pc = _cloud(xyz)
    none = np.zeros(600, dtype=bool)
    got, st = _check(pc, 0.25, conn26, none)
    assert got.size == 0 and st == {"n_refit": 0, "n_components": 0}
    one = none.copy(); one[37] = True
    got, st = _check(pc, 0.25, conn26, one)
    assert got.tolist() == [38] and st["n_components"] == 1
    same = none.copy(); same[100:] = True
    got, st = _check(pc, 0.25, conn26, same)
    assert got.tolist() == list(range(101, 601)) and st == {"n_refit": 500, "n_components": 1}


def test_adjacency_corner_edge_face():
    a = [0.5, 0.5, 0.5]
    for b, joined26, joined6 in (([1.5, 1.5, 1.5], True, False), ([1.5, 1.5, 0.5], True, False), ([1.5, 0.5, 0.5], True, True),
                                 ([0.5, 0.5, 1.5], True, True), ([0.5, 1.5, 0.5], True, True), ([2.5, 0.5, 0.5], False, False)):
        pc = _cloud([a, b, b])
        for conn26, joined in ((True, joined26), (False, joined6)):
            got, st = _check(pc, 1.0, conn26)
            assert (got.tolist(), st["n_components"]) == (([1, 2, 3], 1) if joined else ([2, 3], 2))
    # every one of the 26 directions, from a cell in the middle (the device unites forward neighbours only: both orders)
    for d in [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]:
        b = [5.5 + d[0], 5.5 + d[1], 5.5 + d[2]]
        for pts in ([[5.5, 5.5, 5.5], b, [0.0, 0.0, 0.0], [9.0, 9.0, 9.0]], [b, [5.5, 5.5, 5.5], [0.0, 0.0, 0.0], [9.0, 9.0, 9.0]]):
            pc = _cloud(pts)
            for conn26 in (True, False):
                got, _ = _check(pc, 1.0, conn26)
                assert got.tolist() == ([1, 2] if conn26 or sum(map(abs, d)) == 1 else [1])


@pytest.mark.parametrize("conn26", [True, False])
def test_size_counts_points_and_ties_go_to_the_smallest_index(conn26):
    # a 40-cell component with 40 points against a 2-cell component with 41
    row = [[k + 0.5, 0.5, 0.5] for k in range(40)]
    blob = [[50.5, 7.5, 0.5]] * 20 + [[50.5, 8.5, 0.5]] * 21
    got, st = _check(_cloud(row + blob), 1.0, conn26)
    assert got.tolist() == list(range(41, 82)) and st["n_components"] == 2
    # equal sizes: the component with the smaller point index sits at the LARGER cell coordinates
    far = [[30.5 + k, 30.5, 30.5] for k in range(8)]
    near = [[0.5 + k, 0.5, 0.5] for k in range(8)]
    got, st = _check(_cloud(far + near), 1.0, conn26)
    assert got.tolist() == list(range(1, 9)) and st["n_components"] == 2
    got, st = _check(_cloud(near + far), 1.0, conn26)
    assert got.tolist() == list(range(1, 9)) and st["n_components"] == 2
    # ... and the smallest index may sit anywhere inside its component
    pts = [far[2]] + near[:4] + far[:4] + [far[4], near[4], near[5]]      # six points each
    got, _ = _check(_cloud(pts), 1.0, conn26)
    assert got.tolist() == [1, 6, 7, 8, 9, 10]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("offset", [0.0, -37.0, 1e6])
def test_coordinates_on_cell_faces(offset, f32):
    rng = np.random.default_rng(5)
    xyz = rng.integers(0, 24, size=(1500, 3)) * 0.25 + offset      # multiples of beta: every point on a face
    xyz[:40] += rng.integers(-1, 2, size=(40, 3)) * 2.0 ** -20      # ... and a few a hair off it (not exact in float at 1e6)
    pc = _cloud(xyz, f32)
    for conn26 in (True, False):
        _, st = _check(pc, 0.25, conn26)
        assert st["n_components"] > 1


def _spiral(n):
    x = y = 0
    out = [(0, 0)]
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    seg, d = 2, 0
    while len(out) < n:
        for _ in range(2):
            for _ in range(seg):
                x, y = x + dirs[d][0], y + dirs[d][1]
                out.append((x, y))
            d = (d + 1) % 4
        seg += 2      # arms two cells apart: not adjacent, not even by a corner
    return np.array(out[:n], dtype=np.float64)


@pytest.mark.parametrize("shape", ["chain", "spiral"])
def test_long_thin_components(shape):
    n = 4096
    if shape == "chain":
        cells = np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], axis=1)
    else:
        s = _spiral(n)
        cells = np.stack([s[:, 0], s[:, 1], np.zeros(n)], axis=1)
    order = np.random.default_rng(3).permutation(n)               # point order unrelated to the position on the path
    xyz = ((cells + 0.5) * 0.5)[order]
    pc = _cloud(xyz)
    for conn26 in (True, False):
        got, st = _check(pc, 0.5, conn26, np.ones(n, dtype=bool))
        assert got.size == n and st["n_components"] == 1
    # one cell out of the middle (on a straight stretch: around a corner the path's cells touch diagonally): the longer half wins
    k = next(i for i in range(2000, n) if np.array_equal(cells[i + 1] - cells[i], cells[i] - cells[i - 1]))
    cut = np.ones(n, dtype=bool)
    cut[np.flatnonzero(order == k)[0]] = False
    for conn26 in (True, False):
        got, st = _check(pc, 0.5, conn26, cut)
        assert got.size == n - k - 1 and st["n_components"] == 2
        assert np.array_equal(np.sort(order[got - 1]), np.arange(k + 1, n))


@pytest.mark.parametrize("conn26", [True, False])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_uniform_cube_near_percolation(seed, conn26):
    # 20 000 points in 41^3 cells: 1 - exp(-20000 / 68921) = a quarter of the cells occupied -- below the site-percolation
    # threshold of the cubic lattice with faces only (0.31: hundreds of components), above the 26-neighbourhood's (0.10: one
    # giant component and a few dozen islands); the open-addressing table is at a load of 0.26 either way
    xyz = np.random.default_rng(seed).uniform(0.0, 41.0, size=(20000, 3))
    _, st = _check(_cloud(xyz), 1.0, conn26)
    assert st["n_components"] > (10 if conn26 else 100)


def _scene(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "plane":
        p, n, t = synth.plane_patch(3000, rng, size=40.0)
        e = np.array([1.0, 0, 0]) if abs(t["normal"][0]) < 0.9 else np.array([0, 1.0, 0])
        u = np.cross(t["normal"], e)
        return p, n, R.FittedPlane(t["point"], t["normal"]), (p - t["point"]) @ (u / np.linalg.norm(u))
    if kind == "sphere":
        p, n, t = synth.sphere(3000, rng, radius=10.0)
        return p, n, R.FittedSphere(t["center"], t["radius"], True), p[:, 2] - t["center"][2]
    if kind == "cylinder":
        p, n, t = synth.cylinder(3000, rng)
        return p, n, R.FittedCylinder(t["axis"], t["center"], t["radius"], True), (p - t["center"]) @ t["axis"]
    p, n, t = synth.cone(3000, rng)
    return p, n, R.FittedCone(t["apex"], t["axis"], t["opang"], True), (p - t["apex"]) @ t["axis"]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", ["plane", "sphere", "cylinder", "cone"])
def test_shapes_cut_in_two_by_a_disabled_band(kind, f32):
    """a band of disabled points (a strip of the plane, the sphere's equator, mid-height of cylinder and cone) 4 cells
    wide -- two points in adjacent cells are at most 2 sqrt(3) cells apart -- leaves two unequal parts: the larger comes back"""
    beta = 2.0
    p, n, shape, t = _scene(kind, 21)
    lo = t.min() + 0.2 * (t.max() - t.min())
    band = (t >= lo) & (t < lo + 4 * beta)
    below, above = t < lo, t >= lo + 4 * beta
    assert min(below.sum(), above.sum()) > 50 and abs(int(below.sum()) - int(above.sum())) > 50
    pc = R.RANSACCloud(p, n, [np.arange(1, 3001)], force_eltype=np.float32 if f32 else None)
    params = R.params_to_c(R.ransacparameters(**{kind: {"ϵ": 0.3, "α": math.radians(10.0)}}))
    got, st = _check(pc, beta, True, ~band, shape, params)
    big = below if below.sum() > above.sum() else above
    assert st["n_refit"] > 0.9 * (~band).sum() and st["n_components"] >= 2
    assert big[got - 1].all() and got.size > 0.9 * big.sum()


N_BIG = (1 << 21) + 1000


@pytest.fixture(scope="module")
def big():
    """two coplanar patches (the first the larger) and 1000 noise points; from 2^21 points on the culled scan is the default"""
    rng = np.random.default_rng(8)
    na = 1_200_000
    nb = N_BIG - 1000 - na
    a = np.stack([rng.uniform(0, 30, na), rng.uniform(0, 30, na), rng.normal(0, 0.02, na)], axis=1)
    b = np.stack([rng.uniform(40, 60, nb), rng.uniform(0, 30, nb), rng.normal(0, 0.02, nb)], axis=1)
    noise = rng.uniform(-20, 80, size=(1000, 3))
    xyz = np.concatenate([a, b, noise])
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (N_BIG, 1))
    nv = rng.normal(size=(1000, 3))
    nrm[-1000:] = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    perm = rng.permutation(N_BIG)
    xyz, nrm = np.ascontiguousarray(xyz[perm]), np.ascontiguousarray(nrm[perm])
    pc = R.RANSACCloud(xyz, nrm, [np.arange(1, N_BIG + 1, 64)])
    dis = np.ones(N_BIG, dtype=bool)
    dis[rng.integers(0, N_BIG, size=5000)] = False
    pc.set_enabled(dis)
    return pc, np.flatnonzero(perm < na) + 1


def test_big_cloud_scan_and_culled_agree_and_repeat(big):
    pc, patch_a = big
    shape = R.FittedPlane([0.0, 0.0, 0.0], [0.0, 0.0, 1.0])
    params = R.params_to_c(R.ransacparameters(plane={"ϵ": 0.1, "α": math.radians(5.0)}))
    before = pc.enabled_chunks().copy()
    lists = {}
    for path in ("scan", "culled"):
        with R.option("refit_path", path, cloud=pc):
            first, st = R.refit_component(shape, pc, params, 0.5, True, return_stats=True)
            again, st2 = R.refit_component(shape, pc, params, 0.5, True, return_stats=True)
            refit = R.refit(shape, pc, params).inpoints
        assert first.inpoints.tobytes() == again.inpoints.tobytes() and st == st2
        lists[path] = (first.inpoints, st, refit)
    assert np.array_equal(lists["scan"][0], lists["culled"][0]) and lists["scan"][1] == lists["culled"][1]
    assert np.array_equal(lists["scan"][2], lists["culled"][2])
    got, st, refit = lists["culled"]
    exp, ncomp = ref_component(pc.vertices, refit, 0.5, True)
    assert np.array_equal(got, exp) and st == {"n_refit": refit.size, "n_components": ncomp}
    assert ncomp >= 2 and np.isin(got, patch_a).mean() > 0.999 and got.size > 1_150_000
    assert np.array_equal(pc.enabled_chunks(), before)


def test_errors():
    pc = _cloud([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [1048575.5, 0.0, 0.0], [1048576.0, 0.0, 0.0]])
    for beta in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(R.RansacHipError) as e:
            R.refit_component(ANY_PLANE, pc, ANY, beta)
        assert e.value.code == L.RH_E_INVALID
    on = np.array([True, True, True, True, False])
    pc.set_enabled(on)                                  # cells 0 .. 2^20 - 1 along x: allowed
    got, st = _check(pc, 1.0, True)
    assert got.tolist() == [1, 2, 3] and st["n_components"] == 2
    pc.set_enabled(~on | np.array([True, False, False, False, False]))      # cells 0 and 2^20: one too many
    with pytest.raises(R.RansacHipError) as e:
        R.refit_component(ANY_PLANE, pc, ANY, 1.0)
    assert e.value.code == L.RH_E_INVALID
    # capacity: the needed size comes back
    pc.set_enabled(on)
    out, n, n_refit, n_comp = np.zeros(8, dtype=np.int64), C.c_int64(), C.c_int64(), C.c_int32()
    cs = ANY_PLANE.to_c()
    rc = L.lib().rh_refit_component(pc._h, C.byref(cs), C.byref(ANY), 1.0, 1, out.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                    C.byref(n), C.byref(n_refit), C.byref(n_comp))
    assert rc == L.RH_E_CAPACITY and n.value == 3 and n_refit.value == 4
    rc = L.lib().rh_refit_component(pc._h, C.byref(cs), C.byref(ANY), 1.0, 1, out.ctypes.data_as(C.POINTER(C.c_int64)), 3,
                                    C.byref(n), None, None)
    assert rc == L.RH_OK and n.value == 3 and out[:3].tolist() == [1, 2, 3]
    # the filter setting
    assert pc.component_filter == (0.0, True)
    pc.set_component_filter(0.75, conn26=False)
    assert pc.component_filter == (0.75, False)
    pc.set_component_filter(-3.0)
    assert pc.component_filter == (0.0, True)
    for beta in (float("nan"), float("inf")):
        with pytest.raises(R.RansacHipError) as e:
            pc.set_component_filter(beta)
        assert e.value.code == L.RH_E_INVALID


# ---- the filter inside ransac() ----
RANSAC_BETA = 1.0


def _two_tables():
    """two coplanar 2000-point patches 5 apart, a sphere and 10 % outliers"""
    rng = np.random.default_rng(77)
    t = synth.plane_params(rng, size=10.0)
    pa, na = synth.plane_points(t, 2000, rng)
    t2 = dict(t, point=t["point"] + 15.0 * t["_x"])
    pb, nb = synth.plane_points(t2, 2000, rng)
    ps, ns, _ = synth.sphere(2000, rng, radius=6.0)
    no = 667
    po = rng.uniform(0, synth.BOX, size=(no, 3))
    nn = rng.normal(size=(no, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    xyz, nrm = np.concatenate([pa, pb, ps, po]), np.concatenate([na, nb, ns, nn])
    label = np.concatenate([np.full(2000, 1), np.full(2000, 2), np.zeros(2000 + no, dtype=np.int64)])
    perm = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm]), np.ascontiguousarray(nrm[perm]), label[perm]


TABLES = _two_tables()


def _tables_cloud(f32):
    xyz, nrm, _ = TABLES
    subs = synth.make_subsets(len(xyz), 2, seed=4)
    return R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32 if f32 else None)


def _cparams(streams, octree):
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere], iteration={"minsubsetN": 100, "itermax": 100, "τ": 300, "prob_det": 0.9})
    return R.params_to_c(params, score_mode=L.SCORE_F64, sampling_streams=streams, octree_sampling=octree)


def _both(es):
    lab = TABLES[2][es.inpoints - 1]
    return (lab == 1).sum() > 100 and (lab == 2).sum() > 100


def _same(a, b):
    return len(a) == len(b) and all(bytes(x.c_shape) == bytes(y.c_shape) and np.array_equal(x.inpoints, y.inpoints) for x, y in zip(a, b))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("streams,octree", [(0, False), (1, False), (1, True)])
def test_ransac_with_the_filter(streams, octree, f32):
    pc = _tables_cloud(f32)
    cp = _cparams(streams, octree)
    off, _ = R.ransac(pc, cp, seed=9)
    assert any(_both(e) for e in off)                       # filter off: one plane holds both table tops
    enabled_off = pc.enabled_chunks().copy()
    on, _ = R.ransac(pc, cp, setenabled=True, seed=9, component_beta=RANSAC_BETA)
    assert pc.component_filter == (0.0, True)               # the call's setting is gone again
    lab = TABLES[2]
    for e in on:
        assert not ((lab[e.inpoints - 1] == 1).any() and (lab[e.inpoints - 1] == 2).any())
    # ... with it on each is found as a shape of its own (the second one often as a sphere of huge radius: its coplanar
    # candidates died with the first extraction)
    assert sum((lab[e.inpoints - 1] == 1).sum() > 1000 for e in on) == 1 and sum((lab[e.inpoints - 1] == 2).sum() > 1000 for e in on) == 1
    # replay on a second cloud: every extraction took exactly the twin's component of rh_refit's list, and only that
    # was invalidated
    pc2 = _tables_cloud(f32)
    for e in on:
        lst = R.refit(e.c_shape, pc2, cp).inpoints
        exp, _ = ref_component(pc2.vertices, lst, RANSAC_BETA, True)
        assert np.array_equal(e.inpoints, exp), (e.inpoints.size, exp.size, lst.size)
        R.invalidate_indexes(pc2, exp)
    assert np.array_equal(pc.enabled_chunks(), pc2.enabled_chunks())
    # the filter off again: what the call returned before the filter was ever set
    pc.set_component_filter(0)
    again, _ = R.ransac(pc, cp, setenabled=True, seed=9)
    assert _same(off, again) and np.array_equal(pc.enabled_chunks(), enabled_off)


def test_ransac_filter_with_faces_only_and_the_clouds_own_setting():
    pc = _tables_cloud(False)
    cp = _cparams(1, False)
    pc.set_component_filter(RANSAC_BETA, conn26=False)
    on, _ = R.ransac(pc, cp, seed=9)                        # no keyword: the cloud's setting holds
    assert pc.component_filter == (RANSAC_BETA, False)
    pc2 = _tables_cloud(False)
    for e in on:
        exp, _ = ref_component(pc2.vertices, R.refit(e.c_shape, pc2, cp).inpoints, RANSAC_BETA, False)
        assert np.array_equal(e.inpoints, exp)
        R.invalidate_indexes(pc2, exp)
    assert len(on) >= 3


def test_ransac_mp_refuses_a_filter():
    pc = _tables_cloud(False)
    cp = _cparams(1, False)
    grp = R.MpGroup("/rh_comp_solo_%d" % os.getpid(), 0, 1)
    try:
        pc.set_component_filter(RANSAC_BETA)
        with pytest.raises(R.RansacHipError) as e:
            R.ransac(pc, cp, seed=9, mp=grp)
        assert e.value.code == L.RH_E_INVALID
        pc.set_component_filter(0)
        got, _ = R.ransac(pc, cp, seed=9, mp=grp)
        assert len(got) >= 2
    finally:
        grp.close()


@pytest.mark.parametrize("conn26", [True, False])
def test_minimum_pass_of_258_blocks_folds_past_its_first_trip(conn26):
    """64 * 4 * 257 + 1 inliers of one plane: 258 blocks of the masked minimum pass, so the one folding block
    (cell_grid.h) goes round its loop a second, partial time; the box's corner is the last block's single point."""
    n = 64 * 4 * 257 + 1
    rng = np.random.default_rng(258)
    xyz = np.concatenate([rng.uniform(0, 3, size=(n, 2)), np.zeros((n, 1))], axis=1)
    xyz[n // 2:, 0] += 5.0                             # two slabs two cells apart
    xyz[-1] = [-0.5, -0.5, 0.0]
    got, st = _check(_cloud(xyz), 1.0, conn26, np.ones(n, dtype=bool))
    assert st["n_refit"] == n and st["n_components"] == 2 and got.size >= n // 2
