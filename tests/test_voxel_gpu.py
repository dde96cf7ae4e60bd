"""Voxel-grid downsampling (rh_voxel_downsample) on the GPU, held to the numpy twin of tests/test_voxel_host.py: rows,
first indices, counts, the map and the number of dropped points exactly, output points and normals bit for bit."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from test_voxel_host import ref_voxel

pytestmark = pytest.mark.gpu

MODES = {"first": L.VOX_FIRST, "centroid": L.VOX_CENTROID}


def call(xyz, nrm, beta, mode, align=False, cap=None, want_normals=True):
    """rh_voxel_downsample[_f32] with every output.  Returns (rc, xyz_out, nrm_out or None, first, count, row_of_point,
    n_dropped, n_out); the row outputs are cut to min(n_out, cap)."""
    f32 = xyz.dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(xyz, dtype=t)
    n = len(xyz)
    cap = n if cap is None else cap
    p = lambda a, c: a.ctypes.data_as(C.POINTER(c))
    nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=t)
    xo = np.full((max(cap, 1), 3), -7.0, dtype=t)
    no = np.full((max(cap, 1), 3), -7.0, dtype=t) if nrm is not None and want_normals else None
    first, count = np.full(max(cap, 1), -7, dtype=np.int64), np.full(max(cap, 1), -7, dtype=np.int32)
    rowof = np.full(n, -7, dtype=np.int32)
    m, nd = C.c_int64(-7), C.c_int64(-7)
    prm = L.VoxelParams(beta=beta, mode=MODES[mode], flags=L.VOX_ALIGN_NORMALS if align else 0)
    fn = R.lib().rh_voxel_downsample_f32 if f32 else R.lib().rh_voxel_downsample
    rc = fn(p(xyz, ct), None if nrm is None else p(nrm, ct), n, C.byref(prm), 0, p(xo, ct), None if no is None else p(no, ct),
            p(first, C.c_int64), p(count, C.c_int32), cap, p(rowof, C.c_int32), C.byref(m), C.byref(nd))
    k = min(max(m.value, 0), cap)
    return rc, xo[:k], None if no is None else no[:k], first[:k], count[:k], rowof, nd.value, m.value


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_twin(xyz, nrm, beta, mode, align=False):
    rc, xo, no, first, count, rowof, nd, m = call(xyz, nrm, beta, mode, align)
    ex, en, efirst, ecount, erowof, end = ref_voxel(xyz, nrm, beta, mode, align)
    what = (len(xyz), beta, mode, align, nrm is not None)
    assert rc == L.RH_OK, (what, R.lib().rh_last_error())
    assert m == len(efirst) and nd == end, (what, m, len(efirst), nd, end)
    assert np.array_equal(first, efirst) and np.array_equal(count, ecount) and np.array_equal(rowof, erowof), what
    assert same_bits(xo, ex), (what, np.flatnonzero((xo != ex).any(axis=1))[:5])
    if nrm is not None:
        assert same_bits(no, en), (what, np.flatnonzero((no != en).any(axis=1))[:5])
    return xo, no, first, count, rowof


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes_around_the_wave_and_block_edges(n):
    rng = np.random.default_rng(100 + n)
    xyz = rng.uniform(0, 1, size=(n, 3))
    nrm = unit(rng.normal(size=(n, 3)))
    for beta in (2.0, 0.5, 1e-3):                     # about 1, about 8 and about n occupied cells
        for mode in ("first", "centroid"):
            check_against_twin(xyz, None, beta, mode)
            check_against_twin(xyz, nrm, beta, mode)
            check_against_twin(xyz, nrm, beta, mode, align=True)


def test_all_duplicates_give_one_row_equal_to_the_point():
    pt = np.array([[3.7, -1.25, 1e3 + 0.1]])
    xyz = np.repeat(pt, 500, axis=0)
    nrm = np.repeat(unit(np.array([[1.0, 2.0, -2.0]])), 500, axis=0)
    for mode in ("first", "centroid"):
        xo, no, first, count, rowof = check_against_twin(xyz, nrm, 0.5, mode)
        assert same_bits(xo, pt) and first.tolist() == [1] and count.tolist() == [500] and (rowof == 1).all()
    # next to other points o is no longer the point itself; the centroid stays within the grid's resolution of it
    more = np.concatenate([xyz, pt - [0.3, 0.2, 0.1]])
    xo, _, _, count, _ = check_against_twin(more, None, 0.25, "centroid")
    assert count.tolist() == [500, 1] and np.abs(xo[0] - pt[0]).max() <= 0.25 * 2.0 ** -32 + 4 * np.spacing(1e3)


def test_one_dense_cell_next_to_a_spread():
    rng = np.random.default_rng(7)
    nd = 3 << 20
    dense = rng.uniform(0.75, 0.99, size=(nd, 3)) + [5.0, 5.0, 5.0]          # all in unit cell (5, 5, 5), offsets >= 0.75:
    ijk = np.stack(np.unravel_index(np.arange(1000), (10, 10, 10)), axis=1)   # S >= 3 * 2^20 * 0.75 * 2^32 = 2.25 * 2^52 > 2^53
    spread = ijk + rng.uniform(0.0, 1.0, size=(1000, 3))
    spread[0] = 0.0                                                           # pins o = (0, 0, 0)
    spread = spread[(ijk != 5).any(axis=1)]
    xyz = np.concatenate([spread[:400], dense, spread[400:]])
    nrm = unit(rng.normal(size=(len(xyz), 3)) + [0.0, 0.0, 3.0])
    xo, no, first, count, rowof = check_against_twin(xyz, nrm, 1.0, "centroid", align=True)
    assert len(first) == 1000 and count.max() == nd and count[400] == nd
    check_against_twin(xyz, None, 1.0, "first")


def test_many_cells_each_point_its_own():
    rng = np.random.default_rng(8)
    cells = rng.permutation(128 ** 3 - 1)[:200_000] + 1                       # (not cell 0: the point that pins o has it)
    ijk = np.stack(np.unravel_index(cells, (128, 128, 128)), axis=1)
    xyz = (ijk + rng.uniform(0.05, 0.95, size=ijk.shape)) * 0.37 - 11.0
    xyz = np.concatenate([[[-11.0, -11.0, -11.0]], xyz])                      # pins o
    for mode in ("first", "centroid"):
        _, _, first, count, rowof = check_against_twin(xyz, None, 0.37, mode)
        assert len(first) == 200_001 and count.max() == 1 and np.array_equal(rowof, np.arange(1, 200_002))


def test_dropped_points():
    rng = np.random.default_rng(9)
    n = 5000
    xyz = rng.uniform(-4, 4, size=(n, 3))
    nrm = unit(rng.normal(size=(n, 3)))
    bad = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)[:298]])
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:150], rng.integers(0, 3, 50)] = np.inf
    xyz[bad[150:200], rng.integers(0, 3, 50)] = -np.inf
    for mode in ("first", "centroid"):
        _, _, _, _, rowof = check_against_twin(xyz, None, 0.5, mode)
        assert (rowof[bad[:200]] == 0).all() and rowof[0] == 0 and rowof[-1] == 0 and (rowof != 0).sum() == n - 200
    nrm[bad[200:250], rng.integers(0, 3, 50)] = np.nan
    nrm[bad[250:280], rng.integers(0, 3, 30)] = -np.inf
    nrm[bad[280:300], rng.integers(0, 3, 20)] = 2.5
    for mode in ("first", "centroid"):
        _, _, _, _, rowof = check_against_twin(xyz, nrm, 0.5, mode, align=True)
        assert (rowof[bad] == 0).all() and (rowof != 0).sum() == n - 300
    # everything dropped: no rows, RH_OK
    allbad = np.full((300, 3), np.nan)
    rc, xo, _, first, count, rowof, ndrop, m = call(allbad, None, 1.0, "centroid")
    assert rc == L.RH_OK and m == 0 and ndrop == 300 and not rowof.any() and len(xo) == 0
    out = R.voxeldownsample(allbad, 1.0, return_map=True)
    assert out[0].shape == (0, 3) and not out[1].any()


def test_permutation_permutes_the_rows():
    rng = np.random.default_rng(10)
    n = 30_000
    xyz = rng.uniform(0, 10, size=(n, 3))
    nrm = unit(rng.normal(size=(n, 3)))
    xo, no, first, count, rowof = check_against_twin(xyz, nrm, 0.7, "centroid", align=False)
    perm = rng.permutation(n)
    xp, np_, firstp, countp, rowofp = check_against_twin(xyz[perm], nrm[perm], 0.7, "centroid", align=False)
    rows = lambda x, q, c: sorted(zip(c.tolist(), [r.tobytes() for r in x], [r.tobytes() for r in q]))
    assert rows(xo, no, count) == rows(xp, np_, countp)
    # the same cells, renumbered by the new first indices
    assert (np.diff(firstp) > 0).all()
    new_row_of_old = np.zeros(len(first) + 1, dtype=np.int64)
    new_row_of_old[rowof[perm]] = rowofp
    assert same_bits(xp[new_row_of_old[1:] - 1], xo)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    for r in range(0, len(first), 97):
        assert firstp[new_row_of_old[r + 1] - 1] == inv[np.flatnonzero(rowof == r + 1)].min() + 1


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0, 10, size=(100_000, 3))
    nrm = unit(rng.normal(size=xyz.shape))
    a = call(xyz, nrm, 0.4, "centroid", align=True)
    b = call(xyz, nrm, 0.4, "centroid", align=True)
    assert a[0] == b[0] == L.RH_OK and a[6:] == b[6:]
    for u, v in zip(a[1:6], b[1:6]):
        assert same_bits(u, v)


def test_capacity():
    rng = np.random.default_rng(12)
    xyz = rng.uniform(0, 10, size=(2000, 3))
    ex, _, efirst, _, erowof, _ = ref_voxel(xyz, None, 1.0, "centroid")
    M = len(efirst)
    rc, _, _, _, _, rowof, _, m = call(xyz, None, 1.0, "centroid", cap=M - 1)
    assert rc == L.RH_E_CAPACITY and m == M
    assert np.array_equal(rowof, erowof)                  # the map is still written in full
    rc, xo, _, first, _, _, _, m = call(xyz, None, 1.0, "centroid", cap=M)
    assert rc == L.RH_OK and m == M and same_bits(xo, ex) and np.array_equal(first, efirst)


def test_extent_limit():
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.5]])
    with pytest.raises(R.RansacHipError) as e:
        R.voxeldownsample(xyz, 2.0 ** -20)               # floor(1 / beta) = 2^20: one cell too many along y
    assert e.value.code == L.RH_E_INVALID
    with pytest.raises(ValueError):
        ref_voxel(xyz, None, 2.0 ** -20, "centroid")
    check_against_twin(xyz, None, 2.0 ** -20 * (1 + 2.0 ** -40), "centroid")   # 2^20 - 1 is the last cell allowed
    with pytest.raises(R.RansacHipError) as e:
        R.voxeldownsample(xyz * 1e300, 1e-300)
    assert e.value.code == L.RH_E_INVALID


def test_float32_is_the_double_result_rounded_once():
    rng = np.random.default_rng(13)
    x32 = rng.uniform(-5, 5, size=(20_000, 3)).astype(np.float32)
    n32 = unit(rng.normal(size=x32.shape)).astype(np.float32)
    for mode, align in (("first", False), ("centroid", False), ("centroid", True)):
        rc, xo, no, first, count, rowof, nd, m = call(x32, n32, 0.3, mode, align)
        ex, en, efirst, ecount, erowof, end = ref_voxel(x32.astype(np.float64), n32.astype(np.float64), 0.3, mode, align)
        assert rc == L.RH_OK and xo.dtype == np.float32 and no.dtype == np.float32
        assert m == len(efirst) and nd == end and np.array_equal(first, efirst) and np.array_equal(count, ecount)
        assert np.array_equal(rowof, erowof)
        assert same_bits(xo, ex.astype(np.float32)) and same_bits(no, en.astype(np.float32))
    v, q, idx, cnt, mp = R.voxeldownsample(x32, 0.3, normals=n32, mode="first", return_index=True, return_counts=True, return_map=True)
    assert v.dtype == np.float32 and same_bits(v, x32[idx - 1]) and same_bits(q, n32[idx - 1])
    assert cnt.sum() == len(x32) and np.array_equal(mp, erowof)


def test_cfg2_full_size():
    c = synth.config("cfg2")
    xyz, nrm = c["xyz"], c["nrm"]
    beta = 4.0 * synth.median_nn_distance(xyz)
    for mode in ("first", "centroid"):
        _, _, first, _, _ = check_against_twin(xyz, nrm, beta, mode)
        assert 0.05 * len(xyz) < len(first) < 0.6 * len(xyz)


def _dist_truth(t, p):
    if t["kind"] == "plane":
        return np.abs((p - t["point"]) @ t["normal"])
    if t["kind"] == "sphere":
        return np.abs(np.linalg.norm(p - t["center"], axis=1) - t["radius"])
    v = p - t["center"]
    return np.abs(np.linalg.norm(v - np.outer(v @ t["axis"], t["axis"]), axis=1) - t["radius"])


def _dist_shape(s, p):
    if isinstance(s, R.FittedPlane):
        return np.abs((p - s.point) @ s.normal)
    if isinstance(s, R.FittedSphere):
        return np.abs(np.linalg.norm(p - s.center, axis=1) - s.radius)
    assert isinstance(s, R.FittedCylinder)
    v = p - s.center
    return np.abs(np.linalg.norm(v - np.outer(v @ s.axis, s.axis), axis=1) - s.radius)


def test_thinned_cloud_through_ransac_and_back():
    xyz, nrm, truth = synth.make_cloud(200_000, ["plane", "sphere", "cylinder"], 0.0, seed=21)
    beta = 0.25
    v, q, rowof = R.voxeldownsample(xyz, beta, normals=nrm, mode="centroid", return_map=True)
    m = len(v)
    assert 10_000 < m < 150_000 and rowof.max() == m and rowof.min() == 1
    subs = synth.make_subsets(m, 8, seed=21)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder],
                                iteration={"minsubsetN": 200, "itermax": 200, "τ": 1000, "prob_det": 0.9})
    cp = R.params_to_c(params, score_mode=L.SCORE_F64)
    got, _ = R.ransac(R.RANSACCloud(v, q, subs), cp, seed=1234)
    kinds = {"plane": L.PLANE, "sphere": L.SPHERE, "cylinder": L.CYLINDER}
    found = set()
    for ti, t in enumerate(truth):
        for g in got:
            pts = v[np.asarray(g.inpoints) - 1]
            if g.c_shape.kind == kinds[t["kind"]] and len(pts) > 500 and np.median(_dist_truth(t, pts)) < 0.05:
                found.add(ti)
    assert found == set(range(len(truth))), ([R.strt(g.shape) for g in got], found)
    total = 0
    for g in got:
        full = R.expand_inpoints(g.inpoints, rowof)
        assert len(full) >= len(g.inpoints) and (np.diff(full) > 0).all() and full.min() >= 1 and full.max() <= len(xyz)
        assert np.array_equal(np.unique(rowof[full - 1]), np.unique(g.inpoints))
        eps = params[R.strt(g.shape)]["ϵ"]
        d = _dist_shape(g.shape, xyz[full - 1])
        assert d.max() <= eps + beta, (R.strt(g.shape), d.max(), eps + beta)
        total += len(full)
    assert total > 0.8 * len(xyz)


@pytest.mark.parametrize("mode", ["first", "centroid"])
def test_minimum_pass_of_258_blocks_folds_past_its_first_trip(mode):
    """256 * 257 + 1 points: 258 partial results, so the one folding block (cell_grid.h) goes round its loop a second,
    partial time; the minimum and the maximum sit in the last block's single point."""
    n = 256 * 257 + 1
    rng = np.random.default_rng(258)
    xyz = rng.uniform(0, 6, size=(n, 3))
    xyz[-1] = [-1.25, -0.5, -3.0]
    xyz[256 * 256 + 5] = [7.5, 8.25, 6.125]           # the maximum: block 256, the first of the second trip
    nrm = unit(rng.normal(size=(n, 3)))
    check_against_twin(xyz, nrm, 0.75, mode)
