"""rh_orient_normals on the GPU against the numpy twin (tests/orient_reference.py): the library must EQUAL it -- flips,
components, every integer of the stats, the bytes of the normals and of min_tree_absdot."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import synth
from orient_reference import ANCHOR_FIRST, ANCHOR_TOP, STATS, edges_brute, edges_from_lists, orient_from_edges, ref_orient

pytestmark = pytest.mark.gpu

ANCHORS = {ANCHOR_FIRST: "first", ANCHOR_TOP: "top"}


def line(*xs):
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float64)


def unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def same(got, exp, what=""):
    """got: (normals, info) of R.orientnormals(return_info=True); exp: the twin's dict"""
    nrm, info = got
    assert np.array_equal(info["flip"], exp["flip"]), (what, int((info["flip"] != exp["flip"]).sum()))
    assert np.array_equal(info["component"], exp["component"]), what
    assert [info[f] for f in STATS] == [exp[f] for f in STATS], (what, [info[f] for f in STATS], [exp[f] for f in STATS])
    assert np.float64(info["min_tree_absdot"]).tobytes() == np.float64(exp["min_tree_absdot"]).tobytes(), what
    assert nrm.dtype == exp["normals"].dtype and nrm.tobytes() == exp["normals"].tobytes(), what
    assert info["n_tree_edges"] == info["n_vertices"] - info["n_components"]


def check(X, N, k, radius=0.0, anchor=ANCHOR_TOP, up=(0.0, 0.0, 1.0), what="", edges=None):
    """edges: edges_brute(X, N, k, radius) of an earlier call on the same cloud"""
    exp = ref_orient(X, N, k, radius, anchor, up) if edges is None else orient_from_edges(X, N, edges, anchor, up)
    same(R.orientnormals(X, N, k=k, radius=radius, anchor=ANCHORS[anchor], up=up, return_info=True), exp, what)
    return exp


# ------------------------------------------------------------------------- the hand cases ----
def test_hand_cases_through_the_c_abi():
    X = line(0.0, 1.0, 2.5)
    N = np.array([[0, 0, 1], [0.96, 0, 0.28], [-0.96, 0, 0.28]], dtype=np.float64)
    out, flip, comp = np.zeros((3, 3)), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    prm, st = L.OrientParams(k=2, anchor=L.ORI_ANCHOR_FIRST, radius=0.0), L.OrientStats()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.check(R.lib().rh_orient_normals(X.ctypes.data_as(dp), N.ctypes.data_as(dp), 3, C.byref(prm), 0, out.ctypes.data_as(dp),
                                      flip.ctypes.data_as(ip), comp.ctypes.data_as(ip), C.byref(st)))
    assert flip.tolist() == [0, 0, 1] and comp.tolist() == [1, 1, 1]       # the forest {1-2, 0-1}; {0-1, 0-2} gives [0, 0, 0]
    assert np.array_equal(out, N * [[1], [1], [-1]])
    assert (st.n_vertices, st.n_edges, st.n_components, st.n_tree_edges, st.n_flipped, st.n_inconsistent, st.largest_component,
            st.min_tree_absdot) == (3, 3, 1, 2, 1, 1, 3, 0.28)
    # outputs are optional
    out2 = np.zeros((3, 3))
    L.check(R.lib().rh_orient_normals(X.ctypes.data_as(dp), N.ctypes.data_as(dp), 3, C.byref(prm), 0, out2.ctypes.data_as(dp),
                                      None, None, None))
    assert np.array_equal(out2, out)
    for up in ((1, 0, 0), (-1, 0, 0), (0, 0, -1)):
        check(X, N, 2, anchor=ANCHOR_TOP, up=up, what=up)

    # n = 1 and n = 2
    for nr in ([[0, 0, -1]], [[0, 0, 0]], [[0.3, -0.4, 0.0]]):
        for a in ANCHORS:
            check(line(3.0), np.array(nr, dtype=np.float64), 4, anchor=a, what=nr)
    exp = check(line(0.0, 1.0), np.array([[0, 0, 1], [0, 0.6, -0.8]]), 1, anchor=ANCHOR_FIRST)
    assert exp["flip"].tolist() == [0, 1]
    # a zero normal between two points
    Z = np.array([[0, 0, 1], [0, 0, 0], [0, 0, -1]], dtype=np.float64)
    assert check(line(0.0, 1.0, 2.0), Z, 1, anchor=ANCHOR_FIRST)["component"].tolist() == [1, 0, 2]
    assert check(line(0.0, 1.0, 2.0), Z, 2, anchor=ANCHOR_FIRST)["flip"].tolist() == [0, -1, 1]
    # an isolated point that no point of the blob lists
    exp = check(line(0.0, 0.1, 0.2, 0.3, 100.0), np.array([[0, 0, 1]] * 4 + [[0, 0, -1]], dtype=np.float64), 2, anchor=ANCHOR_FIRST)
    assert exp["n_components"] == 1 and exp["flip"].tolist() == [0, 0, 0, 0, 1]
    # two blobs, numbered by smallest index
    B = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1]], dtype=np.float64)
    assert check(line(50.0, 0.0, 0.1, 50.1, 0.2, 50.2), B, 2, anchor=ANCHOR_FIRST)["component"].tolist() == [1, 2, 2, 1, 2, 1]
    # ANCHOR_TOP: a tie goes to the smaller index, a projection of 0 is kept
    T = np.array([[0, 0, 1], [1, 0, 1], [0.5, 0, 0]], dtype=np.float64)
    TN = np.array([[0.8, 0, 0.6], [0.8, 0, -0.6], [1, 0, 0]], dtype=np.float64)
    assert check(T, TN, 2)["flip"].tolist() == [0, 0, 0]
    assert check(T[[1, 0, 2]], TN[[1, 0, 2]], 2)["flip"].tolist() == [1, 1, 1]
    assert check(line(0.0, 1.0), np.array([[1, 0, -0.0], [1, 0, 0]]), 1)["flip"].tolist() == [0, 0]


# ------------------------------------------------------------------ wave and block edges ----
@pytest.mark.parametrize("k", [1, 2, 8, 63])
@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025])
def test_random_normals_at_wave_and_block_edges(n, k):
    """random unit normals are maximally frustrated: any deviation from the unique forest changes flips"""
    rng = np.random.default_rng(1000 * k + n)
    X = rng.uniform(0, 1, size=(n, 3))
    N = unit(rng.normal(size=(n, 3)))
    exp = check(X, N, k, anchor=ANCHOR_FIRST if n % 2 else ANCHOR_TOP, up=(0.3, -0.2, 0.9))
    assert exp["n_inconsistent"] > 0 or k == 1


def test_a_path_is_a_deep_tree():
    rng = np.random.default_rng(21)
    n = 2000
    X = np.stack([np.arange(n) + rng.uniform(-0.2, 0.2, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)], axis=1)
    X = X[rng.permutation(n)]
    N = unit(rng.normal(size=(n, 3)))
    exp = check(X, N, 2, anchor=ANCHOR_FIRST)
    assert exp["n_components"] == 1 and exp["n_tree_edges"] == n - 1


def test_exact_duplicates():
    rng = np.random.default_rng(22)
    X = rng.uniform(0, 1, size=(1000, 3))
    X[rng.choice(1000, 300, replace=False)] = X[0]
    N = unit(rng.normal(size=(1000, 3)))
    for k in (4, 16):
        check(X, N, k, what=k)


def test_shuffled_lattice_all_ties():
    rng = np.random.default_rng(23)
    g = np.arange(20, dtype=np.float64)
    X = np.stack([np.repeat(g, 20), np.tile(g, 20), np.zeros(400)], axis=1)[rng.permutation(400)]
    N = np.stack([np.zeros(400), np.zeros(400), rng.choice([-1.0, 1.0], size=400)], axis=1)
    for k in (2, 4, 8):
        for a in ANCHORS:
            exp = check(X, N, k, anchor=a, what=(k, a))
            assert exp["n_inconsistent"] == 0 and exp["n_components"] == 1 and len(set(exp["normals"][:, 2].tolist())) == 1


def test_two_blobs_a_thousand_diameters_apart():
    rng = np.random.default_rng(24)
    X = np.concatenate([rng.uniform(0, 1, size=(300, 3)), rng.uniform(0, 1, size=(200, 3)) + [1000.0, 0, 0]])[rng.permutation(500)]
    N = unit(rng.normal(size=(500, 3)))
    exp = check(X, N, 8)
    assert exp["n_components"] == 2 and exp["largest_component"] == 300
    assert check(X, N, 63, anchor=ANCHOR_FIRST)["n_components"] == 2
    # one point alone far away lists the blob and joins it
    X1 = np.concatenate([X[X[:, 0] < 500.0], [[1e5, 0.0, 0.0]]])
    assert check(X1, N[:301], 4)["n_components"] == 1


def test_a_radius_cuts_the_graph_into_many_components():
    rng = np.random.default_rng(25)
    X = rng.uniform(0, 1, size=(1500, 3))
    N = unit(rng.normal(size=(1500, 3)))
    N[::50] = 0.0
    exp = check(X, N, 8, radius=0.05, up=(-0.5, 0.5, 0.1))
    assert exp["n_components"] > 100 and exp["n_vertices"] == 1500 - 30 and exp["largest_component"] > 3
    assert (exp["flip"][::50] == -1).all()


@pytest.mark.parametrize("anchor", [ANCHOR_FIRST, ANCHOR_TOP])
def test_noisy_sphere_both_anchors_and_an_oblique_up(anchor):
    rng = np.random.default_rng(26)
    p = unit(rng.normal(size=(2000, 3)))
    nr = unit(p + 0.05 * rng.normal(size=(2000, 3)))
    big = np.argmax(np.abs(nr), axis=1)
    nr *= np.where(nr[np.arange(2000), big] < 0, -1.0, 1.0)[:, None]           # the canonical sign of rh_estimate_normals
    X = p * 3.0 + 7.0
    e = edges_brute(X, nr, 10)
    for up in ((0, 0, 1), (0.6, -0.64, 0.48), (-1e-3, 0, 0)):
        exp = check(X, nr, 10, anchor=anchor, up=up, what=up, edges=e)
        assert exp["n_components"] == 1 and exp["n_inconsistent"] == 0
        out = np.einsum("ij,ij->i", p, exp["normals"]) > 0
        assert out.all() if anchor == ANCHOR_TOP else (out.all() or not out.any())


def test_float32_in_and_out():
    rng = np.random.default_rng(27)
    X = rng.uniform(0, 1, size=(700, 3)).astype(np.float32)
    N = unit(rng.normal(size=(700, 3))).astype(np.float32)
    N[5] = 0.0
    for a in ANCHORS:
        exp = check(X, N, 7, anchor=a, up=(0.1, 0.2, 0.3), what=a)
        assert exp["normals"].dtype == np.float32
        # the float32 entry is the binary64 call on the widened arrays
        wide = R.orientnormals(X.astype(np.float64), N.astype(np.float64), k=7, anchor=ANCHORS[a], up=(0.1, 0.2, 0.3), return_info=True)
        assert np.array_equal(wide[1]["flip"], exp["flip"]) and np.array_equal(wide[0].astype(np.float32), exp["normals"])


def _dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


def test_device_pointers_in_place_and_two_runs():
    rng = np.random.default_rng(28)
    n = 1200
    X = rng.uniform(0, 1, size=(n, 3))
    N = unit(rng.normal(size=(n, 3)))
    exp = ref_orient(X, N, 9, anchor=ANCHOR_TOP, up=(0.0, 1.0, 0.0))
    a = R.orientnormals(X, N, k=9, up=(0, 1, 0), return_info=True)
    b = R.orientnormals(X, N, k=9, up=(0, 1, 0), return_info=True)
    same(a, exp)
    assert a[0].tobytes() == b[0].tobytes() and a[1]["flip"].tobytes() == b[1]["flip"].tobytes()
    assert a[1]["component"].tobytes() == b[1]["component"].tobytes() and [a[1][f] for f in STATS] == [b[1][f] for f in STATS]
    # device pointers in and out
    prm, st = L.OrientParams(k=9, anchor=L.ORI_ANCHOR_TOP, radius=0.0), L.OrientStats()
    prm.up[:] = [0.0, 1.0, 0.0]
    d_x, d_n = torch.from_numpy(X).cuda(), torch.from_numpy(N).cuda()
    d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_flip = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_comp = torch.zeros(n, dtype=torch.int32, device="cuda")
    L.check(R.lib().rh_orient_normals(_dptr(d_x, C.c_double), _dptr(d_n, C.c_double), n, C.byref(prm), 0, _dptr(d_out, C.c_double),
                                      _dptr(d_flip, C.c_int32), _dptr(d_comp, C.c_int32), C.byref(st)))
    torch.cuda.synchronize()
    same((d_out.cpu().numpy(), dict({f: getattr(st, f) for f, _ in L.OrientStats._fields_}, flip=d_flip.cpu().numpy(),
                                    component=d_comp.cpu().numpy())), exp)
    assert np.array_equal(d_n.cpu().numpy(), N)                             # the input is left alone
    # in place, device and host
    L.check(R.lib().rh_orient_normals(_dptr(d_x, C.c_double), _dptr(d_n, C.c_double), n, C.byref(prm), 0, _dptr(d_n, C.c_double),
                                      None, None, None))
    torch.cuda.synchronize()
    assert d_n.cpu().numpy().tobytes() == exp["normals"].tobytes()
    h = N.copy()
    dp = C.POINTER(C.c_double)
    L.check(R.lib().rh_orient_normals(X.ctypes.data_as(dp), h.ctypes.data_as(dp), n, C.byref(prm), 0, h.ctypes.data_as(dp), None, None, None))
    assert h.tobytes() == exp["normals"].tobytes()


def test_bad_values_are_found_on_the_device_and_nothing_is_written():
    rng = np.random.default_rng(29)
    X = rng.uniform(0, 1, size=(300, 3))
    N = unit(rng.normal(size=(300, 3)))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    prm = L.OrientParams(k=4, anchor=L.ORI_ANCHOR_FIRST, radius=0.0)
    for where, at, val in (("x", (299, 2), np.nan), ("x", (0, 0), np.inf), ("n", (257, 1), np.nan), ("n", (3, 0), -np.inf),
                           ("n", (100, 2), 2.0000000000000004), ("n", (100, 2), -3.0)):
        x, nr = X.copy(), N.copy()
        (x if where == "x" else nr)[at] = val
        out, flip, st = np.full((300, 3), -7.0), np.full(300, -7, dtype=np.int32), L.OrientStats(n_edges=-7)
        rc = R.lib().rh_orient_normals(x.ctypes.data_as(dp), nr.ctypes.data_as(dp), 300, C.byref(prm), 0, out.ctypes.data_as(dp),
                                       flip.ctypes.data_as(ip), None, C.byref(st))
        assert rc == L.RH_E_INVALID, (where, at, val)
        assert (out == -7.0).all() and (flip == -7).all() and st.n_edges == -7
    nr = N.copy()
    nr[100] = [2.0, -2.0, 2.0]                                             # 2 itself is allowed
    check(X, nr, 4, anchor=ANCHOR_FIRST)


# ------------------------------------------------------------------------------ mid size ----
def _mid_scene():
    rng = np.random.default_rng(30)
    m = 10_000
    s = unit(rng.normal(size=(m, 3)))
    ang, hgt = rng.uniform(0, 2 * np.pi, m), rng.uniform(-2, 2, m)
    cyl_n = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    parts = [(s * 1.5 + [0, 0, 4], s),
             (cyl_n * 0.8 + np.stack([np.zeros(m), np.zeros(m), hgt], axis=1) + [5, 0, 0], cyl_n),
             (np.stack([rng.uniform(-4, 4, m), rng.uniform(-4, 4, m), np.full(m, -3.0)], axis=1), np.tile([0.0, 0, 1], (m, 1))),
             (np.stack([np.full(m, -5.0), rng.uniform(-4, 4, m), rng.uniform(-4, 4, m)], axis=1), np.tile([1.0, 0, 0], (m, 1)))]
    X = np.concatenate([p for p, _ in parts] + [rng.uniform(-6, 7, size=(m, 3))])
    N = np.concatenate([unit(q + 0.03 * rng.normal(size=q.shape)) for _, q in parts] + [unit(rng.normal(size=(m, 3)))])
    big = np.argmax(np.abs(N), axis=1)
    N *= np.where(N[np.arange(len(N)), big] < 0, -1.0, 1.0)[:, None]
    perm = rng.permutation(len(X))
    return X[perm], N[perm]


def test_mid_size_scene_against_kruskal_on_the_librarys_own_lists():
    """50 000 points: a sphere, a cylinder, two planes and 20 % clutter with random normals, k = 12.  The edges come from
    R.knn's lists (which have parity tests of their own), the forest from the twin's Kruskal."""
    X, N = _mid_scene()
    e = edges_from_lists(R.knn(X, 12, return_dist=False), N)
    for anchor, up in ((ANCHOR_TOP, (0.0, 0.0, 1.0)), (ANCHOR_FIRST, (0.0, 0.0, 1.0))):
        exp = orient_from_edges(X, N, e, anchor, up)
        same(R.orientnormals(X, N, k=12, anchor=ANCHORS[anchor], up=up, return_info=True), exp, anchor)
        assert exp["n_edges"] > 300_000 and exp["n_inconsistent"] > 1000 and exp["largest_component"] > 40_000


# ---------------------------------------------------------------------------- end to end ----
def _e2e_scene():
    rng = np.random.default_rng(7)
    ns = npl = 3000
    p = unit(rng.normal(size=(ns, 3)))
    pl = np.stack([rng.uniform(-2, 2, npl), rng.uniform(-2, 2, npl), np.zeros(npl)], axis=1)
    X = np.concatenate([p + [0, 0, 2.5], pl])
    A = np.concatenate([p, np.tile([0.0, 0, 1], (npl, 1))])
    perm = rng.permutation(len(X))
    return X[perm], A[perm]


def test_estimatenormals_consistent_and_ransac_on_the_result():
    """A noise-free unit sphere above a plane, no viewpoint: consistent=True is the estimate followed by orientnormals, it
    agrees with the analytic outward normals at EVERY point, and ransac() extracts the sphere with the same inliers as on
    normals oriented by hints = the analytic normals."""
    X, A = _e2e_scene()
    k = 12
    canon, flags = R.estimatenormals(X, k=k, return_flags=True)
    assert not flags.any()
    cons = R.estimatenormals(X, k=k, consistent=True)
    two, info = R.orientnormals(X, canon, k=k, return_info=True)
    assert cons.tobytes() == two.tobytes()
    cons2, flags2 = R.estimatenormals(X, k=k, consistent=True, return_flags=True)
    assert cons2.tobytes() == cons.tobytes() and np.array_equal(flags2, flags)
    # the twin on the library's lists: the same flips, and they agree with the analytic signs at every point
    exp = orient_from_edges(X, canon, edges_from_lists(R.knn(X, k, return_dist=False), canon), ANCHOR_TOP, (0.0, 0.0, 1.0))
    same((two, info), exp)
    assert exp["n_components"] == 2 and exp["n_inconsistent"] == 0
    assert int((np.einsum("ij,ij->i", exp["normals"], A) <= 0).sum()) == 0
    assert 0.2 < (np.einsum("ij,ij->i", canon, A) < 0).mean() < 0.8          # the canonical sign alone is wrong on many
    hinted = R.estimatenormals(X, k=k, hints=A)
    assert hinted.tobytes() == cons.tobytes()

    subs = synth.make_subsets(len(X), 4, seed=3)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere], iteration={"minsubsetN": 30, "itermax": 100, "τ": 300, "prob_det": 0.9})
    cp = R.params_to_c(params)

    def spheres(normals):
        got, _ = R.ransac(R.RANSACCloud(X, normals, subs), cp, seed=1234)
        return [g for g in got if g.c_shape.kind == L.SPHERE]

    a, b = spheres(cons), spheres(hinted)
    assert len(a) == len(b) == 1 and np.array_equal(a[0].inpoints, b[0].inpoints) and len(a[0].inpoints) > 2000
