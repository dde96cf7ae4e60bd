"""Consistent normal orientation (rh_orient_normals, include/ransac_hip.h), CPU side: the numpy twin of
tests/orient_reference.py pinned by hand-derived cases with the expected flips written out, a property of the definition
checked on the twin, the ABI declarations and the argument checks that come before the device is opened.
tests/test_orient_gpu.py holds the library to the twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from orient_reference import (ANCHOR_FIRST, ANCHOR_TOP, boruvka_parity, edges_brute, edges_from_lists, orient_from_edges,
                              ref_orient)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(*xs):
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float64)


def sphere_case(n=600, noise=0.05, seed=1):
    """points on the unit sphere; their outward normals with Gaussian noise, renormalised, in the canonical sign of
    rh_estimate_normals (the component of largest magnitude positive)"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1)[:, None]
    nr = p + noise * rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    big = np.argmax(np.abs(nr), axis=1)
    nr *= np.where(nr[np.arange(n), big] < 0, -1.0, 1.0)[:, None]
    return p, nr


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_frustrated_triangle_takes_the_unique_forest():
    """dots 0.28 (0-1), 0.28 (0-2), -0.8432 (1-2): the forest is {1-2, 0-1}, 0-1 winning the tie over 0-2 by index.  With
    the tree {0-1, 0-2} the flips would be [0, 0, 0]."""
    X = line(0.0, 1.0, 2.5)
    N = np.array([[0, 0, 1], [0.96, 0, 0.28], [-0.96, 0, 0.28]], dtype=np.float64)
    e = edges_brute(X, N, 2)
    assert e.tolist() == [[0, 1], [0, 2], [1, 2]]
    r = orient_from_edges(X, N, e, ANCHOR_FIRST)
    assert r["tree"].tolist() == [[1, 2], [0, 1]]
    assert r["flip"].tolist() == [0, 0, 1] and r["component"].tolist() == [1, 1, 1]
    assert np.array_equal(r["normals"], N * [[1], [1], [-1]])
    assert (r["n_vertices"], r["n_edges"], r["n_components"], r["n_tree_edges"], r["n_flipped"], r["n_inconsistent"],
            r["largest_component"]) == (3, 3, 1, 2, 1, 1, 3)                # 0-2 is left frustrated: a non-tree edge
    assert r["min_tree_absdot"] == 0.28
    # anchored at the top along +x: point 2, whose normal points down the axis: want = 1, par = [0, 0, 1] -> the same flips
    r = orient_from_edges(X, N, e, ANCHOR_TOP, up=(1, 0, 0))
    assert r["flip"].tolist() == [0, 0, 1]
    # along -x the top is point 0, n0 . up = 0 is kept; along -z it is point 0 as well (every t is -0.0 + 0.0), turned over
    assert orient_from_edges(X, N, e, ANCHOR_TOP, up=(-1, 0, 0))["flip"].tolist() == [0, 0, 1]
    assert orient_from_edges(X, N, e, ANCHOR_TOP, up=(0, 0, -1))["flip"].tolist() == [1, 1, 0]


def test_all_ties_lattice_ends_on_one_side():
    """every a is 1: the forest comes from the index order alone"""
    g = np.arange(20, dtype=np.float64)
    X = np.stack([np.repeat(g, 20), np.tile(g, 20), np.zeros(400)], axis=1)
    sign = np.random.default_rng(5).choice([-1.0, 1.0], size=400)
    N = np.stack([np.zeros(400), np.zeros(400), sign], axis=1)
    for k in (2, 4, 8):
        r = ref_orient(X, N, k, anchor=ANCHOR_FIRST)
        assert r["n_components"] == 1 and r["n_inconsistent"] == 0 and r["n_tree_edges"] == 399
        assert (r["normals"][:, 2] == sign[0]).all() and r["min_tree_absdot"] == 1.0
        assert np.array_equal(r["flip"], (sign != sign[0]).astype(np.int32))
        r = ref_orient(X, N, k, anchor=ANCHOR_TOP)                          # every t is 0: the anchor is point 0, turned up
        assert (r["normals"][:, 2] == 1.0).all() and r["n_flipped"] == int((sign < 0).sum())


def test_one_and_two_points():
    r = ref_orient(line(3.0), [[0, 0, -1]], 4, anchor=ANCHOR_FIRST)
    assert r["flip"].tolist() == [0] and r["component"].tolist() == [1] and r["min_tree_absdot"] == float("inf")
    assert (r["n_vertices"], r["n_edges"], r["n_components"], r["n_tree_edges"], r["largest_component"]) == (1, 0, 1, 0, 1)
    r = ref_orient(line(3.0), [[0, 0, -1]], 4, anchor=ANCHOR_TOP)
    assert r["flip"].tolist() == [1] and r["normals"].tolist() == [[0, 0, 1]]
    r = ref_orient(line(3.0), [[0, 0, 0]], 4)
    assert r["flip"].tolist() == [-1] and r["component"].tolist() == [0] and r["n_vertices"] == 0 and r["n_components"] == 0
    assert r["largest_component"] == 0
    r = ref_orient(line(0.0, 1.0), [[0, 0, 1], [0, 0.6, -0.8]], 1, anchor=ANCHOR_FIRST)
    assert r["flip"].tolist() == [0, 1] and r["n_edges"] == 1 and r["n_tree_edges"] == 1 and r["min_tree_absdot"] == 0.8
    assert r["normals"].tolist() == [[0, 0, 1], [-0.0, -0.6, 0.8]] and r["n_inconsistent"] == 0


def test_a_zero_normal_between_two_points_does_not_connect_them():
    X = line(0.0, 1.0, 2.0)
    N = np.array([[0, 0, 1], [0, 0, 0], [0, 0, -1]], dtype=np.float64)
    r = ref_orient(X, N, 1, anchor=ANCHOR_FIRST)                             # 0 and 2 list 1, 1 lists 0
    assert r["n_edges"] == 0 and r["component"].tolist() == [1, 0, 2] and r["flip"].tolist() == [0, -1, 0]
    assert np.array_equal(r["normals"], N) and r["n_vertices"] == 2 and r["n_components"] == 2
    r = ref_orient(X, N, 2, anchor=ANCHOR_FIRST)                             # with k = 2 they list each other
    assert r["n_edges"] == 1 and r["component"].tolist() == [1, 0, 1] and r["flip"].tolist() == [0, -1, 1]


def test_an_isolated_point_joins_through_its_own_list_only():
    """the point at 100 lists two points of the blob, no point of the blob lists it"""
    X = line(0.0, 0.1, 0.2, 0.3, 100.0)
    N = np.array([[0, 0, 1]] * 4 + [[0, 0, -1]], dtype=np.float64)
    e = edges_brute(X, N, 2)
    assert [3, 4] in e.tolist() and [2, 4] in e.tolist()
    r = orient_from_edges(X, N, e, ANCHOR_FIRST)
    assert r["n_components"] == 1 and r["flip"].tolist() == [0, 0, 0, 0, 1]


def test_two_far_blobs_are_numbered_by_smallest_index():
    X = line(50.0, 0.0, 0.1, 50.1, 0.2, 50.2)
    N = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1]], dtype=np.float64)
    r = ref_orient(X, N, 2, anchor=ANCHOR_FIRST)
    assert r["component"].tolist() == [1, 2, 2, 1, 2, 1] and r["n_components"] == 2 and r["largest_component"] == 3
    assert r["flip"].tolist() == [0, 0, 1, 1, 1, 0]


def test_anchor_top_ties_and_a_projection_of_zero():
    X = np.array([[0, 0, 1], [1, 0, 1], [0.5, 0, 0]], dtype=np.float64)      # 0 and 1 tie at the top: 0 is the anchor
    N = np.array([[0.8, 0, 0.6], [0.8, 0, -0.6], [1, 0, 0]], dtype=np.float64)
    r = ref_orient(X, N, 2, anchor=ANCHOR_TOP)
    assert r["flip"].tolist() == [0, 0, 0]                                  # (anchored at 1, want = 1: all three turned)
    r = ref_orient(X[[1, 0, 2]], N[[1, 0, 2]], 2, anchor=ANCHOR_TOP)
    assert r["flip"].tolist() == [1, 1, 1]
    r = ref_orient(line(0.0, 1.0), [[1, 0, 0], [1, 0, 0]], 1, anchor=ANCHOR_TOP)       # n . up == 0: kept
    assert r["flip"].tolist() == [0, 0]
    r = ref_orient(line(0.0, 1.0), [[1, 0, -0.0], [1, 0, 0]], 1, anchor=ANCHOR_TOP)    # -0.0 is not < 0
    assert r["flip"].tolist() == [0, 0]


def test_edges_from_lists_is_edges_brute():
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, size=(200, 3))
    N = rng.normal(size=(200, 3))
    N[::17] = 0.0
    k = 5
    dx, dy, dz = (X[None, :, a] - X[:, None, a] for a in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    np.fill_diagonal(d, -1.0)
    idx = np.argsort(d, axis=1, kind="stable")[:, 1:k + 1] + 1
    e = edges_from_lists(idx, N)
    assert np.array_equal(e, edges_brute(X, N, k))
    assert (e[:, 0] < e[:, 1]).all() and not (N[e.ravel()] == 0).all(axis=1).any()
    assert np.array_equal(np.unique(e, axis=0), e)
    idx[:, 3:] = 0                                                           # lists cut short: the first three of every row
    assert np.array_equal(edges_from_lists(idx, N), edges_brute(X, N, 3))


# ------------------------------------------------------- a property of the definition ----
def test_sphere_with_canonical_signs_comes_out_outward():
    p, nr = sphere_case()
    assert 0.3 < (np.einsum("ij,ij->i", p, nr) > 0).mean() < 0.7            # the canonical sign is wrong on about half
    e = edges_brute(p, nr, 8)
    r = orient_from_edges(p, nr, e, ANCHOR_TOP)
    print("sphere: %d edges, %d components, %d inconsistent, min_tree_absdot %.3f, outward %.3f"
          % (len(e), r["n_components"], r["n_inconsistent"], r["min_tree_absdot"], (np.einsum("ij,ij->i", p, r["normals"]) > 0).mean()))
    assert r["n_components"] == 1 and r["n_inconsistent"] == 0
    assert (np.einsum("ij,ij->i", p, r["normals"]) > 0).all()
    assert r["min_tree_absdot"] > 0.9
    # rounds of smallest-outgoing-edge picks with parity links reproduce Kruskal's parities, in a handful of rounds
    root, par, rounds = boruvka_parity(len(p), e, nr)
    assert len(set(root.tolist())) == 1 and 2 <= rounds <= 10
    flip = r["flip"]
    assert ((par ^ par[0]) == (flip ^ flip[0])).all()


def test_boruvka_rounds_reproduce_kruskal_on_frustrated_graphs():
    rng = np.random.default_rng(9)
    for n, k in ((40, 1), (97, 3), (150, 6)):
        X = rng.uniform(0, 1, size=(n, 3))
        N = rng.normal(size=(n, 3))
        N[::13] = 0.0
        e = edges_brute(X, N, k)
        r = orient_from_edges(X, N, e, ANCHOR_FIRST)
        root, par, _ = boruvka_parity(n, e, N)
        v = r["component"] > 0
        for c in range(1, r["n_components"] + 1):
            mem = np.flatnonzero(r["component"] == c)
            assert len(set(root[mem].tolist())) == 1
            assert ((par[mem] ^ par[mem[0]]) == r["flip"][mem]).all()        # ANCHOR_FIRST: the smallest index is kept
        assert len(set(root[v].tolist())) == r["n_components"]


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_orient_normals", "rh_orient_normals_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_orient_params\s*;", src) and re.search(r"}\s*rh_orient_stats\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 121
    assert R.lib().rh_version() >= 121
    assert re.search(r"RH_ORI_ANCHOR_FIRST\s*=\s*0\s*,\s*RH_ORI_ANCHOR_TOP\s*=\s*1", src)
    assert (L.ORI_ANCHOR_FIRST, L.ORI_ANCHOR_TOP) == (ANCHOR_FIRST, ANCHOR_TOP) == (0, 1)


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["k", "anchor", "radius", "up"]
    sf = ["n_vertices", "n_edges", "n_components", "n_tree_edges", "n_flipped", "n_inconsistent", "largest_component",
          "min_tree_absdot"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_orient_params), sizeof(rh_orient_stats));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_orient_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_orient_stats, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.OrientParams), C.sizeof(L.OrientStats)]
    mine += [getattr(L.OrientParams, f).offset for f in pf] + [getattr(L.OrientStats, f).offset for f in sf]
    assert got == mine and got[:2] == [40, 64]
    assert [f for f, _ in L.OrientStats._fields_] == sf


def test_python_and_julia_names_are_exported():
    assert callable(R.orientnormals) and "orientnormals" in R.__all__
    jl = open(os.path.join(ROOT, "julia", "RANSACHIP.jl")).read()
    assert re.search(r"^function orientnormals\(", jl, re.M)
    assert "rh_orient_normals_f32" in jl and "struct RhOrientParams" in jl and "struct RhOrientStats" in jl
    with pytest.raises(ValueError):
        R.orientnormals(np.zeros((8, 3)), np.ones((8, 3)), anchor="bottom")
    with pytest.raises(ValueError):
        R.orientnormals(np.zeros((8, 3)), np.ones((7, 3)))
    with pytest.raises(ValueError):
        R.estimatenormals(np.zeros((8, 3)), consistent=True, viewpoint=(0, 0, 9))
    with pytest.raises(ValueError):
        R.estimatenormals(np.zeros((8, 3)), consistent=True, hints=np.ones((8, 3)))


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    xyz, nrm = np.zeros((8, 3)), np.ones((8, 3))
    inf, nan = float("inf"), float("nan")
    for dt in (np.float64, np.float32):
        x, nr = xyz.astype(dt), nrm.astype(dt)
        for kw in (dict(k=0), dict(k=-3), dict(k=64), dict(radius=-1.0), dict(radius=inf), dict(radius=nan), dict(anchor=2),
                   dict(anchor=-1), dict(up=(0, 0, 0)), dict(up=(0, inf, 1)), dict(up=(nan, 0, 1)), dict(up=(-0.0, 0.0, 0.0))):
            with pytest.raises(R.RansacHipError) as e:
                R.orientnormals(x, nr, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        with pytest.raises(R.RansacHipError) as e:
            R.orientnormals(x[:0], nr[:0])
        assert e.value.code == L.RH_E_INVALID
    lib = R.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    px, pn = xyz.ctypes.data_as(dp), nrm.ctypes.data_as(dp)
    out, flip = np.full((8, 3), -7.0), np.full(8, -7, dtype=np.int32)
    po, pf = out.ctypes.data_as(dp), flip.ctypes.data_as(i32p)
    prm, st = L.OrientParams(k=4, anchor=L.ORI_ANCHOR_FIRST, radius=0.0), L.OrientStats(n_edges=-7)
    fn = lib.rh_orient_normals
    assert fn(None, pn, 8, C.byref(prm), 0, po, pf, None, C.byref(st)) == L.RH_E_INVALID
    assert fn(px, None, 8, C.byref(prm), 0, po, pf, None, C.byref(st)) == L.RH_E_INVALID
    assert fn(px, pn, 8, None, 0, po, pf, None, C.byref(st)) == L.RH_E_INVALID
    assert fn(px, pn, 8, C.byref(prm), 0, None, pf, None, C.byref(st)) == L.RH_E_INVALID
    for n in (0, -1, 2 ** 31 - 1, 2 ** 31, 2 ** 40):                         # (n is refused before anything is read through xyz)
        assert fn(px, pn, n, C.byref(prm), 0, po, pf, None, C.byref(st)) == L.RH_E_INVALID, n
    assert fn(px, pn, 2 ** 29, C.byref(prm), 0, po, pf, None, C.byref(st)) == L.RH_E_INVALID    # n * k = 2^31 directed pairs
    assert (out == -7.0).all() and (flip == -7).all() and st.n_edges == -7   # nothing was written
    assert b"rh_orient_normals" in lib.rh_last_error()
    # an all-zero up is fine when the anchor does not use it: the call gets as far as the device
    n = C.c_int()
    has_gpu = lib.rh_device_count(C.byref(n)) == 0 and n.value > 0
    prm = L.OrientParams(k=4, anchor=L.ORI_ANCHOR_FIRST, radius=0.0)
    assert fn(px, pn, 8, C.byref(prm), 0, po, pf, None, C.byref(st)) == (L.RH_OK if has_gpu else L.RH_E_NODEVICE)


def test_a_valid_call_fails_loudly_without_gpu():
    n = C.c_int()
    if R.lib().rh_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    for dt in (np.float64, np.float32):
        with pytest.raises(R.RansacHipError) as e:
            R.orientnormals(np.zeros((8, 3), dtype=dt), np.ones((8, 3), dtype=dt))
        assert e.value.code == L.RH_E_NODEVICE
        with pytest.raises(R.RansacHipError) as e:
            R.estimatenormals(np.random.default_rng(0).uniform(size=(8, 3)).astype(dt), k=4, consistent=True)
        assert e.value.code == L.RH_E_NODEVICE
