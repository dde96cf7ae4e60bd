"""Global registration (rh_describe, rh_match_features, rh_register_global; include/ransac_hip.h), CPU side: the numpy twins
of tests/global_reference.py pinned by hand-derived cases, the condition of the whole chain on the scene of
tests/global_scene.py, and the ABI declarations.  tests/test_global_gpu.py holds the library to the twins, byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
import global_reference as G
import global_scene as GS
from register_reference import apply
from test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = [0.0, 0.0, 1.0]


def _pair(pj, nj, pi=(0.0, 0.0, 0.0), ni=Z):
    f1, f2, psi, deg = G.ref_pair(np.array(pi), np.array(ni), np.array(pj), np.array(nj))
    return float(f1), float(f2), float(psi), bool(deg)


# ------------------------------------------------------------------ 1. pair features by hand ----
def test_pair_features_by_hand():
    """p_i = 0, n_i = e_z, p_j = e_x, n_j = e_z: d = e_x, v = e_z x e_x = e_y, w = e_z x e_y = -e_x; f1 = u.d = 0, f2 = v.s = 0,
    a = w.s = 0, b = u.s = 1, g = 1, r = 1, psi = 1 - 1 = 0.  Bins floor(1 * 5.5) = 5, 5 and floor(0) = 0."""
    f1, f2, psi, deg = _pair([1.0, 0.0, 0.0], Z)
    assert (f1, f2, psi, deg) == (0.0, 0.0, 0.0, False)
    assert [int(b) for b in G.ref_bins(f1, f2, psi)] == [5, 5, 0]
    # n_j = e_x: a = w.s = -1 < 0, b = 0, r = 0, psi = 3; n_j = -e_x: a = 1, psi = 1; n_j = -e_z: b = -1, a = 0 (as -0.0 >= 0), psi = 2
    assert _pair([1.0, 0.0, 0.0], [1.0, 0.0, 0.0])[2] == 3.0
    assert _pair([1.0, 0.0, 0.0], [-1.0, 0.0, 0.0])[2] == 1.0
    assert _pair([1.0, 0.0, 0.0], [0.0, 0.0, -1.0])[2] == 2.0
    assert [int(G.ref_bin(p * 2.75)) for p in (1.0, 2.0, 3.0)] == [2, 5, 8]
    # d = (3, 0, 4): len = 5, f1 = 4 / 5; v = e_z x d = (0, 3, 0), vl = 3, f2 = 0
    f1, f2, psi, deg = _pair([3.0, 0.0, 4.0], Z)
    assert (f1, f2, psi, deg) == (0.8, 0.0, 0.0, False) and int(G.ref_bin((f1 + 1.0) * 5.5)) == 9


def test_every_degenerate_clause():
    assert _pair([0.0, 0.0, 0.0], Z)[3]                              # d2 == 0: a duplicate
    assert _pair([0.0, 0.0, 2.0], Z)[3]                              # v2 == 0: the neighbour lies along the normal
    assert _pair([1.0, 0.0, 0.0], Z, ni=[0.0, 0.0, 0.0])[3]          # v2 == 0: a zero normal at i
    assert _pair([1.0, 0.0, 0.0], [0.0, 1.0, 0.0])[3]                # g == 0: n_j along v, a = b = 0 (and psi = 0/0 is NaN)
    assert _pair([1.0, 0.0, 0.0], [0.0, 0.0, 0.0])[3]                # g == 0: a zero normal at j
    big = 1e200                                                      # f1 = (inf - inf) / len is NaN while d2, v2 and g are not 0
    f1, f2, psi, deg = _pair([big, 0.0, big], Z, ni=[big, 0.0, -big])
    assert np.isnan(f1) and deg
    assert not _pair([1.0, 0.0, 0.0], Z)[3]


def test_bin_edges_and_clamping():
    assert [int(G.ref_bin(x)) for x in (5.0, np.nextafter(5.0, 0.0), 0.0, -0.0, -1e-300, 11.0, 10.999, 1e300, -1e300, np.inf)] \
        == [5, 4, 0, 0, 0, 10, 10, 10, 0, 10]
    # the edge of psi at a = 0: a = +1e-30 gives psi = 1 - 1 = 0, bin 0; a = -1e-30 gives psi = 3 + 1 = 4.0 (rounded up to
    # the end of the range), psi * 2.75 = 11, clamped to bin 10
    lo = _pair([1.0, 0.0, 0.0], [-1e-30, 0.0, 1.0])
    hi = _pair([1.0, 0.0, 0.0], [1e-30, 0.0, 1.0])
    assert (lo[2], hi[2]) == (0.0, 4.0) and not lo[3] and not hi[3]
    assert (int(G.ref_bin(lo[2] * 2.75)), int(G.ref_bin(hi[2] * 2.75))) == (0, 10)
    # a normal of length 2 at j: f2 = v.s / vl = 2, (2 + 1) * 5.5 = 16.5 -> 10; at i: f1 = u.d / len = 2 * 0.8 = 1.6 -> floor(14.3) -> 10
    f1, f2, psi, deg = _pair([1.0, 0.0, 0.0], [0.0, 2.0, 1.0])
    assert (f2, deg) == (2.0, False) and int(G.ref_bin((f2 + 1.0) * 5.5)) == 10
    f1, f2, psi, deg = _pair([3.0, 0.0, 4.0], Z, ni=[0.0, 0.0, 2.0])
    assert (f1, deg) == (1.6, False) and int(G.ref_bin((f1 + 1.0) * 5.5)) == 10
    f1 = _pair([3.0, 0.0, -4.0], Z, ni=[0.0, 0.0, 2.0])[0]
    assert f1 == -1.6 and int(G.ref_bin((f1 + 1.0) * 5.5)) == 0


def test_descriptor_of_five_points_written_out():
    """Five points on the x axis, all normals e_z, k = 2, radius 2.5: every pair that is not degenerate has f1 = f2 = psi = 0,
    bins 5, 11 + 5, 22 + 0.  Lists: 0 -> (1, 2); 1 -> (2 at d2 = 0: degenerate, 0); 2 -> (1: degenerate, 0); 3 -> (1, 2);
    4 -> nobody within 2.5.  S = 2, 1, 1, 2, 0 and D_i = count_i * S_i + the neighbours' S: 4 + 2, 2 + 3, 2 + 3, 4 + 2, 0."""
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [10.0, 0, 0]])
    nrm = np.tile(Z, (5, 1))
    D, count, S = G.ref_describe(pts, nrm, 2, radius=2.5)
    assert count.tolist() == [2, 2, 2, 2, 0]
    exp = np.zeros((5, 33), dtype=np.uint16)
    exp[:, [5, 16, 22]] = np.array([6, 5, 5, 6, 0], dtype=np.uint16)[:, None]
    assert D.dtype == np.uint16 and np.array_equal(D, exp)
    assert S[:, 5].tolist() == [2, 1, 1, 2, 0]
    # the largest value any entry can take: k = 63 and every pair in one bin
    line = np.zeros((64, 3))
    line[:, 0] = np.arange(64)
    D, count, _ = G.ref_describe(line, np.tile(Z, (64, 1)), 63)
    assert count.tolist() == [63] * 64 and int(D.max()) == 2 * 63 * 63 == G.DESC_MAX == L.DESC_MAX


def test_a_rigid_motion_moves_values_between_bins_only():
    """In exact arithmetic D does not change under a motion of points and normals.  In floating point a pair on a bin
    edge -- on the scene's planes, where every normal is the same, a = +-0 puts psi at 0 or at 4 -- can change its bin;
    which pairs are degenerate does not change, so the three groups of 11 bins keep their sums exactly."""
    s = GS.make()
    a, ca, _ = G.ref_describe(s["truth"][:600], s["qry_nrm"][:600] @ s["motion"][:, :3], 16)
    b, cb, _ = G.ref_describe(s["qry"][:600], s["qry_nrm"][:600], 16)
    moved = np.abs(a.astype(int) - b.astype(int)).sum(axis=1)
    print("rows changed by the motion: %d of 600, largest L1 change %d" % ((moved > 0).sum(), moved.max()))
    assert np.array_equal(ca, cb)
    for g in range(3):
        assert np.array_equal(a[:, 11 * g:11 * g + 11].astype(int).sum(axis=1), b[:, 11 * g:11 * g + 11].astype(int).sum(axis=1))
    assert np.array_equal(a[:, :11].astype(int).sum(axis=1), 2 * 16 * 16 * np.ones(600, dtype=int))   # no pair is degenerate here


# ------------------------------------------------------------------------------ 2. matching ----
def test_sqdist_is_the_literal_integer_sum():
    rng = np.random.default_rng(2)
    r = rng.integers(0, G.DESC_MAX + 1, size=(50, 33)).astype(np.uint16)
    q = rng.integers(0, G.DESC_MAX + 1, size=(40, 33)).astype(np.uint16)
    r[0], q[0], q[1] = 0, G.DESC_MAX, 0
    lit = ((q[:, None, :].astype(np.int64) - r[None, :, :].astype(np.int64)) ** 2).sum(axis=2)
    assert np.array_equal(G.ref_sqdist(r, q), lit) and lit[0, 0] == 33 * G.DESC_MAX ** 2 < 2 ** 31


def _rows(first):
    d = np.zeros((len(first), 33), dtype=np.uint16)
    d[:, 0] = first
    return d


def test_match_ties_go_to_the_smaller_index():
    ref = _rows([7, 3, 7, 3, 5])
    idx, dist = G.ref_match(ref, _rows([3, 7, 5, 4, 6]))
    assert idx.tolist() == [2, 1, 5, 2, 1] and dist.tolist() == [0, 0, 0, 1, 1]    # 4: rows 2, 4 (1) and 5 (1) tie -> 2


def test_mutual_match_four_by_three_by_hand():
    """ref 0, 10, 20, 30 and queries 1, 11, 12 in the first component.  Queries -> 1 (1), 2 (1), 2 (4).  From the reference
    side: row 1 -> query 1, row 2 -> query 2 (1 against 4), rows 3 and 4 -> query 3.  Query 3's row 2 prefers query 2."""
    ref, qry = _rows([0, 10, 20, 30]), _rows([1, 11, 12])
    assert G.ref_match(ref, qry)[0].tolist() == [1, 2, 2]
    idx, dist = G.ref_match(ref, qry, mutual=True)
    assert idx.tolist() == [1, 2, 0] and dist.tolist() == [1, 1, 4]
    idx, _ = G.ref_match(_rows([5, 5]), _rows([5, 5]), mutual=True)    # ties on both sides: row 1 <-> query 1 only
    assert idx.tolist() == [1, 0]


# ---------------------------------------------------------------------------- 3. hypotheses ----
RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
SHIFT = np.array([5.0, -7.0, 2.0])
QP = np.array([[0.0, 0, 0], [3.0, 0, 0], [0.0, 3, 0], [6.0, 0, 0], [1.0, 2, 3], [-4.0, 5, 1], [2.0, 2, 2]])
RP = QP @ RZ.T + SHIFT


def test_a_quarter_turn_and_an_integer_shift_come_back_exactly():
    """q = 0, 3 e_x, 3 e_y: e1 = e_x, gv = (0, 0, 3), e3 = e_z, e2 = e_y, Fq = I, cq = (1, 1, 0).  Their images: e1 = e_y,
    gv = (0, 0, 3), e3 = e_z, e2 = e_z x e_y = -e_x, so Fr = Rz and R = Fr Fq^T = Rz; cr = (-1, 1, 0) + s, t = cr - R cq = s."""
    h = G.ref_hypothesis(QP[:3].tolist(), RP[:3].tolist())
    assert not isinstance(h, str)
    assert np.array_equal(np.array(h[0]), RZ)                      # every entry exact (a zero may carry either sign)
    assert h[1] == SHIFT.tolist()
    one = np.arange(1, 8, dtype=np.int32)
    out = G.ref_global(RP, QP, one, one, 1e-9, triples=[[0, 1, 2]])
    assert (out["status"], out["best_trial"], out["best_count"], out["n_valid_trials"]) == (G.OK, 0, 7, 1)
    assert np.array_equal(out["transform"], np.hstack([RZ, SHIFT[:, None]])) and out["counts"].tolist() == [7]
    assert np.array_equal(apply(out["transform"], QP), RP)


def test_every_validity_clause():
    one = np.arange(1, 8, dtype=np.int32)
    tri = [[0, 1, 1], [0, 0, 2], [2, 1, 2],       # a repeated index
           [0, 1, 3],                               # collinear: 0, 3 e_x, 6 e_x -> g2 = 0, no frame
           [0, 1, 2]]
    out = G.ref_global(RP, QP, one, one, 1e-9, triples=tri)
    assert out["counts"].tolist() == [-1, -1, -1, -1, 7] and (out["best_trial"], out["n_valid_trials"]) == (4, 1)
    assert G.ref_hypothesis(QP[[0, 1, 3]].tolist(), RP[[0, 1, 3]].tolist()) == "frame"
    # the edge ratio: the reference triple twice as large, lq = 9 < 0.81 * 36; and the other way round
    assert G.ref_hypothesis(QP[:3].tolist(), (2.0 * RP[:3]).tolist()) == "edge"
    assert G.ref_hypothesis((2.0 * QP[:3]).tolist(), RP[:3].tolist()) == "edge"
    assert not isinstance(G.ref_hypothesis(QP[:3].tolist(), (2.0 * RP[:3]).tolist(), edge_ratio=0.5), str)   # 9 >= 0.25 * 36 exactly
    # min_edge: the shortest query edge is 3
    assert not isinstance(G.ref_hypothesis(QP[:3].tolist(), RP[:3].tolist(), min_edge=3.0), str)
    assert G.ref_hypothesis(QP[:3].tolist(), RP[:3].tolist(), min_edge=3.0000001) == "edge"
    # nothing valid: the identity
    out = G.ref_global(RP, QP, one, one, 1e-9, triples=tri[:4])
    assert (out["status"], out["best_trial"], out["best_count"], out["n_valid_trials"]) == (G.NO_TRIAL, -1, -1, 0)
    assert np.array_equal(out["transform"], np.eye(4)[:3])
    # ties go to the smaller trial
    out = G.ref_global(RP, QP, one, one, 1e-9, triples=[[0, 1, 3], [0, 1, 2], [1, 0, 2], [0, 1, 2]])
    assert out["counts"].tolist() == [-1, 7, 7, 7] and out["best_trial"] == 1


def test_the_drawn_triples_are_three_draws_per_trial():
    """rh_rng_range is a host function: the twin's draws are its, replayed here one by one -- three per trial whatever
    they are, so trial t starts at draw 3 t."""
    c, trials = 11, 40
    tri = G.ref_draw_triples(5, trials, c)
    rng = L.Rng()
    R.lib().rh_rng_seed(C.byref(rng), 5)
    flat = [R.lib().rh_rng_range(C.byref(rng), c) - 1 for _ in range(3 * trials)]
    assert tri.dtype == np.int32 and tri.reshape(-1).tolist() == flat and 0 <= min(flat) and max(flat) < c
    assert any(len(set(t)) < 3 for t in tri.tolist())              # (c is small: some trials repeat an index and still took three)
    assert not np.array_equal(tri, G.ref_draw_triples(6, trials, c))
    rngp = np.random.default_rng(0)
    q = rngp.uniform(-1.0, 1.0, size=(c, 3))
    one = np.arange(1, c + 1, dtype=np.int32)
    a = G.ref_global(apply(np.hstack([RZ, SHIFT[:, None]]), q), q, one, one, 1e-6, trials=trials, seed=5, edge_ratio=0.5)
    b = G.ref_global(apply(np.hstack([RZ, SHIFT[:, None]]), q), q, one, one, 1e-6, triples=tri, edge_ratio=0.5)
    assert np.array_equal(a["counts"], b["counts"]) and a["transform"].tobytes() == b["transform"].tobytes()
    assert a["n_valid_trials"] > 0 and a["best_count"] == c


def test_hypotheses_under_the_sanitizers(tmp_path):
    """csrc/global_hyp.h -- the library's own validity tests, frames and transform, host code without the HIP runtime -- in
    a stand-alone program under AddressSanitizer and UBSan: the quarter turn with every entry exact, every validity clause,
    the last pair of the array addressed, a zero edge never divided by."""
    exe = str(tmp_path / "global_hyp_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ransac.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "global_hyp_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("44 checks, 0 bad")


# -------------------------------------------------------------------------------- 4. the scene ----
def test_the_chain_lands_inside_icp_basin_on_the_scene():
    """The condition of the definition itself, on the twin alone: two disjoint 2048-point samples of the scene, an
    arbitrary motion between them.  For seeds 1 to 3 the best hypothesis is within 10 degrees of the true rotation (the
    basin tests/test_register_host.py documents for ICP), and ref_register from it ends within 0.01 of the truth."""
    s = GS.make()
    dref, _, _ = G.ref_describe(s["ref"], s["ref_nrm"], GS.K)
    dqry, _, _ = G.ref_describe(s["qry"], s["qry_nrm"], GS.K)
    idx, _ = G.ref_match(dref, dqry)
    cq, cr = np.arange(1, GS.N + 1, dtype=np.int32), idx
    good = np.linalg.norm(s["truth"] - s["ref"][idx - 1], axis=1) <= GS.TAU
    print("correct matches: %.1f %%" % (100.0 * good.mean()))
    for seed in GS.SEEDS:
        out = G.ref_global(s["ref"], s["qry"], cq, cr, GS.TAU, GS.TRIALS, seed, GS.EDGE_RATIO)
        rot, err = GS.rotation_error_deg(out["transform"], s["inverse"]), GS.point_error(out["transform"], s)
        reg = G.ref_register(s["ref"], s["qry"], normals=s["ref_nrm"], metric="plane", radius=3.0 * GS.TAU, init=out["transform"])
        fin = GS.point_error(reg["transform"], s)
        print("seed %d: %d valid trials, best count %d, coarse %.2f deg / %.3f, refined %.5f after %d iterations" % (
            seed, out["n_valid_trials"], out["best_count"], rot, err, fin, reg["iterations"]))
        assert out["status"] == G.OK and rot < 10.0
        assert fin <= 0.01


# ------------------------------------------------------------------------------ bookkeeping ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_describe", "rh_describe_f32", "rh_match_features", "rh_register_global", "rh_register_global_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES and hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_global_params\s*;", src) and re.search(r"}\s*rh_global_result\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 124 and R.lib().rh_version() >= 124
    assert int(re.search(r"#define\s+RH_DESC_DIM\s+(\d+)", src).group(1)) == L.DESC_DIM == G.DIM == 33
    assert int(re.search(r"#define\s+RH_DESC_MAX\s+(\d+)", src).group(1)) == L.DESC_MAX == 2 * 63 * 63
    assert re.search(r"#define\s+RH_GLOBAL_MAX_TRIALS\s+\(1 << 20\)", src) and L.GLOBAL_MAX_TRIALS == 1 << 20
    assert re.search(r"RH_GLOB_OK\s*=\s*0\s*,\s*RH_GLOB_NO_TRIAL\s*=\s*1", src) and (L.GLOB_OK, L.GLOB_NO_TRIAL) == (G.OK, G.NO_TRIAL)
    assert header_symbols() == sorted(L.SIGNATURES)
    for name in ("describe", "match_features", "register_global"):
        assert callable(getattr(R, name)) and name in R.__all__


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["trials", "reserved", "seed", "tau", "edge_ratio", "min_edge"]
    sf = ["status", "best_trial", "best_count", "n_valid_trials"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_global_params), sizeof(rh_global_result));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_global_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_global_result, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.GlobalParams), C.sizeof(L.GlobalResult)]
    mine += [getattr(L.GlobalParams, f).offset for f in pf] + [getattr(L.GlobalResult, f).offset for f in sf]
    assert got == mine and mine[:2] == [40, 16]


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    pts, nrm = np.zeros((8, 3)), np.tile(Z, (8, 1))
    for dt in (np.float64, np.float32):
        for kw in (dict(k=0), dict(k=64), dict(k=-1), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf"))):
            with pytest.raises(R.RansacHipError) as e:
                R.describe(pts.astype(dt), nrm.astype(dt), **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        with pytest.raises(R.RansacHipError) as e:
            R.describe(pts[:0].astype(dt), nrm[:0].astype(dt))
        assert e.value.code == L.RH_E_INVALID
    with pytest.raises(ValueError):
        R.describe(pts, nrm[:7])
    with pytest.raises(ValueError):
        R.match_features(np.zeros((4, 32), dtype=np.uint16), np.zeros((4, 33), dtype=np.uint16))
    lib = R.lib()
    u16, i32p, dp = C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    d = np.zeros((4, 33), dtype=np.uint16)
    idx = np.full(4, -5, dtype=np.int32)
    pd, pi = d.ctypes.data_as(u16), idx.ctypes.data_as(i32p)
    for args in ((pd, 4, pd, 4, 2, 0, pi, None), (pd, 4, pd, 4, -1, 0, pi, None), (pd, 0, pd, 4, 0, 0, pi, None),
                 (pd, 4, pd, 0, 0, 0, pi, None), (None, 4, pd, 4, 0, 0, pi, None), (pd, 4, None, 4, 0, 0, pi, None),
                 (pd, 4, pd, 4, 0, 0, None, None)):
        assert lib.rh_match_features(*args) == L.RH_E_INVALID, args[1:6]
    assert idx.tolist() == [-5] * 4
    ref, qry = np.zeros((8, 3)), np.ones((7, 3))
    corr = np.arange(1, 5, dtype=np.int32)
    out = np.full((3, 4), -5.0)
    pr, pq, pc, po = ref.ctypes.data_as(dp), qry.ctypes.data_as(dp), corr.ctypes.data_as(i32p), out.ctypes.data_as(dp)
    good = dict(trials=10, seed=1, tau=0.1, edge_ratio=0.9, min_edge=0.0)

    def call(c=4, r=pr, q=pq, cq=pc, cr=pc, n=8, m=7, o=po, **kw):
        prm = L.GlobalParams(**dict(good, **kw))
        return lib.rh_register_global(r, n, q, m, cq, cr, c, C.byref(prm), None, 0, o, None, None)

    for kw in (dict(trials=0), dict(trials=-3), dict(trials=(1 << 20) + 1), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")),
               dict(tau=float("inf")), dict(edge_ratio=0.0), dict(edge_ratio=1.0000001), dict(edge_ratio=float("nan")),
               dict(min_edge=-1e-9), dict(min_edge=float("nan")), dict(c=2), dict(c=0), dict(n=0), dict(m=0), dict(r=None),
               dict(q=None), dict(cq=None), dict(cr=None), dict(o=None)):
        assert call(**kw) == L.RH_E_INVALID, kw
    assert lib.rh_register_global(pr, 8, pq, 7, pc, pc, 4, None, None, 0, po, None, None) == L.RH_E_INVALID
    assert np.all(out == -5.0)
    assert call(edge_ratio=1.0, trials=1 << 20) in (L.RH_OK, L.RH_E_NODEVICE)   # the ends of the ranges are allowed
