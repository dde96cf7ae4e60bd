"""The score launch and the refit scan on clouds far from the origin -- extent 100, max |coordinate| up to 3 x 2^20 -- held to the
oracle and to their own answer at the origin.

Every margin, box slack and mask of the culled score kernel is built from M = max |coordinate| and T = M + |centre|
(csrc/score4_device.h, cls_make); where M is a few thousand times the extent, as in a georeferenced scan, u T reaches the size
of eps: most points become ambiguous, small round candidates turn exact-only through nrmin / n2min / the mv guard, and above
2^20 everything does.  The scene of tests/translated_scene.py makes the right answer independent of the offset for planes,
spheres and cones (an exact translation on a binary grid; the cylinder's chain reads p itself and is held to the oracle only),
so there are two anchors: the oracle on the translated cloud, and the arrays obtained at offset 0.

Product library: rh_score_batch (masks and counts-only) on Float64 and Float32 clouds, 20000 and 8193 points, groups (lists on /
off, normal cells on / off, rows default / 4) and brute; rh_score_batch_dev with 3 batches in flight; 30 % and 1 % enabled;
rh_refit culled and scan with invalidation; huge round candidates through a cloud at the origin (D up to 3e6: exact-only); a
cloud with one point at 2^20 (classifier on) and at 2^20 + 0.125 (exact-only).  Diag library: the census of the shortcuts'
decisions and the audit of the binary32 error at every offset, and 20-case slices of the fuzzers with `shift`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import translated_scene as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

CASES = [(f32, t) for f32 in (False, True) for t in T.OFFSETS[f32]]
IDS = ["%s-%s" % ("f32" if f32 else "f64", T.offset_id(t)) for f32, t in CASES]
# (st_cull, nsig, s4_rows) of the culled kernel: lists on (1) / off (2), normal-cell masks on (0) / off (2), rows: the library's / 4
GROUP_CONFIGS = [(lists, nsig, rows) for lists in (1, 2) for nsig in (0, 2) for rows in (None, 4)]
_OPTS = ("score_path", "s4_rows", "refit_path", "st_cull")


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    for k in _OPTS:
        R.set_option(k, None)


class Case:
    """one (element type, offset, size[, extra point / other candidates]): the clouds on both sides, the batch, the oracle's answer"""

    def __init__(self, sc, cands, eps=None):
        self.sc, self.f32, self.n = sc, sc.f32, sc.n
        self.b = len(cands)
        self.inv = T.is_invariant(cands)
        self.kinds = T.kind_ids(cands)
        self.arr = T.rh_shapes(cands, sc.f32)
        self.oarr = T.as_orc(self.arr, self.b)
        self.cp, self.op = T.params(sc.f32, eps)
        self.oc = sc.oracle_cloud()
        self.pcs = {}
        self.ref_c, self.ref_m = self.oc.score_batch(self.oarr, self.op, want_masks=True)
        self.ref_c.setflags(write=False); self.ref_m.setflags(write=False)
        self._dev0 = None

    def pc(self, path="groups"):
        if path not in self.pcs:
            with R.option("score_path", path):             # (read when a cloud is created)
                self.pcs[path] = self.sc.device_cloud()
        return self.pcs[path]

    def device_answer(self):
        """what the library itself gives with its own settings: the second anchor, taken at offset 0"""
        if self._dev0 is None:
            self._dev0 = R.score_batch(self.pc(), self.arr, self.cp, want_masks=True)
        return self._dev0

    def set_enabled(self, en):
        for pc in self.pcs.values():
            pc.set_enabled(en)
        self.oc.set_enabled(T.enabled_chunks(en))

    def enable_all(self):
        for pc in self.pcs.values():
            pc.enable_all()
        self.oc.enable_all()


_CACHE = {}


def _case(f32, t, n=T.N):
    key = (f32, tuple(t), n)
    if key not in _CACHE:
        sc = T.scene(f32) if n == T.N else T.scene(f32).head(n)
        _CACHE[key] = Case(T.translate(sc, t), T.moved(T.candidates(f32), t, f32))
    return _CACHE[key]


def _zero(f32, n=T.N):
    return _case(f32, T.OFFSETS[f32][0], n)


def _check_batch(cs, pc, exp_c, exp_m, tag, zero=None):
    got_c, got_m = R.score_batch(pc, cs.arr, cs.cp, want_masks=True)
    assert np.array_equal(got_c, exp_c), (tag, np.flatnonzero(got_c != exp_c)[:8], got_c[got_c != exp_c][:8], exp_c[got_c != exp_c][:8])
    assert np.array_equal(got_m, exp_m), tag
    assert np.array_equal(R.score_batch(pc, cs.arr, cs.cp), exp_c), (tag, "counts only")
    if zero is not None:
        z_c, z_m = zero
        assert np.array_equal(got_c[cs.inv], z_c[cs.inv]) and np.array_equal(got_m[cs.inv], z_m[cs.inv]), (tag, "against offset 0")


def _every_config(cs, exp_c, exp_m, tag, zero=None):
    pc = cs.pc("groups")
    for lists, nsig, rows in GROUP_CONFIGS:
        with R.option("st_cull", lists, cloud=pc), R.option("nsig", nsig, cloud=pc), R.option("s4_rows", rows, cloud=pc):
            _check_batch(cs, pc, exp_c, exp_m, (tag, "groups", lists, nsig, rows), zero)
    _check_batch(cs, cs.pc("brute"), exp_c, exp_m, (tag, "brute"), zero)


# ------------------------------------------------------------------------------------------------------- product library
@pytest.mark.parametrize("f32,t", CASES, ids=IDS)
def test_counts_and_masks_equal_the_oracle_and_the_answer_at_the_origin(f32, t):
    for n in (T.N, T.N_SMALL):
        cs = _case(f32, t, n)
        assert cs.b == T.B and (cs.n + 63) // 64 == {T.N: 313, T.N_SMALL: 129}[n]
        assert (cs.ref_c > 300).sum() >= 24 and len(np.unique(cs.ref_c)) > 16       # the thresholds cut through the point sets
        _every_config(cs, cs.ref_c, cs.ref_m, (f32, t, n), zero=_zero(f32, n).device_answer())


@pytest.mark.parametrize("f32,t", CASES, ids=IDS)
def test_three_batches_in_flight(f32, t):
    import fuzz_score
    cs = _case(f32, t)
    rng = np.random.default_rng(77)
    for path in ("groups", "brute"):
        assert fuzz_score.score_in_flight(cs.pc(path), cs.arr, cs.b, cs.cp, 3, rng, cs.ref_c, cs.ref_m), (f32, t, path, "masks")
        assert fuzz_score.score_in_flight(cs.pc(path), cs.arr, cs.b, cs.cp, 3, rng, cs.ref_c, None), (f32, t, path, "counts")


@pytest.mark.parametrize("f32,t", CASES, ids=IDS)
def test_partly_enabled_clouds(f32, t):
    cs, zero = _case(f32, t), _zero(f32)
    cs.pc("groups"), cs.pc("brute"), zero.pc("groups")
    rng = np.random.default_rng(5)
    try:
        for share in (0.3, 0.01):
            en = rng.random(cs.n) < share
            cs.set_enabled(en)
            exp_c, exp_m = cs.oc.score_batch(cs.oarr, cs.op, want_masks=True)
            assert exp_c.max() > 10 * share * 100
            z = None
            if any(t):
                zero.set_enabled(en)
                z = R.score_batch(zero.pc("groups"), zero.arr, zero.cp, want_masks=True)
            pc = cs.pc("groups")
            for lists in (1, 2):
                with R.option("st_cull", lists, cloud=pc):
                    _check_batch(cs, pc, exp_c, exp_m, (f32, t, share, "groups", lists), z)
            _check_batch(cs, cs.pc("brute"), exp_c, exp_m, (f32, t, share, "brute"), z)
    finally:
        cs.enable_all()
        zero.enable_all()


def _check_refits(cs, which, tag, invalidate):
    for path in ("culled", "scan"):
        pc = cs.pc("groups")
        cs.enable_all()
        try:
            with R.option("refit_path", path, cloud=pc):
                total = 0
                for i in which:
                    got = R.refit(cs.arr[i], pc, cs.cp).inpoints
                    exp = cs.oc.refit(cs.oarr[i], cs.op)
                    assert np.array_equal(got, exp), (tag, path, i, len(got), len(exp))
                    total += len(exp)
                    if invalidate and len(exp):
                        R.invalidate_indexes(pc, exp)
                        cs.oc.invalidate(exp)
                        assert np.array_equal(pc.enabled_chunks(), cs.oc.get_enabled()), (tag, path, i)
                assert total > 1000 * len(which) // 2, (tag, path, total)
        finally:
            cs.enable_all()


@pytest.mark.parametrize("f32,t", CASES, ids=IDS)
def test_refit_of_the_truths_and_invalidation(f32, t):
    cs = _case(f32, t)
    _check_refits(cs, range(0, T.B, T.PER_KIND), (f32, t), invalidate=True)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_huge_round_candidates_through_a_cloud_at_the_origin(f32):
    """T grows from the candidate's side: D = 2^20 - 200 is the last radius the classifier takes, D = 3e6 is exact-only and
    must still give the oracle's answer"""
    for eps in (T.EPS[f32], 0.3):
        key = (f32, "huge", eps)
        if key not in _CACHE:
            _CACHE[key] = Case(T.scene(f32), T.huge_candidates(f32), eps)
        cs = _CACHE[key]
        assert cs.b == 2 * len(T.HUGE_D) and cs.ref_c.min() > 1000, cs.ref_c
        _every_config(cs, cs.ref_c, cs.ref_m, (f32, "huge", eps))
        _check_refits(cs, range(cs.b), (f32, "huge", eps), invalidate=False)


def _edge_case(f32, which):
    key = (f32, "edge", which)
    if key not in _CACHE:
        _CACHE[key] = Case(T.guard_edge_scenes(f32)[which], list(T.candidates(f32)) + T.huge_candidates(f32))
    return _CACHE[key]


@pytest.mark.parametrize("which", [0, 1], ids=["at_2^20", "beyond_2^20"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_cloud_with_one_point_at_the_classifier_s_limit(f32, which):
    """one far point decides whether the whole batch is classified (M = 2^20) or exact-only (M = 2^20 + 0.125): the answer is the
    oracle's either way, and for the 64 candidates of the scene it is the scene's own (the far point is nobody's inlier)"""
    cs, base = _edge_case(f32, which), _zero(f32)
    assert cs.n == T.N + 1 and np.abs(cs.sc.xyz).max() == T.BIG + (0.125 if which else 0.0)
    _every_config(cs, cs.ref_c, cs.ref_m, (f32, "edge", which))
    assert np.array_equal(cs.ref_c[:T.B], base.ref_c) and np.array_equal(cs.ref_m[:T.B], base.ref_m)
    _check_refits(cs, range(0, T.B, T.PER_KIND), (f32, "edge", which), invalidate=True)


# -------------------------------------------------------------------------------------------------------- fuzzer slices
@pytest.mark.parametrize("f32,shift", [(False, True), (True, 7e5)], ids=["f64", "f32"])
def test_score_fuzz_slice_far_from_the_origin(f32, shift):
    import fuzz_score
    rng = np.random.default_rng(8101 + f32)
    bad = []
    for case in range(20):
        ok, desc = fuzz_score.one(case, rng, f32=f32, shift=shift)
        if not ok:
            bad.append(desc)
    assert not bad, bad[:5]


def test_refit_fuzz_slice_far_from_the_origin():
    import fuzz_refit
    rng = np.random.default_rng(8103)
    bad = []
    for case in range(20):
        ok, desc = fuzz_refit.one(case, rng, f32=bool(case % 4 == 3), shift=True)
        if not ok:
            bad.append(desc)
    assert not bad, bad[:5]


@pytest.mark.diag
def test_soundness_fuzz_slice_far_from_the_origin():
    import fuzz_sound
    rng = np.random.default_rng(8104)
    bad = []
    for case in range(20):
        ok, desc, out = fuzz_sound.one(case, rng, f32=bool(case % 4 == 3), shift=True)
        if not ok:
            bad.append(desc)
    assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------------------- diag library
FIELDS = ("pairs", "pairs_skipped", "V_skipped_with_inlier", "points", "sure_in", "sure_out", "V_sure_in_rejected", "V_sure_out_accepted",
          "exact_inliers", "V_zero_point_in")
_CENSUS = {}


def _u64(n):
    a = np.zeros(n, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def _census(cs, key):
    """rh_dbg_cls_soundness, _tiles and _nsig of a case's batch, once: (4 x 10 per kind, super-tile skips / violations, tile
    skips / violations, normal-cell counters)"""
    if key not in _CENSUS:
        lib, pc = R.lib(), cs.pc("groups")
        snd, p_snd = _u64(56)
        til, p_til = _u64(8)
        nsg, p_nsg = _u64(4)
        L.check(lib.rh_dbg_cls_soundness(pc._h, cs.arr, cs.b, C.byref(cs.cp), p_snd))
        L.check(lib.rh_dbg_cls_soundness_tiles(pc._h, cs.arr, cs.b, C.byref(cs.cp), p_til))
        L.check(lib.rh_dbg_cls_soundness_nsig(pc._h, cs.arr, cs.b, C.byref(cs.cp), p_nsg))
        _CENSUS[key] = (snd[:40].reshape(4, 10).astype(np.int64), snd[48:52].astype(np.int64), snd[52:56].astype(np.int64),
                        til[:4].astype(np.int64), til[4:].astype(np.int64), nsg.astype(np.int64))
    return _CENSUS[key]


def _no_violation(cen, tag):
    per, st_skip, st_viol, t_skip, t_viol, nsg = cen
    assert per[:, [2, 6, 7, 9]].sum() == 0, (tag, per[:, [2, 6, 7, 9]].tolist())
    assert st_viol.sum() == 0 and t_viol.sum() == 0 and nsg[1] == 0 and nsg[3] == 0, (tag, st_viol, t_viol, nsg)


@pytest.mark.diag
@pytest.mark.parametrize("f32,t", CASES, ids=IDS)
def test_census_of_the_shortcuts_decisions(f32, t):
    cs = _case(f32, t)
    cen = _census(cs, (f32, tuple(t)))
    per, st_skip, st_viol, t_skip, t_viol, nsg = cen
    M = float(np.abs(cs.sc.xyz).max())
    for k, name in enumerate(T.KINDS):
        d = dict(zip(FIELDS, per[k].tolist()))
        print("census %s %s %-8s decided %.4f skipped %.4f tile %d st %d %s" % (
            "f32" if f32 else "f64", T.offset_id(t), name, (d["sure_in"] + d["sure_out"]) / d["points"], d["pairs_skipped"] / d["pairs"],
            t_skip[k], st_skip[k], d))
    print("census %s %s nsig group skips %d super-tile skips %d" % ("f32" if f32 else "f64", T.offset_id(t), nsg[0], nsg[2]))
    _no_violation(cen, (f32, t))
    # it looked at something
    assert (per[:, 3] == T.PER_KIND * cs.n).all() and (per[:, 3] > 1e5).all() and (per[:, 8] > 0).all(), per
    decided = per[:, 4] + per[:, 5]
    if M <= T.BIG:
        assert decided.sum() > 0 and decided[L.PLANE] > 0, per
        # the culling records are filled: planes, spheres and cylinders have pairs their boxes rule out at every offset.  The
        # cone's box test never skips a box within rho^2 <= alpha |t|^2 + beta of the axis, beta = S 1.75 u T^2 (cls_make): from
        # T ~ 1e5 on that holds the whole scene -- asserted where beta is below 10^2
        assert (per[:3, 1] > 0).all(), per[:, 1]
        if (6.0 if f32 else 2.0) * 1.75 * 2.0 ** -24 * (2.0 * M) ** 2 < 100.0:
            assert per[L.CONE, 1] > 0, per[:, 1]
    else:
        # cls_make's first guard: M > 2^20 leaves every candidate exact-only.  (Skipped pairs are not asserted here: a candidate
        # with a position parameter above 2^20 -- every one of this batch -- has no culling record either, DESIGN.md section 5;
        # test_census_at_the_classifier_s_limit has the candidates whose records are filled beyond the limit)
        assert (decided == 0).all(), per


@pytest.mark.diag
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_margins_grow_with_the_offset(f32):
    """the plane's margins are proportional to M: fewer of its points are decided at 7e5 than at the origin"""
    share = {}
    for t in (T.OFFSETS[f32][0], (7e5, -7e5, 7e5)):
        per = _census(_case(f32, t), (f32, tuple(t)))[0]
        share[t] = (per[L.PLANE, 4] + per[L.PLANE, 5]) / per[L.PLANE, 3]
    assert share[(7e5, -7e5, 7e5)] < share[T.OFFSETS[f32][0]], share


@pytest.mark.diag
@pytest.mark.parametrize("which", [0, 1], ids=["at_2^20", "beyond_2^20"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_at_the_classifier_s_limit(f32, which):
    """candidates at the origin, one point at M = 2^20 / 2^20 + 0.125: beyond the limit nothing is decided by the classifier, while
    the culling records of planes, spheres and cylinders -- the candidates' parameters are finite and small -- are still filled
    and still skip pairs (the cone's is not: its band form is only made for a candidate the classifier takes, cls_make's band_ok)"""
    cs = _edge_case(f32, which)
    cen = _census(cs, (f32, "edge", which))
    per = cen[0]
    print("census %s edge %d decided %s skipped %s" % ("f32" if f32 else "f64", which, (per[:, 4] + per[:, 5]).tolist(), per[:, 1].tolist()))
    _no_violation(cen, (f32, "edge", which))
    decided = per[:, 4] + per[:, 5]
    if which == 0:
        assert decided.sum() > 0 and decided[L.PLANE] > 0, per
        assert (per[:3, 1] > 0).all(), per[:, 1]           # (the cone: beta = S 1.75 u T^2 holds the scene at T = 2^20, see above)
    else:
        assert (decided == 0).all(), per
        assert (per[:3, 1] > 0).all(), per[:, 1]
    assert (per[:, 8] > 0).all(), per


@pytest.mark.diag
@pytest.mark.parametrize("f32,t", [c for c in CASES if T.offset_mag(c[1]) < T.BIG], ids=[i for c, i in zip(CASES, IDS) if T.offset_mag(c[1]) < T.BIG])
def test_binary32_error_stays_inside_the_margins(f32, t):
    """rh_dbg_cls_audit: the classifier's error in units of a margin's width is sound below 0.5; the project's own bound
    (test_binary32_classifier_stays_inside_its_margins) is 0.3 -- a value between the two would mean that a first-order bound of
    cls_make is too small on its T term"""
    cs = _case(f32, t)
    out = np.zeros(12)
    L.check(R.lib().rh_dbg_cls_audit(cs.pc("groups")._h, cs.arr, cs.b, C.byref(cs.cp), out.ctypes.data_as(C.POINTER(C.c_double))))
    print("audit %s %s worst %s pairs %s" % ("f32" if f32 else "f64", T.offset_id(t), np.round(out[:8], 4).tolist(), out[8:].tolist()))
    per = _census(cs, (f32, tuple(t)))[0]
    usable = (per[:, 4] + per[:, 5]) > 0                   # kinds that still have a candidate the classifier takes
    assert usable[L.PLANE]
    assert (out[8:12][usable] > 0).all(), (out, usable)
    assert out[:8].max() < 0.5, out
    assert out[:8].max() < 0.3, out
