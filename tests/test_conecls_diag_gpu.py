"""The cone code of the score kernel on the scene of tests/cone_scene.py, diag build: the census of the shortcuts' decisions
against the exact test (rh_dbg_cls_soundness / _tiles), the audit of the binary32 error (rh_dbg_cls_audit), the classifier
itself on every (candidate, point) of the scene (rh_dbg_cls_cone: cls_make's record on the host, the kernel's own cls_cone_ab
on the device) against the closed form in numpy longdouble, and the box test on the library's own group boxes
(rh_dbg_conebox over rh_dbg_group_boxes: as many skips as the census counts, none of a box that holds an oracle inlier, none of a
box centred inside the axis guard).

The classifier, per candidate with a record, over all 8262 points (D = c' rho + s' h and L = sgn (c' q . n + s' rho a^ . n) -
cos(alpha) rho from the binary64 inputs, the axis as stored and normalised, c', s' from the shape's own cos / sin):
  - away from the axis guard  |ua - (|D| - eD_lo) / wD| < 1/2  and  |ub - (1/2 - L / wL)| < 1/2  (the margins are half a width);
  - every on-axis point, the apex and the points that binary32 puts on it (rho = NaN) come back `near` for the candidates through
    them; wherever `near` is 0, rho / |t| >= sqrt(RH_CONE_ALPHA) (1 - 2^-9), sqrt(162 2^-24): the guard is n2 > alpha |t|^2 + beta
    in binary32, whose sums of squares are exact to 4 u relative; the binary32 q is off by d <= sqrt(3) e_q <= 30 u T, and
    beta = 3.5 u T^2 >= 2 d rho up to rho = T / 17, beyond which d / rho < 2^-14; both values of `near` occur on the guard families;
  - wherever u = max(ua, ub) < 0 away from the guard the oracle accepts, wherever u > 1 it rejects;
  - a candidate no binary32 record can hold (an apex coordinate above 2^20) carries the NaN flag, and so does, on the Float32
    cloud, a candidate without the band form (opening angles from pi on).
The worst ua / ub errors per candidate family are printed."""
import ctypes as C
import math

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc

import cone_scene as S
import test_conecls_gpu as T

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

LD = np.longdouble
_fp, _dp, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
F32 = pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])


def _census(cs):
    pc, lib = cs.pc("groups"), R.lib()
    snd, snt = np.zeros(56, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    L.check(lib.rh_dbg_cls_soundness(pc._h, cs.arr, S.B, C.byref(cs.cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    L.check(lib.rh_dbg_cls_soundness_tiles(pc._h, cs.arr, S.B, C.byref(cs.cp), snt.ctypes.data_as(C.POINTER(C.c_uint64))))
    return snd.astype(np.int64), snt.astype(np.int64)


@F32
def test_census_shows_decisions_skips_and_no_violation(f32):
    cs = T.case(f32)
    snd, snt = _census(cs)
    s10 = snd[10 * L.CONE:10 * L.CONE + 10]
    print("census", "f32" if f32 else "f64", "cone", s10.tolist(), "band pairs", int(snd[40 + L.CONE]), "inlier pairs", int(snd[44 + L.CONE]),
          "super-tile skips", int(snd[48 + L.CONE]), "tile skips", int(snt[L.CONE]))
    assert s10[2] == 0 and s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
    assert snd[52 + L.CONE] == 0 and snt[4 + L.CONE] == 0
    assert s10[0] == S.B * ((S.N + 63) // 64) and s10[3] == S.N * S.B
    assert s10[8] > 1000
    assert s10[1] > 0
    if not f32:
        assert s10[4] + s10[5] > 0
    assert s10[4] > 0 or f32                     # (a Float32 cloud's normal half is never decided: no surely-in there)
    assert s10[5] > S.N * S.B // 4, s10          # most pairs are nowhere near the cone


@F32
def test_binary32_error_stays_below_0_3_of_a_width(f32):
    cs = T.case(f32)
    out = np.zeros(12)
    L.check(R.lib().rh_dbg_cls_audit(cs.pc("groups")._h, cs.arr, S.B, C.byref(cs.cp), out.ctypes.data_as(_dp)))
    print("audit", "f32" if f32 else "f64", out[6:8].tolist(), int(out[8 + L.CONE]))
    assert out[8 + L.CONE] > 1e5, out
    assert out[6:8].max() < 0.5, out              # soundness: the margin is half the width
    assert out[6:8].max() < 0.3, out              # what the project holds everywhere else


def _cls_cone(shape, cp, M, Nm, f32, xyz, nrm):
    n = len(xyz)
    ua, ub, near = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8)
    rec, d4 = np.zeros(16, dtype=np.float32), np.zeros(4)
    L.check(R.lib().rh_dbg_cls_cone(C.byref(shape), C.byref(cp), float(M), float(Nm), int(f32), n, xyz.ctypes.data_as(_dp), nrm.ctypes.data_as(_dp), 0,
                                    ua.ctypes.data_as(_fp), ub.ctypes.data_as(_fp), near.ctypes.data_as(_u8p), rec.ctypes.data_as(_fp), d4.ctypes.data_as(_dp)))
    return ua, ub, near.astype(bool), rec, d4


def _closed_form(shape, xyz, nrm):
    """D, L + cos(alpha) rho =: P (the part with the normal), rho, |t| in longdouble"""
    A, a = np.array(shape.v[0:3], dtype=LD), np.array(shape.v[3:6], dtype=LD)
    a = a / np.sqrt((a * a).sum())
    c, s = LD(shape.v[7]), LD(shape.v[8])
    nn = np.sqrt(c * c + s * s)
    c, s = c / nn, s / nn
    t = xyz.astype(LD) - A
    n = nrm.astype(LD)
    h = t @ a
    q = t - h[:, None] * a
    rho = np.sqrt((q * q).sum(axis=1))
    sgn = LD(1.0 if shape.outwards else -1.0)
    return c * rho + s * h, sgn * (c * (q * n).sum(axis=1) + s * rho * (n @ a)), rho, np.sqrt((t * t).sum(axis=1))


@F32
def test_classifier_against_the_closed_form_on_every_pair(f32):
    cs = T.case(f32)
    sc = cs.sc
    xyz, nrm = np.ascontiguousarray(cs.xyz, dtype=np.float64), np.ascontiguousarray(cs.nrm, dtype=np.float64)
    M, Nm = float(np.abs(xyz).max()), float(np.abs(nrm).max())
    cosa = LD(math.cos(S.ALPHA))
    # the oracle's verdict on every pair, all points enabled
    oc = (orc.Cloud32 if f32 else orc.Cloud)(cs.xyz, cs.nrm, cs.subs[0])
    _c, m = oc.score_batch(cs.oarr, cs.op, want_masks=True)
    acc = np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :S.N].astype(bool)
    through = {i: name for name in ("ord", "narrow") for i in sc.through(name)}
    worst, decided = {}, {}
    guard_near = guard_far = 0
    ratio_floor = math.sqrt(S.CONE_ALPHA) * (1.0 - 2.0 ** -9)
    for i in range(S.B):
        tag = sc.tags[i]
        ua, ub, near, rec, d4 = _cls_cone(cs.arr[i], cs.cp, M, Nm, f32, xyz, nrm)
        if tag == "huge" or (f32 and tag == "opang" and not cs.arr[i].v[7] > 1e-6):
            assert np.isnan(rec[15]), (i, tag)
            continue
        assert not np.isnan(rec[15]), (i, tag, rec)
        wL, eDlo, wD = d4[1], d4[2], d4[3]
        assert wD > 0 and wL > 0 and (np.isinf(wL) == bool(f32))
        D, P, rho, tn = _closed_form(cs.arr[i], xyz, nrm)
        ua_ref = ((np.abs(D) - LD(eDlo)) / LD(wD)).astype(np.float64)
        ub_ref = (0.5 - (P - cosa * rho) / LD(wL)).astype(np.float64) if not f32 else np.full(S.N, 0.5)
        far = ~near
        ea, eb = np.abs(ua[far] - ua_ref[far]), np.abs(ub[far] - ub_ref[far])
        assert far.sum() > S.N // 2 and not np.isnan(ea).any() and not np.isnan(eb).any(), (i, tag)
        w = worst.setdefault(tag, [0.0, 0.0])
        w[0], w[1] = max(w[0], float(ea.max())), max(w[1], float(eb.max()))
        assert ea.max() < 0.5 and eb.max() < 0.5, (i, tag, float(ea.max()), float(eb.max()))
        # the guard
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (rho / tn).astype(np.float64)
        assert (ratio[far] >= ratio_floor).all(), (i, tag, float(ratio[far].min()))
        if i in through:
            name = through[i]
            on = np.concatenate([sc.fam[(name, "axis")], sc.fam[(name, "apex")], sc.fam[(name, "apexulp")]])
            assert near[on].all(), (i, tag, on[~near[on]])
            g = np.concatenate([sc.fam[(name, "guard")], sc.fam[(name, "guardsweep")]])
            guard_near += int(near[g].sum())
            guard_far += int(far[g].sum())
        # what the classifier decides by itself, against the oracle
        u = np.maximum(ua, ub)
        sure_in, sure_out = far & (u < 0), far & (u > 1)
        assert acc[i][sure_in].all(), (i, tag, np.flatnonzero(sure_in & ~acc[i])[:6])
        assert not acc[i][sure_out].any(), (i, tag, np.flatnonzero(sure_out & acc[i])[:6])
        d = decided.setdefault(tag, [0, 0])
        d[0] += int(sure_in.sum()); d[1] += int(sure_out.sum())
    for tag in sorted(worst):
        print("cls_cone %s %-8s worst |ua - ref| %.4f  |ub - ref| %.4f widths; surely in %d, surely out %d"
              % ("f32" if f32 else "f64", tag, worst[tag][0], worst[tag][1], decided[tag][0], decided[tag][1]))
    assert guard_near > 200 and guard_far > 100, (guard_near, guard_far)
    assert decided["exact"][1] > S.N // 2
    if not f32:
        assert decided["exact"][0] > 300          # the classifier does accept points by itself


def _group_boxes(pc):
    n = C.c_int64()
    L.check(R.lib().rh_dbg_group_boxes(pc._h, None, 0, C.byref(n)))
    out = np.zeros((n.value, 6), dtype=np.float64)
    L.check(R.lib().rh_dbg_group_boxes(pc._h, out.ctypes.data_as(_dp), n.value, C.byref(n)))
    return out


@F32
def test_box_test_on_the_library_s_group_boxes(f32):
    cs = T.case(f32)
    pc, lib = cs.pc("groups"), R.lib()
    snd, _snt = _census(cs)
    ngroups = (S.N + 63) // 64
    gb = _group_boxes(pc)
    assert gb.shape == (ngroups, 6)
    xyz = np.ascontiguousarray(cs.xyz, dtype=np.float64)
    M, Nm = float(np.abs(xyz).max()), float(np.abs(np.asarray(cs.nrm, dtype=np.float64)).max())
    oc = (orc.Cloud32 if f32 else orc.Cloud)(cs.xyz, cs.nrm, cs.subs[0])
    _c, m = oc.score_batch(cs.oarr, cs.op, want_masks=True)
    acc = np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :S.N].astype(bool)
    lo, hi = gb[:, :3] - gb[:, 3:], gb[:, :3] + gb[:, 3:]
    host_skip = n_guarded = 0
    for i in range(S.B):
        skip, fld = np.zeros(ngroups, dtype=np.uint8), np.zeros(11, dtype=np.float32)
        L.check(lib.rh_dbg_conebox(C.byref(cs.arr[i]), C.byref(cs.cp), M, Nm, int(f32), gb.ctypes.data_as(_dp), ngroups, skip.ctypes.data_as(_u8p),
                                   fld.ctypes.data_as(_fp)))
        host_skip += int(skip.sum())
        if np.isfinite(fld).all():
            # a box whose centre lies inside the axis guard (rho^2 < (alpha |t|^2 + beta) / 2, the record's fields 10 and 9) stays
            t = gb[:, :3] - fld[0:3].astype(np.float64)
            hh = t @ fld[3:6].astype(np.float64)
            tt = (t * t).sum(axis=1)
            guarded = tt - hh * hh < 0.5 * (float(fld[10]) * tt + float(fld[9]))
            n_guarded += int(guarded.sum())
            assert not (guarded & skip.astype(bool)).any(), (i, cs.sc.tags[i], np.flatnonzero(guarded & skip.astype(bool))[:4])
        # no skipped box holds an inlier of the oracle (every point lies in its own group's box)
        pts = xyz[acc[i]]
        inside = (lo[None] <= pts[:, None]).all(axis=2) & (pts[:, None] <= hi[None]).all(axis=2)      # (inliers, groups)
        assert inside.any(axis=1).all() and not inside[:, skip.astype(bool)].any(), (i, cs.sc.tags[i])
    pairs, skips = int(snd[10 * L.CONE]), int(snd[10 * L.CONE + 1])
    print("f32 %d: cone pairs %d, the box test skips %d (host, over the library's boxes: %d), pairs with an inlier %d" % (f32, pairs, skips, host_skip, int(snd[44 + L.CONE])))
    assert int(snd[44 + L.CONE]) > 0 and 0 < skips <= pairs - int(snd[44 + L.CONE])
    assert host_skip == skips          # the very function on the very boxes with the very record
    assert n_guarded > 0           # (49 of the 24960 pairs on this scene)
