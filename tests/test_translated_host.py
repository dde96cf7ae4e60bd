"""Clouds far from the origin, on the host (no GPU): what tests/test_translated_gpu.py rests on, and the host forms of the score
kernel's shortcuts at the magnitudes of georeferenced scans (M / extent of 1e3 .. 1e4 where every other test has about 1).

1. The invariance (tests/translated_scene.py).  On the snapped scene a translation by a grid vector is exact, so the exact test
   of a plane, a sphere and a cone -- which read the point only through p - p0, p - o, p - apex -- gives the same counts and
   masks at every offset, bit for bit: asserted on the oracle and on its rounding variants 0 .. 5, in binary64 and in binary32.
   The CYLINDER is NOT invariant and is not asserted: its chain is (p - a sd) - c, which reads p itself after the difference
   p - c went into sd, so the rounding of a sd against p moves with the offset (in binary32 1 to 8 of its 8 outward rows change;
   in binary64 the change is real too but too small to move a point of this scene across a threshold).
2. The scene's own conditions, from the oracle alone: the thresholds cut through the point sets.
3. rh_dbg_cls_round (the kernel's cls_make + cls_round_ab on the host, diag build) against the numpy twin of
   test_rootfree_host.py at offsets 1e5 and 7e5, where u T is 0.01 .. 0.2 and the guards nrmin, n2min and mv start to bind; the
   guards are recomputed here from cls_make's formulas, checked against the margins the library reports, and must explain
   every exact-only flag.
4. rh_dbg_cylbox and rh_dbg_nsig at the same magnitudes: no box with a twin inlier is skipped, no cell with an accepted normal
   is missing from a plane's mask; the mask is all ones exactly from M > 2^20 on."""
import math

import numpy as np
import pytest

import translated_scene as T
from oracle import oracle as orc
from ransac_jl_amd import _lib as L
from test_cylbox_host import _cylbox
from test_nsig_host import ALL, _cells, _mask, _params as plane_params
from test_rootfree_host import _params as round_params, _points, _run, _shape, _twin

BIG = T.BIG
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------- 1, 2: the oracle
@pytest.mark.parametrize("variant", range(6))
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_plane_sphere_cone_do_not_depend_on_an_exact_translation(f32, variant):
    """counts and masks at every offset equal those at 0 for the 48 candidates that are no cylinder (why not the cylinder: the
    module's text, item 1)"""
    lib = orc.variant_lib(variant) if variant else None
    sc0, c0 = T.scene(f32), T.candidates(f32)
    inv = T.is_invariant(c0)
    assert inv.sum() == 48
    op = T.orc_params(f32)
    ref = None
    for t in T.OFFSETS[f32]:
        sc = T.translate(sc0, t)
        assert np.abs(sc.xyz).max() >= T.offset_mag(t) - 100.0       # (the scene lies in [0, 100]^3)
        cn, mk = sc.oracle_cloud(lib).score_batch(T.orc_shapes(T.moved(c0, t, f32), f32), op, want_masks=True)
        if ref is None:
            assert not any(t)
            ref = (cn.copy(), mk.copy())
            assert cn[inv].max() > 3000
        assert np.array_equal(cn[inv], ref[0][inv]), (t, np.flatnonzero(cn != ref[0]))
        assert np.array_equal(mk[inv], ref[1][inv]), t


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_thresholds_cut_through_the_point_sets(f32):
    """Every family has candidates with more than 1000 and fewer than 3500 inliers (3500 = a truth's points), and between
    eps 0.05 and 0.3 at least 5 % of the truth's points change side: counted over the family's outward candidates, as
    sum (count at 0.3 - count at 0.05) >= 0.05 x 3500 x candidates.  (The truth candidate ALONE moves only 1 to 10 % of its
    points -- the scene's noise is small against 0.05 --; its position jitters of 0.05 are what spreads the points over the band.)"""
    sc, c0 = T.scene(f32), T.candidates(f32)
    oc = sc.oracle_cloud()
    arr = T.orc_shapes(c0, f32)
    at = oc.score_batch(arr, T.orc_params(f32))
    lo, hi = oc.score_batch(arr, T.orc_params(f32, 0.05)), oc.score_batch(arr, T.orc_params(f32, 0.3))
    kinds = T.kind_ids(c0)
    for k, name in enumerate(T.KINDS):
        assert sc.truth[k]["kind"] == name and sc.truth[k]["n_points"] == 3500
        mine = at[kinds == k]
        assert ((mine > 1000) & (mine < 3500)).sum() >= 4, (name, mine)
        out = (kinds == k) & (hi > 0)
        assert out.sum() >= T.PER_KIND // 2
        assert (hi[out] >= lo[out]).all()
        assert int((hi[out] - lo[out]).sum()) >= 0.05 * 3500 * out.sum(), (name, lo[out], hi[out])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_huge_round_candidates_hold_the_plane(f32):
    """a sphere and a cylinder of radius D touching the true plane in its point hold most of the plane's points at eps 0.3 for
    every D (the cap's sag over the patch is below 0.3 from D = 1e3 on: (25 sqrt 2)^2 / 2 D)"""
    sc = T.scene(f32)
    cn = sc.oracle_cloud().score_batch(T.orc_shapes(T.huge_candidates(f32), f32), T.orc_params(f32, 0.3))
    assert len(cn) == 2 * len(T.HUGE_D) and (cn > 1750).all(), cn


def test_guard_edge_scenes_sit_on_either_side_of_2_to_the_20():
    for f32 in (False, True):
        a, b = T.guard_edge_scenes(f32)
        assert a.n == b.n == T.N + 1
        assert np.abs(a.xyz).max() == BIG and np.abs(b.xyz).max() == BIG + 0.125
        assert np.float32(BIG + 0.125) == BIG + 0.125


# ------------------------------------------------------------------------------------------- 3: the round kinds' classifier

RADII = (50.0, 500.0)
FAR = (1e5, 7e5)
AXES = ((0.0, 0.0, 1.0), (0.48, -0.6, 0.64))
EPS, ALPHA_DEG = 0.3, 5.0
N_RANDOM = 20_000


def _guards(kind, v, eps, cosa, M, Nm, f32):
    """cls_make's margins and guards for a sphere / cylinder (csrc/score4_device.h), stated again: (m2, mv, usable, which guard)"""
    S = 6.0 if f32 else 2.0
    s3 = 1.7320508075688774
    if kind == L.SPHERE:
        c, Rr, a1, ai = v[:3], v[3], 0.0, 0.0
    else:
        c, Rr = v[3:6], v[6]
        a1, ai = sum(abs(x) for x in v[:3]), max(abs(x) for x in v[:3])
    Tm = M + max(abs(x) for x in c)
    e = 2.01 * U * Tm if kind == L.SPHERE else U * Tm * (3.01 + 8.04 * ai * a1)
    mD = S * (s3 * e + 7.0 * U * (abs(Rr) + abs(eps))) + 1e-30
    nrmax, nrmin = Rr + eps + 3.0 * mD, Rr - eps - 3.0 * mD
    nq = nrmax + s3 * e
    K, ca2 = Rr * Rr + eps * eps, cosa * cosa
    dn2 = 2.0 * nrmax * s3 * e + 3.0 * e * e + 4.0 * U * nq * nq + 6.0 * U * K
    m2 = S * dn2 + 1e-30
    ds = 3.0 * Nm * e + 5.0 * U * Nm * s3 * nq
    mv = S * (2.0 * (abs(cosa) * nrmax + ds) * ds + ds * ds + ca2 * dn2 + 8.0 * U * ca2 * nq * nq) + 1e-30
    n2min = (Rr - eps) * (Rr - eps) - 2.0 * m2
    big = 2.0 ** 120
    n2max = 3.1 * Tm * Tm * (1.0 + ai * a1) ** 2
    failed = [name for name, good in (
        ("magnitude", M <= BIG and Nm <= BIG and all(abs(x) <= BIG for x in v) and ai <= 16.0),
        ("nrmin", nrmin > 0.0), ("n2min", n2min > 0.0), ("mv", ca2 * n2min > 1.001 * mv),
        ("overflow", (n2max + K) / (2.0 * m2) < big and 3.0 * Nm * Nm * n2max / (2.0 * mv) < big and n2max * ca2 / (2.0 * mv) < big)) if not good]
    return m2, mv, not failed, failed


def _far_cloud(kind, v, sgn, rng):
    """the threshold points, the zero point and the centre point of test_rootfree_host._points, then N_RANDOM points of a box of
    half side 50 about a point of the shell, half of them with a normal within a few degrees of the shell's -- and of those the
    ones within 10 of the shell moved to within 1 of it"""
    P, Nn, i_zero, n_built = _points(kind, v, sgn, EPS, math.radians(ALPHA_DEG), 0, rng)
    if kind == L.SPHERE:
        c0, Rr, ah = np.array(v[:3]), v[3], None
    else:
        c0, Rr, ah = np.array(v[3:6]), v[6], np.array(v[:3])
    d = rng.normal(size=3)
    if ah is not None:
        d -= ah * (d @ ah)
    d /= np.linalg.norm(d)
    pts = c0 + Rr * d + rng.uniform(-50.0, 50.0, (N_RANDOM, 3))
    q = pts - c0
    if ah is not None:
        q -= np.outer(q @ ah, ah)
    qh = q / np.linalg.norm(q, axis=1)[:, None]
    nn = rng.normal(size=(N_RANDOM, 3))
    near = rng.random(N_RANDOM) < 0.5
    nn[near] = sgn * qh[near] + rng.normal(scale=0.06, size=(int(near.sum()), 3))
    onto = near & (np.abs(np.linalg.norm(q, axis=1) - Rr) < 10.0)          # those next to the shell: within 1 of it
    pts[onto] += qh[onto] * ((Rr + rng.uniform(-1.0, 1.0, int(onto.sum()))) - np.linalg.norm(q[onto], axis=1))[:, None]
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    return np.vstack([P[:n_built], pts]), np.vstack([Nn[:n_built], nn]), i_zero, n_built


def _round_cases():
    for kind in (L.SPHERE, L.CYLINDER):
        for Rr in RADII:
            for far in FAR:
                for outwards in (1, 0):
                    c0 = [far, -0.75 * far, 0.5 * far]
                    if kind == L.SPHERE:
                        yield kind, outwards, c0 + [Rr]
                    else:
                        for a in AXES:
                            yield kind, outwards, list(a) + c0 + [Rr]


@pytest.mark.parametrize("f32", [0, 1], ids=["f64cloud", "f32cloud"])
def test_round_classifier_far_from_the_origin_is_sound_and_flags_what_its_guards_say(f32):
    cp = round_params(EPS, ALPHA_DEG)
    rng = np.random.default_rng(2027 + f32)
    usable = flagged = 0
    reasons = set()
    decided = total = accepted = 0
    for kind, outwards, v in _round_cases():
        eps_c, cosa = cp.eps[kind], cp.cos_alpha[kind]
        sgn = 1.0 if outwards else -1.0
        xyz, nrm, i_zero, n_built = _far_cloud(kind, v, sgn, rng)
        M, Nm = float(np.abs(xyz).max()), float(np.abs(nrm).max())
        assert max(FAR) * 0.99 < M <= BIG or M < 2e5
        ua, ub, rec, d4 = _run(_shape(kind, outwards, v), cp, M, Nm, xyz, nrm, f32=f32)
        m2, mv, ok, failed = _guards(kind, v, eps_c, cosa, M, Nm, f32)
        assert not np.isnan(ua).any() and not np.isnan(ub).any(), (kind, v)
        # an exact-only flag exactly where a guard fails
        assert bool(np.isnan(rec[15])) == (not ok), (kind, v, f32, failed, d4)
        if not ok:
            flagged += 1
            reasons.update(failed)
            continue
        usable += 1
        # (the guards above were computed from the very margins the library uses)
        assert abs(d4[0] - m2) <= 1e-12 * m2 and abs(d4[2] - mv) <= 1e-12 * mv and d4[1] == 2.0 * d4[0] and d4[3] == 2.0 * d4[2], (d4, m2, mv)
        acc, n2, s = _twin(kind, v, sgn, xyz, nrm, eps_c, cosa)
        u = np.maximum(ua, ub)
        sure_in, sure_out = u < 0, u > 1
        assert not (sure_in & ~acc).any(), (kind, v, f32, np.flatnonzero(sure_in & ~acc)[:5])
        assert not (sure_out & acc).any(), (kind, v, f32, np.flatnonzero(sure_out & acc)[:5])
        assert u[i_zero] > 1, (kind, v, u[i_zero])
        decided += int((sure_in | sure_out)[n_built:].sum())
        accepted += int(acc[n_built:].sum())
        total += len(u) - n_built
    print("f32cloud=%d usable %d flagged %d (%s) decided %.4f of %d random points, %d accepted by the twin"
          % (f32, usable, flagged, sorted(reasons), decided / max(1, total), total, accepted))
    # from the formulas: at R = 500 every guard holds for a Float64 cloud; a Float32 cloud's tripled margins flag some of R = 50
    assert usable >= (12 if not f32 else 1) and accepted > 1000
    if f32:
        assert flagged > 0 and reasons <= {"nrmin", "n2min", "mv"}, (flagged, reasons)


# ------------------------------------------------------------------------------------------------ 4: boxes and normal cells
@pytest.mark.parametrize("f32", [0, 1], ids=["f64cloud", "f32cloud"])
def test_no_cylinder_box_with_a_twin_inlier_is_skipped_far_from_the_origin(f32):
    cp = round_params(EPS, ALPHA_DEG)
    rng = np.random.default_rng(31 + f32)
    nbox = nskip = ninl = 0
    for kind, outwards, v in _round_cases():
        if kind != L.CYLINDER or not outwards:
            continue
        xyz, nrm, _, n_built = _far_cloud(kind, v, 1.0, rng)
        xyz, nrm = xyz[n_built:], nrm[n_built:]
        acc, _, _ = _twin(kind, v, 1.0, xyz, nrm, cp.eps[kind], cp.cos_alpha[kind])
        # boxes of the points of one grid cell each (side 6: a few points per box, like a 64-point group's quarter)
        cell = np.floor((xyz - xyz.min(axis=0)) / 6.0).astype(np.int64)
        key = (cell[:, 0] * 64 + cell[:, 1]) * 64 + cell[:, 2]
        order = np.argsort(key, kind="stable")
        starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
        lo = np.minimum.reduceat(xyz[order], starts)
        hi = np.maximum.reduceat(xyz[order], starts)
        inl = np.logical_or.reduceat(acc[order], starts)
        boxes = np.hstack([(lo + hi) / 2.0, (hi - lo) / 2.0 * (1.0 + 1e-12) + 1e-9])
        assert (np.abs(boxes[:, :3] - (lo + hi) / 2.0) == 0).all()
        skip, ball, fields = _cylbox(np.array(v[:3]), np.array(v[3:6]), v[6], EPS, float(np.abs(xyz).max()), f32, boxes)
        assert np.isfinite(fields[:10]).all(), (v, fields)                 # the culling record is filled at these magnitudes
        assert not (skip & inl).any(), (v, f32, boxes[skip & inl][:2])
        assert not (ball & ~skip).any()
        nbox += len(boxes); nskip += int(skip.sum()); ninl += int(inl.sum())
    print("f32cloud=%d boxes %d skipped %d with a twin inlier %d" % (f32, nbox, nskip, ninl))
    assert nskip > nbox // 10 and ninl > 100, (nbox, nskip, ninl)


@pytest.mark.parametrize("f32", [0, 1], ids=["f64cloud", "f32cloud"])
def test_no_cell_with_an_accepted_normal_is_missing_from_a_far_plane_s_mask(f32):
    cp = plane_params(ALPHA_DEG)
    cosa = float(cp.cos_alpha[L.PLANE])
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(12, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    normals = np.vstack([normals, [[0.0, 0.0, 1.0], [1.0, 1.0, 0.0] / np.sqrt(2.0)]])
    for n in normals:
        dirs = rng.normal(size=(20_000, 3))
        dirs[::2] = n + rng.normal(scale=0.06, size=(10_000, 3))          # half of them about the plane's normal
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        cells = _cells(dirs)
        ok = (n[0] * dirs[:, 0] + n[1] * dirs[:, 1]) + n[2] * dirs[:, 2] > cosa     # the exact test's normal half (plane.jl), binary64
        assert 1000 < ok.sum() < 9000
        hit = np.unique(cells[ok])
        for far in FAR + (BIG - 50.0,):
            p0 = (far, -0.75 * far, 0.5 * far)
            for M in (far + 50.0, BIG):
                m = _mask(n, cp, M=M, f32=f32, p0=p0)
                assert m != ALL and bin(m).count("1") <= 16, (n, far, M)
                assert all((m >> int(k)) & 1 for k in hit), (n, far, M, [int(k) for k in hit if not (m >> int(k)) & 1])
            # beyond 2^20 the candidate is exact-only and its mask rules nothing out
            assert _mask(n, cp, M=BIG + 0.125, f32=f32, p0=p0) == ALL
        assert _mask(n, cp, M=100.0, f32=f32, p0=(BIG + 0.125, 0.0, 0.0)) == ALL
