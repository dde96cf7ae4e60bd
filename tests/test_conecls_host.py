"""Cones, host side (no GPU): the scene of tests/cone_scene.py against the oracle alone, and the cone's box test of the score
kernel's stage 1 (csrc/score4_device.h: cone_box_skip32 with the culling record of cls_make) as the HOST runs it --
rh_dbg_conebox, diag build: the very function of the kernel -- against brute force in numpy.

The scene is not vacuous (oracle only, binary64 and binary32 cloud): the exact copies hold more than 300 inliers, the inward
ones more than 50; in every band-edge and angle-edge family the exact test gives both verdicts; every on-axis and apex point is
rejected by every candidate through it; the points next to the apex and the in-band points at the axis guard are accepted by the
binary64 exact copy; between 0.30 and 0.37 of the points are disabled.

The box test.  D = c' rho + s' h is the closed form of the reference's distance (score4_device.h at cls_cone_ab), evaluated here
in numpy longdouble with the axis as stored and normalised.
Sound: whenever the function skips a (cone, box) pair, no point of the box has |D| < eps.  The points looked at: the 8 corners,
the centre, 200 random points, and the end points of a projected descent on |D| (p <- clip(p - D grad D), grad D being a unit
vector) from the centre and from each corner.
Not vacuous: for a finite record with band_ok (c > 1e-6 |(c, s)|) the function MUST skip whenever the centre lies outside the
axis guard four times over, rho_c^2 >= 4 s2 with s2 = f10 |t|^2 + f9, and
    |D_c| f7 > E (1 + 1e-3) + sqrt(s2) + 8 sl8 + 1e-3 (1 + |t| / 100),        E = hr f7 + f8,   sl8 = f8 - eps f7,
f6 .. f10 being the record's own fields (k, 1 / cn, (eps + slack) / cn + ek, beta, alpha) and hr the half diagonal: |D| at the
centre exceeds hr + eps by the record's own slack and the guard's width.  Why it then skips: with cn = c' > 0 and k = -s' / c',
D_c = cn (rho_c - k h_c), so g := |D_c| / cn - E is how far rho_c lies above hi = k h_c + E (D_c > 0) or below lo = k h_c - E
(D_c < 0).  The function wants rho_c^2 > hi^2 + s2 (or hi <= 0), resp. lo > 0 and rho_c^2 < lo^2 - s2; rho_c^2 - hi^2 =
g (hi + rho_c) >= g^2 + 2 g hi, and g > sqrt(s2) settles both in exact arithmetic.  In binary32: k h is off by at most ek <= sl8
(that is what ek holds: S 19.1 |k| u T and the binary64 prefilter's part), e by 1e-6 E, so hi and lo move by less than
2 sl8 + 1e-6 E and their squares by 2 hi (2 sl8 + 1e-6 E) + 3 u hi^2 <= g hi (g >= 8 sl8 + 1e-3 E, sl8 >= 19 |k| u T >= 3 u hi);
rho2 = tt - h^2 is off by 4 u |t|^2 <= s2 / 40 (alpha >= 162 u), which the factor 4 of the guard condition and
g^2 >= s2 + 2e-3 sqrt(s2) absorb.  The pairs held are counted per box shape (cube, plate, rod, flat) and per position family that
can lie clear of the band (around, far nappe, inside, far); the tangent boxes touch the band by design, boxes on the axis or about
the apex lie inside the guard and fall under "safe".
Safe: NaN or infinite fields, a zero axis, c <= 1e-6 |(c, s)| (opening angles from pi on), a NaN box and a box whose centre is
inside the axis guard (rho_c^2 < (f10 |t|^2 + f9) / 2) never skip."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc

import cone_scene as S

LD = np.longdouble
NRAND = 200
_dp = C.POINTER(C.c_double)


# ---------------------------------------------------------------- the scene against the oracle

def _params(eps=S.EPS, alpha=S.ALPHA):
    params = R.ransacparameters([R.FittedCone])
    params["cone"]["ϵ"] = float(eps)
    params["cone"]["α"] = float(alpha)
    return R.params_to_c(params)


def _orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


def _bits(masks):
    """(B, words) uint64 -> (B, N) bool"""
    return np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little")[:, :S.N].astype(bool)


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def verdicts(request):
    """the oracle's verdict on every (candidate, point) with all points enabled, and its counts with the scene's enabled bits"""
    f32 = request.param
    sc = S.scene()
    xyz, nrm = sc.arrays(f32)
    subs = np.arange(1, S.N + 1, dtype=np.int64)
    oc = orc.Cloud32(xyz, nrm, subs) if f32 else orc.Cloud(xyz, nrm, subs)
    arr = _orc(S.shapes(L.lib("diag"), L.Shape, f32), S.B)
    op = orc.Params.from_buffer_copy(bytes(_params()))
    _c, m = oc.score_batch(arr, op, want_masks=True)
    acc = _bits(m)
    oc.set_enabled(sc.enabled_chunks())
    counts = oc.score_batch(arr, op)
    assert np.array_equal(counts, (acc & sc.en).sum(axis=1))
    return f32, sc, acc, counts


def test_between_30_and_37_percent_of_the_points_are_disabled():
    sc = S.scene()
    assert 0.30 < 1.0 - sc.en.mean() < 0.37
    for name in ("ord", "narrow"):
        i = sc.fam[(name, "apex")]
        assert sc.en[i[0]] and not sc.en[i[1]]
    assert len(sc.cands) == S.B and sc.xyz.shape == (S.N, 3)


def test_exact_copies_hold_their_cones(verdicts):
    f32, sc, acc, counts = verdicts
    assert [sc.tags[i] for i in range(4)] == ["exact", "exact-in", "exact", "exact-in"]
    assert counts[0] > 300 and counts[2] > 300, counts[:4]
    assert counts[1] > 50 and counts[3] > 50, counts[:4]
    assert (counts[[i for i, t in enumerate(sc.tags) if t == "jitter"]] > 0).sum() > 80


def test_both_verdicts_in_every_edge_family(verdicts):
    f32, sc, acc, counts = verdicts
    for ci, name in ((0, "ord"), (2, "narrow")):
        for fam in ("band+", "band-", "angle"):
            idx = sc.fam[(name, fam)]
            v = acc[ci][idx]
            assert v.any() and not v.all(), (name, fam, int(v.sum()), len(v))
        vi = acc[ci + 1][sc.fam[(name, "angle")]]          # the flipped normals: the inward copy
        assert vi.any() and not vi.all(), (name, "angle, inwards")
        if not f32:
            # binary64 resolves the steps: inside the edge accepted, outside rejected, in order of k (k = 0 aside)
            idx = sc.fam[(name, "band+")]
            assert 0.4 * len(idx) < acc[ci][idx].sum() < 0.6 * len(idx)


def test_points_on_the_axis_and_apex_points_are_rejected_by_every_candidate_through_them(verdicts):
    f32, sc, acc, counts = verdicts
    for name in ("ord", "narrow"):
        thr = sc.through(name)
        assert len(thr) >= 6
        idx = np.concatenate([sc.fam[(name, "axis")], sc.fam[(name, "apex")]])
        assert len(idx) >= 11
        assert not acc[np.ix_(thr, idx)].any(), (name, np.argwhere(acc[np.ix_(thr, idx)])[:5])
    pinned = [i for i, t in enumerate(sc.tags) if t == "pinned"]
    assert len(pinned) == 2 and not acc[np.ix_(pinned, sc.fam[("-", "pin")])].any()


def test_points_beside_the_apex_and_in_band_points_at_the_guard_are_inliers_in_binary64_only(verdicts):
    f32, sc, acc, counts = verdicts
    for ci, name in ((0, "ord"), (2, "narrow")):
        if f32:          # binary32 puts the points beside the apex ON it: the frame is NaN
            assert not acc[ci][sc.fam[(name, "apexulp")]].any(), name
        else:
            assert acc[ci][sc.fam[(name, "apexulp")]].all(), name
            assert acc[ci][sc.fam[(name, "guard")]].sum() >= 100, name      # the two in-band heights: 132 points


def test_the_binary32_conversion_of_a_point_beside_the_apex_is_the_apex():
    sc = S.scene()
    for cone in S.CONES:
        p = sc.xyz[sc.fam[(cone["name"], "apexulp")]]
        assert (p != cone["apex"]).any(axis=1).all()
        assert (p.astype(np.float32) == cone["apex"].astype(np.float32)).all()


# ---------------------------------------------------------------- the box test on the host

def _shape(apex, axis, opang, f32=0, outwards=1):
    s = L.Shape()
    s.kind, s.outwards = L.CONE, outwards
    for i, v in enumerate(list(apex) + list(axis) + [opang]):
        s.v[i] = float(v)
    L.lib("diag").rh_shape_finalize(C.byref(s))
    if f32:
        L.lib("diag").rh_shape_finalize_f32(C.byref(s))
    return s


def _conebox(shape, eps, M, f32, boxes):
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    n = len(boxes)
    skip = np.zeros(n, dtype=np.uint8)
    fields = np.zeros(11, dtype=np.float32)
    cp = _params(eps)
    L.check(L.lib("diag").rh_dbg_conebox(C.byref(shape), C.byref(cp), float(M), 1.0, int(f32), boxes.ctypes.data_as(_dp), n,
                                         skip.ctypes.data_as(C.POINTER(C.c_uint8)), fields.ctypes.data_as(C.POINTER(C.c_float))))
    return skip.astype(bool), fields


def _D(apex, axis, cs, p, dtype=LD):
    """closed form with c', s' from the shape's own cos / sin; returns D, rho, h, |t|^2 and grad D (binary64 accuracy is enough for it)"""
    A, a = np.asarray(apex, dtype=dtype), np.asarray(axis, dtype=dtype)
    a = a / np.sqrt((a * a).sum())
    c, s = dtype(cs[0]), dtype(cs[1])
    n = np.sqrt(c * c + s * s)
    c, s = c / n, s / n
    t = np.asarray(p, dtype=dtype) - A
    h = t @ a
    q = t - h[..., None] * a
    rho = np.sqrt((q * q).sum(axis=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        er = np.where(rho[..., None] > 0, q / rho[..., None], 0)
    return c * rho + s * h, rho, h, (t * t).sum(axis=-1), c * er + s * a


def _descend(apex, axis, cs, start, lo, hi):
    p = start.copy()
    for _ in range(40):
        D, _r, _h, _t, g = _D(apex, axis, cs, p, np.float64)
        p = np.clip(p - D[..., None] * g, lo, hi)
    return p


def _extents(rng, s):
    """(shape name, half extents): cube, plates, rods, and a box with a zero half extent"""
    out = [("cube", np.full(3, s))]
    for k in range(3):
        p = np.full(3, s); p[k] = 1e-3 * s; out.append(("plate", p))
        r = np.full(3, 1e-2 * s); r[k] = s; out.append(("rod", r))
    z = np.full(3, s); z[rng.integers(3)] = 0.0; out.append(("flat", z))
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _cone_boxes(rng, A, a, opang, eps, far):
    """~30 boxes about one cone: (position family, shape name, box)"""
    hw = opang / 2
    tan, sin, cos = math.tan(hw), math.sin(hw), math.cos(hw)
    e1 = _unit(np.cross(a, [0.0, 1.0, 0.0]) if abs(a[1]) < 0.9 else np.cross(a, [1.0, 0.0, 0.0]))
    e2 = np.cross(a, e1)
    reach = min(far, 100.0)

    def er(phi):
        return math.cos(phi) * e1 + math.sin(phi) * e2

    def pick(s):
        ex = _extents(rng, s)
        return ex[rng.integers(len(ex))]
    out = []
    sizes = 10.0 ** rng.uniform(-3, math.log10(min(30.0, far)), 3)
    # around the surface of the nappe h > 0, from well inside to well outside
    for s in sizes:
        for shp, h3 in _extents(rng, s):
            h, e = rng.uniform(0.05, 0.6) * reach, er(rng.uniform(0, 2 * np.pi))
            d = rng.choice([-8.0, -2.0, -0.5, 0.0, 0.5, 1.0, 2.0, 8.0, 30.0]) * max(s, eps) + rng.normal() * eps
            out.append(("around", shp, np.concatenate([A + h * a + h * tan * e + d * (cos * e - sin * a), h3])))
    # tangent from outside at eps (1 +- 1e-6): the box's support point towards the surface lies on D = eps rel (a face, an edge
    # or a corner, by the zeros of the normal's components)
    for phi in (0.0, rng.uniform(0, 2 * np.pi)):
        for rel in (1 - 1e-6, 1 + 1e-6):
            h, e = rng.uniform(0.05, 0.6) * reach, er(phi)
            n = cos * e - sin * a
            n[np.abs(n) < 1e-12] = 0.0
            shp, h3 = pick(sizes[1])
            pt = A + h * a + h * tan * e + n * (eps * rel)
            out.append(("tangent", shp, np.concatenate([pt + np.sign(n) * h3, h3])))
    # about the apex, on the axis (both nappes)
    shp, h3 = pick(sizes[0])
    out.append(("apex", shp, np.concatenate([A + rng.uniform(-0.3, 0.3, 3) * h3, h3])))
    for sg in (1.0, -1.0):
        shp, h3 = pick(sizes[2])
        out.append(("axis", shp, np.concatenate([A + sg * rng.uniform(0.01, 0.5) * reach * a, h3])))
    # the far nappe: far from the apex, and tiny boxes INSIDE the band next to it (D = c' rho + sin |h| < eps)
    for _ in range(2):
        shp, h3 = pick(sizes[rng.integers(3)])
        h = rng.uniform(0.02, 0.5) * reach
        out.append(("farnappe", shp, np.concatenate([A - h * a + rng.uniform(0.05, 2.0) * h * er(rng.uniform(0, 2 * np.pi)), h3])))
    for _ in range(2):
        D = rng.uniform(0.3, 0.9) * eps
        h = rng.uniform(0.1, 0.8) * D / sin
        shp, h3 = pick(10.0 ** rng.uniform(-4, -2) * eps)
        out.append(("nearapex-", shp, np.concatenate([A - h * a + (D - sin * h) / cos * er(rng.uniform(0, 2 * np.pi)), h3])))
    # deep inside the cone, and far outside it
    for _ in range(2):
        shp, h3 = pick(sizes[rng.integers(3)])
        h = rng.uniform(0.2, 0.6) * reach
        out.append(("inside", shp, np.concatenate([A + h * a + rng.uniform(0.05, 0.5) * h * tan * er(rng.uniform(0, 2 * np.pi)), h3])))
        shp, h3 = pick(sizes[rng.integers(3)])
        out.append(("far", shp, np.concatenate([A + h * a + (h * tan + rng.uniform(5.0, 50.0) * (1 + far / 100.0)) / cos * er(rng.uniform(0, 2 * np.pi)), h3])))
    return out


def _cases():
    """(tag, apex, axis, opang, eps, boxes with their families): 104 cones, each with the Float64 and the Float32 flag"""
    rng = np.random.default_rng(2025)
    out = []
    for opang in (0.004, 0.1, 0.8, math.pi / 2, 2.5, math.pi - 1e-5):
        hw = opang / 2
        # "tilt": at azimuth 0 the surface normal is the x axis -- a box FACE faces the surface; "z": an EDGE; the others: a corner
        axes = [("z", (0.0, 0.0, 1.0)), ("tilt", (-math.sin(hw), 0.0, math.cos(hw))), ("skew", (0.36, 0.48, 0.8)), ("rnd", None), ("rnd2", None)]
        for name, av in axes:
            for eps, far, scale in ((0.3, 100.0, 1.0), (0.01, 2.0, 1.0), (0.3, 1e4, 1.0), (0.3, 100.0, 7.5), (0.3, 100.0, 1e-3)):
                if scale != 1.0 and name not in ("tilt", "rnd"):
                    continue
                if far == 1e4 and name not in ("z", "skew", "rnd"):
                    continue
                a = _unit(av) if av is not None else _unit(rng.normal(size=3))
                A = rng.uniform(-far, far, 3) if far <= 100.0 else np.array([9.1e3, -9.6e3, 9.9e3]) + rng.uniform(-50, 50, 3)
                out.append(("%s-w=%g-eps=%g-far=%g-x%g" % (name, opang, eps, far, scale), A, a * scale, opang, eps, _cone_boxes(rng, A, a, opang, eps, far)))
    return out


@pytest.fixture(scope="module")
def results():
    """every case run once: the function's decisions with both flags, the record, and the brute-force distances"""
    rng = np.random.default_rng(77)
    corners = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
    res = []
    for tag, A, a, opang, eps, fb in _cases():
        boxes = np.array([b for _f, _s, b in fb])
        c, h = boxes[:, :3], boxes[:, 3:]
        M = float(np.abs(np.concatenate([c - h, c + h])).max())
        starts = np.concatenate([c[:, None, :], c[:, None, :] + corners[None] * h[:, None, :]], axis=1)
        for f32 in (0, 1):
            sh = _shape(A, a, opang, f32)
            cs = (sh.v[7], sh.v[8])
            apex, axis = np.array(sh.v[0:3]), np.array(sh.v[3:6])
            skip, fields = _conebox(sh, eps, M, f32, boxes)
            pts = np.concatenate([starts, c[:, None, :] + rng.uniform(-1, 1, size=(len(boxes), NRAND, 3)) * h[:, None, :],
                                  _descend(apex, axis, cs, starts, (c - h)[:, None, :], (c + h)[:, None, :])], axis=1)
            D = _D(apex, axis, cs, pts)[0]
            Dc, rc, hc, ttc, _g = _D(apex, axis, cs, c)
            res.append(dict(tag=tag + "-f32=%d" % f32, eps=eps, f32=f32, boxes=boxes, fam=[f for f, _s, _b in fb], shp=[s for _f, s, _b in fb],
                            skip=skip, fields=fields.astype(np.float64), absD=np.abs(D).min(axis=1).astype(np.float64),
                            Dc=Dc.astype(np.float64), rc=rc.astype(np.float64), hc=hc.astype(np.float64), ttc=ttc.astype(np.float64),
                            hr=np.sqrt((h * h).sum(axis=1))))
    return res


def test_enough_pairs_of_every_sort(results):
    n = sum(len(r["boxes"]) for r in results)
    assert len(results) >= 200 and n >= 6000, (len(results), n)
    assert sum(r["skip"].sum() for r in results) > n // 6 and sum((~r["skip"]).sum() for r in results) > n // 6
    for fam in ("around", "farnappe", "inside", "far"):
        assert sum((r["skip"] & (np.array(r["fam"]) == fam)).sum() for r in results) > 20, fam
    # the tangent boxes touch D = eps (1 +- 1e-6): half of them hold a point of the band -- by a hair --, and the brute force sees it
    tang = [(r["absD"][i] < r["eps"]) for r in results for i in np.flatnonzero(np.array(r["fam"]) == "tangent")]
    assert len(tang) >= 800 and 0.4 * len(tang) <= sum(tang) <= 0.6 * len(tang), (len(tang), sum(tang))
    near = [(r["absD"][i] < r["eps"]) for r in results for i in np.flatnonzero(np.array(r["fam"]) == "nearapex-")]
    assert len(near) >= 400 and all(near)
    band = sum((r["absD"] < r["eps"]).sum() for r in results)
    assert band > n // 10


def test_a_skipped_box_holds_no_point_of_the_band(results):
    for r in results:
        bad = r["skip"] & (r["absD"] < r["eps"])
        assert not bad.any(), (r["tag"], np.flatnonzero(bad)[:4], [r["fam"][i] for i in np.flatnonzero(bad)[:4]], r["boxes"][bad][:2], r["absD"][bad][:4])


def _guard_s2(r):
    f = r["fields"]
    return f[10] * r["ttc"] + f[9]


def test_skips_whenever_the_centre_clears_the_widened_band(results):
    by_shape, by_fam = {}, {}
    for r in results:
        f = r["fields"]
        if not np.isfinite(f).all():
            continue
        s2 = _guard_s2(r)
        E = r["hr"] * f[7] + f[8]
        sl8 = f[8] - r["eps"] * f[7]
        assert sl8 > 0
        clear = (r["rc"] ** 2 >= 4.0 * s2) & (np.abs(r["Dc"]) * f[7] > E * (1 + 1e-3) + np.sqrt(s2) + 8.0 * sl8 + 1e-3 * (1.0 + np.sqrt(r["ttc"]) / 100.0))
        assert r["skip"][clear].all(), (r["tag"], np.flatnonzero(clear & ~r["skip"])[:4], [r["fam"][i] for i in np.flatnonzero(clear & ~r["skip"])[:4]])
        for i in np.flatnonzero(clear):
            by_shape[r["shp"][i]] = by_shape.get(r["shp"][i], 0) + 1
            by_fam[r["fam"][i]] = by_fam.get(r["fam"][i], 0) + 1
    print("pairs held to skip, by box shape:", by_shape, "by position:", by_fam)
    for shp in ("cube", "plate", "rod", "flat"):
        assert by_shape.get(shp, 0) > 0, shp
    for fam in ("around", "farnappe", "inside", "far"):
        assert by_fam.get(fam, 0) > 0, fam


def test_a_box_centred_inside_the_axis_guard_is_never_skipped(results):
    seen = 0
    for r in results:
        if not np.isfinite(r["fields"]).all():
            continue
        inside = r["rc"] ** 2 < 0.5 * _guard_s2(r)
        assert not (r["skip"] & inside).any(), (r["tag"], np.flatnonzero(r["skip"] & inside)[:4])
        seen += int(inside.sum())
        fam = np.array(r["fam"])
        assert inside[fam == "axis"].all()
    assert seen >= 3 * len(results) // 2


BOXES = np.array([[50.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.0, 300.0, 5.0, 2.0, 1e-3, 2.0], [1e3, 1e3, -1e3, 0.5, 0.5, 0.5], [10.0, 2.0, -40.0, 0.5, 0.5, 0.5]])


def _raw(v, eps, M, f32, boxes=BOXES):
    s = L.Shape()
    s.kind, s.outwards = L.CONE, 1
    for i, x in enumerate(v):
        s.v[i] = float(x)
    return _conebox(s, eps, M, f32, boxes)


@pytest.mark.parametrize("f32", [0, 1])
def test_nan_inf_a_zero_axis_and_wide_cones_never_skip(f32):
    hw = 0.4
    good = [1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 2 * hw, math.cos(-hw), math.sin(-hw)]
    skip, fields = _raw(good, 0.3, 2e3, f32)
    assert skip.all() and np.isfinite(fields).all()             # (these boxes are far outside, one on the far nappe: a usable record skips them)
    for bad in (np.nan, np.inf, -np.inf):
        for i in (0, 1, 2, 3, 4, 5, 7, 8):
            v = list(good)
            v[i] = bad
            skip, _ = _raw(v, 0.3, 2e3, f32)
            assert not skip.any(), (bad, i)
        assert not _raw(good, bad, 2e3, f32)[0].any(), ("eps", bad)
        assert not _raw(good, 0.3, bad, f32)[0].any(), ("M", bad)
    v = list(good); v[3:6] = [0.0, 0.0, 0.0]
    skip, fields = _raw(v, 0.3, 2e3, f32)
    assert not skip.any() and np.isnan(fields).all()
    # c <= 1e-6 |(c, s)|: opening angles at and beyond pi, and a hair below
    for w in (math.pi, math.pi + 0.3, 2 * math.pi - 0.1, math.pi - 1e-6):
        sh = _shape(good[:3], good[3:6], w, f32)
        assert not sh.v[7] > 1e-6
        skip, fields = _conebox(sh, 0.3, 2e3, f32, BOXES)
        assert not skip.any() and np.isnan(fields).all(), w
    for i in range(6):
        for bad in (np.nan, np.inf):
            b = BOXES.copy()
            b[:, i] = bad
            assert not _raw(good, 0.3, 2e3, f32, b)[0].any(), ("box", i, bad)


def test_an_apex_too_far_for_binary32_keeps_its_record_unusable():
    hw = 0.4
    skip, fields = _raw([2.0 ** 20 + 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2 * hw, math.cos(-hw), math.sin(-hw)], 0.3, 2e3, 0)
    assert not skip.any() and np.isnan(fields).all()


# ---------------------------------------------------------------- the widths of the classifier record

def _record(shape, M, Nm, f32):
    """cls_make's cone record and its dbg4 = (0, wL, eD_lo, wD) through rh_dbg_cls_cone with no points: host code only"""
    rec, d4 = np.zeros(16, dtype=np.float32), np.zeros(4)
    L.check(L.lib("diag").rh_dbg_cls_cone(C.byref(shape), C.byref(_params()), float(M), float(Nm), int(f32), 0, None, None, 0, None, None, None,
                                          rec.ctypes.data_as(C.POINTER(C.c_float)), d4.ctypes.data_as(_dp)))
    return rec, d4


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
def test_the_widths_are_twice_the_safety_factor_times_the_first_order_bounds(f32):
    """On this scene the binary32 error of the cone's ua and ub stays below 0.04 of a width (test_conecls_diag_gpu.py prints it), so
    no point can notice a margin that lost half its size: the widths are held to the derivation itself (score4_device.h, Margins),
        mD = S (|c'| (sqrt(3) e_q + 5.5 u rmax) + |s'| (6 u |a^|_1 T + 2 u rmax) + 4 u eps) + 1e-11 (1 + T),
        mL = S (e_q (3 Nm |c'| + sqrt(3) G) + u rmax (8.7 Nm |c'| + 6.5 G + 7 |s'| |a^|_1 Nm + 2 |c|)) + 1e-11 (1 + T) (1 + Nm),
    S = 2, u = 2^-24, T = M + max |apex|, rmax = sqrt(3) T, e_q = u T (3.01 + 8.04 |a^|_inf |a^|_1), G = sqrt(3) Nm (|c'| + |s'|) + |c| + 1/4,
    c = cos(alpha), restated here from the header's text: wD = 2 mD and wL = 2 mL to 1e-9 on the Float64 cloud; on the Float32
    cloud wD is no smaller (it adds the exact chain's part) and wL is infinite.  eD_lo = eps - wD / 2, and the axis guard's beta is
    no smaller than S 1.75 u T^2."""
    sc = S.scene()
    xyz, nrm = sc.arrays(bool(f32))
    M, Nm = float(np.abs(xyz).max()), float(np.abs(nrm).max())
    arr = S.shapes(L.lib("diag"), L.Shape, bool(f32))
    u, s3, Sf, c = S.U24, math.sqrt(3.0), 2.0, math.cos(S.ALPHA)
    seen = 0
    for i in range(S.B):
        rec, d4 = _record(arr[i], M, Nm, f32)
        if np.isnan(rec[15]):
            assert sc.tags[i] == "huge" or (f32 and sc.tags[i] == "opang"), (i, sc.tags[i])
            continue
        v = np.array(arr[i].v[:9])
        a = v[3:6] / np.linalg.norm(v[3:6])
        cn = math.hypot(v[7], v[8])
        cp, sp = abs(v[7]) / cn, abs(v[8]) / cn
        T = M + np.abs(v[:3]).max()
        a1, ai = np.abs(a).sum(), np.abs(a).max()
        eq, rmax = u * T * (3.01 + 8.04 * ai * a1), s3 * T
        mD = Sf * (cp * (s3 * eq + 5.5 * u * rmax) + sp * (6.0 * u * a1 * T + 2.0 * u * rmax) + 4.0 * u * S.EPS)
        G = s3 * Nm * (cp + sp) + c + 0.25
        mL = Sf * (eq * (3.0 * Nm * cp + s3 * G) + u * rmax * (8.7 * Nm * cp + 6.5 * G + 7.0 * sp * a1 * Nm + 2.0 * c))
        wL, eDlo, wD = d4[1], d4[2], d4[3]
        assert abs(eDlo - (S.EPS - 0.5 * wD)) <= 1e-12 * (1 + wD), (i, sc.tags[i])
        assert rec[12] >= Sf * 1.75 * u * T * T
        if f32:
            assert wD >= 2.0 * mD and np.isinf(wL), (i, sc.tags[i], wD, 2 * mD)
        else:
            assert abs(wD - 2.0 * (mD + 1e-11 * (1 + T))) <= 1e-9 * wD, (i, sc.tags[i], wD, 2 * mD)
            assert abs(wL - 2.0 * (mL + 1e-11 * (1 + T) * (1 + Nm))) <= 1e-9 * wL, (i, sc.tags[i], wL, 2 * mL)
        seen += 1
    assert seen >= S.B - 6
