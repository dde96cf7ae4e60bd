"""The cylinder's box test of the score kernel's stage 1 (csrc/score4_device.h: cyl_box_skip32 with the culling record of
cls_make, "The cylinder's box by its support") as the HOST runs it -- rh_dbg_cylbox, diag build, no GPU: the very function of the
kernel -- against brute force in numpy.

Sound: whenever the function skips a (cylinder, box) pair, no point of the box lies in the band |rho - R| < eps, rho being the
distance from the axis in binary64 with the axis as stored.  The points looked at: the 8 corners, the centre, 200 random
points, and the point of the box nearest the axis (the best of the 27 sign patterns of the KKT conditions, each coordinate at
its lower face, its upper face or free).

Not vacuous: for a unit axis and a finite record the function MUST skip whenever the exact-arithmetic bound clears the band,
    rho_c - s / rho_c > (R + eps) (1 + 1e-3) + max(1e-3, 8 sB (1 + (hx + hy + hz) / rho_c)),
sB = record field 6 - (R + eps) being cls_make's own slack of the box test.  Why the function then skips: its clause is
w^2 > A2 rho_c^2 with A = (R + eps) + sB + S 3.01 u c_g M <= (R + eps) + 2.75 sB (sB >= S sqrt(3) e_q, c_g against e_q's
constants), evaluated on binary32 values that differ from the exact ones by |rho' - rho_c| <= sqrt(3) e_q <= sB / 2, by
|s' / rho' - s / rho_c| <= 2 e_q (hx + hy + hz) / rho_c + 2 sqrt(3) e_q <= sB (0.6 (hx + hy + hz) / rho_c + 1) (the direction of
q moves by e_q / rho_c, which the box's long sides multiply; rho' >= rho_c / 2 since rho_c > 27 e_q), and by the factor
0.999999 on rho_c^2, below sB; the parts in 10^6 of the squares and of the rounded-up fields vanish in (R + eps) 1e-3.
Together 5.25 sB + 0.6 sB (hx + hy + hz) / rho_c.  At coordinates beyond some tens (and on a Float32 cloud, whose slack is
tripled) 8 sB exceeds 1e-3 -- binary32 resolves 1e4 to 1e-3 --, which is why the margin is taken from the record there; the
test counts the pairs it held at the plain 1e-3.

Monotone and safe: the two ball clauses alone skip => the function skips; NaN or infinite shape fields, a zero axis and a NaN
box never skip."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

NRAND = 200
U = 2.0 ** -24


def _params(eps):
    params = R.ransacparameters([R.FittedCylinder])
    params["cylinder"]["ϵ"] = float(eps)
    return R.params_to_c(params)


def _shape(a, c0, Rr):
    s = L.Shape()
    s.kind, s.outwards = L.CYLINDER, 1
    for i, v in enumerate(list(a) + list(c0) + [Rr]):
        s.v[i] = float(v)
    return s


def _cylbox(a, c0, Rr, eps, M, f32, boxes):
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    n = len(boxes)
    skip, ball = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    fields = np.zeros(11, dtype=np.float32)
    s, cp = _shape(a, c0, Rr), _params(eps)
    L.check(L.lib("diag").rh_dbg_cylbox(C.byref(s), C.byref(cp), float(M), 1.0, int(f32), boxes.ctypes.data_as(C.POINTER(C.c_double)), n,
                                        skip.ctypes.data_as(C.POINTER(C.c_uint8)), ball.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        fields.ctypes.data_as(C.POINTER(C.c_float))))
    return skip.astype(bool), ball.astype(bool), fields


def _rho(a, c0, p):
    """distance from the axis as the exact test states it: |t - a (a . t)|, the axis as stored"""
    t = p - c0
    q = t - a * (t @ a)[..., None]
    return np.sqrt((q * q).sum(axis=-1))


def _nearest(a, c0, boxes):
    """per box the point nearest the axis among the 27 KKT sign patterns (coordinate k at c - h, at c + h, or free: the free
    ones minimise |M (t_fixed + x_free)|^2, M = I - a a'), clipped into the box"""
    c, h = boxes[:, :3], boxes[:, 3:]
    Mm = np.eye(3) - np.outer(a, a)
    best, bestp = np.full(len(boxes), np.inf), c.copy()
    for pat in itertools.product((-1, 0, 1), repeat=3):
        pat = np.array(pat)
        free = pat == 0
        p = c + pat * h
        if free.any():
            A = Mm[:, free]
            x = -(np.linalg.pinv(A) @ (Mm @ (p - c0).T)).T        # offsets of the free coordinates from the centre
            p[:, free] = np.clip(c[:, free] + x, c[:, free] - h[:, free], c[:, free] + h[:, free])
        r = _rho(a, c0, p)
        take = r < best
        best[take], bestp[take] = r[take], p[take]
    return bestp


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _perp(a, rng):
    v = rng.normal(size=3)
    return _unit(v - a * (v @ a) / (a @ a))


def _extents(rng, s):
    """cube, plates (one half extent 1e-3 of the others, each axis in turn), rods, and a box with a zero half extent"""
    out = [np.full(3, s)]
    for k in range(3):
        p = np.full(3, s); p[k] = 1e-3 * s; out.append(p)
        r = np.full(3, 1e-2 * s); r[k] = s; out.append(r)
    z = np.full(3, s); z[rng.integers(3)] = 0.0; out.append(z)
    return out


AXES = [("x", (1, 0, 0)), ("z", (0, 0, 1)), ("face", (1, 1, 0)), ("face2", (0, -1, 1)), ("space", (1, 1, 1)), ("space2", (1, -1, 1)),
        ("rnd", None), ("rnd2", None)]
# tangent directions n (perpendicular to the axis): a box FACE, EDGE or CORNER faces the shell
TANGENT = {"x": [(0, 1, 0), (0, 1, -1)], "z": [(1, 0, 0), (1, 1, 0)], "face": [(0, 0, 1), (1, -1, 0), (1, -1, 1)], "face2": [(1, 0, 0), (0, 1, 1), (1, 1, 1)],
           "space": [(1, -1, 0), (1, 1, -2)], "space2": [(1, 1, 0), (1, 2, 1)]}


def _cases():
    """(tag, a, c0, R, eps, f32, boxes, unit): 214 cylinders (each with the Float64 and the Float32 flag), ~30 boxes each"""
    rng = np.random.default_rng(2024)
    out = []
    for name, av in AXES:
        for scale2 in (1.0, 1.0 + 1e-3, 1.0 - 1e-3, 2.0):
            for eps, Rr, far in ((0.3, 1e-3, 100.0), (0.3, 5.0, 100.0), (0.01, 1.0, 100.0), (0.3, 40.0, 100.0), (0.3, 1e3, 100.0), (0.3, 7.0, 1e4),
                                   (0.3, 1.0, 2.0), (0.01, 0.5, 2.0)):         # (far = 2: coordinates small enough for the plain 1e-3 margin)
                if scale2 != 1.0 and (Rr not in (5.0, 40.0) or far != 100.0):
                    continue
                if far == 1e4 and name not in ("z", "space", "rnd"):
                    continue
                a1 = _unit(av) if av is not None else _unit(rng.normal(size=3))
                a = a1 * np.sqrt(scale2)
                c0 = rng.uniform(-far, far, 3) if far <= 100.0 else np.array([9.1e3, -9.6e3, 9.9e3]) + rng.uniform(-50, 50, 3)
                boxes = []
                sizes = 10.0 ** rng.uniform(-3, np.log10(min(50.0, far)), 3)
                along = 0.3 * min(far, 100.0)
                for s in sizes:
                    for h in _extents(rng, s):
                        n = _perp(a1, rng)
                        # centres around the shell: from well inside to well outside, in units of the box and of eps
                        d = rng.choice([-2.0, -0.5, 0.0, 0.5, 1.0, 2.0, 8.0]) * max(s, eps) + rng.normal() * eps
                        boxes.append(np.concatenate([c0 + a1 * rng.uniform(-along, along) + n * (Rr + d), h]))
                # the axis through the box centre
                boxes.append(np.concatenate([c0 + a1 * rng.uniform(-along, along), _extents(rng, sizes[0])[rng.integers(8)]]))
                # the shell tangent to a face, an edge, a corner from outside at eps (1 +- 1e-6)
                for nv in TANGENT.get(name, [tuple(_perp(a1, rng))]):
                    n = _unit(nv)
                    assert abs(n @ a1) < 1e-12
                    for rel in (1 - 1e-6, 1 + 1e-6):
                        h = _extents(rng, sizes[1])[rng.integers(7)]
                        pt = c0 + a1 * rng.uniform(-along, along) + n * (Rr + eps * rel)
                        boxes.append(np.concatenate([pt + np.sign(n) * h, h]))
                for f32 in (0, 1):
                    out.append(("%s-a2=%g-R=%g-eps=%g-far=%g-f32=%d" % (name, scale2, Rr, eps, far, f32), a, c0, Rr, eps, f32, np.array(boxes), scale2 == 1.0))
    return out


@pytest.fixture(scope="module")
def results():
    """every case run once: the function's decisions, the record, and the brute-force distances"""
    rng = np.random.default_rng(99)
    res = []
    for tag, a, c0, Rr, eps, f32, boxes, unit in _cases():
        c, h = boxes[:, :3], boxes[:, 3:]
        M = float(np.abs(np.concatenate([c - h, c + h])).max())
        skip, ball, fields = _cylbox(a, c0, Rr, eps, M, f32, boxes)
        corners = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
        pts = np.concatenate([c[:, None, :] + corners[None] * h[:, None, :], c[:, None, :],
                              c[:, None, :] + rng.uniform(-1, 1, size=(len(boxes), NRAND, 3)) * h[:, None, :],
                              _nearest(a, c0, boxes)[:, None, :]], axis=1)
        rho = _rho(a, c0, pts)
        res.append(dict(tag=tag, a=a, c0=c0, R=Rr, eps=eps, f32=f32, boxes=boxes, unit=unit, skip=skip, ball=ball, fields=fields, rho=rho))
    return res


def test_enough_pairs_of_every_sort(results):
    n = sum(len(r["boxes"]) for r in results)
    assert n >= 3000
    assert sum(r["skip"].sum() for r in results) > n // 5 and sum((~r["skip"]).sum() for r in results) > n // 5
    assert sum((r["skip"] & ~r["ball"]).sum() for r in results) > 100      # the support clause adds pairs of its own


def test_a_skipped_box_holds_no_point_of_the_band(results):
    for r in results:
        band = (np.abs(r["rho"] - r["R"]) < r["eps"]).any(axis=1)
        bad = r["skip"] & band
        assert not bad.any(), (r["tag"], np.flatnonzero(bad)[:4], r["boxes"][bad][:2])


def test_the_ball_clauses_alone_never_skip_more(results):
    for r in results:
        assert not (r["ball"] & ~r["skip"]).any(), r["tag"]


def test_skips_whenever_the_exact_bound_clears_the_band(results):
    held = plain = 0
    for r in results:
        if not r["unit"] or not np.isfinite(r["fields"][:10]).all():
            continue
        a, c0, Rr, eps = r["a"], r["c0"], r["R"], r["eps"]
        c, h = r["boxes"][:, :3], r["boxes"][:, 3:]
        t = c - c0
        q = t - a * (t @ a)[:, None]
        rc = np.sqrt((q * q).sum(axis=1))
        s = (np.abs(q) * h).sum(axis=1)
        sB = float(r["fields"][6]) - (Rr + eps)
        assert sB > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            derived = 8.0 * sB * (1.0 + h.sum(axis=1) / rc)
            clear = rc - s / rc > (Rr + eps) * (1 + 1e-3) + np.maximum(1e-3, derived)
        clear &= rc > 0
        assert r["skip"][clear].all(), (r["tag"], np.flatnonzero(clear & ~r["skip"])[:4], sB)
        held += int(clear.sum())
        plain += int((clear & (derived <= 1e-3)).sum())
    print("pairs held to skip: %d, of them at the plain margin 1e-3: %d" % (held, plain))
    assert held >= 500 and plain >= 100


def test_coordinates_near_1e4_are_among_the_cases(results):
    assert sum(np.abs(r["c0"]).max() > 9e3 for r in results) >= 4


BOXES = np.array([[50.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.0, 300.0, 5.0, 2.0, 1e-3, 2.0], [1e3, 1e3, 1e3, 0.5, 0.5, 0.5]])


@pytest.mark.parametrize("f32", [0, 1])
def test_nan_inf_and_a_zero_axis_never_skip(f32):
    good = dict(a=np.array([0.0, 0.0, 1.0]), c0=np.array([1.0, 2.0, 3.0]), Rr=2.0)
    skip, ball, fields = _cylbox(good["a"], good["c0"], good["Rr"], 0.3, 2e3, f32, BOXES)
    assert skip.all() and np.isfinite(fields[:10]).all()            # (these boxes are far outside: a usable record skips them)
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(7):
            v = list(good["a"]) + list(good["c0"]) + [good["Rr"]]
            v[i] = bad
            skip, ball, _ = _cylbox(v[:3], v[3:6], v[6], 0.3, 2e3, f32, BOXES)
            assert not skip.any() and not ball.any(), (bad, i)
        skip, ball, _ = _cylbox(good["a"], good["c0"], good["Rr"], bad, 2e3, f32, BOXES)
        assert not skip.any() and not ball.any(), ("eps", bad)
        skip, ball, _ = _cylbox(good["a"], good["c0"], good["Rr"], 0.3, bad, f32, BOXES)
        assert not skip.any() and not ball.any(), ("M", bad)
    skip, ball, fields = _cylbox(np.zeros(3), good["c0"], good["Rr"], 0.3, 2e3, f32, BOXES)
    assert not skip.any() and not ball.any() and np.isnan(fields[:10]).all()
    for i in range(6):
        for bad in (np.nan, np.inf):
            b = BOXES.copy()
            b[:, i] = bad
            skip, ball, _ = _cylbox(good["a"], good["c0"], good["Rr"], 0.3, 2e3, f32, b)
            assert not skip.any() and not ball.any(), ("box", i, bad)


def test_an_axis_too_long_for_binary32_keeps_its_record_unusable():
    skip, ball, fields = _cylbox(np.array([0.0, 0.0, 17.0]), np.zeros(3), 2.0, 0.3, 2e3, 0, BOXES)
    assert not skip.any() and not ball.any() and np.isnan(fields[:10]).all()
