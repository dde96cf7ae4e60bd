"""The root-free classifier of the round kinds (csrc/score4_device.h, "Round kinds without a square root": cls_make's record and
the kernel's own cls_round_ab) as the HOST runs it -- rh_dbg_cls_round, diag build, no GPU -- against a numpy binary64 twin of
the exact tests (csrc/score_device.h test_sphere / test_cylinder) in the reference's operation order.

Sound: u = max(ua, ub) < 0 only where the twin accepts, u > 1 only where it rejects, without exception; the all-zero point a
disabled point is staged as has u > 1; no u is NaN; candidates outside a guard carry the NaN flag (exact-only).

Not vacuous: a point farther than 4 widths (W2, Wv as cls_make reports them) from both thresholds, measured in the twin's own
binary64 quantities  | |n2 - K| - H |  and  | s |s| - cos^2(alpha) n2 |,  MUST be decided.  (Why it then is: the margins are
half a width, and they are bounds of the binary32 error wherever ua can be <= 1; beyond nrmax the error of n2 is relative and
|n2 - K| - H grows faster; for a normal far against the shape's the error 2 |s| ds <= s^2 / 2 + 2 ds^2 stays below |v| / 2 + mv / 3.)
The twin alone places more than 99 % of the random points there: the share is asserted from the twin.

Candidates: spheres and cylinders, outwards and inwards, R in {0.5, 5, 500}, centres offset by 0, 100 and 1e4, cylinder axes of
length 1e-3, 1 and 7.5 along a coordinate axis and oblique, (eps, alpha) as in test_binary32_classifier_stays_inside_its_margins.
Points: at nr = (R +- eps) (1 +- k 2^-24), k = 0 .. 64, with the shell's normal; at nr = R with the normal at alpha (1 +- k 2^-23)
from it; the all-zero point; a point on the centre / axis; and random points of a box of half side max(50, 2 R) about the centre with random
unit normals (2 10^5 over the candidates of a kind and setting)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

SETTINGS = [(0.3, 5.0), (0.01, 1.0), (5.0, 60.0)]
RADII = (0.5, 5.0, 500.0)
OFFSETS = (0.0, 100.0, 1e4)
AXES = [(s, d) for s in (1e-3, 1.0, 7.5) for d in ((0.0, 0.0, 1.0), (0.48, -0.6, 0.64))]
N_RANDOM = 200_000
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)


def _params(eps, alpha_deg):
    params = R.ransacparameters([R.FittedSphere, R.FittedCylinder])
    for k in ("sphere", "cylinder"):
        params[k]["ϵ"] = float(eps)
        params[k]["α"] = math.radians(alpha_deg)
    return R.params_to_c(params)


def _shape(kind, outwards, v):
    s = L.Shape()
    s.kind, s.outwards = kind, int(outwards)
    for i, x in enumerate(v):
        s.v[i] = float(x)
    return s


def _run(shape, cp, M, Nm, xyz, nrm, f32=0):
    n = len(xyz)
    xyz, nrm = np.ascontiguousarray(xyz, dtype=np.float64), np.ascontiguousarray(nrm, dtype=np.float64)
    ua, ub = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    rec, d4 = np.zeros(16, dtype=np.float32), np.zeros(4)
    L.check(L.lib("diag").rh_dbg_cls_round(C.byref(shape), C.byref(cp), float(M), float(Nm), int(f32), n, xyz.ctypes.data_as(_dp),
                                           nrm.ctypes.data_as(_dp), ua.ctypes.data_as(_fp), ub.ctypes.data_as(_fp), rec.ctypes.data_as(_fp),
                                           d4.ctypes.data_as(_dp)))
    return ua, ub, rec, d4


def _twin(kind, v, sgn, xyz, nrm, eps, cosa):
    """the exact test in binary64, operation for operation (score_device.h); also n2 and s = sgn (q . n) of the same q"""
    px, py, pz = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if kind == L.SPHERE:
        qx, qy, qz = px - v[0], py - v[1], pz - v[2]
        Rr = v[3]
    else:
        ax, ay, az, cx, cy, cz = v[:6]
        tx, ty, tz = px - cx, py - cy, pz - cz
        sd = (ax * tx + ay * ty) + az * tz
        qx, qy, qz = (px - ax * sd) - cx, (py - ay * sd) - cy, (pz - az * sd) - cz
        Rr = v[6]
    n2 = (qx * qx + qy * qy) + qz * qz
    with np.errstate(divide="ignore", invalid="ignore"):
        nr = np.sqrt(n2)
        inv = 1.0 / nr
        ux, uy, uz = inv * qx, inv * qy, inv * qz
        dt = (ux * nx + uy * ny) + uz * nz
        acc = (np.abs(nr - Rr) < eps) & (sgn * dt > cosa)
    s = sgn * ((qx * nx + qy * ny) + qz * nz)
    return acc, n2, s


def _perp(d):
    t = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
    return t / np.linalg.norm(t)


def _points(kind, v, sgn, eps, alpha, n_random, rng):
    """the points of one candidate: built on the thresholds, the zero point, one on the centre / axis, random ones"""
    if kind == L.SPHERE:
        c0, Rr, axis = np.array(v[:3]), v[3], None
    else:
        c0, Rr, axis = np.array(v[3:6]), v[6], np.array(v[:3])
    ah = None if axis is None else axis / np.linalg.norm(axis)
    k = np.arange(65)
    P, Nn = [], []
    for trial in range(3):
        d = rng.normal(size=3)
        if ah is not None:
            d -= ah * (d @ ah)          # perpendicular to the axis: q = t whatever the axis' length
        d /= np.linalg.norm(d)
        t = _perp(d) if ah is None else np.cross(ah, d)
        # a unit axis may carry the point along itself as well
        shift = ah * rng.uniform(-20, 20) if ah is not None and abs(np.linalg.norm(axis) - 1.0) < 1e-12 else 0.0
        for edge in (Rr - eps, Rr + eps):
            for sg in (-1.0, 1.0):
                nr = edge * (1.0 + sg * k * 2.0 ** -24)
                P.append(c0 + shift + nr[:, None] * d)
                Nn.append(np.tile(sgn * d, (65, 1)))
        for sg in (-1.0, 1.0):
            th = alpha * (1.0 + sg * k * 2.0 ** -23)
            P.append(np.tile(c0 + shift + Rr * d, (65, 1)))
            Nn.append(sgn * (np.cos(th)[:, None] * d + np.sin(th)[:, None] * t))
    P.append(np.zeros((1, 3))); Nn.append(np.zeros((1, 3)))                                 # the zero point, then one on the centre / axis
    P.append((c0 if ah is None else c0 + 3.0 * axis)[None, :]); Nn.append(np.array([[0.6, 0.0, 0.8]]))
    n_built = sum(len(p) for p in P)
    half = max(50.0, 2.0 * Rr)          # a cloud about the shape: the box holds the whole sphere / the cylinder's cross-section
    P.append(c0 + rng.uniform(-half, half, (n_random, 3)))
    nn = rng.normal(size=(n_random, 3))
    Nn.append(nn / np.linalg.norm(nn, axis=1)[:, None])
    return np.vstack(P), np.vstack(Nn), n_built - 2, n_built


def _candidates(kind):
    for outwards, Rr, off in itertools.product((1, 0), RADII, OFFSETS):
        c0 = [off, off * 0.75, -off * 0.5]
        if kind == L.SPHERE:
            yield outwards, c0 + [Rr], True
        else:
            for s, d in AXES:
                yield outwards, [s * x for x in d] + c0 + [Rr], s == 1.0


@pytest.mark.parametrize("eps,alpha_deg", SETTINGS)
@pytest.mark.parametrize("kind", [L.SPHERE, L.CYLINDER], ids=["sphere", "cylinder"])
def test_decisions_are_sound_and_far_points_are_decided(kind, eps, alpha_deg):
    cp = _params(eps, alpha_deg)
    eps_c, cosa = cp.eps[kind], cp.cos_alpha[kind]
    rng = np.random.default_rng(11 + kind)
    cands = list(_candidates(kind))
    n_random = -(-N_RANDOM // len(cands))
    usable = far_total = rand_total = 0
    for outwards, v, plain_axis in cands:
        sgn = 1.0 if outwards else -1.0
        xyz, nrm, i_zero, n_built = _points(kind, v, sgn, eps_c, math.radians(alpha_deg), n_random, rng)
        M, Nm = np.abs(xyz).max(), np.abs(nrm).max()
        ua, ub, rec, d4 = _run(_shape(kind, outwards, v), cp, M, Nm, xyz, nrm)
        Rr = v[3] if kind == L.SPHERE else v[6]
        if np.isnan(rec[15]):
            # exact-only.  Legitimate only outside a guard: here the band that holds the centre (R - eps - 3 mD <= 0 or the
            # zero point's guard), which a small radius at a large offset or a long axis brings about
            assert Rr <= 5.0 or not plain_axis, (kind, v, eps, alpha_deg)
            continue
        usable += 1
        assert d4[1] == 2.0 * d4[0] and d4[3] == 2.0 * d4[2] and d4[0] > 0 and d4[2] > 0, d4
        acc, n2, s = _twin(kind, v, sgn, xyz, nrm, eps_c, cosa)
        u = np.maximum(ua, ub)
        assert not np.isnan(ua).any() and not np.isnan(ub).any(), (kind, v)
        sure_in, sure_out = u < 0, u > 1
        assert not (sure_in & ~acc).any(), (kind, v, eps, alpha_deg, np.flatnonzero(sure_in & ~acc)[:5])
        assert not (sure_out & acc).any(), (kind, v, eps, alpha_deg, np.flatnonzero(sure_out & acc)[:5])
        assert u[i_zero] > 1, (kind, v, u[i_zero])
        if plain_axis:
            assert u[i_zero + 1] > 1, (kind, v, u[i_zero + 1])      # on the centre / a unit axis: nr = 0 to rounding, surely out
        K, H = Rr * Rr + eps_c * eps_c, 2.0 * Rr * eps_c
        far = (np.abs(np.abs(n2 - K) - H) > 4.0 * d4[1]) & (np.abs(s * np.abs(s) - cosa * cosa * n2) > 4.0 * d4[3])
        assert (sure_in | sure_out)[far].all(), (kind, v, eps, alpha_deg, np.flatnonzero(far & ~(sure_in | sure_out))[:5])
        far_total += int(far[n_built:].sum())
        rand_total += len(far) - n_built
    # spheres and unit axes with R - eps well above the margins are within every guard, at every offset
    want = sum(1 for o, v, plain in cands if plain and (v[3] if kind == L.SPHERE else v[6]) - eps >= 4.0)
    assert usable >= want > 0, (usable, want)
    assert far_total > 0.99 * rand_total, (far_total, rand_total)


def _flag(kind, v, eps=0.3, alpha_deg=5.0, M=100.0, Nm=1.0, outwards=1):
    cp = _params(eps, alpha_deg)
    ua, ub, rec, d4 = _run(_shape(kind, outwards, v), cp, M, Nm, np.zeros((1, 3)), np.zeros((1, 3)))
    return bool(np.isnan(rec[15])), d4


def test_candidates_outside_a_guard_are_exact_only():
    sph, cyl = [10.0, 20.0, 30.0, 5.0], [0.0, 0.0, 1.0, 10.0, 20.0, 30.0, 5.0]
    assert not _flag(L.SPHERE, sph)[0] and not _flag(L.CYLINDER, cyl)[0]
    for kind, v, r in ((L.SPHERE, sph, 3), (L.CYLINDER, cyl, 6)):
        def with_(i, x):
            w = list(v); w[i] = x
            return w
        assert _flag(kind, with_(r, 0.2))[0]                      # the band holds the centre / axis: R - eps < 0
        assert _flag(kind, with_(r, 0.3))[0]                      # R - eps = 0
        assert _flag(kind, with_(r, 0.3000001))[0]                # R - eps > 0 but inside the margins
        assert _flag(kind, with_(r, -5.0))[0]
        assert _flag(kind, v, alpha_deg=90.0)[0]                  # cos(alpha) <= 0 (to rounding: 6e-17, far inside the margins)
        assert _flag(kind, v, alpha_deg=120.0)[0]
        assert _flag(kind, v, eps=-0.1)[0]
        assert _flag(kind, with_(0, 2.0 ** 21))[0] and _flag(kind, with_(r, 2.0 ** 21))[0]
        assert _flag(kind, with_(1, float("nan")))[0] and _flag(kind, with_(r, float("inf")))[0]
        assert _flag(kind, v, M=2.0 ** 21)[0] and _flag(kind, v, Nm=2.0 ** 21)[0]
        assert _flag(kind, v, M=float("nan"))[0] and _flag(kind, v, Nm=float("inf"))[0]
        # magnitudes at the guards' edge stay usable only while the zero point is surely out; whatever comes out is flagged or finite
        flagged, d4 = _flag(kind, with_(r, 2.0 ** 19), M=2.0 ** 20, Nm=2.0 ** 20)
        assert flagged or (np.isfinite(d4).all() and d4[0] > 0)
    assert _flag(L.CYLINDER, [0.0, 0.0, 16.5] + cyl[3:])[0]       # an axis component above 16


def test_float32_margins_are_three_times_the_binary64_ones():
    """a Float32 cloud's exact test is itself a binary32 chain: every margin carries two more parts for it"""
    for kind, v in ((L.SPHERE, [10.0, 20.0, 30.0, 5.0]), (L.CYLINDER, [0.0, 0.6, 0.8, 10.0, 20.0, 30.0, 5.0])):
        cp = _params(0.3, 5.0)
        z = np.zeros((1, 3))
        d64 = _run(_shape(kind, 1, v), cp, 100.0, 1.0, z, z, f32=0)[3]
        d32 = _run(_shape(kind, 1, v), cp, 100.0, 1.0, z, z, f32=1)[3]
        # (to first order: the radii nrmax the bounds are taken at move with the margin itself)
        assert np.all(d32 > 2.99 * d64) and np.all(d32 < 3.2 * d64), (d64, d32)
