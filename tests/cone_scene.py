"""The scene of the cone tests (test_conecls_host.py, test_conecls_gpu.py, test_conecls_diag_gpu.py): one subset of 8192 + 70
points -- the smallest cloud the culled score kernel takes, ending in a partial group -- laid where the cone code of
csrc/score4_device.h (cls_make's cone record, cls_cone_ab, cone_box_skip32) could go wrong, and a batch of 192 cone candidates.
Built with numpy alone; nothing here needs a GPU or a library.

Geometry.  A cone is an apex A, an axis a and an opening angle w; with t = p - A, h = t . a^ (a^ = a / |a|), rho = |t - h a^| and
c', s' = cos(w / 2), -sin(w / 2) the exact test (shapes/cone.jl, csrc/score_device.h cone_frame) reduces to
    D = c' rho + s' h,  |D| < eps,    sgn (c' e_rho + s' a^) . n > cos(alpha)
(e_rho the unit radial direction; closed form: csrc/score4_device.h at cls_cone_ab).  The surface is rho = tan(w / 2) h on the
nappe h > 0; on the nappe h < 0 D >= sin(w / 2) |h| > 0, so the band reaches over to it next to the apex only.

Point families (Scene.fam: (cone, family) -> indices into the cloud), for each of the two true cones -- ORD, opang 0.8 with a skew axis,
and NARROW, opang 0.1:
  band+      D = +-eps (1 +- k 2^-24), k = 0 .. 64, on the nappe h > 0, with the surface normal
  band-      D = eps (1 +- k 2^-24) on the nappe h < 0 (heights |h| < eps / sin(w / 2)), the normal of the formula above
  angle      on the surface, the normal rotated from the surface normal by alpha (1 +- k 2^-23), as given and flipped
  guard      rho / |t| = sqrt(RH_CONE_ALPHA) (1 +- j 2^-10), j = 0 .. 32: both sides of the classifier's axis guard, at five
             heights, two of them (one on each nappe) with |h| < eps / sin(w / 2): inside the band
  guardsweep the same rays at two heights with rho / |t| = sqrt(RH_CONE_ALPHA) 2^(j / 8), j = 0 .. 48: across the guard's edge
             where its additive part beta counts
  axis       exactly on the axis (as exactly as binary64 puts them), both sides of the apex, |h| >= 0.5
  apex       the apex itself, twice: one copy enabled, one disabled
  apexulp    within 4e-7 of the apex along a generator of the surface, with the surface normal: a point the exact binary64 test
             accepts, and whose binary32 conversion IS the apex (n2 = 0: the reciprocal root's infinity, rho = NaN)
  noisy      ~1500 points within 0.6 of the surface, normals a few degrees off, 30 % flipped
and uniform outliers, two of which (PIN) carry the apex and the axis of one candidate.  A third of the points is disabled."""
import math

import numpy as np

N = 8192 + 70
B = 192
EPS = 0.3
ALPHA = float(np.radians(10.0))
U24 = 2.0 ** -24
CONE_ALPHA = 162.0 * U24          # RH_CONE_ALPHA = (2 * 49 + 64) 2^-24 (score4_device.h)
K = np.arange(65)
J = np.arange(33)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


ORD = dict(name="ord", apex=np.array([30.0, 35.0, 20.0]), axis=_unit([0.36, 0.48, 0.8]), opang=0.8, hmax=40.0,
           guard_h=(0.3, -0.5, 5.0, 20.0, -3.0))
NARROW = dict(name="narrow", apex=np.array([75.0, 20.0, 10.0]), axis=_unit([-0.3, 0.4, 0.75 ** 0.5]), opang=0.1, hmax=60.0,
              guard_h=(2.0, -4.0, 15.0, 40.0, -10.0))
CONES = (ORD, NARROW)
PIN = (np.array([52.0, 47.0, 31.0]), np.array([61.0, 40.0, 66.0]))     # apex and a point of the axis of candidate "pinned"


def frame(cone, phi):
    """a^, e_rho(phi), the surface normal c' e_rho + s' a^ and the generator's direction, for azimuths phi (array)"""
    a = _unit(cone["axis"])
    e1 = _unit(np.cross(a, [0.0, 0.0, 1.0]))
    e2 = np.cross(a, e1)
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    er = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    hw = cone["opang"] / 2
    nrm = math.cos(hw) * er - math.sin(hw) * a
    gen = math.cos(hw) * a + math.sin(hw) * er
    return a, er, nrm, gen


def _families(cone, rng):
    """list of (family, xyz, nrm)"""
    A, hw = cone["apex"], cone["opang"] / 2
    tan, sin, cos = math.tan(hw), math.sin(hw), math.cos(hw)
    out = []
    # band edges on the nappe h > 0: the surface point at (h, phi) moved by D along the surface normal
    P, Nn = [], []
    for _ in range(2):
        h, phi = rng.uniform(0.25, 0.9) * cone["hmax"], rng.uniform(0, 2 * np.pi)
        a, er, nrm, _g = frame(cone, phi)
        base = A + h * a + h * tan * er[0]
        for edge in (-EPS, EPS):
            for sg in (-1.0, 1.0):
                D = edge * (1.0 + sg * K * U24)
                P.append(base + D[:, None] * nrm[0])
                Nn.append(np.tile(nrm[0], (65, 1)))
    out.append(("band+", np.vstack(P), np.vstack(Nn)))
    # ... and on the nappe h < 0: D = c' rho + sin |h| = eps (1 +- k u) needs |h| < eps / sin
    P, Nn = [], []
    for _ in range(3):       # (three places: on the Float32 cloud a place's 130 points round to a handful, on one side of the edge or the other)
        h, phi = -rng.uniform(0.3, 0.7) * EPS / sin, rng.uniform(0, 2 * np.pi)
        a, er, nrm, _g = frame(cone, phi)
        for sg in (-1.0, 1.0):
            D = EPS * (1.0 + sg * K * U24)
            rho = (D - sin * abs(h)) / cos
            assert (rho > 0).all()
            P.append(A + h * a + rho[:, None] * er[0])
            Nn.append(np.tile(nrm[0], (65, 1)))
    out.append(("band-", np.vstack(P), np.vstack(Nn)))
    # the angle test's edge: on the surface, the normal rotated about the generator by alpha (1 +- k 2^-23), as it is and flipped
    P, Nn = [], []
    h, phi = rng.uniform(0.25, 0.9) * cone["hmax"], rng.uniform(0, 2 * np.pi)
    a, er, nrm, gen = frame(cone, phi)
    side = np.cross(gen[0], nrm[0])
    for sg in (-1.0, 1.0):
        th = ALPHA * (1.0 + sg * K * 2.0 ** -23)
        n = np.cos(th)[:, None] * nrm[0] + np.sin(th)[:, None] * side
        for flip in (1.0, -1.0):
            P.append(np.tile(A + h * a + h * tan * er[0], (65, 1)))
            Nn.append(flip * n)
    out.append(("angle", np.vstack(P), np.vstack(Nn)))
    # both sides of the axis guard rho^2 = alpha |t|^2 (+ beta): rho / |t| = r, i.e. rho = |h| r / sqrt(1 - r^2)
    P, Nn = [], []
    for h in cone["guard_h"]:
        phi = rng.uniform(0, 2 * np.pi)
        a, er, nrm, _g = frame(cone, phi)
        for sg in (-1.0, 1.0):
            r = math.sqrt(CONE_ALPHA) * (1.0 + sg * J * 2.0 ** -10)
            rho = abs(h) * r / np.sqrt(1.0 - r * r)
            P.append(A + h * a + rho[:, None] * er[0])
            Nn.append(np.tile(nrm[0], (33, 1)))
    out.append(("guard", np.vstack(P), np.vstack(Nn)))
    # the guard's additive part (beta ~ 3.5 2^-24 T^2, T the candidate's own magnitude) moves its edge outwards at these heights:
    # the same rays in steps of 2^(1/8), up to 64 times the ratio
    P, Nn = [], []
    for h in cone["guard_h"][2:4]:
        a, er, nrm, _g = frame(cone, rng.uniform(0, 2 * np.pi))
        r = math.sqrt(CONE_ALPHA) * 2.0 ** (np.arange(49) / 8.0)
        rho = abs(h) * r / np.sqrt(1.0 - r * r)
        P.append(A + h * a + rho[:, None] * er[0])
        Nn.append(np.tile(nrm[0], (49, 1)))
    out.append(("guardsweep", np.vstack(P), np.vstack(Nn)))
    # on the axis (the normal half way between the axis and a radial direction: no cone of the batch through these points has
    # its normal within alpha of that, whatever radial direction the exact frame makes up), and the apex itself, twice
    a, er, nrm, gen = frame(cone, rng.uniform(0, 2 * np.pi))
    hs = np.array([0.5, 0.7, 2.0, 10.0, 30.0, -0.5, -0.7, -2.0, -10.0])
    out.append(("axis", A + hs[:, None] * a, np.tile(_unit(er[0] + a), (len(hs), 1))))
    out.append(("apex", np.tile(A, (2, 1)), np.tile(nrm[0], (2, 1))))
    # next to the apex on the surface: |p - A| <= 4e-7 is below half a binary32 step (4.8e-7) of every coordinate of A (>= 8)
    phi = rng.uniform(0, 2 * np.pi, 12)
    a, er, nrm, gen = frame(cone, phi)
    d = np.tile([1e-7, 2e-7, 4e-7], 4)
    out.append(("apexulp", A + d[:, None] * gen, nrm))
    # the surface with noise
    n = 1500
    h, phi = rng.uniform(2.0, cone["hmax"], n), rng.uniform(0, 2 * np.pi, n)
    a, er, nrm, gen = frame(cone, phi)
    nn = nrm + rng.normal(scale=0.08, size=(n, 3))
    nn *= np.where(rng.random(n) < 0.3, -1.0, 1.0)[:, None]
    out.append(("noisy", A + h[:, None] * a + (h * tan)[:, None] * er + rng.uniform(-0.6, 0.6, n)[:, None] * nrm,
                nn / np.linalg.norm(nn, axis=1)[:, None]))
    return out


def candidates(rng):
    """(tag, ("cone", outwards, apex + axis + [opang])) x B; tags name the family of the candidate"""
    def c(tag, cone, outw=True, scale=1.0, opang=None, apex=None, axis=None):
        ap = cone["apex"] if apex is None else apex
        ax = cone["axis"] * scale if axis is None else axis
        return (tag, ("cone", bool(outw), list(ap) + list(ax) + [cone["opang"] if opang is None else opang]))
    out = [c("exact", ORD, True), c("exact-in", ORD, False), c("exact", NARROW, True), c("exact-in", NARROW, False)]
    for cone in CONES:
        for i, s in enumerate((1e-3, 1.5, 7.5)):
            out.append(c("axislen", cone, i != 1, scale=s))
    for w in (0.004, math.pi / 2, math.pi - 1e-5, math.pi, math.pi + 0.3):
        out.append(c("opang", ORD, True, opang=w))
    out.append(c("opang", NARROW, False, opang=math.pi / 2))
    # the band holds the origin, where a disabled point is staged: (0, 0, 0) at h = 3, rho = 4 of a cone with tan(w / 2) = 4 / 3,
    # and 0.2 off that surface
    w0 = 2.0 * math.atan2(4.0, 3.0)
    out.append(c("origin", ORD, True, opang=w0, apex=np.array([0.0, -4.0, -3.0]), axis=np.array([0.0, 0.0, 1.0])))
    out.append(c("origin", ORD, False, opang=w0, apex=np.array([0.0, -4.2, -3.1]), axis=np.array([0.0, 0.0, 2.0])))
    # the apex on one cloud point, the axis (as the difference: length 36) through another
    out.append(c("pinned", ORD, True, opang=0.6, apex=PIN[0], axis=PIN[1] - PIN[0]))
    out.append(c("pinned", ORD, False, opang=0.6, apex=PIN[0], axis=PIN[1] - PIN[0]))
    # large T: the apex 2^19 away, the cloud's middle on the surface
    for cone, outw in ((ORD, True), (NARROW, False)):
        a, er, nrm, gen = frame(cone, [1.0])
        out.append(c("far", cone, outw, apex=np.array([50.0, 50.0, 50.0]) - 2.0 ** 19 * gen[0]))
    # an apex coordinate above 2^20: no binary32 record
    out.append(c("huge", ORD, True, apex=ORD["apex"] + np.array([2.0 ** 20 + 100.0, 0.0, 0.0])))
    out.append(c("huge", NARROW, True, apex=np.array([75.0, -(2.0 ** 21), 10.0])))
    while len(out) < B:
        cone = CONES[len(out) % 2]
        j = 1.0 + 0.01 * rng.normal(size=7)
        out.append(c("jitter", cone, len(out) % 4 < 2, apex=cone["apex"] * j[:3], axis=_unit(cone["axis"] * j[3:6]), opang=cone["opang"] * j[6]))
    return out


class Scene:
    """xyz, nrm (binary64; the Float32 variant is these arrays rounded), en (enabled), fam[(cone name, family)] -> indices,
    cands / tags"""

    def __init__(self):
        rng = np.random.default_rng(4242)
        parts, names = [], []
        for cone in CONES:
            for fam, P, Nn in _families(cone, rng):
                parts.append((P, Nn)); names.append((cone["name"], fam))
        nn = rng.normal(size=(2, 3))
        parts.append((np.array(PIN), nn / np.linalg.norm(nn, axis=1)[:, None])); names.append(("-", "pin"))
        n_out = N - sum(len(p[0]) for p in parts)
        assert n_out > 1500
        nn = rng.normal(size=(n_out, 3))
        parts.append((rng.uniform(0.0, 100.0, (n_out, 3)), nn / np.linalg.norm(nn, axis=1)[:, None])); names.append(("-", "outlier"))
        xyz, nrm = np.vstack([p[0] for p in parts]), np.vstack([p[1] for p in parts])
        assert xyz.shape == (N, 3) and xyz.min() >= 0.0 and xyz.max() <= 100.0
        where = rng.permutation(N)            # new position i holds old point where[i]
        inv = np.empty(N, dtype=np.int64); inv[where] = np.arange(N)
        self.xyz, self.nrm = np.ascontiguousarray(xyz[where]), np.ascontiguousarray(nrm[where])
        self.fam, at = {}, 0
        for name, p in zip(names, parts):
            self.fam[name] = np.sort(inv[at:at + len(p[0])])
            at += len(p[0])
        en = rng.random(N) >= 1.0 / 3.0
        for cone in CONES:
            i = self.fam[(cone["name"], "apex")]
            en[i[0]], en[i[1]] = True, False
            en[self.fam[(cone["name"], "apexulp")][::2]] = True
        en[self.fam[("-", "pin")]] = True
        self.en = en
        tagged = candidates(rng)
        self.tags = [t for t, _ in tagged]
        self.cands = [c for _, c in tagged]
        for a in (self.xyz, self.nrm, self.en):
            a.setflags(write=False)

    def arrays(self, f32):
        if f32:
            return self.xyz.astype(np.float32), self.nrm.astype(np.float32)
        return self.xyz, self.nrm

    def enabled_chunks(self):
        bits = np.zeros(((N + 63) // 64) * 64, dtype=np.uint8)
        bits[:N] = self.en
        return np.packbits(bits, bitorder="little").view(np.uint64)

    def through(self, name):
        """the candidates whose apex and axis line are the named cone's: they pass through its on-axis and apex points"""
        cone = ORD if name == "ord" else NARROW
        return [i for i, (_k, _o, v) in enumerate(self.cands)
                if np.array_equal(v[:3], cone["apex"]) and np.linalg.norm(np.cross(_unit(v[3:6]), cone["axis"])) < 1e-12]


_SCENE = None


def scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = Scene()
    return _SCENE


def shapes(lib, Shape, f32):
    """the batch as the library finalises it (lib: any build of the library; Shape: its ctypes record)"""
    import ctypes as C
    sc = scene()
    arr = (Shape * B)()
    for i, (_name, outw, v) in enumerate(sc.cands):
        arr[i].kind, arr[i].outwards = 3, int(outw)
        for j, x in enumerate(v):
            arr[i].v[j] = float(x)
        lib.rh_shape_finalize(C.byref(arr[i]))
        if f32:
            lib.rh_shape_finalize_f32(C.byref(arr[i]))
    return arr
