"""The scene the translated-cloud tests share (tests/test_translated_host.py, tests/test_translated_gpu.py): a helper, no test.

Why a grid.  The scene's coordinates and the candidates' POSITION parameters (a plane's point, a sphere's and a cylinder's
centre, a cone's apex) are multiples of GRID[f32], and so is every offset.  A translation by such an offset is then exact --
translate() asserts (xyz + t) - t == xyz -- and so p - p0, p - o and p - apex are the very same numbers before and after.  The
exact test of a PLANE, a SPHERE and a CONE starts with that difference and never reads p again: its answer does not depend on
the offset, bit for bit, in binary64 and in binary32.  The CYLINDER's does: its chain (p - a sd) - c reads p itself, so its
rounding moves with the offset.  Whatever else changes between offsets is a shortcut's doing: a margin, a box, a guard -- all
of which csrc/score4_device.h builds from M = max |coordinate| and T = M + |centre|.

binary64: grid 2^-10, eps 0.05; binary32: grid 2^-4 (coordinates below 2^20 stay exact in 24 bits), eps 0.1; alpha 5 degrees.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as orc
from ransac_jl_amd import synth

N = 20_000
N_SMALL = 8193
KINDS = ("plane", "sphere", "cylinder", "cone")
KIND_ID = {"plane": 0, "sphere": 1, "cylinder": 2, "cone": 3}
PER_KIND = 16
B = PER_KIND * len(KINDS)
GRID = {False: 2.0 ** -10, True: 2.0 ** -4}
EPS = {False: 0.05, True: 0.1}
ALPHA_DEG = 5.0
BIG = 2.0 ** 20                      # RH_CLS_BIG (csrc/score4_device.h): above it every candidate is exact-only
OFFSETS = {
    False: [(0.0, 0.0, 0.0), (1024.0, 2048.0, -4096.0), (7e5, 0.0, 0.0), (7e5, -7e5, 7e5), (3 * BIG, -3 * BIG, 2 * BIG)],
    True: [(0.0, 0.0, 0.0), (1024.0, 2048.0, -4096.0), (2.0 ** 19, -2.0 ** 19, 2.0 ** 18), (7e5, -7e5, 7e5)],
}
HUGE_D = (1e3, 1e5, BIG - 200.0, 3e6)
# where a kind's position parameter sits in the shape's fields (rh_shape field order: include/ransac_hip.h)
_POS = {"plane": 0, "sphere": 0, "cylinder": 3, "cone": 0}


def offset_id(t):
    return "0" if not any(t) else "%g_%g_%g" % tuple(t)


def offset_mag(t):
    return max(abs(x) for x in t)


def snap(x, grid):
    return np.round(np.asarray(x, dtype=np.float64) / grid) * grid


class Scene:
    """xyz, nrm (float64 arrays, of float32 values when f32), truth (synth's dictionaries, positions snapped), f32, shift"""

    def __init__(self, xyz, nrm, truth, f32, shift=(0.0, 0.0, 0.0)):
        self.xyz, self.nrm, self.truth, self.f32, self.shift = xyz, nrm, truth, f32, tuple(shift)
        self.n = len(xyz)

    @property
    def subsets(self):
        return [np.arange(1, self.n + 1, dtype=np.int64)]           # subset 1 = the whole cloud

    def head(self, n):
        return Scene(self.xyz[:n].copy(), self.nrm[:n].copy(), self.truth, self.f32, self.shift)

    def with_point(self, p, normal=(0.0, 0.0, 1.0)):
        return Scene(np.vstack([self.xyz, [p]]), np.vstack([self.nrm, [normal]]), self.truth, self.f32, self.shift)

    def oracle_cloud(self, L=None):
        """the oracle's cloud: Cloud32 for a binary32 scene under the default build, the flagged Cloud under a rounding variant"""
        if self.f32:
            if L is None:
                return orc.Cloud32(self.xyz.astype(np.float32), self.nrm.astype(np.float32), self.subsets[0])
            return orc.Cloud(self.xyz, self.nrm, self.subsets[0], L=L, f32=True)
        return orc.Cloud(self.xyz, self.nrm, self.subsets[0], L=L)

    def device_cloud(self):
        import ransac_jl_amd as R
        if self.f32:
            return R.RANSACCloud(self.xyz.astype(np.float32), self.nrm.astype(np.float32), self.subsets, force_eltype=np.float32)
        return R.RANSACCloud(self.xyz, self.nrm, self.subsets)


@functools.lru_cache(maxsize=None)
def scene(f32):
    xyz, nrm, truth = synth.make_cloud(N, list(KINDS), 0.3, seed=7)
    xyz = snap(xyz, GRID[f32])
    if f32:
        nrm = nrm.astype(np.float32).astype(np.float64)
        assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)
    truth = [dict(t) for t in truth]
    for t in truth:
        for k in ("point", "center", "apex"):
            if k in t:
                t[k] = snap(t[k], GRID[f32])
    xyz.setflags(write=False); nrm.setflags(write=False)
    return Scene(xyz, nrm, truth, f32)


def _exact_sum(a, t, f32):
    t = np.asarray(t, dtype=np.float64)
    b = a + t
    if f32:
        b = b.astype(np.float32).astype(np.float64)
    assert np.array_equal(b - t, a), "the translation is not exact: leave the grid or 2^53 (2^24 for binary32) behind?"
    return b


def translate(sc, t):
    """the scene moved by t, exactly: (xyz + t) - t == xyz is asserted (for a binary32 scene on the rounded sums)"""
    truth = [dict(x) for x in sc.truth]
    for x in truth:
        for k in ("point", "center", "apex"):
            if k in x:
                x[k] = _exact_sum(x[k], t, sc.f32)
    return Scene(_exact_sum(sc.xyz, t, sc.f32), sc.nrm, truth, sc.f32, tuple(np.add(sc.shift, t)))


def _fields(t):
    if t["kind"] == "plane":
        return list(t["point"]) + list(t["normal"])
    if t["kind"] == "sphere":
        return list(t["center"]) + [t["radius"]]
    if t["kind"] == "cylinder":
        return list(t["axis"]) + list(t["center"]) + [t["radius"]]
    return list(t["apex"]) + list(t["axis"]) + [t["opang"]]


@functools.lru_cache(maxsize=None)
def candidates(f32):
    """64 (kind, outwards, fields) of the scene at the origin: per truth the truth itself, then 15 copies whose position carries a
    jitter N(0, 0.05) per component, snapped; `outwards` alternates (the odd ones point inwards; a plane has no such flag)"""
    rng = np.random.default_rng(70)
    out = []
    for t in scene(f32).truth:
        v0, at = _fields(t), _POS[t["kind"]]
        for i in range(PER_KIND):
            v = list(v0)
            if i:
                v[at:at + 3] = snap(np.asarray(v0[at:at + 3]) + rng.normal(0.0, 0.05, 3), GRID[f32])
            out.append((t["kind"], i % 2 == 0, [float(x) for x in v]))
    return tuple(out)


def moved(cands, t, f32):
    """the candidates translated by t (their position parameters only; exactness asserted)"""
    out = []
    for kind, outw, v in cands:
        v, at = list(v), _POS[kind]
        v[at:at + 3] = _exact_sum(np.asarray(v[at:at + 3]), t, f32)
        out.append((kind, outw, [float(x) for x in v]))
    return out


def is_invariant(cands):
    """which candidates' exact test does not depend on an exact translation: all but the cylinders"""
    return np.array([kind != "cylinder" for kind, _, _ in cands])


def kind_ids(cands):
    return np.array([KIND_ID[kind] for kind, _, _ in cands])


def huge_candidates(f32):
    """Round candidates of radius D through the cloud AT THE ORIGIN: with (p0, n0) the scene's true plane, a sphere about
    p0 - D n0 and a cylinder with its axis perpendicular to n0 through the same centre, both of radius D and pointing outwards --
    they touch the plane in p0, so they hold most of its points, and T = M + |centre| grows from the candidate's side."""
    t = scene(f32).truth[0]
    p0, n0 = np.asarray(t["point"]), np.asarray(t["normal"])
    ax = np.cross(n0, [1.0, 0.0, 0.0] if abs(n0[0]) < 0.9 else [0.0, 1.0, 0.0])
    ax /= np.linalg.norm(ax)
    out = []
    for D in HUGE_D:
        c = p0 - D * n0
        out.append(("sphere", True, [float(x) for x in c] + [D]))
        out.append(("cylinder", True, [float(x) for x in ax] + [float(x) for x in c] + [D]))
    return out


def guard_edge_scenes(f32):
    """the scene at the origin plus one more (enabled) point whose largest coordinate is exactly 2^20 -- M <= RH_CLS_BIG, the
    classifier stays on -- and one at 2^20 + 0.125, one binary32 ulp further: exact-only"""
    return [scene(f32).with_point((BIG, 48.0, 52.0)), scene(f32).with_point((BIG + 0.125, 48.0, 52.0))]


def orc_shapes(cands, f32):
    """the candidates as the oracle finalises them (needs the oracle alone)"""
    mk = orc.make_shape32 if f32 else orc.make_shape
    return orc.shapes_array([mk(KIND_ID[kind], outw, v) for kind, outw, v in cands])


def rh_shapes(cands, f32):
    """the candidates as the library finalises them: rh_shape_finalize, then rh_shape_finalize_f32 for a Float32 cloud"""
    import ransac_jl_amd as R
    from ransac_jl_amd import _lib as L
    arr = (L.Shape * max(1, len(cands)))()
    for i, (kind, outw, v) in enumerate(cands):
        arr[i].kind, arr[i].outwards = KIND_ID[kind], int(outw)
        for j, x in enumerate(v):
            arr[i].v[j] = float(x)
        R.lib().rh_shape_finalize(C.byref(arr[i]))
        if f32:
            R.lib().rh_shape_finalize_f32(C.byref(arr[i]))
    return arr


def as_orc(arr, b):
    """the library's records, byte for byte, as the oracle's"""
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(orc.Shape) * b)
    return out


def params(f32, eps=None):
    """(library parameter record, oracle parameter record): eps (default EPS[f32]) and alpha = 5 degrees for every kind"""
    import ransac_jl_amd as R
    from ransac_jl_amd import _lib as L
    p = R.ransacparameters()
    for k in KINDS:
        p[k]["ϵ"] = float(EPS[f32] if eps is None else eps)
        p[k]["α"] = float(np.radians(ALPHA_DEG))
    cp = R.params_to_c(p, score_mode=L.SCORE_F64)
    return cp, orc.Params.from_buffer_copy(bytes(cp))


def orc_params(f32, eps=None):
    """the oracle's parameter record from the oracle alone"""
    e = float(EPS[f32] if eps is None else eps)
    return orc.default_params(eps=[e] * 4, alpha=[float(np.radians(ALPHA_DEG))] * 4, score_mode=orc.SCORE_F64)


def enabled_chunks(mask):
    bits = np.zeros(((len(mask) + 63) // 64) * 64, dtype=np.uint8)
    bits[:len(mask)] = mask
    return np.packbits(bits, bitorder="little").view(np.uint64)
