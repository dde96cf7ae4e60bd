"""The scene of the two-bit books' GPU tests (test_books2_gpu.py, test_books2_diag_gpu.py; csrc/score4_device.h, "Two-bit books"):
one subset of 8192 + 70 points -- 129 full groups and a last one with 6 valid points -- and 192 candidates (three chunks) of planes, spheres
and cylinders, on a Float64 or a Float32 cloud.

Points: on both thresholds of every kind -- the band's edges (R +- eps) (1 +- k 2^-24) resp. d = +-eps (1 +- k 2^-24) with the
shape's normal, and on the shape with the normal at alpha (1 +- k 2^-23) from it, k = 0 .. 64 (the round kinds' by the
constructions of test_rootfree_gpu.py) --, noisy points of a plane, a sphere and a cylinder, outliers, and ONE point with an
infinite coordinate: its tile treats every candidate as exact-only.  A third of the points is disabled before scoring.

Candidates: exact copies in both orientations, exact-only ones -- spheres and a cylinder with R <= eps, a plane through the cloud
given by a point 2^21 away, a sphere about a centre 2^21 away -- whose culling records skip nothing, so that every group of the
cloud has all its enabled points undecided for them (far more than 64 in every batch that holds such a pair: full ring drains
inside the pair loop), shapes whose band holds the origin (where a disabled point is staged), and 1 % jitters of the truth,
whose bands cut through the noisy points: ambiguous groups with a third of their points disabled."""
import ctypes as C

import numpy as np

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc

import test_rootfree_gpu as RF

N = 8192 + 70
B = 192
EPS = RF.EPS
ALPHA = RF.ALPHA
SPH, CYL = RF.SPH, RF.CYL
PLN = dict(p=np.array([50.0, 45.0, 60.0]), n=np.array([0.36, 0.48, 0.8]))
KINDS = ("plane", "sphere", "cylinder")


def params():
    p = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder])
    for k in KINDS:
        p[k]["ϵ"] = EPS
        p[k]["α"] = ALPHA
    return R.params_to_c(p)


def _plane_frame():
    n = PLN["n"] / np.linalg.norm(PLN["n"])
    e1 = np.cross(n, [0.0, 0.0, 1.0]); e1 /= np.linalg.norm(e1)
    return n, e1, np.cross(n, e1)


def plane_threshold_points(rng, trials):
    """d = +-eps (1 +- k 2^-24) with the plane's normal; on the plane with the normal at alpha (1 +- k 2^-23) from it"""
    n, e1, e2 = _plane_frame()
    k = np.arange(65)
    P, Nn = [], []
    for _ in range(trials):
        base = PLN["p"] + rng.uniform(-25, 25) * e1 + rng.uniform(-25, 25) * e2
        for edge in (-EPS, EPS):
            for sg in (-1.0, 1.0):
                d = edge * (1.0 + sg * k * 2.0 ** -24)
                P.append(base + d[:, None] * n)
                Nn.append(np.tile(n, (65, 1)))
        for sg in (-1.0, 1.0):
            th = ALPHA * (1.0 + sg * k * 2.0 ** -23)
            P.append(np.tile(base, (65, 1)))
            Nn.append(np.cos(th)[:, None] * n + np.sin(th)[:, None] * e1)
    return np.vstack(P), np.vstack(Nn)


def plane_noisy_points(m, rng):
    n, e1, e2 = _plane_frame()
    nn = n + rng.normal(scale=0.08, size=(m, 3))
    nn *= np.where(rng.random(m) < 0.3, -1.0, 1.0)[:, None]
    p = PLN["p"] + np.outer(rng.uniform(-30, 30, m), e1) + np.outer(rng.uniform(-30, 30, m), e2) + np.outer(rng.uniform(-0.6, 0.6, m), n)
    return p, nn / np.linalg.norm(nn, axis=1)[:, None]


def candidates(rng):
    o, Rs = SPH["o"], SPH["R"]
    a, c, Rc = CYL["a"], CYL["c"], CYL["R"]
    n, e1, _e2 = _plane_frame()
    p0 = PLN["p"]
    out = [("plane", True, list(p0) + list(n)), ("plane", False, list(p0) + list(-n)),
           ("sphere", True, list(o) + [Rs]), ("sphere", False, list(o) + [Rs]),
           ("cylinder", True, list(a) + list(c) + [Rc]), ("cylinder", False, list(a) + list(c) + [Rc]),
           # exact-only: R <= eps; a parameter above 2^20
           ("sphere", True, list(o) + [0.2]), ("sphere", True, list(o) + [EPS]), ("cylinder", True, list(a) + list(c) + [0.2]),
           ("plane", True, list(p0 + 2.0 ** 21 * e1) + list(n)),
           ("sphere", True, list(o + np.array([2.0 ** 21, 0.0, 0.0])) + [2.0 ** 21]),
           # the band holds the origin
           ("sphere", True, [6.0, 0.0, 0.0, 6.0]), ("plane", True, [0.0, 0.0, 0.1] + [0.0, 0.0, 1.0]),
           ("cylinder", True, list(a) + list(Rc * np.cross(a, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(a, [0.0, 0.0, 1.0]))) + [Rc])]
    while len(out) < B:
        j = 1.0 + 0.01 * rng.normal(size=7)
        r = len(out) % 3
        if r == 0:
            nj = n * j[:3]
            out.append(("plane", bool(len(out) % 2), list(p0 * j[3:6]) + list((nj if len(out) % 2 else -nj) / np.linalg.norm(nj))))
        elif r == 1:
            out.append(("sphere", bool(len(out) % 4 < 2), list(o * j[:3]) + [Rs * j[3]]))
        else:
            aj = a * j[:3]
            out.append(("cylinder", bool(len(out) % 4 < 2), list(aj / np.linalg.norm(aj)) + list(c * j[3:6]) + [Rc * j[6]]))
    return out


def orc_shapes(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


class Scene:
    def __init__(self, f32):
        import bench
        rng = np.random.default_rng(1212)
        ah = CYL["a"] / np.linalg.norm(CYL["a"])
        parts = [RF._threshold_points(SPH["o"], SPH["R"], None, rng, 2), RF._threshold_points(CYL["c"], CYL["R"], ah, rng, 2),
                 plane_threshold_points(rng, 2),
                 RF._shell_points(SPH["o"], SPH["R"], None, 1100, rng), RF._shell_points(CYL["c"], CYL["R"], ah, 1400, rng),
                 plane_noisy_points(1200, rng)]
        n_out = N - sum(len(p[0]) for p in parts)
        assert n_out > 1500
        nn = rng.normal(size=(n_out, 3))
        parts.append((rng.uniform(0.0, 100.0, (n_out, 3)), nn / np.linalg.norm(nn, axis=1)[:, None]))
        where = rng.permutation(N)
        xyz = np.ascontiguousarray(np.vstack([p[0] for p in parts])[where])
        nrm = np.ascontiguousarray(np.vstack([p[1] for p in parts])[where])
        assert xyz.shape == (N, 3)
        self.i_inf = int(np.flatnonzero(where >= N - n_out)[0])          # an outlier
        xyz[self.i_inf, 1] = np.inf
        subs = [np.arange(1, N + 1, dtype=np.int64)]
        self.f32 = f32
        with R.option("score_path", "groups"):          # the culled kernel, whatever the size says
            if f32:
                xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
                self.pc = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
                self.oc = orc.Cloud32(xyz, nrm, subs[0])
            else:
                self.pc = R.RANSACCloud(xyz, nrm, subs)
                self.oc = orc.Cloud(xyz, nrm, subs[0])
        self.cands = candidates(rng)
        assert len(self.cands) == B
        self.arr = bench.shapes_to_c(R, L, self.cands)
        if f32:
            for i in range(B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
        self.cp = params()
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        self.en = rng.random(N) >= 1.0 / 3.0
        self.en[self.i_inf] = True
        bits = np.zeros(((N + 63) // 64) * 64, dtype=np.uint8); bits[:N] = self.en
        self.pc.set_enabled(self.en)
        self.oc.set_enabled(np.packbits(bits, bitorder="little").view(np.uint64))
        # the reference, once per scene
        self.ref_c, self.ref_m = self.oc.score_batch(orc_shapes(self.arr, B), self.op, want_masks=True)
        self.ref_c.setflags(write=False); self.ref_m.setflags(write=False)


_SCENES = {}


def scene(f32):
    if f32 not in _SCENES:
        _SCENES[f32] = Scene(f32)
    return _SCENES[f32]


FIELDS = {"second_pass_pairs": 9, "undecided_points": 10, "ring_drains_full": 11, "exact_accepted": 13}


def counters(sc, lists):
    """the event counters (rh_dbg_s4_stats, diag build) of ONE counts-only launch on the scene: {kind: {field: n}}; the launch's
    counts are checked against the oracle on the way"""
    import torch
    lib = R.lib()
    from ransac_jl_amd import dist as rdist
    batch = rdist.DeviceBatch(sc.pc, sc.arr, B)
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = np.zeros(128, dtype=np.uint64)
    try:
        with R.option("st_cull", lists, cloud=sc.pc):
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 1, None))
            L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), B, C.byref(sc.cp), C.c_void_p(counts.data_ptr()), None))
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 0, st.ctypes.data_as(C.POINTER(C.c_uint64))))
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 2, None))
    finally:
        batch.free()
    assert np.array_equal(counts.cpu().numpy(), sc.ref_c)
    return {name: {f: int(st[24 * k + i]) for f, i in FIELDS.items()} for k, name in enumerate(KINDS)}
