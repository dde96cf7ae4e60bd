"""The scene of the plane order's GPU tests (test_plane_order_gpu.py, test_plane_order_diag_gpu.py; csrc/kdorder.hip, DESIGN.md
section 3): one subset of 8300 points -- enough for the culled score kernel, 130 groups, 9 super-tiles, 10 nodes of the
position tree with at most 1024 points (512 to 1024 of them; the last holds 556: eight full groups and one of 44) -- on a
Float64 or a Float32 cloud.

Points: three noisy planes, a sphere and a cylinder, 30 % outliers with random normals (what fills a k-d leaf's normal-cell mask
with cells that no surface of the leaf has), and ONE point whose normal has a NaN component (it may land anywhere in the order).

Candidates (192, three chunks): exact copies of the shapes in both orientations, 1 % jitters of them, and plane candidates that
are exact-only (a point 2^21 away: no culling, every enabled point of every group goes to the exact test)."""
import ctypes as C

import numpy as np

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc

N = 8300
B = 192
EPS = 0.3
ALPHA = float(np.radians(10.0))
KINDS = ("plane", "sphere", "cylinder")
PLANES = [dict(p=np.array([50.0, 45.0, 60.0]), n=np.array([0.36, 0.48, 0.8])),
          dict(p=np.array([20.0, 70.0, 30.0]), n=np.array([1.0, 0.0, 0.0])),
          dict(p=np.array([60.0, 20.0, 20.0]), n=np.array([-0.6, 0.64, -0.48]))]
SPH = dict(o=np.array([30.0, 40.0, 50.0]), R=8.0)
CYL = dict(a=np.array([0.48, -0.6, 0.64]), c=np.array([70.0, 60.0, 40.0]), R=5.0)


def params():
    p = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder])
    for k in KINDS:
        p[k]["ϵ"] = EPS
        p[k]["α"] = ALPHA
    return R.params_to_c(p)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(n):
    n = _unit(n)
    e1 = _unit(np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0]))
    return n, e1, np.cross(n, e1)


def plane_points(pl, m, rng):
    n, e1, e2 = _frame(pl["n"])
    nn = _unit(n + rng.normal(scale=0.05, size=(m, 3)))
    p = pl["p"] + np.outer(rng.uniform(-25, 25, m), e1) + np.outer(rng.uniform(-25, 25, m), e2) + np.outer(rng.uniform(-0.5, 0.5, m), n)
    return p, nn


def round_points(c0, Rr, axis, m, rng):
    d = rng.normal(size=(m, 3))
    shift = np.zeros((m, 3))
    if axis is not None:
        ah = _unit(axis)
        d -= np.outer(d @ ah, ah)
        shift = np.outer(rng.uniform(-20, 20, m), ah)
    d = _unit(d)
    p = c0 + shift + d * (Rr + rng.uniform(-0.5, 0.5, (m, 1)))
    return p, _unit(d + rng.normal(scale=0.05, size=(m, 3)))


def candidates(rng):
    out = []
    for pl in PLANES:
        n = _unit(pl["n"])
        out += [("plane", True, list(pl["p"]) + list(n)), ("plane", False, list(pl["p"]) + list(-n))]
    out += [("sphere", True, list(SPH["o"]) + [SPH["R"]]), ("sphere", False, list(SPH["o"]) + [SPH["R"]]),
            ("cylinder", True, list(_unit(CYL["a"])) + list(CYL["c"]) + [CYL["R"]]),
            ("cylinder", False, list(_unit(CYL["a"])) + list(CYL["c"]) + [CYL["R"]])]
    # exact-only planes: a point 2^21 away in the plane (the classifier has no margin left: its record says "exact test only")
    for pl in PLANES[:2]:
        n, e1, _e2 = _frame(pl["n"])
        out.append(("plane", True, list(pl["p"] + 2.0 ** 21 * e1) + list(n)))
    while len(out) < B:
        j = 1.0 + 0.01 * rng.normal(size=7)
        r = len(out) % 4
        if r < 2:     # (half of the batch: the kind the order is for)
            pl = PLANES[len(out) % 3]
            nj = _unit(_unit(pl["n"]) * j[:3])
            out.append(("plane", True, list(pl["p"] * j[3:6]) + list(nj if len(out) % 8 < 6 else -nj)))
        elif r == 2:
            out.append(("sphere", bool(len(out) % 8 < 4), list(SPH["o"] * j[:3]) + [SPH["R"] * j[3]]))
        else:
            out.append(("cylinder", bool(len(out) % 8 < 4), list(_unit(CYL["a"] * j[:3])) + list(CYL["c"] * j[3:6]) + [CYL["R"] * j[6]]))
    return out


def orc_shapes(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


class Scene:
    def __init__(self, f32):
        import bench
        rng = np.random.default_rng(1313)
        n_out = int(0.3 * N)
        parts = [plane_points(PLANES[0], 1500, rng), plane_points(PLANES[1], 1200, rng), plane_points(PLANES[2], 1000, rng),
                 round_points(SPH["o"], SPH["R"], None, 1000, rng)]
        parts.append(round_points(CYL["c"], CYL["R"], CYL["a"], N - n_out - sum(len(p[0]) for p in parts), rng))
        parts.append((rng.uniform(0.0, 100.0, (n_out, 3)), _unit(rng.normal(size=(n_out, 3)))))
        where = rng.permutation(N)
        xyz = np.ascontiguousarray(np.vstack([p[0] for p in parts])[where])
        nrm = np.ascontiguousarray(np.vstack([p[1] for p in parts])[where])
        assert xyz.shape == (N, 3)
        self.i_nan = int(np.flatnonzero(where < 1500)[0])          # a point of the first plane
        nrm[self.i_nan, 1] = np.nan
        subs = [np.arange(1, N + 1, dtype=np.int64)]
        self.f32 = f32
        if f32:
            xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
            self.pc = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
            self.oc = orc.Cloud32(xyz, nrm, subs[0])
        else:
            self.pc = R.RANSACCloud(xyz, nrm, subs)
            self.oc = orc.Cloud(xyz, nrm, subs[0])
        self.xyz, self.nrm = xyz, nrm
        self.cands = candidates(rng)
        assert len(self.cands) == B
        self.arr = bench.shapes_to_c(R, L, self.cands)
        if f32:
            for i in range(B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
        self.cp = params()
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        self.gone = np.flatnonzero(rng.random(N) < 1.0 / 3.0) + 1          # the third rh_invalidate clears (1-based)
        # the references, once per scene: every point enabled, and without the third
        osh = orc_shapes(self.arr, B)
        self.ref_all, self.ref_all_m = self.oc.score_batch(osh, self.op, want_masks=True)
        self.oc.invalidate(self.gone)
        self.ref_cut, self.ref_cut_m = self.oc.score_batch(osh, self.op, want_masks=True)
        self.oc.enable_all()
        for a in (self.ref_all, self.ref_all_m, self.ref_cut, self.ref_cut_m):
            a.setflags(write=False)


_SCENES = {}


def scene(f32):
    if f32 not in _SCENES:
        _SCENES[f32] = Scene(f32)
    return _SCENES[f32]


def plane_order(pc):
    """rh_dbg_plane_order (diag build) -> dict of what the cloud holds"""
    lib = R.lib()
    info = np.zeros(4, dtype=np.int64)
    L.check(lib.rh_dbg_plane_order(pc._h, info.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None, None, None))
    s, ng, nst, has = (int(v) for v in info)
    assert has == 1
    sub, pl = np.zeros((6, s)), np.zeros((6, s))
    src = np.zeros(s, dtype=np.int32)
    gb, gm = np.zeros((ng, 8), dtype=np.float32), np.zeros((ng, 4), dtype=np.uint32)
    en = np.zeros((2, (s + 63) // 64), dtype=np.uint64)
    dp = C.POINTER(C.c_double)
    L.check(lib.rh_dbg_plane_order(pc._h, info.ctypes.data_as(C.POINTER(C.c_int64)), sub.ctypes.data_as(dp), pl.ctypes.data_as(dp),
                                   src.ctypes.data_as(C.POINTER(C.c_int32)), gb.ctypes.data_as(C.POINTER(C.c_float)),
                                   gm.ctypes.data_as(C.POINTER(C.c_uint32)), en.ctypes.data_as(C.POINTER(C.c_uint64))))
    return dict(s=s, ngroups=ng, nst=nst, sub=sub, pl=pl, src=src.astype(np.int64), gb32=gb, gm32=gm, en_leaf=en[0], en_plane=en[1])


def tree_nodes(s, most=1024):
    """the nodes of the position tree with at most `most` points, in position order: [(lo, hi)]"""
    out, stack = [], [(0, s)]
    while stack:
        lo, hi = stack.pop()
        cnt = hi - lo
        if cnt <= most:
            out.append((lo, hi))
            continue
        nl = ((cnt // 64 + 1) // 2) * 64
        stack.append((lo + nl, hi))
        stack.append((lo, lo + nl))
    return out
