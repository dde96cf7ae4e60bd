"""The scene of the aligned tree shape's GPU tests (test_kd_align_gpu.py, test_kd_align_diag_gpu.py; csrc/rh_internal.h:
kd_left_count): one subset of 9421 points on a Float64 or a Float32 cloud -- the smallest on which the
aligned rule does something today's rule does not and every edge is there.  Aligned, its position tree ends in nine nodes of
exactly 1024 points and a last node of 205 (three full groups and one of 13: not a multiple of 64); today's rule gives it 16
nodes of 576 .. 640 points, and none of its splits above 1024 points falls where the aligned one puts it.

Points: three noisy planes, a sphere, a cylinder and a cone, 30 % outliers with random normals, one point whose normal has a NaN
component.  Candidates (192, three chunks): exact copies of the six shapes in both orientations, two exact-only planes (a point
2^21 away: no culling, every enabled point goes to the exact test), and 1 % jitters of the shapes -- all four kinds.

The clouds are created under "kd_align" = mode (process-wide: the option is read when a cloud is created), 1 = aligned, 2 =
today's shape, 0 = by size, which at this size is today's."""
import ctypes as C
import math

import numpy as np

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from oracle import oracle as orc

import plane_order_scene as P

N = 9421
B = 192
EPS = P.EPS
ALPHA = P.ALPHA
KINDS = ("plane", "sphere", "cylinder", "cone")
CONE = dict(apex=np.array([80.0, 80.0, 15.0]), axis=np.array([-0.48, -0.36, 0.8]), opang=0.7, hmax=45.0)


def params():
    p = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone])
    for k in KINDS:
        p[k]["ϵ"] = EPS
        p[k]["α"] = ALPHA
    return R.params_to_c(p)


def cone_points(cone, m, rng):
    a = P._unit(cone["axis"])
    e1 = P._unit(np.cross(a, [0.0, 0.0, 1.0]))
    e2 = np.cross(a, e1)
    h, phi = rng.uniform(3.0, cone["hmax"], m), rng.uniform(0, 2 * np.pi, m)
    er = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    hw = cone["opang"] / 2
    nrm = math.cos(hw) * er - math.sin(hw) * a
    p = cone["apex"] + h[:, None] * a + (h * math.tan(hw))[:, None] * er + rng.uniform(-0.5, 0.5, (m, 1)) * nrm
    return p, P._unit(nrm + rng.normal(scale=0.05, size=(m, 3)))


def candidates(rng):
    out = []
    for pl in P.PLANES:
        n = P._unit(pl["n"])
        out += [("plane", True, list(pl["p"]) + list(n)), ("plane", False, list(pl["p"]) + list(-n))]
    cone = list(CONE["apex"]) + list(P._unit(CONE["axis"])) + [CONE["opang"]]
    cyl = list(P._unit(P.CYL["a"])) + list(P.CYL["c"]) + [P.CYL["R"]]
    out += [("sphere", True, list(P.SPH["o"]) + [P.SPH["R"]]), ("sphere", False, list(P.SPH["o"]) + [P.SPH["R"]]),
            ("cylinder", True, cyl), ("cylinder", False, cyl), ("cone", True, cone), ("cone", False, cone)]
    for pl in P.PLANES[:2]:          # exact-only planes
        n, e1, _e2 = P._frame(pl["n"])
        out.append(("plane", True, list(pl["p"] + 2.0 ** 21 * e1) + list(n)))
    while len(out) < B:
        j = 1.0 + 0.01 * rng.normal(size=7)
        r = len(out) % 8
        outw = bool(len(out) % 16 < 12)
        if r < 3:
            pl = P.PLANES[len(out) % 3]
            nj = P._unit(P._unit(pl["n"]) * j[:3])
            out.append(("plane", True, list(pl["p"] * j[3:6]) + list(nj if outw else -nj)))
        elif r < 5:
            out.append(("sphere", outw, list(P.SPH["o"] * j[:3]) + [P.SPH["R"] * j[3]]))
        elif r < 7:
            out.append(("cylinder", outw, list(P._unit(P.CYL["a"] * j[:3])) + list(P.CYL["c"] * j[3:6]) + [P.CYL["R"] * j[6]]))
        else:
            out.append(("cone", outw, list(CONE["apex"] * j[:3]) + list(P._unit(CONE["axis"] * j[3:6])) + [CONE["opang"] * j[6]]))
    return out


class Scene:
    def __init__(self, f32, mode):
        import bench
        rng = np.random.default_rng(1414)
        n_out = int(0.3 * N)
        parts = [P.plane_points(P.PLANES[0], 1400, rng), P.plane_points(P.PLANES[1], 1100, rng), P.plane_points(P.PLANES[2], 1000, rng),
                 P.round_points(P.SPH["o"], P.SPH["R"], None, 1000, rng), cone_points(CONE, 1000, rng)]
        parts.append(P.round_points(P.CYL["c"], P.CYL["R"], P.CYL["a"], N - n_out - sum(len(p[0]) for p in parts), rng))
        parts.append((rng.uniform(0.0, 100.0, (n_out, 3)), P._unit(rng.normal(size=(n_out, 3)))))
        where = rng.permutation(N)
        xyz = np.ascontiguousarray(np.vstack([p[0] for p in parts])[where])
        nrm = np.ascontiguousarray(np.vstack([p[1] for p in parts])[where])
        assert xyz.shape == (N, 3)
        self.i_nan = int(np.flatnonzero(where < 1400)[0])          # a point of the first plane
        nrm[self.i_nan, 1] = np.nan
        subs = [np.arange(1, N + 1, dtype=np.int64)]
        self.f32, self.mode = f32, mode
        with R.option("kd_align", mode):
            if f32:
                xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
                self.pc = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
            else:
                self.pc = R.RANSACCloud(xyz, nrm, subs)
        self.oc = orc.Cloud32(xyz, nrm, subs[0]) if f32 else orc.Cloud(xyz, nrm, subs[0])
        self.xyz, self.nrm, self.subs = xyz, nrm, subs
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
        self.osh = P.orc_shapes(self.arr, B)
        self.ref_all, self.ref_all_m = self.oc.score_batch(self.osh, self.op, want_masks=True)
        self.oc.invalidate(self.gone)
        self.ref_cut, self.ref_cut_m = self.oc.score_batch(self.osh, self.op, want_masks=True)
        self.oc.enable_all()
        for a in (self.ref_all, self.ref_all_m, self.ref_cut, self.ref_cut_m):
            a.setflags(write=False)


_SCENES = {}


def scene(f32, mode=1):
    if (f32, mode) not in _SCENES:
        _SCENES[(f32, mode)] = Scene(f32, mode)
    return _SCENES[(f32, mode)]
