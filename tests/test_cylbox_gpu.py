"""The cylinder's box test of the culled score kernel with its support clause (csrc/score4_device.h, "The cylinder's box by its
support"; score4.hip: stage 1 of score4_segment, st_cull_kind<cylinder>): a (cylinder, box) pair is not walked when the tangent
plane of the distance from the axis at the box's centre already clears the band.  That changes which pairs are walked, never
what a walked pair computes: counts and dense masks must equal the oracle's bit for bit, with and without lists ("st_cull" 1 / 2),
in rows of 2 and of 16, with one and three batches in flight, on a Float64 and on a Float32 cloud; and the refit's index lists
are the same by the plain scan, by the culled scan (whose binary64 box test carries the same clause) and by the oracle.

The cloud is the smallest that takes the culled kernel with more than one super-tile (9765 points as subset 1: nine whole
super-tiles, one of three tiles with a partial last group): three cylinders, two planes and a sphere, 30 % outliers, and plane
patches laid out as FLAT k-d leaves (128 points each, 4 x 1 wide, zero thick) tangent to the shells of the hostile candidates at
eps (1 +- 1e-6) and eps (1 +- 1e-3) outside them: just inside and just outside the band.  The hostile cylinders: axes along a
coordinate axis, a face and a space diagonal and a random direction, of squared length 1, 1 +- 1e-3 and 2, radii above and
below eps, the truth's exact copies; then jittered copies of the truth of every kind, so that the bins of the one launch are
mixed."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N = 9 * 1024 + 2 * 256 + 37
B = 512
EPS = 0.3
N_PATCH = 128
RELS = (1 - 1e-6, 1 + 1e-6, 1 - 1e-3, 1 + 1e-3)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _params():
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder])
    for k in ("plane", "sphere", "cylinder"):
        params[k]["ϵ"] = EPS
        params[k]["α"] = float(np.radians(20.0))
    return R.params_to_c(params)


def _hostile(rng):
    """(axis, centre, radius, tangent direction) of the hostile cylinders"""
    mid = np.full(3, synth.BOX / 2)
    out = []
    for av, nv in (((0, 0, 1), (1, 0, 0)), ((1, 1, 0), (0, 0, 1)), ((1, 1, 1), (1, -1, 0)), (None, None)):
        a = _unit(av) if av is not None else _unit(rng.normal(size=3))
        n = _unit(nv) if nv is not None else _unit(np.cross(a, [0.3, -0.8, 0.5]))
        for Rr in (6.0, 0.2):
            out.append((a, mid + rng.uniform(-15, 15, 3), Rr, n))
    return out


def _patches(hostile, rng):
    """per hostile cylinder of radius 6 and band offset: 128 points on the plane tangent to the cylinder of radius R + eps rel,
    4 along the axis and 1 across, every fourth exactly ON the tangent line (distance R + eps rel from the axis), normals = the
    shell's"""
    P, Nn = [], []
    for a, c0, Rr, n in hostile:
        if Rr != 6.0:
            continue
        b = np.cross(a, n)
        for rel in RELS:
            u = rng.uniform(-2.0, 2.0, N_PATCH)
            v = rng.uniform(-0.5, 0.5, N_PATCH)
            v[::4] = 0.0
            P.append(c0 + a * rng.uniform(-10, 10) + n * (Rr + EPS * rel) + u[:, None] * a + v[:, None] * b)
            Nn.append(np.tile(n, (N_PATCH, 1)))
    return np.vstack(P), np.vstack(Nn)


def _candidates(truth, hostile):
    out = []
    for a, c0, Rr, _ in hostile:
        for s2 in (1.0, 1.0 + 1e-3, 1.0 - 1e-3, 2.0):
            out.append(("cylinder", True, list(a * np.sqrt(s2)) + list(c0) + [Rr]))
        out.append(("cylinder", False, list(-a) + list(c0) + [Rr]))
        out.append(("cylinder", True, list(a) + list(c0 + 40.0 * a) + [Rr]))          # the same axis through another point
    for t in truth:
        if t["kind"] == "cylinder":
            out.append(("cylinder", True, list(t["axis"]) + list(t["center"]) + [float(t["radius"])]))
    assert len(out) < B // 4
    out += synth.jittered_candidates(truth, B - len(out), seed=5)
    return out


def _orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


class Scene:
    def __init__(self, f32):
        rng = np.random.default_rng(23)
        self.hostile = _hostile(rng)
        px, pn = _patches(self.hostile, rng)
        prim = ["cylinder", "plane", "cylinder", "sphere", "plane", "cylinder"]
        xyz, nrm, self.truth = synth.make_cloud(N - len(px), prim, 0.30, seed=43)
        where = rng.permutation(N)
        xyz, nrm = np.ascontiguousarray(np.vstack([xyz, px])[where]), np.ascontiguousarray(np.vstack([nrm, pn])[where])
        subs = [np.arange(1, N + 1, dtype=np.int64)]
        self.f32 = f32
        if f32:
            xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
            self.pc = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
            self.oc = orc.Cloud32(xyz, nrm, subs[0])
        else:
            self.pc = R.RANSACCloud(xyz, nrm, subs)
            self.oc = orc.Cloud(xyz, nrm, subs[0])
        self.xyz = xyz
        import bench
        self.cands = _candidates(self.truth, self.hostile)
        self.kinds = [c[0] for c in self.cands]
        self.arr = bench.shapes_to_c(R, L, self.cands)
        if f32:
            for i in range(B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
        self.cp = _params()
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        # the reference, once per scene: every launch shape below is held to it
        self.ref_c, self.ref_m = self.oc.score_batch(_orc(self.arr, B), self.op, want_masks=True)


_SCENES = {}


def _scene(f32):
    if f32 not in _SCENES:
        _SCENES[f32] = Scene(f32)
    return _SCENES[f32]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counts_and_masks_equal_the_oracle_whatever_the_switches(f32):
    sc = _scene(f32)
    cyl = np.array([k == "cylinder" for k in sc.kinds])
    assert cyl.sum() >= 150 and (~cyl).sum() >= 150
    assert sc.ref_c[cyl].sum() > 0 and (sc.ref_c[cyl] == 0).any()
    if not f32:
        # the patches just inside the band give the unit-axis hostile cylinders of radius 6 inliers of their own: the 32 points ON
        # each tangent line at eps (1 - 1e-6) and eps (1 - 1e-3)
        for i in (0, 12, 24, 36):
            assert sc.ref_c[i] >= 32, (i, sc.ref_c[i])
    for lists in (1, 2):
        for rows in (2, 16):
            with R.option("st_cull", lists, cloud=sc.pc), R.option("s4_rows", rows, cloud=sc.pc):
                got_c, got_m = R.score_batch(sc.pc, sc.arr, sc.cp, want_masks=True)
                assert np.array_equal(got_c, sc.ref_c), (f32, lists, rows, np.flatnonzero(got_c != sc.ref_c)[:8])
                assert np.array_equal(got_m, sc.ref_m), (f32, lists, rows)
                assert np.array_equal(R.score_batch(sc.pc, sc.arr, sc.cp), sc.ref_c), (f32, lists, rows)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("in_flight", [1, 3])
def test_device_batches_in_flight(in_flight, f32):
    """the step bench.py times: rh_score_batch_dev, one batch at a time and three in flight"""
    sc = _scene(f32)
    lib = R.lib()
    batch = rdist.DeviceBatch(sc.pc, sc.arr, B)
    ring = [C.c_void_p() for _ in range(3)]
    for d in ring:
        L.check(lib.rh_dev_alloc(sc.pc._h, 4 * B, C.byref(d)))
    fill = np.full(B, -1, dtype=np.int32)
    try:
        with R.option("batches_in_flight", in_flight, cloud=sc.pc):
            for lists in (1, 2):
                for rows in (2, 16):
                    with R.option("st_cull", lists, cloud=sc.pc), R.option("s4_rows", rows, cloud=sc.pc):
                        for d in ring:
                            L.check(lib.rh_dev_upload(sc.pc._h, d, fill.ctypes.data_as(C.c_void_p), 4 * B))
                        for k in range(6):
                            L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), B, C.byref(sc.cp), ring[k % 3], None))
                        L.check(lib.rh_cloud_sync(sc.pc._h))
                        info = (C.c_int32 * 4)()
                        L.check(lib.rh_score_launch_info(sc.pc._h, info))
                        assert info[0] == rows and info[1] == (1 if lists == 1 else 0), (list(info), rows, lists)
                        for d in ring:
                            got = np.zeros(B, dtype=np.int32)
                            L.check(lib.rh_dev_download(sc.pc._h, got.ctypes.data_as(C.c_void_p), d, 4 * B))
                            assert np.array_equal(got, sc.ref_c), (f32, in_flight, lists, rows)
    finally:
        for d in ring:
            lib.rh_dev_free(sc.pc._h, d)
        batch.free()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_refit_lists_are_the_same_by_scan_culled_scan_and_oracle(f32):
    sc = _scene(f32)
    picks = [i for i, k in enumerate(sc.kinds) if k == "cylinder"]
    picks = picks[:4] + picks[24:28] + picks[-6:]          # hostile ones (a unit and three non-unit axes each) and jittered truths
    some = 0
    for i in picks:
        exp = sc.oc.refit(_orc(sc.arr, B)[i], sc.op)
        got = {}
        for path in ("scan", "culled"):
            with R.option("refit_path", path, cloud=sc.pc):
                got[path] = R.refit(sc.arr[i], sc.pc, sc.cp).inpoints
        assert np.array_equal(got["scan"], got["culled"]), (f32, i)
        assert np.array_equal(got["culled"], exp), (f32, i)
        some += len(exp) > 0
    assert some >= 6
