"""The culled score kernel with the root-free classifier of the round kinds (csrc/score4_device.h, "Round kinds without a square
root"): spheres and cylinders are classified in n2 = |q|^2 and qn |qn| instead of nr and qn / nr.  That changes which points the
binary32 classifier decides by itself, never what a candidate counts: counts and dense masks must equal the oracle's bit for
bit, with the super-tile lists on and off, on a Float64 and on a Float32 cloud; the census of the classifier's decisions against
the exact test (rh_dbg_cls_soundness) shows no violation, the audit of its error (rh_dbg_cls_audit) stays below 0.3 of a width,
and the classifier decides no fewer points than the form with the reciprocal root did (1 % of room for the margins' other shape).

The cloud: one subset of 8192 + 70 points -- the smallest the culled kernel takes, ending in a partial last group -- with one
sphere and one cylinder whose points sit ON the thresholds (nr = (R +- eps) (1 +- k 2^-24), normals at alpha (1 +- k 2^-23) from
the shell's, k = 0 .. 64), noisy shell points and outliers; a third of the points disabled.  The batch: 192 candidates (three
chunks): exact copies in both orientations, one exact-only candidate of each kind (the band holds the centre / axis),
cylinders with a non-unit axis, a sphere and a cylinder whose band holds the origin (where a disabled point is staged), and 1 %
jitters of the truth."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N = 8192 + 70
B = 192
EPS = 0.3
ALPHA = float(np.radians(10.0))
SPH = dict(o=np.array([30.0, 40.0, 50.0]), R=8.0)
CYL = dict(a=np.array([0.48, -0.6, 0.64]), c=np.array([70.0, 60.0, 40.0]), R=5.0)

# points the classifier decides by itself (census columns 4 + 5: surely in + surely out) on this very scene and batch with the
# library of the commit before the root-free form (its diag build loaded through RH_LIB_PATH, once, on an MI355X):
# (f32 cloud, kind) -> points
PARENT_DECIDED = {(False, L.SPHERE): 775416, (False, L.CYLINDER): 790930, (True, L.SPHERE): 775333, (True, L.CYLINDER): 789698}


def _params():
    params = R.ransacparameters([R.FittedSphere, R.FittedCylinder])
    for k in ("sphere", "cylinder"):
        params[k]["ϵ"] = EPS
        params[k]["α"] = ALPHA
    return R.params_to_c(params)


def _threshold_points(c0, Rr, ah, rng, trials):
    """points on the two edges of the band with the shell's normal, and points at nr = R with the normal on the edge of the
    angle test: (R +- eps) (1 +- k 2^-24), alpha (1 +- k 2^-23)"""
    k = np.arange(65)
    P, Nn = [], []
    for _ in range(trials):
        d = rng.normal(size=3)
        shift = 0.0
        if ah is not None:
            d -= ah * (d @ ah)
            shift = ah * rng.uniform(-15, 15)
        d /= np.linalg.norm(d)
        t = np.cross(d, [0.0, 0.0, 1.0]) if ah is None else np.cross(ah, d)
        t /= np.linalg.norm(t)
        for edge in (Rr - EPS, Rr + EPS):
            for sg in (-1.0, 1.0):
                nr = edge * (1.0 + sg * k * 2.0 ** -24)
                P.append(c0 + shift + nr[:, None] * d)
                Nn.append(np.tile(d, (65, 1)))
        for sg in (-1.0, 1.0):
            th = ALPHA * (1.0 + sg * k * 2.0 ** -23)
            P.append(np.tile(c0 + shift + Rr * d, (65, 1)))
            Nn.append(np.cos(th)[:, None] * d + np.sin(th)[:, None] * t)
    return np.vstack(P), np.vstack(Nn)


def _shell_points(c0, Rr, ah, n, rng):
    d = rng.normal(size=(n, 3))
    shift = 0.0
    if ah is not None:
        d -= np.outer(d @ ah, ah)
        shift = np.outer(rng.uniform(-15, 15, n), ah)
    d /= np.linalg.norm(d, axis=1)[:, None]
    nn = d + rng.normal(scale=0.08, size=(n, 3))          # normals a few degrees off: both sides of the angle test
    nn *= np.where(rng.random(n) < 0.3, -1.0, 1.0)[:, None]   # (some point inwards: the inward candidates' inliers)
    return c0 + shift + (Rr + rng.uniform(-0.6, 0.6, n))[:, None] * d, nn / np.linalg.norm(nn, axis=1)[:, None]


def _candidates(rng):
    o, Rs = SPH["o"], SPH["R"]
    a, c, Rc = CYL["a"], CYL["c"], CYL["R"]
    perp = np.cross(a, [0.0, 0.0, 1.0]); perp /= np.linalg.norm(perp)
    out = [("sphere", True, list(o) + [Rs]), ("sphere", False, list(o) + [Rs]),
           ("cylinder", True, list(a) + list(c) + [Rc]), ("cylinder", False, list(a) + list(c) + [Rc]),
           ("sphere", True, list(o) + [0.2]), ("cylinder", True, list(a) + list(c) + [0.2]),              # exact-only: R < eps
           ("cylinder", True, list(1.5 * a) + list(c) + [Rc]), ("cylinder", False, list((1 + 1e-3) * a) + list(c) + [Rc]),
           ("cylinder", True, list(7.5 * a) + list(c) + [Rc]),
           ("sphere", True, [6.0, 0.0, 0.0, 6.0]), ("sphere", False, [0.0, 4.0, 3.0, 5.1]),                # the band holds the origin
           ("cylinder", True, list(a) + list(Rc * perp) + [Rc]), ("cylinder", False, list(a) + list(4.9 * perp + 12.0 * a) + [Rc])]
    while len(out) < B:
        j = 1.0 + 0.01 * rng.normal(size=7)
        if len(out) % 2:
            out.append(("sphere", bool(len(out) % 4 == 1), list(o * j[:3]) + [Rs * j[3]]))
        else:
            aj = a * j[:3]
            out.append(("cylinder", bool(len(out) % 4 == 0), list(aj / np.linalg.norm(aj)) + list(c * j[3:6]) + [Rc * j[6]]))
    return out


def _orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


class Scene:
    def __init__(self, f32):
        import bench
        rng = np.random.default_rng(101)
        ah = CYL["a"] / np.linalg.norm(CYL["a"])
        parts = [_threshold_points(SPH["o"], SPH["R"], None, rng, 3), _threshold_points(CYL["c"], CYL["R"], ah, rng, 3),
                 _shell_points(SPH["o"], SPH["R"], None, 1500, rng), _shell_points(CYL["c"], CYL["R"], ah, 2000, rng)]
        n_out = N - sum(len(p[0]) for p in parts)
        nn = rng.normal(size=(n_out, 3))
        parts.append((rng.uniform(0.0, 100.0, (n_out, 3)), nn / np.linalg.norm(nn, axis=1)[:, None]))
        where = rng.permutation(N)
        xyz = np.ascontiguousarray(np.vstack([p[0] for p in parts])[where])
        nrm = np.ascontiguousarray(np.vstack([p[1] for p in parts])[where])
        assert xyz.shape == (N, 3)
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
        self.cands = _candidates(rng)
        self.arr = bench.shapes_to_c(R, L, self.cands)
        if f32:
            for i in range(B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
        self.cp = _params()
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        self.en = rng.random(N) >= 1.0 / 3.0
        bits = np.zeros(((N + 63) // 64) * 64, dtype=np.uint8); bits[:N] = self.en
        self.pc.set_enabled(self.en)
        self.oc.set_enabled(np.packbits(bits, bitorder="little").view(np.uint64))
        # the reference, once per scene
        self.ref_c, self.ref_m = self.oc.score_batch(_orc(self.arr, B), self.op, want_masks=True)


_SCENES = {}


def _scene(f32):
    if f32 not in _SCENES:
        _SCENES[f32] = Scene(f32)
    return _SCENES[f32]


def census(sc):
    """rh_dbg_cls_soundness of the scene's batch (diag build): 56 counters, ten per kind"""
    snd = np.zeros(56, dtype=np.uint64)
    L.check(R.lib().rh_dbg_cls_soundness(sc.pc._h, sc.arr, B, C.byref(sc.cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    return snd


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counts_and_masks_equal_the_oracle_with_and_without_lists(f32):
    sc = _scene(f32)
    assert 0.3 < 1.0 - sc.en.mean() < 0.37
    # the exact copies hold their shells' points, the inward ones the points whose normals point inwards, the exact-only candidates (R < eps) nothing
    assert sc.ref_c[0] > 300 and sc.ref_c[2] > 300, sc.ref_c[:13]
    assert sc.ref_c[1] > 50 and sc.ref_c[3] > 50 and sc.ref_c[4] == 0 and sc.ref_c[5] == 0, sc.ref_c[:13]
    assert (sc.ref_c[13:] > 0).sum() > 100
    lib = R.lib()
    batch = rdist.DeviceBatch(sc.pc, sc.arr, B)
    d_cn = C.c_void_p()
    L.check(lib.rh_dev_alloc(sc.pc._h, 4 * B, C.byref(d_cn)))
    try:
        for lists in (1, 2):
            with R.option("st_cull", lists, cloud=sc.pc):
                got_c, got_m = R.score_batch(sc.pc, sc.arr, sc.cp, want_masks=True)
                assert np.array_equal(got_c, sc.ref_c), (f32, lists, np.flatnonzero(got_c != sc.ref_c)[:8])
                assert np.array_equal(got_m, sc.ref_m), (f32, lists)
                assert np.array_equal(R.score_batch(sc.pc, sc.arr, sc.cp), sc.ref_c), (f32, lists)
                # the step bench.py times, which also says what it launched: the culled kernel, lists as asked
                L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), B, C.byref(sc.cp), d_cn, None))
                L.check(lib.rh_cloud_sync(sc.pc._h))
                info = (C.c_int32 * 4)()
                L.check(lib.rh_score_launch_info(sc.pc._h, info))
                assert info[0] > 0 and info[1] == (1 if lists == 1 else 0) and info[3] == (N + 255) // 256, list(info)
                got = np.zeros(B, dtype=np.int32)
                L.check(lib.rh_dev_download(sc.pc._h, got.ctypes.data_as(C.c_void_p), d_cn, 4 * B))
                assert np.array_equal(got, sc.ref_c), (f32, lists)
    finally:
        lib.rh_dev_free(sc.pc._h, d_cn)
        batch.free()


@pytest.mark.diag
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_shows_no_violation_and_no_fewer_decided_points(f32):
    sc = _scene(f32)
    snd = census(sc)
    for kind in (L.SPHERE, L.CYLINDER):
        s10 = snd[10 * kind:10 * kind + 10].astype(np.int64)
        print("census", "f32" if f32 else "f64", L.KIND_NAMES[kind], s10.tolist())
        assert s10[3] == N * sum(1 for c in sc.cands if c[0] == L.KIND_NAMES[kind])
        assert s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
        assert s10[8] > 1000                                             # exact inliers: the census looked at real shells
        assert s10[4] + s10[5] >= 0.99 * PARENT_DECIDED[(f32, kind)], (s10[4] + s10[5], PARENT_DECIDED[(f32, kind)])


@pytest.mark.diag
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_binary32_error_stays_below_0_3_of_a_width(f32):
    sc = _scene(f32)
    out = np.zeros(12)
    L.check(R.lib().rh_dbg_cls_audit(sc.pc._h, sc.arr, B, C.byref(sc.cp), out.ctypes.data_as(C.POINTER(C.c_double))))
    print("audit", "f32" if f32 else "f64", out.tolist())
    assert out[8 + L.SPHERE] > 1e5 and out[8 + L.CYLINDER] > 1e5, out
    assert out[2:6].max() < 0.3, out
