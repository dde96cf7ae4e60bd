"""The normal-cell masks of the culled score kernel (csrc/score4_device.h, "normal cells"; boxes32.hip: nsig_kernel; score4.hip: stage 1
of score4_segment, st_cull_kind<plane>; rh_set_option "nsig"): a (plane candidate, 64-point group) pair is not walked when no point
of the group has its normal in a cell the candidate can accept, and the list launch drops a plane from a super-tile's list the
same way.  That changes which pairs are walked, never what a walked pair computes: counts and dense masks must equal the
oracle's bit for bit, and each other with the masks on ("nsig" = 0) and off (2), with and without lists ("st_cull" 1 / 2), in
rows of 2 and of 16, on a Float64 and on a Float32 cloud.

The clouds are the smallest that take the culled kernel with more than one super-tile (9765 points as subset 1: nine whole
super-tiles, one of three tiles with a partial last group).  The plane candidates are hostile: exact copies of the planes in the
cloud, the same with the normal flipped, tilted by alpha (1 +- 1e-7), alpha (1 +- 1e-3) and 2 alpha, and planes whose normals
point exactly at the cube map's face edges, corners and cell borders -- where the cloud also holds patches whose point normals
are exactly those directions."""
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
N_PATCH = 240
ALPHAS = [5.0, 60.0, 95.0]
BORDER = [np.array(v, dtype=np.float64) for v in ((1, 1, 0), (1, 1, 1), (1, 0.5, 0), (1, 0, 0), (0, -1, 1), (-1, 0.5, 0.5), (0, 0, -1), (-0.5, -1, 0))]


def _unit(v):
    return v / np.linalg.norm(v)


def _params(alpha):
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder])
    for k in ("plane", "sphere", "cylinder"):
        params[k]["ϵ"] = 0.3
        params[k]["α"] = float(np.radians(alpha))
    return R.params_to_c(params)


def _patch(rng, nb, m):
    """a plane patch through the middle of the box whose points ALL carry the normal nb / |nb| exactly"""
    z = _unit(nb)
    x = _unit(np.cross(z, [0.3, -0.2, 0.9]))
    y = np.cross(z, x)
    c = np.full(3, synth.BOX / 2) + rng.uniform(-10, 10, 3)
    uv = rng.uniform(-15, 15, size=(m, 2))
    return c + uv[:, :1] * x + uv[:, 1:] * y, np.tile(z, (m, 1)), dict(kind="plane", point=c, normal=z)


def _two_planes(rng, n):
    """two planes that cross the whole box + 30 % outliers: every k-d leaf holds points of both and of neither"""
    P, Nn, truth = [], [], []
    m = int(n * 0.35)
    for nb in ([0.3, 0.5, 0.81], [-0.7, 0.2, 0.4]):
        z = _unit(np.array(nb))
        x = _unit(np.cross(z, [0.1, 0.9, -0.2]))
        y = np.cross(z, x)
        c = np.full(3, synth.BOX / 2)
        uv = rng.uniform(-synth.BOX / 2, synth.BOX / 2, size=(m, 2))
        P.append(c + uv[:, :1] * x + uv[:, 1:] * y)
        Nn.append(synth._perturb(np.tile(z, (m, 1)), rng))
        truth.append(dict(kind="plane", point=c, normal=z))
    k = n - 2 * m
    P.append(rng.uniform(0, synth.BOX, size=(k, 3)))
    Nn.append(synth._unit(rng.normal(size=(k, 3))))
    return np.vstack(P), np.vstack(Nn), truth


def _tilted(n, t, ang):
    return n * np.cos(ang) + t * np.sin(ang)


def _candidates(truth, alpha, rng):
    """B candidates: the hostile planes first, then jittered truths of every kind"""
    a = np.radians(alpha)
    out = []
    centre = np.full(3, synth.BOX / 2)
    for t in truth:
        if t["kind"] != "plane":
            continue
        n, p = np.asarray(t["normal"], dtype=np.float64), np.asarray(t["point"], dtype=np.float64)
        tng = _unit(np.cross(n, [0.2, 0.7, -0.4]))
        for nn in (n, -n, _tilted(n, tng, a * (1 + 1e-7)), _tilted(n, tng, a * (1 - 1e-7)), _tilted(n, tng, a * (1 + 1e-3)),
                   _tilted(n, tng, a * (1 - 1e-3)), _tilted(n, tng, 2 * a), _tilted(n, -tng, a * (1 - 1e-7)), 3.0 * n, 0.5 * n):
            out.append(("plane", False, list(p) + list(nn)))
    for nb in BORDER:
        for nn in (nb, _unit(nb), -nb):
            out.append(("plane", False, list(centre) + list(nn)))
    assert len(out) < B // 2
    out += synth.jittered_candidates(truth[:6], B - len(out), seed=int(alpha))   # (the first six: half of them spheres and cylinders)
    return out


def _orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


def _chunks(en):
    bits = np.zeros(((en.size + 63) // 64) * 64, dtype=np.uint8)
    bits[:en.size] = en
    return np.packbits(bits, bitorder="little").view(np.uint64)


def _build(name):
    rng = np.random.default_rng(len(name) + 17)
    if name == "two_planes":
        xyz, nrm, truth = _two_planes(rng, N)
    else:
        prim = ["plane", "sphere", "cylinder", "plane", "plane", "cylinder"]
        xyz, nrm, truth = synth.make_cloud(N - len(BORDER) * N_PATCH, prim, 0.30, seed=41)
        P, Nn = [xyz], [nrm]
        for nb in BORDER:
            p, n, t = _patch(rng, nb, N_PATCH)
            P.append(p); Nn.append(n); truth.append(t)
        where = rng.permutation(N)
        xyz, nrm = np.vstack(P)[where], np.vstack(Nn)[where]
    en = None
    if name.startswith("awkward"):
        nrm = nrm * (0.5 if name == "awkward_half" else 3.0)
        nrm[rng.choice(N, 300, replace=False)] = 0.0
        near = np.argsort(((xyz - xyz[5]) ** 2).sum(axis=1))[:12]        # twelve neighbours: one tile of the k-d order, or two
        nrm[near[:4], 0] = np.nan
        nrm[near[4:8], 1] = np.inf
        nrm[near[8:], 2] = -np.inf
    if name == "extracted":
        # the inliers of the first plane and of a patch are gone, as after their extraction
        d0 = np.abs((xyz - truth[0]["point"]) @ truth[0]["normal"]) < 0.3
        d1 = np.abs((xyz - truth[-1]["point"]) @ truth[-1]["normal"]) < 0.3
        en = ~(d0 | d1)
        assert 200 < (~en).sum() < N // 2
    return np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), truth, en


class Scene:
    def __init__(self, name, f32):
        xyz, nrm, self.truth, self.en = _build(name)
        subs = [np.arange(1, N + 1, dtype=np.int64)]
        rng = np.random.default_rng(3)
        self.cases = {}
        if f32:
            xyz, nrm = xyz.astype(np.float32), nrm.astype(np.float32)
            self.pc = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
            self.oc = orc.Cloud32(xyz, nrm, subs[0])
        else:
            self.pc = R.RANSACCloud(xyz, nrm, subs)
            self.oc = orc.Cloud(xyz, nrm, subs[0])
        if self.en is not None:
            self.pc.set_enabled(self.en)
            self.oc.set_enabled(_chunks(self.en))
        import bench
        for alpha in ALPHAS:
            cands = _candidates(self.truth, alpha, rng)
            arr = bench.shapes_to_c(R, L, cands)
            if f32:
                for i in range(B):
                    R.lib().rh_shape_finalize_f32(C.byref(arr[i]))
            cp = _params(alpha)
            # the reference, once per scene and alpha: every launch shape below is held to it
            ref_c, ref_m = self.oc.score_batch(_orc(arr, B), orc.Params.from_buffer_copy(bytes(cp)), want_masks=True)
            self.cases[alpha] = (arr, cp, ref_c, ref_m, [c[0] for c in cands])


_SCENES = {}


def _scene(name, f32):
    key = (name, f32)
    if key not in _SCENES:
        _SCENES[key] = Scene(name, f32)
    return _SCENES[key]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", ["mixed", "awkward_half", "awkward_x3", "two_planes", "extracted"])
def test_counts_and_masks_equal_the_oracle_whatever_the_switches(name, alpha, f32):
    sc = _scene(name, f32)
    arr, cp, ref_c, ref_m, kinds = sc.cases[alpha]
    planes = np.array([k == "plane" for k in kinds])
    assert planes.sum() >= 60 and ((~planes).sum() >= 150 or name == "two_planes")
    if alpha == 5.0 and not name.startswith("awkward"):
        assert ref_c[planes].sum() > 0 and (ref_c[planes] == 0).any()       # planes with inliers and planes without
    for nsig in (0, 2):
        for lists in (1, 2):
            for rows in (2, 16):
                with R.option("nsig", nsig, cloud=sc.pc), R.option("st_cull", lists, cloud=sc.pc), R.option("s4_rows", rows, cloud=sc.pc):
                    got_c, got_m = R.score_batch(sc.pc, arr, cp, want_masks=True)
                    assert np.array_equal(got_c, ref_c), (name, alpha, f32, nsig, lists, rows, np.flatnonzero(got_c != ref_c)[:8])
                    assert np.array_equal(got_m, ref_m), (name, alpha, f32, nsig, lists, rows)
                    assert np.array_equal(R.score_batch(sc.pc, arr, cp), ref_c), (name, alpha, f32, nsig, lists, rows)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_device_batches_in_flight_take_the_launch_they_are_told(f32):
    """the step bench.py times: rh_score_batch_dev with three batches in flight -- and the launch is the one asked for"""
    sc = _scene("mixed", f32)
    arr, cp, ref_c, _, _ = sc.cases[5.0]
    lib = R.lib()
    batch = rdist.DeviceBatch(sc.pc, arr, B)
    ring = [C.c_void_p() for _ in range(3)]          # three count buffers on the device, buffer k mod 3 for call k
    for d in ring:
        L.check(lib.rh_dev_alloc(sc.pc._h, 4 * B, C.byref(d)))
    fill = np.full(B, -1, dtype=np.int32)
    try:
        with R.option("batches_in_flight", 3, cloud=sc.pc):     # (once: setting it joins the batches and probes for streams)
            for nsig in (0, 2):
                for lists in (1, 2):
                    for rows in (2, 16):
                        with R.option("nsig", nsig, cloud=sc.pc), R.option("st_cull", lists, cloud=sc.pc), R.option("s4_rows", rows, cloud=sc.pc):
                            for d in ring:
                                L.check(lib.rh_dev_upload(sc.pc._h, d, fill.ctypes.data_as(C.c_void_p), 4 * B))
                            for k in range(6):
                                L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), B, C.byref(cp), ring[k % 3], None))
                            L.check(lib.rh_cloud_sync(sc.pc._h))
                            info = (C.c_int32 * 4)()
                            L.check(lib.rh_score_launch_info(sc.pc._h, info))
                            assert info[0] == rows and info[1] == (1 if lists == 1 else 0), (list(info), rows, lists)
                            for d in ring:
                                got = np.zeros(B, dtype=np.int32)
                                L.check(lib.rh_dev_download(sc.pc._h, got.ctypes.data_as(C.c_void_p), d, 4 * B))
                                assert np.array_equal(got, ref_c), (f32, nsig, lists, rows)
    finally:
        for d in ring:
            lib.rh_dev_free(sc.pc._h, d)
        batch.free()


def test_option_values():
    sc = _scene("mixed", False)
    for v in (0, 2):
        R.set_option("nsig", v, cloud=sc.pc)
        assert R.get_option("nsig", cloud=sc.pc) == v
    R.set_option("nsig", None, cloud=sc.pc)
    assert R.get_option("nsig", cloud=sc.pc) == R.get_option("nsig")       # the cloud's own setting is gone: what the process says
    for bad in (1, 3, -1):
        with pytest.raises(R.RansacHipError):
            R.set_option("nsig", bad, cloud=sc.pc)
