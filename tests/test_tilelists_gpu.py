"""The candidate lists of the culled score kernel (score4.hip: st_cull_kernel + the LIST instantiations) at the sizes where their
ragged ends are most of the cloud, and the byte budget of their workspace ("st_list_mb").  The list launch tests every
candidate against the box of a super-tile (1024 points) and a block of the score kernel walks its super-tile's list.  Results
must not depend on it: with the lists forced on ("st_cull" = 1) counts and dense masks equal the oracle's bit for bit, and the
same call with the lists off ("st_cull" = 2).  (Written for lists per TILE of 256 points -- HISTORY.md, round 6: measured, not
kept -- the cases are the ones at which either level can go wrong.)

The clouds are as small as the culled path allows (8192 points and up, the whole cloud as subset 1), so that the ragged ends
are a large part of them: a last group of one point / last tile of one group / last super-tile of one tile (8193 points), a
last super-tile of three tiles with a partial last tile (9765), and whole super-tiles only (10240)."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIZES = [8192 + 1, 9 * 1024 + 2 * 256 + 37, 10 * 1024]
B = 4096
KINDS = {"plane": L.PLANE, "sphere": L.SPHERE, "cylinder": L.CYLINDER, "cone": L.CONE}
N_SMALL = 60          # points on each of the two small shapes


def _params(eps=0.3):
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone])
    for k in KINDS:
        params[k]["ϵ"] = eps
        params[k]["α"] = float(np.radians(5.0))
    return R.params_to_c(params)


def _small_shapes(rng):
    """a sphere of radius 0.4 and a cylinder of radius 0.3 and length 2 (the tiles of these clouds are ~30 units wide: each
    fits inside one tile's box with room to spare) -- points, outward normals and the candidates that describe them"""
    cs = np.array([31.0, 62.0, 47.0])
    d = rng.normal(size=(N_SMALL, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    ps, ns = cs + 0.4 * d, d
    cc, ax = np.array([71.0, 28.0, 55.0]), np.array([0.0, 0.6, 0.8])
    x = np.array([1.0, 0.0, 0.0]); y = np.cross(ax, x)
    th, t = rng.uniform(0, 2 * np.pi, N_SMALL), rng.uniform(-1, 1, N_SMALL)
    rad = np.cos(th)[:, None] * x + np.sin(th)[:, None] * y
    pcy, ncy = cc + 0.3 * rad + t[:, None] * ax, rad
    cands = [("sphere", True, list(cs) + [0.4]), ("cylinder", True, list(ax) + list(cc) + [0.3])]
    return np.vstack([ps, pcy]), np.vstack([ns, ncy]), cands


def _candidates(truth, small):
    """4096 candidates, all four kinds mixed; the special ones sit in the first 63, so every batch size but 1 holds them"""
    import bench
    cands = synth.jittered_candidates(truth, B, seed=5)
    far = [("plane", False, [1e4, 1e4, 1e4, 0.0, 0.0, 1.0]), ("sphere", True, [-5e3, 2e4, 1e4, 3.0]),
           ("cylinder", True, [0.0, 0.0, 1.0, 1e4, -1e4, 0.0, 2.0]), ("cone", True, [1e4, 1e4, -1e4, 0.0, 1.0, 0.0, 0.5])]
    for i, c in enumerate(small + far):
        cands[2 + 3 * i] = c                  # 2, 5, .., 17: the small sphere, the small cylinder, four shapes far outside
    arr = bench.shapes_to_c(R, L, cands)
    arr[24].v[0] = float("nan")               # a plane, a sphere, a cylinder and a cone with a non-finite parameter each
    arr[25].v[3] = float("inf")
    arr[26].v[6] = float("nan")
    arr[27].v[1] = float("inf")
    return arr, [c[0] for c in cands]


def _take(arr, idx):
    out = (L.Shape * max(1, len(idx)))()
    for j, i in enumerate(idx):
        C.memmove(C.byref(out[j]), C.byref(arr[int(i)]), C.sizeof(L.Shape))
    return out


def _orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


def _chunks(en):
    bits = np.zeros(((en.size + 63) // 64) * 64, dtype=np.uint8)
    bits[:en.size] = en
    return np.packbits(bits, bitorder="little").view(np.uint64)


class Scene:
    def __init__(self, n, f32=False):
        rng = np.random.default_rng(n)
        xs, ns, small = _small_shapes(rng)
        prim = ["plane", "sphere", "cylinder", "cone", "plane", "cylinder"]
        xyz, nrm, self.truth = synth.make_cloud(n - 2 * N_SMALL, prim, 0.25, seed=n % 89)
        where = rng.permutation(n)
        self.xyz = np.ascontiguousarray(np.vstack([xyz, xs])[where])
        self.nrm = np.ascontiguousarray(np.vstack([nrm, ns])[where])
        self.n = n
        subs = [np.arange(1, n + 1, dtype=np.int64)]          # subset 1 = the whole cloud: its size is n exactly
        self.arr, self.kinds = _candidates(self.truth, small)
        self.cp = _params()
        self.ocp = orc.Params.from_buffer_copy(bytes(self.cp))
        if f32:
            self.xyz, self.nrm = self.xyz.astype(np.float32), self.nrm.astype(np.float32)
            for i in range(B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
            self.pc = R.RANSACCloud(self.xyz, self.nrm, subs, force_eltype=np.float32)
            self.oc = orc.Cloud32(self.xyz, self.nrm, subs[0])
        else:
            self.pc = R.RANSACCloud(self.xyz, self.nrm, subs)
            self.oc = orc.Cloud(self.xyz, self.nrm, subs[0])
        # the reference of the whole batch with every point enabled, once: a candidate's row does not depend on its batch
        self.ref_c, self.ref_m = self.oc.score_batch(_orc(self.arr, B), self.ocp, want_masks=True)

    def enable(self, en):
        if en is None:
            self.pc.enable_all(); self.oc.enable_all()
        else:
            self.pc.set_enabled(en); self.oc.set_enabled(_chunks(en))


@pytest.fixture(scope="module", params=SIZES)
def scene(request):
    return Scene(request.param)


@pytest.fixture(scope="module")
def scene32():
    return Scene(SIZES[1], f32=True)


def _both_modes(sc, arr, b, want_c, want_m, tag):
    for mode in (1, 2):
        with R.option("st_cull", mode, cloud=sc.pc):
            got_c, got_m = R.score_batch(sc.pc, arr, sc.cp, want_masks=True)
            assert np.array_equal(got_c, want_c), (tag, mode)
            assert np.array_equal(got_m, want_m), (tag, mode)
            assert np.array_equal(R.score_batch(sc.pc, arr, sc.cp), want_c), (tag, mode)


@pytest.mark.parametrize("b", [1, 63, 257, 1025, 4096])
def test_mixed_batches_of_every_size(scene, b):
    """one candidate, a partial chunk, the list launch's round of 4 x 256 partial, full + 1, and four full rounds"""
    scene.enable(None)
    _both_modes(scene, _take(scene.arr, range(b)), b, scene.ref_c[:b], scene.ref_m[:b], b)
    if b >= 63:
        assert scene.ref_c[:b].sum() > 0
        assert (scene.ref_c[8:18:3] == 0).all()                  # far outside the cloud: no list holds them


@pytest.mark.parametrize("kind", list(KINDS))
def test_batches_of_a_single_kind(scene, kind):
    """the other three bins are empty: their tiles' counts must read zero"""
    scene.enable(None)
    idx = [i for i, k in enumerate(scene.kinds) if k == kind]
    assert len(idx) > 256
    _both_modes(scene, _take(scene.arr, idx), len(idx), scene.ref_c[idx], scene.ref_m[idx], kind)
    assert scene.ref_c[idx].sum() > 0


def test_small_shapes_inside_one_tile(scene):
    """a sphere and a short thin cylinder far smaller than a tile's box, at a tight threshold: all lists but their own
    super-tile's (at most a k-d cut's two) leave them out, and their points are still all found"""
    scene.enable(None)
    cp = _params(eps=0.05)
    arr = _take(scene.arr, [2, 5] + list(range(30, 30 + 300)))
    want_c, want_m = scene.oc.score_batch(_orc(arr, 302), orc.Params.from_buffer_copy(bytes(cp)), want_masks=True)
    assert want_c[0] > N_SMALL // 2 and want_c[1] > N_SMALL // 2
    for mode in (1, 2):
        with R.option("st_cull", mode, cloud=scene.pc):
            got_c, got_m = R.score_batch(scene.pc, arr, cp, want_masks=True)
            assert got_c[0] > 0 and got_c[1] > 0
            assert np.array_equal(got_c, want_c) and np.array_equal(got_m, want_m), mode


def test_non_finite_candidates_are_never_skipped(scene):
    scene.enable(None)
    idx = [24, 25, 26, 27]
    for i in idx:
        assert not np.isfinite(np.array(scene.arr[i].v[:7])).all()
    _both_modes(scene, _take(scene.arr, idx), 4, scene.ref_c[idx], scene.ref_m[idx], "nonfinite")


@pytest.mark.parametrize("pattern", ["random60", "tiles_off", "all_off"])
def test_enabled_bits(scene, pattern):
    """(all on: every other test.)  tiles_off: every point of the lower 40 % in x is off -- the k-d leaves that lie wholly in
    that slab are tiles without an enabled point, the ones its face cuts are partly off."""
    rng = np.random.default_rng(scene.n + 1)
    if pattern == "random60":
        en = rng.random(scene.n) < 0.6
    elif pattern == "tiles_off":
        en = scene.xyz[:, 0] >= np.quantile(scene.xyz[:, 0], 0.4)
    else:
        en = np.zeros(scene.n, dtype=bool)
    b = 1025
    arr = _take(scene.arr, range(b))
    try:
        scene.enable(en)
        want_c, want_m = scene.oc.score_batch(_orc(arr, b), scene.ocp, want_masks=True)
        _both_modes(scene, arr, b, want_c, want_m, pattern)
        # (the reference's sphere test does not look at the enabled bits, sphere.jl:121,131: spheres keep their counts)
        others = np.array([k != "sphere" for k in scene.kinds[:b]])
        assert want_c[~others].sum() > 0 and (want_c[others].sum() > 0) == (pattern != "all_off")
    finally:
        scene.enable(None)


def _dev_counts(sc, batch, b, in_flight, nbuf=3, calls=6):
    """`calls` calls of rh_score_batch_dev on the same batch, count buffer k mod nbuf for call k"""
    import torch
    lib = R.lib()
    with R.option("batches_in_flight", in_flight, cloud=sc.pc):
        ring = [torch.full((b,), -1, dtype=torch.int32, device="cuda") for _ in range(nbuf)]
        torch.cuda.synchronize()
        for k in range(calls):
            L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), b, C.byref(sc.cp), C.c_void_p(ring[k % nbuf].data_ptr()), None))
        L.check(lib.rh_cloud_sync(sc.pc._h))
        info = (C.c_int32 * 4)()
        L.check(lib.rh_score_launch_info(sc.pc._h, info))
        return [r.cpu().numpy() for r in ring], list(info)


@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("rows", [2, 4, 8, 12, 16])
def test_launch_shapes(scene, rows, in_flight):
    scene.enable(None)
    batch = rdist.DeviceBatch(scene.pc, scene.arr, B)
    try:
        for mode in (1, 2):
            with R.option("st_cull", mode, cloud=scene.pc), R.option("s4_rows", rows, cloud=scene.pc):
                got, info = _dev_counts(scene, batch, B, in_flight)
                assert info[0] == rows and info[1] == (1 if mode == 1 else 0), (info, mode)
                for g in got:
                    assert np.array_equal(g, scene.ref_c), (rows, in_flight, mode)
    finally:
        batch.free()


@pytest.mark.parametrize("b", [257, 4096])
def test_float32_cloud(scene32, b):
    sc = scene32
    _both_modes(sc, _take(sc.arr, range(b)), b, sc.ref_c[:b], sc.ref_m[:b], ("f32", b))
    assert sc.ref_c[:b].sum() > 0
    batch = rdist.DeviceBatch(sc.pc, sc.arr, b)
    try:
        with R.option("st_cull", 1, cloud=sc.pc), R.option("s4_rows", 12, cloud=sc.pc):
            got, info = _dev_counts(sc, batch, b, 3)
            assert info[1] == 1
            for g in got:
                assert np.array_equal(g, sc.ref_c[:b])
    finally:
        batch.free()


def test_budget_below_need_takes_the_plain_launch(scene):
    """the lists of the largest batch (16384 candidates) on these clouds take 8 bytes x 16384 x (9 or 10 super-tiles) > 1 MiB:
    with "st_list_mb" = 1 the launch succeeds without lists, with the same counts; with the budget back at its default it
    takes them again"""
    scene.enable(None)
    b = 4 * B
    assert 8 * b * ((scene.n + 1023) // 1024) > 1 << 20
    arr = _take(scene.arr, list(range(B)) * 4)
    want = np.tile(scene.ref_c, 4)
    batch = rdist.DeviceBatch(scene.pc, arr, b)
    try:
        with R.option("st_cull", 1, cloud=scene.pc):
            with R.option("st_list_mb", 1, cloud=scene.pc):
                got, info = _dev_counts(scene, batch, b, 1, nbuf=1, calls=1)
                assert info[1] == 0 and np.array_equal(got[0], want)
            got, info = _dev_counts(scene, batch, b, 1, nbuf=1, calls=1)
            assert info[1] == 1 and np.array_equal(got[0], want)
    finally:
        batch.free()
