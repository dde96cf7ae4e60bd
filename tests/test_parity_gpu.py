"""GPU parity tests: the HIP path through the C ABI against the CPU oracle on the same seeded
inputs.  Integer / index outputs must be bit-exact (counts, masks, inlier index lists)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ransac_jl_amd as R
from oracle import oracle as orc
from ransac_jl_amd import _lib as L
from ransac_jl_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["groups", "brute"], autouse=True)
def score_path(request):
    """Every test runs against both scoring kernels: the culled one (k-d leaf groups + box tests)
    and the brute-force one.  The path is chosen when a cloud is created."""
    with R.option("score_path", request.param):   # rh_set_option(NULL, "score_path", ..): read when a cloud is created
        yield request.param


def to_orc_params(cp):
    return orc.Params.from_buffer_copy(bytes(cp))


def to_orc_shapes(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


def make_candidates(truth, b, seed, kinds=None):
    cands = synth.jittered_candidates(truth, b, seed=seed)
    tcls = {"plane": R.FittedPlane, "sphere": R.FittedSphere, "cylinder": R.FittedCylinder, "cone": R.FittedCone}
    out = []
    for name, outw, v in cands:
        if name == "plane":
            out.append(R.FittedPlane(v[0:3], v[3:6]))
        elif name == "sphere":
            out.append(R.FittedSphere(v[0:3], v[3], outw))
        elif name == "cylinder":
            out.append(R.FittedCylinder(v[0:3], v[3:6], v[6], outw))
        else:
            out.append(R.FittedCone(v[0:3], v[3:6], v[6], outw))
    return out


def shape_array(cands):
    arr = (L.Shape * max(1, len(cands)))()
    for i, s in enumerate(cands):
        arr[i] = s.to_c()
    return arr


@pytest.fixture(scope="module")
def small_scene(score_path):
    prim = ["plane", "plane", "sphere", "sphere", "cylinder", "cylinder", "cone", "cone"]
    xyz, nrm, truth = synth.make_cloud(60_000, prim, 0.2, seed=11)
    subs = synth.make_subsets(60_000, 3, seed=11)
    pc = R.RANSACCloud(xyz, nrm, subs)
    oc = orc.Cloud(xyz, nrm, subs[0])
    return pc, oc, truth


def test_score_counts_and_masks_all_kinds(small_scene):
    pc, oc, truth = small_scene
    cp = R.params_to_c(R.ransacparameters())
    cands = make_candidates(truth, 203, seed=1)       # 203: ragged last candidate tile
    arr = shape_array(cands)
    counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
    ocounts, omasks = oc.score_batch(to_orc_shapes(arr, len(cands)), to_orc_params(cp), want_masks=True)
    assert counts.sum() > 10000                          # the batch really hits the primitives
    assert np.array_equal(counts, ocounts)
    assert np.array_equal(masks, omasks)                 # bit-exact inlier sets in subset order
    for k in (L.PLANE, L.SPHERE, L.CYLINDER, L.CONE):
        sel = [i for i, c in enumerate(cands) if c.kind == k]
        assert len(sel) > 10 and counts[sel].max() > 500, "kind %d never scored inliers" % k
    # counts without masks go through the other kernel instantiation
    assert np.array_equal(R.score_batch(pc, arr, cp), ocounts)


@pytest.mark.parametrize("seg_words", [0, 128, 8])
def test_masks_through_every_form_of_the_list_to_row_pass(small_scene, seg_words):
    """The culled kernel leaves the masks as per-candidate entry lists; a second pass turns them into dense rows in
    subset order, one block per (row, segment of the row).  the option "unp_words" (read per call) sets the segment width, so that the
    20000-point subset of this scene (313 words per row) is one segment (wave-per-entry form), 3 segments (the per-segment
    bit masks that full-size clouds with up to 16 segments use) or 40 (the form without them) -- bit-equal rows every time,
    with and without disabled points."""
    pc, oc, truth = small_scene
    R.set_option("unp_words", seg_words if seg_words else None, cloud=pc)
    cp = R.params_to_c(R.ransacparameters())
    arr = shape_array(make_candidates(truth, 130, seed=5))
    for frac in (1.0, 0.6):
        en = np.random.default_rng(3).random(60_000) < frac
        pc.set_enabled(en)
        bits = np.zeros(((60_000 + 63) // 64) * 64, dtype=np.uint8); bits[:60_000] = en
        oc.set_enabled(np.packbits(bits, bitorder="little").view(np.uint64))
        counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
        ocounts, omasks = oc.score_batch(to_orc_shapes(arr, 130), to_orc_params(cp), want_masks=True)
        assert counts.sum() > 5000
        assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks)
    pc.enable_all()
    oc.enable_all()


@pytest.mark.diag
def test_binary32_classifier_stays_inside_its_margins(small_scene):
    """The batched score decides most pairs in binary32 and sends only those within a rounding margin of a
    threshold to the binary64 test (csrc/score4_device.h).  The audit evaluates every (candidate, point) pair of
    the batch with the kernel's own binary32 functions against the reference's binary64 arithmetic: the error has
    to stay below 1/2 of the ambiguity band's width for the classification to be sound; the margins are built
    with a safety factor of 2, so it stays below 1/4."""
    pc, oc, truth = small_scene
    rng = np.random.default_rng(3)
    for eps, alpha_deg in [(0.3, 5.0), (0.01, 1.0), (5.0, 60.0)]:
        params = R.ransacparameters()
        for k in ("plane", "sphere", "cylinder", "cone"):
            params[k]["ϵ"] = eps
            params[k]["α"] = math.radians(alpha_deg)
        cp = R.params_to_c(params)
        cands = make_candidates(truth, 96, seed=int(rng.integers(0, 1000)))
        arr = shape_array(cands)
        out = np.zeros(12)
        L.check(R.lib().rh_dbg_cls_audit(pc._h, arr, len(cands), C.byref(cp), out.ctypes.data_as(C.POINTER(C.c_double))))
        assert out[8:12].min() > 1e5, out          # planes, spheres, cylinders and cones were all looked at
        assert out[:8].max() < 0.3, out            # sound below 0.5


@pytest.mark.parametrize("eps,alpha_deg,seed", [(0.3, 5.0, 0), (0.01, 1.0, 1), (5.0, 60.0, 2), (40.0, 89.0, 3)])
def test_score_fuzz_arbitrary_candidates(small_scene, eps, alpha_deg, seed):
    """Candidates nowhere near a primitive, degenerate, non-unit, huge, tiny, NaN / inf: the box culling
    may only ever skip pairs that cannot pass, so counts and masks still equal the oracle's bit for bit."""
    pc, oc, truth = small_scene
    pc.enable_all(); oc.enable_all()
    rng = np.random.default_rng(1000 + seed)
    a = math.radians(alpha_deg)
    kinds = {k: {"ϵ": eps, "α": a} for k in ("plane", "sphere", "cylinder", "cone")}
    cp = R.params_to_c(R.ransacparameters(**kinds))
    b = 160
    arr = (L.Shape * b)()
    for i in range(b):
        s = arr[i]
        s.kind = i % 4
        s.outwards = int(rng.integers(0, 2))
        v = np.zeros(10)
        v[0:3] = rng.uniform(-20, 120, 3)                       # point / centre / axis / apex
        d = rng.normal(size=3)
        scale = [1.0, 1.0, 1e-3, 7.5, 1e3][int(rng.integers(0, 5))]   # non-unit directions must not break the bounds
        if s.kind == L.PLANE:
            v[3:6] = d / np.linalg.norm(d) * scale
        elif s.kind == L.SPHERE:
            v[3] = [0.01, 1.0, 10.0, 60.0, 500.0, -3.0][int(rng.integers(0, 6))]
        elif s.kind == L.CYLINDER:
            v[0:3] = d / np.linalg.norm(d) * scale
            v[3:6] = rng.uniform(-20, 120, 3)
            v[6] = [0.01, 1.0, 8.0, 80.0, -1.0][int(rng.integers(0, 5))]
        else:
            v[3:6] = d / np.linalg.norm(d) * scale
            v[6] = rng.uniform(0.01, 3.1)
        if i % 37 == 36:
            v[int(rng.integers(0, 7))] = [float("nan"), float("inf"), -float("inf"), 1e300][int(rng.integers(0, 4))]
        if i % 41 == 40:
            v[3:6] = 0.0                                          # zero normal / axis
        for j in range(10):
            s.v[j] = float(v[j])
        R.lib().rh_shape_finalize(C.byref(s))
    counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
    ocounts, omasks = oc.score_batch(to_orc_shapes(arr, b), to_orc_params(cp), want_masks=True)
    assert np.array_equal(counts, ocounts)
    assert np.array_equal(masks, omasks)
    assert np.array_equal(R.score_batch(pc, arr, cp), ocounts)
    # points that touch a group's bounding-box corner exactly: put a plane exactly eps off a point
    p0 = pc.vertices[pc.subsets[0][0] - 1]
    edge = R.FittedPlane(p0 + np.array([0, 0, eps]), [0, 0, 1.0])
    c1 = R.score_batch(pc, [edge], cp)
    assert np.array_equal(c1, oc.score_batch(to_orc_shapes(shape_array([edge]), 1), to_orc_params(cp)))


def test_scorecandidate_mirror_returns_reference_tuple(small_scene):
    pc, oc, truth = small_scene
    params = R.ransacparameters()
    cp = R.params_to_c(params)
    for cand in make_candidates(truth, 8, seed=2):
        ci, inpoints = R.scorecandidate(pc, cand, 1, params)
        cnt, oin = oc.scorecandidate(orc.Shape.from_buffer_copy(bytes(cand.to_c())), to_orc_params(cp))
        assert np.array_equal(inpoints, oin)             # subset order, 1-based original indices
        assert (ci.min, ci.max, ci.E) == orc.estimatescore(oc.s, oc.n, cnt)
    with pytest.raises(ValueError):
        R.scorecandidate(pc, cand, 2, params)


@pytest.mark.parametrize("no_spread", [False, pytest.param(True, marks=pytest.mark.diag)])
def test_score_is_invariant_to_the_order_of_the_batch(small_scene, monkeypatch, no_spread):
    """The library spreads neighbouring candidates over different 64-candidate chunks (diag build, RH_NO_SPREAD=1: batch
    order); counts and masks follow the caller's order whatever the internal one, host and device batches."""
    pc, oc, truth = small_scene
    cp = R.params_to_c(R.ransacparameters())
    cands = make_candidates(truth, 700, seed=21)
    order = np.random.default_rng(5).permutation(len(cands))
    by_prim = sorted(range(len(cands)), key=lambda i: (cands[i].__class__.__name__, i % len(truth)))
    ref_counts, ref_masks = R.score_batch(pc, shape_array(cands), cp, want_masks=True)
    for perm in (order, np.asarray(by_prim)):
        arr = shape_array([cands[i] for i in perm])
        counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
        assert np.array_equal(counts, ref_counts[perm]) and np.array_equal(masks, ref_masks[perm])
    if no_spread:
        monkeypatch.setenv("RH_NO_SPREAD", "1")
        counts, _ = R.score_batch(pc, shape_array(cands), cp, want_masks=True)
        assert np.array_equal(counts, ref_counts)


def test_score_respects_enabled_bits_and_sphere_quirk(small_scene):
    pc, oc, truth = small_scene
    rng = np.random.default_rng(3)
    mask = rng.random(pc.size) < 0.6
    pc.set_enabled(mask)
    oc.set_enabled(pc.enabled_chunks())
    assert pc.count_enabled() == int(mask.sum()) == oc.count_enabled()
    assert np.array_equal(pc.isenabled, mask)
    cands = make_candidates(truth, 64, seed=4)
    arr = shape_array(cands)
    for fixed in (0, 1):
        cp = R.params_to_c(R.ransacparameters(), sphere_uses_enabled=bool(fixed))
        counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
        ocounts, omasks = oc.score_batch(to_orc_shapes(arr, 64), to_orc_params(cp), want_masks=True)
        assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks)
    # Q4 (sphere.jl:121,131): in reference mode sphere counts ignore the enabled bits
    pc.enable_all(); oc.enable_all()
    cp = R.params_to_c(R.ransacparameters())
    full = R.score_batch(pc, arr, cp)
    pc.set_enabled(mask)
    part = R.score_batch(pc, arr, cp)
    for i, c in enumerate(cands):
        if c.kind == L.SPHERE:
            assert part[i] == full[i]
        elif full[i] > 100:
            assert part[i] < full[i]
    pc.enable_all(); oc.enable_all()


def test_refit_invalidate_select(small_scene):
    pc, oc, truth = small_scene
    pc.enable_all(); oc.enable_all()
    params = R.ransacparameters()
    cp = R.params_to_c(params)
    op = to_orc_params(cp)
    rng = np.random.default_rng(5)
    for cand in make_candidates(truth, 8, seed=6):
        ex = R.refit(cand, pc, params)
        oidx = oc.refit(orc.Shape.from_buffer_copy(bytes(cand.to_c())), op)
        assert np.array_equal(ex.inpoints, oidx)         # ascending original indices
        assert np.all(np.diff(ex.inpoints) > 0)
        R.invalidate_indexes(pc, ex.inpoints)
        oc.invalidate(oidx)
        assert np.array_equal(pc.enabled_chunks(), oc.get_enabled())
        n_en = pc.count_enabled()
        assert n_en == oc.count_enabled()
        ranks = np.concatenate([[1, n_en, n_en + 1, 0], rng.integers(1, n_en + 1, 50)])
        got = R.select_enabled(pc, ranks)
        exp = np.array([oc.select_enabled(int(r)) for r in ranks])
        assert np.array_equal(got, exp)
        # scoring after the extraction sees the new enabled bits
        arr = shape_array([cand])
        assert np.array_equal(R.score_batch(pc, arr, cp), oc.score_batch(to_orc_shapes(arr, 1), op))
    # refit with too small a buffer reports the needed size
    cs = R.FittedPlane(truth[0]["point"], truth[0]["normal"]).to_c()
    pc.enable_all()
    n = C.c_int64()
    small = np.zeros(4, dtype=np.int64)
    rc = R.lib().rh_refit(pc._h, C.byref(cs), C.byref(cp), small.ctypes.data_as(C.POINTER(C.c_int64)), 4, C.byref(n))
    assert rc == L.RH_E_CAPACITY and n.value > 4
    oc.enable_all()


@pytest.mark.parametrize("n,s", [(1, 1), (63, 63), (64, 64), (65, 33), (1023, 1023), (1025, 1025), (5000, 777)])
def test_ragged_sizes(n, s):
    rng = np.random.default_rng(n * 7 + s)
    xyz, nrm, truth = synth.make_cloud(n, ["plane", "sphere"], 0.1, seed=n)
    sub = (rng.permutation(n)[:s] + 1).astype(np.int64)
    pc = R.RANSACCloud(xyz, nrm, [sub])
    oc = orc.Cloud(xyz, nrm, sub)
    cp = R.params_to_c(R.ransacparameters(plane={"ϵ": 2.0}, sphere={"ϵ": 2.0}))
    cands = make_candidates(truth, 5, seed=n)
    arr = shape_array(cands)
    counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
    ocounts, omasks = oc.score_batch(to_orc_shapes(arr, 5), to_orc_params(cp), want_masks=True)
    assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks)
    for c in cands:
        ex = R.refit(c, pc, cp)
        assert np.array_equal(ex.inpoints, oc.refit(orc.Shape.from_buffer_copy(bytes(c.to_c())), to_orc_params(cp)))


def test_c_example_runs(score_path):
    """The plain-C example (examples/score_demo.c) through the same library, as a child process."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "score_demo")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "score_demo.c"),
                           "-L", os.path.join(root, "ransac.jl_amd"), "-lransac_hip", "-lm",
                           "-Wl,-rpath,$ORIGIN/../ransac.jl_amd", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "score_demo ok" in r.stdout, r.stdout + r.stderr


def test_empty_cloud_and_empty_subset():
    cp = R.params_to_c(R.ransacparameters())
    pc0 = R.RANSACCloud(np.zeros((0, 3)), np.zeros((0, 3)), [np.zeros(0, dtype=np.int64)])
    assert pc0.count_enabled() == 0
    plane = R.FittedPlane([0, 0, 0.0], [0, 0, 1.0])
    assert list(R.score_batch(pc0, [plane], cp)) == [0]
    assert R.refit(plane, pc0, cp).inpoints.size == 0
    got, _ = R.ransac(pc0, cp, seed=1)
    assert got == []
    # points but an empty subset 1: every score is 0, refit still scans the cloud
    xyz = np.array([[0, 0, 0.0], [1, 0, 0.1], [0, 1, -0.1], [5, 5, 5.0]])
    nrm = np.array([[0, 0, 1.0]] * 4)
    pc1 = R.RANSACCloud(xyz, nrm, [np.zeros(0, dtype=np.int64)])
    counts, masks = R.score_batch(pc1, [plane], cp, want_masks=True)
    assert list(counts) == [0] and masks.shape == (1, 0)
    assert list(R.refit(plane, pc1, cp).inpoints) == [1, 2, 3]
    assert list(R.select_enabled(pc1, [1, 4, 5])) == [1, 4, 0]


def test_empty_batch_and_bad_arguments(small_scene):
    pc, oc, truth = small_scene
    cp = R.params_to_c(R.ransacparameters())
    assert R.score_batch(pc, [], cp).size == 0
    bad = L.Shape()
    bad.kind = 9
    with pytest.raises(R.RansacHipError) as e:
        R.score_batch(pc, (L.Shape * 1)(bad), cp)
    assert e.value.code == L.RH_E_INVALID
    with pytest.raises(R.RansacHipError):
        R.invalidate_indexes(pc, [0])
    with pytest.raises(R.RansacHipError):
        R.invalidate_indexes(pc, [pc.size + 1])
    with pytest.raises(R.RansacHipError):      # subset index out of range
        R.RANSACCloud(np.zeros((4, 3)), np.zeros((4, 3)), [np.array([5], dtype=np.int64)])


def test_points_on_cone_axis_are_incompatible():
    # cone.jl:68-85: a point on the axis gives NaN -> incompatible
    apex, axis = np.array([0.0, 0, 0]), np.array([0.0, 0, 1.0])
    pts = np.array([[0, 0, 5.0], [0, 0, 0.0], [3.0, 0, 3.0], [-3.0, 0, 3.0]])
    nrm = np.array([[0, 0, 1.0], [0, 0, 1.0], [math.sqrt(.5), 0, -math.sqrt(.5)], [-math.sqrt(.5), 0, -math.sqrt(.5)]])
    sub = np.array([1, 2, 3, 4], dtype=np.int64)
    pc, oc = R.RANSACCloud(pts, nrm, [sub]), orc.Cloud(pts, nrm, sub)
    cone = R.FittedCone(apex, axis, math.pi / 2, True)
    cp = R.params_to_c(R.ransacparameters())
    counts, masks = R.score_batch(pc, [cone], cp, want_masks=True)
    ocounts, omasks = oc.score_batch(to_orc_shapes(shape_array([cone]), 1), to_orc_params(cp), want_masks=True)
    assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks)
    assert int(masks[0, 0]) == 0b1100


@pytest.mark.parametrize("f32", [False, True])
def test_candidates_through_cloud_points_match_oracle(f32):
    """Spheres centred ON a point of the cloud, cylinders and cones whose axis runs THROUGH points, cones with the apex on a
    point: the reference's normalisations give NaN there (incompatible), and the classifier of the culled kernel must not
    read anything else off its own 0 x inf (score4_device.h: the 1e-37 under the square root, the cone's axis guard).  A
    20 000-point subset so that the culled kernel runs; candidates with tiny and with scene-sized radii."""
    rng = np.random.default_rng(17)
    xyz, nrm, truth = synth.make_cloud(20_000, ["plane", "sphere", "cylinder", "cone"], 0.2, seed=31)
    if f32:
        xyz, nrm = xyz.astype(np.float32).astype(np.float64), nrm.astype(np.float32).astype(np.float64)
    subs = synth.make_subsets(20_000, 1, seed=31)
    cands = []
    for i in rng.integers(0, 20_000, size=40):
        p, q = xyz[i], xyz[rng.integers(0, 20_000)]
        ax = q - p
        if not np.linalg.norm(ax) > 1e-6:
            continue
        for r in (0.0, 1e-3, 0.3, 5.0, 40.0):
            cands.append(R.FittedSphere(p, r, bool(rng.integers(0, 2))))
            cands.append(R.FittedCylinder(ax / np.linalg.norm(ax), p, r, bool(rng.integers(0, 2))))     # axis through p and q
        for om in (0.05, 0.8, 2.5):
            cands.append(R.FittedCone(p, ax, om, bool(rng.integers(0, 2))))                            # apex on p, axis through q
    arr = shape_array(cands)
    if f32:
        for i in range(len(cands)):
            R.lib().rh_shape_finalize_f32(C.byref(arr[i]))
        pc = R.RANSACCloud(xyz.astype(np.float32), nrm.astype(np.float32), subs, force_eltype=np.float32)
        oc = orc.Cloud32(xyz.astype(np.float32), nrm.astype(np.float32), subs[0])
    else:
        pc, oc = R.RANSACCloud(xyz, nrm, subs), orc.Cloud(xyz, nrm, subs[0])
    for eps in (0.3, 5.0):
        prm = R.ransacparameters()
        for k in ("plane", "sphere", "cylinder", "cone"):
            prm[k]["ϵ"] = eps
        cp = R.params_to_c(prm)
        counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
        ocounts, omasks = oc.score_batch(to_orc_shapes(arr, len(cands)), to_orc_params(cp), want_masks=True)
        assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks)
        assert np.array_equal(R.score_batch(pc, arr, cp), ocounts)
    assert counts.sum() > 1000


def run_both(xyz, nrm, subs, params, seed, **kw):
    pc = R.RANSACCloud(xyz, nrm, subs)
    oc = orc.Cloud(xyz, nrm, subs[0])
    cp = R.params_to_c(params, **kw)
    got, secs, stats = R.ransac(pc, cp, seed=seed, return_stats=True)
    exp = oc.ransac(to_orc_params(cp), seed=seed)
    assert exp["rc"] == 0
    return pc, oc, got, exp, stats


def assert_same_run(pc, oc, got, exp, stats):
    assert stats["iterations"] == exp["iterations"]
    assert stats["candidates_scored"] == exp["candidates_scored"]
    assert stats["scored_left"] == exp["scored_left"]
    assert stats["draws"] == exp["draws"]                 # same RNG consumption
    assert len(got) == len(exp["shapes"])
    for g, e in zip(got, exp["shapes"]):
        assert bytes(g.c_shape) == bytes(e["shape"])      # parameters bit-identical (bar is 1e-5 rel)
        assert np.array_equal(g.inpoints, e["inpoints"])  # identical inlier index sets
        assert g.score_E == e["score_E"] and g.iteration == e["iteration"]
    assert np.array_equal(pc.enabled_chunks(), oc.get_enabled())


def test_ransac_cfg1_end_to_end():
    """BASELINE configs[0]: 50k plane+sphere, the reference's defaults, faithful mode
    (wrapping Int64 score, sphere ignores enabled): same minimal-set stream in => identical
    extracted shapes and index sets out."""
    c = synth.config("cfg1")
    subs = synth.make_subsets(50000, c["r"], c["seed"])
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere])
    pc, oc, got, exp, stats = run_both(c["xyz"], c["nrm"], subs, params, seed=1234)
    assert len(got) == 2 and {R.strt(g.shape) for g in got} == {"plane", "sphere"}
    assert sorted(len(g.inpoints) for g in got) == [25000, 25000]
    assert_same_run(pc, oc, got, exp, stats)


@pytest.mark.parametrize("seed,fixed", [(1, False), (2, False), (3, True)])
def test_ransac_multi_primitive_all_kinds(seed, fixed):
    """Many extractions with surviving / dying stored candidates of every kind: exercises the
    recomputed candidate liveness (driver.hip) against the oracle's stored index lists."""
    prim = ["plane", "sphere", "cylinder", "cone", "plane", "sphere"]
    xyz, nrm, truth = synth.make_cloud(24_000, prim, 0.05, seed=40 + seed)
    subs = synth.make_subsets(24_000, 2, seed=seed)
    params = R.ransacparameters(iteration={"minsubsetN": 60, "τ": 300, "itermax": 40, "prob_det": 0.5})
    kw = dict(score_mode=L.SCORE_F64, sphere_uses_enabled=True) if fixed else {}
    pc, oc, got, exp, stats = run_both(xyz, nrm, subs, params, seed=seed, **kw)
    assert len(got) >= 3
    assert_same_run(pc, oc, got, exp, stats)


@pytest.mark.parametrize("prims,kinds,seed,host", [
    (["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, False),   # device sampler + speculation
    (["plane", "sphere", "cylinder", "cone"], "all", 12, False),                             # cones on the device as well
    pytest.param(["plane", "sphere", "cylinder", "cone"], "all", 12, True, marks=pytest.mark.diag),                              # host twin of the sampler
    (["plane", "plane"], "p", 13, False),
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_NO_PIPELINE", marks=pytest.mark.diag),      # one window at a time
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_NO_FUSED_SCORE", marks=pytest.mark.diag),   # scores through the host
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_NO_FAST_EXTRACT", marks=pytest.mark.diag),  # liveness after the host saw the lengths
    # windows this short search the select directory; RH_LONG_WINDOW_SETS=0 sends them down the long-window
    # path (flat select list, rank-ordered compact records, sampling + fits in one kernel) and its variants
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_LONG_WINDOW_SETS", marks=pytest.mark.diag),
    pytest.param(["plane", "sphere", "cylinder", "cone"], "all", 12, "RH_LONG_WINDOW_SETS", marks=pytest.mark.diag),
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_LONG_WINDOW_SETS,RH_NO_FUSED_SAMPLER", marks=pytest.mark.diag),  # sample + fit as two kernels
    pytest.param(["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"], "psc", 11, "RH_LONG_WINDOW_SETS,RH_NO_CREC", marks=pytest.mark.diag),           # index-space sampling
])
def test_ransac_per_set_streams(prims, kinds, seed, host, monkeypatch):
    """sampling_streams = 1: sampling + fitting + scoring on the device, iterations speculated in
    pipelined windows; must equal the oracle's strictly sequential loop over the same per-set streams
    (also with each pipeline stage switched off)."""
    if isinstance(host, str):
        for name in host.split(","):
            monkeypatch.setenv(name, "0" if name == "RH_LONG_WINDOW_SETS" else "1")
    elif host:
        monkeypatch.setenv("RH_HOST_SAMPLER", "1")
    xyz, nrm, truth = synth.make_cloud(30_000, prims, 0.1, seed=60 + seed)
    subs = synth.make_subsets(30_000, 2, seed=seed)
    types = {"psc": [R.FittedPlane, R.FittedSphere, R.FittedCylinder], "p": [R.FittedPlane],
             "all": [R.FittedPlane, R.FittedCone, R.FittedCylinder, R.FittedSphere]}[kinds]
    params = R.ransacparameters(types, iteration={"minsubsetN": 50, "τ": 300, "itermax": 300, "prob_det": 0.6})
    pc, oc, got, exp, stats = run_both(xyz, nrm, subs, params, seed=seed, score_mode=L.SCORE_F64,
                                       sphere_uses_enabled=True, sampling_streams=1)
    assert len(got) >= 2
    assert_same_run(pc, oc, got, exp, stats)
    # and it differs from the sequential-stream run (different draws), while both find the big shapes
    pc2 = R.RANSACCloud(xyz, nrm, subs)
    got0, _ = R.ransac(pc2, R.params_to_c(params, score_mode=L.SCORE_F64, sphere_uses_enabled=True), seed=seed)
    assert len(got0) >= 2


@pytest.mark.parametrize("prims,kinds,seed,host", [
    (["plane", "sphere", "cylinder", "plane", "sphere", "cylinder", "plane", "sphere"], "psc", 21, False),
    (["plane", "sphere", "cylinder", "cone", "cone"], "all", 22, False),     # cones fitted on the device too
    pytest.param(["plane", "sphere", "cylinder", "cone", "cone"], "all", 22, True, marks=pytest.mark.diag),      # same streams drawn on the host
])
def test_ransac_octree_sampling(prims, kinds, seed, host, monkeypatch):
    """octree_sampling = 1 (fixed behaviour, docs/src/ransac.md:73-96): level-weighted cells of a
    linear octree, level distribution updated from the scores -- device windows vs the oracle's
    sequential loop, identical shapes / index sets / draw counts."""
    if host:
        monkeypatch.setenv("RH_HOST_SAMPLER", "1")
    xyz, nrm, truth = synth.make_cloud(40_000, prims, 0.25, seed=80 + seed)
    subs = synth.make_subsets(40_000, 4, seed=seed)
    types = {"psc": [R.FittedPlane, R.FittedSphere, R.FittedCylinder],
             "all": [R.FittedPlane, R.FittedCone, R.FittedCylinder, R.FittedSphere]}[kinds]
    params = R.ransacparameters(types, iteration={"minsubsetN": 40, "τ": 300, "itermax": 200, "prob_det": 0.6})
    kw = dict(score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    pc, oc, got, exp, stats = run_both(xyz, nrm, subs, params, seed=seed, octree_sampling=True, **kw)
    assert len(got) >= 4
    assert_same_run(pc, oc, got, exp, stats)
    # local sampling produces far more candidates per minimal set than root-cell sampling
    pc2 = R.RANSACCloud(xyz, nrm, subs)
    _, _, st_root = R.ransac(pc2, R.params_to_c(params, **kw), seed=seed, return_stats=True)
    assert stats["candidates_scored"] > 5 * max(1, st_root["candidates_scored"])
    with pytest.raises(R.RansacHipError):   # needs per-set streams
        R.ransac(pc2, R.params_to_c(params, octree_sampling=True), seed=seed)


def test_ransac_octree_window_longer_than_its_launch_bound():
    """A window of the candidate loop is put on the stream before the length of its candidate list is known: the score
    launch is sized from the previous windows' lengths.  Thousands of minimal sets per iteration with octree sampling
    give a first window with more candidates than that bound covers (1024 at the start) -- every one of them has to
    be scored all the same (the kernel walks its rows grid-stride).  Regression: the culled kernel once left the
    candidates beyond the bound at count 0, and WHICH ones depended on the order the fits were appended in."""
    prims = ["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"]
    xyz, nrm, truth = synth.make_cloud(60_000, prims, 0.2, seed=701)
    subs = synth.make_subsets(60_000, 6, seed=7)
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    params = R.ransacparameters(types, iteration={"minsubsetN": 6000, "τ": 300, "itermax": 10, "prob_det": 0.9})
    kw = dict(score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    pc, oc, got, exp, stats = run_both(xyz, nrm, subs, params, seed=5, octree_sampling=True, **kw)
    assert stats["candidates_scored"] > 1024 * 1.5 * stats["iterations"]   # the first window alone is beyond the bound
    assert_same_run(pc, oc, got, exp, stats)
    # and the same run again on the same cloud gives the same thing (the defect was a race on list positions)
    pc.enable_all()
    got2, _, stats2 = R.ransac(pc, R.params_to_c(params, octree_sampling=True, **kw), seed=5, return_stats=True)
    assert stats2["draws"] == stats["draws"] and len(got2) == len(got)
    for a, b in zip(got, got2):
        assert np.array_equal(a.inpoints, b.inpoints)


def test_ransac_octree_iterations_beyond_the_advance_kernels_lds_buffer():
    """The kernel that ends an iteration of a chained octree window (sampler.hip, oct_advance_kernel) sorts the
    iteration's scores into candidate order in LDS when there are at most 6144 of them and in global memory beyond:
    10 000 minimal sets per iteration on a dense cloud give ~7000 candidates per iteration -- the second form, a store of
    tens of thousands after the first iteration, an extraction in every iteration."""
    prims = ["plane", "sphere", "cylinder", "plane", "sphere", "cylinder"]
    xyz, nrm, truth = synth.make_cloud(60_000, prims, 0.1, seed=702)
    subs = synth.make_subsets(60_000, 6, seed=8)
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    params = R.ransacparameters(types, iteration={"minsubsetN": 10000, "τ": 300, "itermax": 4, "prob_det": 0.999})
    kw = dict(score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    pc, oc, got, exp, stats = run_both(xyz, nrm, subs, params, seed=5, octree_sampling=True, **kw)
    assert stats["candidates_scored"] > 6144 * stats["iterations"]
    assert_same_run(pc, oc, got, exp, stats)


@pytest.mark.parametrize("cache", [True, pytest.param(False, marks=pytest.mark.diag)])
def test_ransac_calls_in_a_row_on_one_cloud(cache, monkeypatch):
    """rh_ransac parks its windows, device store and pinned scratch on the cloud for the next call
    (RH_NO_DRIVER_CACHE=1: every call allocates its own).  Four runs in a row on one cloud, with different shape
    types, window sizes and sampling modes, a continuation on the points the previous run left and a failing
    call in between: every run equals the oracle's."""
    if not cache:
        monkeypatch.setenv("RH_NO_DRIVER_CACHE", "1")
    prims = ["plane", "sphere", "cylinder", "plane", "cone", "sphere"]
    xyz, nrm, truth = synth.make_cloud(36_000, prims, 0.15, seed=314)
    subs = synth.make_subsets(36_000, 3, seed=15)
    pc, oc = R.RANSACCloud(xyz, nrm, subs), orc.Cloud(xyz, nrm, subs[0])
    kw = dict(score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    runs = [
        ([R.FittedPlane, R.FittedSphere, R.FittedCylinder], {"minsubsetN": 60, "τ": 300, "itermax": 120, "prob_det": 0.6}, kw, 5, True),
        ([R.FittedPlane, R.FittedCone, R.FittedCylinder, R.FittedSphere], {"minsubsetN": 25, "τ": 200, "itermax": 60, "prob_det": 0.5},
         dict(kw, octree_sampling=True), 6, True),
        ([R.FittedSphere, R.FittedPlane], {"minsubsetN": 200, "τ": 500, "itermax": 40, "prob_det": 0.7}, kw, 7, False),   # goes on
        ([R.FittedPlane, R.FittedSphere, R.FittedCylinder], {"minsubsetN": 15, "τ": 900, "itermax": 30, "prob_det": 0.9}, {}, 8, True),
    ]
    for i, (types, it, kws, seed, reset) in enumerate(runs):
        if reset:
            pc.enable_all()
            oc.enable_all()
        cp = R.params_to_c(R.ransacparameters(types, iteration=it), **kws)
        got, _, stats = R.ransac(pc, cp, seed=seed, return_stats=True)
        exp = oc.ransac(to_orc_params(cp), seed=seed)
        assert exp["rc"] == 0
        assert_same_run(pc, oc, got, exp, stats)
        if i == 1:
            with pytest.raises(R.RansacHipError):   # an invalid call between two runs leaves the parked buffers alone
                R.ransac(pc, R.params_to_c(R.ransacparameters(types, iteration=it), octree_sampling=True), seed=seed)


def test_ransac_injected_stream_and_preexisting_disabled_points():
    xyz, nrm, truth = synth.make_cloud(12_000, ["plane", "sphere", "cylinder"], 0.1, seed=77)
    subs = synth.make_subsets(12_000, 2, seed=77)
    pc, oc = R.RANSACCloud(xyz, nrm, subs), orc.Cloud(xyz, nrm, subs[0])
    dis = np.random.default_rng(1).random(12_000) < 0.15
    pc.set_enabled(~dis)
    oc.set_enabled(pc.enabled_chunks())
    stream = np.random.default_rng(2).integers(0, 2 ** 63, size=500, dtype=np.uint64) * np.uint64(2)
    cp = R.params_to_c(R.ransacparameters(iteration={"minsubsetN": 40, "τ": 200, "itermax": 25, "prob_det": 0.5}))
    got, secs, stats = R.ransac(pc, cp, seed=9, stream=stream, return_stats=True)
    exp = oc.ransac(to_orc_params(cp), seed=9, stream=stream)
    assert len(got) >= 1
    assert_same_run(pc, oc, got, exp, stats)
    # ransac(pc, params, true) re-enables everything first (iterations.jl:14-21)
    got2, _ = R.ransac(pc, cp, setenabled=True, seed=9)
    oc.enable_all()
    exp2 = oc.ransac(to_orc_params(cp), seed=9)
    assert [bytes(g.c_shape) for g in got2] == [bytes(e["shape"]) for e in exp2["shapes"]]


def test_refit_lsq_recovers_primitives_and_matches_oracle(small_scene):
    """Least-squares refit (f64 MFMA normal equations).  No reference behaviour exists (the reference's
    refit returns the shape unchanged), so the oracle's sequential twin is the specification: floating
    point sums differ only in order -> parameters agree to 1e-8 relative; and the refit pulls a 1 %-jittered
    candidate back onto the ground-truth primitive."""
    pc, oc, truth = small_scene
    pc.enable_all(); oc.enable_all()
    params = R.ransacparameters()
    cp = R.params_to_c(params)
    op = to_orc_params(cp)
    cands = make_candidates(truth, 16, seed=3)
    seen = set()
    for cand, t in zip(cands, truth * 2):
        if cand.kind != L.PLANE:
            cand.outwards = True      # the synthetic primitives' normals point outwards
        got, n, rms, it = R.refit_lsq(cand, pc, cp, max_iter=12)
        exp, on, orms, oit = oc.refit_lsq(orc.Shape.from_buffer_copy(bytes(cand.to_c())), op, max_iter=12)
        assert n == on and n > 500, (R.strt(cand), n, on)
        assert 1 <= it < 12 and abs(it - oit) <= 1, (R.strt(cand), it, oit)   # converged; the stop test sits at a threshold
        gv, ev = np.array(list(got.to_c().v)), np.array(list(exp.v))
        assert np.allclose(gv, ev, rtol=1e-8, atol=1e-9), (R.strt(cand), gv, ev)
        assert abs(rms - orms) <= 1e-9 + 1e-6 * orms
        assert rms < 0.05          # synthetic noise sigma = 0.02
        seen.add(got.kind)
        if got.kind == L.PLANE:
            tn = np.asarray(t["normal"])
            assert abs(abs(got.normal @ tn) - 1) < 1e-6
            assert abs((got.point - np.asarray(t["point"])) @ tn) < 0.01
        elif got.kind == L.SPHERE:
            assert np.linalg.norm(got.center - t["center"]) < 0.01 and abs(got.radius - t["radius"]) < 0.01
        elif got.kind == L.CYLINDER:
            ta = np.asarray(t["axis"])
            assert abs(abs(got.axis @ ta) - 1) < 1e-5 and abs(got.radius - t["radius"]) < 0.01
            d = got.center - np.asarray(t["center"])
            assert np.linalg.norm(d - ta * (d @ ta)) < 0.02
        else:
            ta = np.asarray(t["axis"])
            assert abs(abs(got.axis @ ta) - 1) < 1e-4 and abs(got.opang - t["opang"]) < 2e-3
            assert np.linalg.norm(got.apex - t["apex"]) < 0.1
    assert seen == {L.PLANE, L.SPHERE, L.CYLINDER, L.CONE}
    far = R.FittedSphere([1e4, 1e4, 1e4], 1.0, True)      # nothing within 3 eps: a clear error, not a NaN shape
    with pytest.raises(R.RansacHipError):
        R.refit_lsq(far, pc, cp)


def test_largestconncomp_known_answers(golden):  # test/parameterspacebitmap.jl:1-55
    from test_oracle_golden import build_cc_case
    g = golden["largestconncomp"]
    for case in ("dense", "eight"):
        bm, idx = build_cc_case(g["size"], g[case]["patches"])
        indmap = [[idx.get((x, y), []) for y in range(bm.shape[1])] for x in range(bm.shape[0])]
        for conn, key in (("default", "expected_conn4"), ("eight", "expected_conn8")):
            exp = g[case][key]
            assert R.largestconncomp(bm, indmap, conn) == exp["idx"] * exp["repeat"]


@pytest.mark.parametrize("shape,density,seed", [((1, 1), 1.0, 0), ((7, 300), 0.55, 1), ((257, 129), 0.45, 2),
                                                 ((640, 480), 0.6, 3), ((64, 64), 0.0, 4), ((300, 300), 1.0, 5)])
def test_largestconncomp_random_bitmaps(shape, density, seed):
    bm = np.random.default_rng(seed).random(shape) < density
    for conn8 in (False, True):
        got = R.largestconncomp(bm, None, "eight" if conn8 else "default")
        assert np.array_equal(got, orc.largestconncomp(bm, conn8=conn8))


def _serpentine():
    """64 x 64, one path: every other column full, joined to the next at alternating ends -- 2079 pixels in a chain"""
    bm = np.zeros((64, 64), dtype=bool)
    bm[0::2, :] = True
    for k, x in enumerate(range(1, 63, 2)):
        bm[x, 63 if k % 2 == 0 else 0] = True
    return bm


@pytest.mark.parametrize("cut", [False, True])
def test_largestconncomp_serpentine(cut):
    """one long chain: finds that walk far and halve their paths on the way (union_find.h); cut in two by one cleared
    pixel in the middle, the halves differ by a few pixels"""
    bm = _serpentine()
    assert bm.sum() == 32 * 64 + 31
    if cut:
        bm[32, 30] = False
    for conn8 in (False, True):
        got = R.largestconncomp(bm, None, "eight" if conn8 else "default")
        exp = orc.largestconncomp(bm, conn8=conn8)
        assert np.array_equal(got, exp)
        assert len(got) == (bm.sum() if not cut else max(16 * 64 + 16 + 30, 15 * 64 + 15 + 33))


@pytest.mark.diag
def test_full_size_octree_leg_is_the_same_run_under_every_switch(monkeypatch):
    """The bench's octree-sampling leg at full size (cfg3: 10M points, minsubsetN = 4096, ~1000 candidates per iteration,
    a store of ~100 000 candidates at the first extraction) -- too large for the oracle, so the size-independent property:
    the run is ONE run whichever of its pieces is switched off (chained windows, the device-managed store, the v4
    liveness pass, the sampler's cell directory, two windows in flight, scoring fused into the window), and the same
    run twice in a row.  Regression: the v4 score launch once left the candidates beyond its launch bound unscored and the
    leg's draw counts varied from run to run."""
    c = synth.config("cfg3")
    subs = synth.make_subsets(c["xyz"].shape[0], c["r"], c["seed"])
    pc = R.RANSACCloud(c["xyz"], c["nrm"], subs)
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    params = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 128, "τ": 900, "prob_det": 0.9})
    cp = R.params_to_c(params, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1, octree_sampling=True)

    def run():
        pc.enable_all()
        got, _, st = R.ransac(pc, cp, seed=1234, return_stats=True)
        return (st["draws"], st["candidates_scored"], st["scored_left"], [(g.iteration, bytes(g.c_shape), g.inpoints.tobytes()) for g in got])

    ref = run()
    assert len(ref[3]) >= 10 and ref[1] > 100_000
    assert run() == ref
    for sw in ("RH_NO_OCT_CHAIN", "RH_NO_MANAGED_STORE", "RH_NO_OCT_TAB", "RH_OCT_ONE_WINDOW", "RH_NO_FUSED_SCORE"):
        monkeypatch.setenv(sw, "1")
        assert run() == ref, sw
        monkeypatch.delenv(sw)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg5"])
def test_full_size_properties(cfg):
    """BASELINE configs[1], [2] and [4] at full size (1M / 10M / 50M points, r = 32, B = 4096; cfg5 with cones):
    size-independent properties, plus an oracle check on a slice of the batch that holds every kind."""
    c = synth.config(cfg)
    n = c["xyz"].shape[0]
    subs = synth.make_subsets(n, c["r"], c["seed"])
    pc = R.RANSACCloud(c["xyz"], c["nrm"], subs)
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder] + ([R.FittedCone] if cfg == "cfg5" else [])
    cp = R.params_to_c(R.ransacparameters(types))
    cands = make_candidates(c["truth"], 4096, seed=8)
    arr = shape_array(cands)
    nmask = 4096 if cfg != "cfg5" else 480           # cfg5: 24 415 mask words per candidate -- masks for 10 rounds of the 48 primitives
    counts_m, masks = R.score_batch(pc, shape_array(cands[:nmask]), cp, want_masks=True)
    pop = np.bitwise_count(masks).sum(axis=1, dtype=np.int64)
    assert np.array_equal(pop, counts_m)                  # checksum of checksums
    counts = R.score_batch(pc, arr, cp)
    assert np.array_equal(counts[:nmask], counts_m)       # idempotent, both instantiations
    assert np.array_equal(R.score_batch(pc, arr, cp), counts)
    assert counts.max() <= subs[0].size and counts.sum() > 4096 * 100
    oc = orc.Cloud(c["xyz"], c["nrm"], subs[0])
    # oracle on: the whole batch (cfg2), every second candidate (cfg3; bench.py --full checks all 4096 on every run), every fourth
    # (cfg5: 1024 candidates, 170 of them cones; ~5 s on 16 threads at S = 1 562 500)
    sel = list(range(0, 4096, {"cfg2": 1, "cfg3": 2, "cfg5": 4}[cfg]))
    kinds_in = {cands[i].kind for i in sel}
    assert kinds_in == ({L.PLANE, L.SPHERE, L.CYLINDER, L.CONE} if cfg == "cfg5" else {L.PLANE, L.SPHERE, L.CYLINDER})
    sub_arr = shape_array([cands[i] for i in sel])
    ocounts = oc.score_batch_mt(to_orc_shapes(sub_arr, len(sel)), to_orc_params(cp), 16)
    assert np.array_equal(ocounts, counts[sel])
    if cfg == "cfg5":
        cone_sel = [i for i in sel if cands[i].kind == L.CONE]
        assert len(cone_sel) >= 8 and counts[cone_sel].max() > 1000       # cones of the batch really collect inliers
    # masks against the oracle's, bit for bit: every row the GPU wrote (4096 at cfg2 / cfg3; cfg5: 480 rows = ten rounds of the
    # 48 primitives), in slices that bound the oracle's memory
    for m0 in range(0, nmask, 512):
        msel = list(range(m0, min(nmask, m0 + 512)))
        oc_c, oc_m = oc.score_masks_mt(to_orc_shapes(shape_array([cands[i] for i in msel]), len(msel)), to_orc_params(cp), 16)
        assert np.array_equal(oc_m, masks[msel]) and np.array_equal(oc_c, counts[msel]), (cfg, m0)
    # refit: ascending, all enabled before, none after invalidation, disjoint extractions
    seen = np.zeros(n, dtype=bool)
    todo = cands[:6] if cfg == "cfg2" else [cands[0], cands[16], cands[28], cands[40], cands[47]]   # cfg5: every kind, two cones
    if cfg == "cfg3":
        todo = [cands[0], cands[16], cands[28], cands[1], cands[29], cands[2]]      # plane, sphere, cylinder, ...
    for j, cand in enumerate(todo):
        ex = R.refit(cand, pc, cp)
        assert np.all(np.diff(ex.inpoints) > 0) and not seen[ex.inpoints - 1].any()
        if cfg == "cfg5" and j in (0, 3):      # a plane and a cone scan against the oracle's list, on the enabled set as it stands
            assert np.array_equal(ex.inpoints, oc.refit(to_orc_shapes(shape_array([cand]), 1)[0], to_orc_params(cp)))
        if cfg == "cfg3" and j in (0, 2):      # a plane and a cylinder: the 10M-point scan against the oracle's list, both scans
            want = oc.refit(to_orc_shapes(shape_array([cand]), 1)[0], to_orc_params(cp))
            assert want.size > 1000 and np.array_equal(ex.inpoints, want)
            try:
                for path in ("scan", "culled"):        # (the option is read on every refit)
                    R.set_option("refit_path", path, cloud=pc)
                    assert np.array_equal(R.refit(cand, pc, cp).inpoints, want), path
            finally:
                R.set_option("refit_path", None, cloud=pc)
        seen[ex.inpoints - 1] = True
        R.invalidate_indexes(pc, ex.inpoints)
        oc.invalidate(ex.inpoints)
        assert R.refit(cand, pc, cp).inpoints.size == 0
    assert pc.count_enabled() == n - int(seen.sum())
    assert np.array_equal(pc.isenabled, ~seen)
    if cfg == "cfg5":   # and the batch again on the thinned cloud (enabled bits in play at full size)
        again = R.score_batch(pc, sub_arr, cp)
        assert np.array_equal(again, oc.score_batch_mt(to_orc_shapes(sub_arr, len(sel)), to_orc_params(cp), 16))


@pytest.mark.diag
def test_subset_order_made_on_the_device_or_on_the_host_gives_the_same_results(monkeypatch):
    """The internal order of subset 1 (k-d leaves of 64 points) is made on the device (kdorder.hip) unless RH_KD_HOST=1
    keeps the host's nth_element recursion, the bounding cube on the device unless RH_AABB_HOST=1: counts, masks (in
    SUBSET order) and an octree-sampling run (its Morton codes hang on the cube) must not depend on either -- and both must
    equal the oracle's."""
    prim = ["plane", "plane", "sphere", "cylinder", "cone", "cylinder"]
    xyz, nrm, truth = synth.make_cloud(200_000, prim, 0.25, seed=77)
    xyz[5] = [np.nan, 3.0, 4.0]                      # a NaN among the points: neither order may trip on it
    subs = synth.make_subsets(200_000, 3, seed=77)
    oc = orc.Cloud(xyz, nrm, subs[0])
    cp = R.params_to_c(R.ransacparameters())
    cands = make_candidates(truth, 300, seed=5)
    arr = shape_array(cands)
    ocounts, omasks = oc.score_batch(to_orc_shapes(arr, len(cands)), to_orc_params(cp), want_masks=True)
    rp = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder], iteration={"minsubsetN": 300, "itermax": 40, "τ": 300, "prob_det": 0.9})
    rcp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1, octree_sampling=True)
    exp = oc.ransac(to_orc_params(rcp), seed=5)
    assert ocounts.sum() > 10000 and len(exp["shapes"]) >= 3
    radii = {}
    for host in (False, True):
        if host:
            monkeypatch.setenv("RH_KD_HOST", "1")
            monkeypatch.setenv("RH_AABB_HOST", "1")
        pc = R.RANSACCloud(xyz, nrm, subs)
        counts, masks = R.score_batch(pc, arr, cp, want_masks=True)
        assert np.array_equal(counts, ocounts) and np.array_equal(masks, omasks), host
        got, _, st = R.ransac(pc, rcp, seed=5, return_stats=True)
        assert st["draws"] == exp["draws"] and len(got) == len(exp["shapes"])
        for g, e in zip(got, exp["shapes"]):
            assert bytes(g.c_shape) == bytes(e["shape"]) and np.array_equal(g.inpoints, e["inpoints"])
        out = np.zeros(56, dtype=np.uint64)
        L.check(R.lib().rh_dbg_cls_soundness(pc._h, arr, len(cands), C.byref(cp), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        out = out[:40].reshape(4, 10).astype(np.int64)
        assert out[:, [2, 6, 7, 9]].sum() == 0
        radii[host] = out[:, 1].sum() / out[:, 0].sum()      # share of (candidate, group) pairs the box tests skip
    # the two orders cull alike (same tree, ties and binary32 keys aside)
    assert abs(radii[True] - radii[False]) < 0.02, radii


def test_full_size_ransac_cfg3_replays_through_the_abi():
    """BASELINE configs[2] at full size, end to end: every shape rh_ransac extracted is replayed with
    the single-shot ABI calls on a second cloud (refit on the enabled set as it stood, then invalidate);
    the index lists must agree bit for bit, be ascending and pairwise disjoint."""
    c = synth.config("cfg3")
    n = c["xyz"].shape[0]
    subs = synth.make_subsets(n, c["r"], c["seed"])
    pc = R.RANSACCloud(c["xyz"], c["nrm"], subs)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder],
                                iteration={"minsubsetN": 4096, "itermax": 2048})
    got, _, stats = R.ransac(pc, params, seed=7, score_mode=L.SCORE_F64, sampling_streams=1, return_stats=True)
    assert len(got) >= 40 and stats["iterations"] == 2048
    replay = R.RANSACCloud(c["xyz"], c["nrm"], subs)
    cp = R.params_to_c(params, score_mode=L.SCORE_F64)
    seen = np.zeros(n, dtype=bool)
    for g in got:
        ex = R.refit(g.c_shape, replay, cp)
        assert np.array_equal(ex.inpoints, g.inpoints)
        assert np.all(np.diff(g.inpoints) > 0) and not seen[g.inpoints - 1].any()
        seen[g.inpoints - 1] = True
        R.invalidate_indexes(replay, ex.inpoints)
    assert np.array_equal(pc.isenabled, ~seen) and np.array_equal(replay.isenabled, ~seen)
    # the 40 ground-truth primitives carry 175 000 points each; every one must have been found
    assert sorted(len(g.inpoints) for g in got)[-40] > 150_000


def test_score_on_callers_stream_matches():
    """rh_cloud_set_stream: the cloud's work goes to a torch stream; a fill before and a read after are
    ordered by that stream alone (what dist.score_batch_sharded(same_stream=True) relies on)."""
    import torch
    from ransac_jl_amd import dist as rdist
    xyz, nrm, truth = synth.make_cloud(200_000, ["plane", "sphere", "cylinder", "cone"], 0.2, seed=77)
    subs = synth.make_subsets(200_000, 4, seed=77)
    pc = R.RANSACCloud(xyz, nrm, subs)
    cp = R.params_to_c(R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone]))
    shapes = make_candidates(truth, 300, seed=3)
    want = R.score_batch(pc, shapes, cp)
    arr = (L.Shape * len(shapes))(*[s.to_c() for s in shapes])
    batch = rdist.DeviceBatch(pc, arr, len(shapes))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pc.set_stream(st.cuda_stream)
        counts = torch.full((len(shapes),), -7, dtype=torch.int32, device="cuda")
        fn = rdist.gpu_local_score(pc, batch, cp, wait=False)
        for _ in range(3):
            rdist.score_batch_sharded(len(shapes), 0, 1, fn, counts, same_stream=True)
        got = counts.cpu().numpy()      # stream-ordered copy on `st`
    pc.set_stream(None)
    batch.free()
    assert np.array_equal(got, np.asarray(want))


def test_non_finite_and_duplicate_points_match_oracle():
    """NaN / inf coordinates and normals and heavy duplication in subset 1: the k-d leaf order, the
    group boxes and the band prefilter must leave every count equal to the oracle's (NaN never passes)."""
    rng = np.random.default_rng(5)
    xyz, nrm, truth = synth.make_cloud(40_000, ["plane", "sphere", "cylinder", "cone"], 0.2, seed=91)
    xyz = xyz.copy(); nrm = nrm.copy()
    bad = rng.choice(40_000, size=400, replace=False)
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:200], rng.integers(0, 3, 100)] = np.inf
    xyz[bad[200:250], rng.integers(0, 3, 50)] = -np.inf
    nrm[bad[250:350], rng.integers(0, 3, 100)] = np.nan
    nrm[bad[350:400]] = 0.0
    xyz[5000:9000] = xyz[4999]          # 4000 copies of one point: zero-extent k-d nodes
    nrm[5000:9000] = nrm[4999]
    subs = synth.make_subsets(40_000, 2, seed=9)
    pc = R.RANSACCloud(xyz, nrm, subs)
    oc = orc.Cloud(xyz, nrm, subs[0])
    cp = R.params_to_c(R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone]))
    shapes = make_candidates(truth, 200, seed=2)
    got, gmask = R.score_batch(pc, shapes, cp, want_masks=True)
    arr = (L.Shape * len(shapes))(*[s.to_c() for s in shapes])
    exp, emask = oc.score_batch(to_orc_shapes(arr, len(shapes)), to_orc_params(cp), want_masks=True)
    assert np.array_equal(got, exp)
    assert np.array_equal(gmask, emask)
    assert got.max() > 100


def test_results_own_their_index_lists_until_freed():
    """Two rh_ransac results alive at once: each owns its own pinned arena (the pool hands a block out
    once), freeing in either order is fine, and a later run re-uses a returned block."""
    c = synth.config("cfg1")
    subs = synth.make_subsets(50000, c["r"], c["seed"])
    cp = R.params_to_c(R.ransacparameters([R.FittedPlane, R.FittedSphere]), sampling_streams=1)
    lib = R.lib()

    def run(seed):
        pc = R.RANSACCloud(c["xyz"], c["nrm"], subs)
        rng = L.Rng()
        lib.rh_rng_seed(C.byref(rng), seed)
        res = L.Result()
        L.check(lib.rh_ransac(pc._h, pc.vertices.ctypes.data_as(C.POINTER(C.c_double)),
                              pc.normals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cp), C.byref(rng), C.byref(res)))
        lists = [np.ctypeslib.as_array(res.shapes[i].inpoints, shape=(res.shapes[i].n_inpoints,)) for i in range(res.n_shapes)]
        return pc, res, lists

    pc1, r1, l1 = run(1)
    snap = [a.copy() for a in l1]
    pc2, r2, l2 = run(1)
    assert r1.arena and r2.arena and r1.arena != r2.arena
    assert r1.n_shapes == r2.n_shapes == 2
    for a, b, s0 in zip(l1, l2, snap):
        assert np.array_equal(a, s0) and np.array_equal(a, b)       # the second run did not touch the first result
        assert np.all(np.diff(a) > 0) and a[0] >= 1 and a[-1] <= 50000
    first = r1.arena
    lib.rh_result_free(C.byref(r1))
    assert not r1.arena and r1.n_shapes == 0
    pc3, r3, l3 = run(1)
    assert r3.arena == first                                        # recycled block
    assert all(np.array_equal(a, b) for a, b in zip(l2, l3))
    lib.rh_result_free(C.byref(r3))
    lib.rh_result_free(C.byref(r2))


def test_scorecandidates_and_removeinvalidshapes_mirror(small_scene):
    """The reference's per-iteration bookkeeping on top of the batched launch: scorecandidates! records
    (score, inpoints) per candidate in order and empties its inputs; after an extraction
    removeinvalidshapes! drops exactly the candidates that own a disabled point (fitting.jl:181-221)."""
    pc, oc, truth = small_scene
    params = R.ransacparameters()
    pc.enable_all()
    cands = make_candidates(truth, 12, seed=4)
    keep = list(cands)
    levels = [1] * len(cands)
    ic = R.IterationCandidates()
    R.scorecandidates(pc, ic, cands, 1, params, levels)
    assert cands == [] and levels == [] and len(ic) == len(keep)
    for shp, sc, ip in zip(keep, ic.scores, ic.inpoints):
        sc1, ip1 = R.scorecandidate(pc, shp, 1, params)
        assert (sc.min, sc.max) == (sc1.min, sc1.max) and np.array_equal(ip, ip1)
    best = R.findhighestscore(ic)["index"]
    ex = R.refit(ic.shapes[best - 1], pc, params)
    R.invalidate_indexes(pc, ex.inpoints)
    en = pc.isenabled
    expect = [i for i, ip in enumerate(ic.inpoints) if ip.size == 0 or en[ip - 1].all()]
    shapes_before = list(ic.shapes)
    R.deleteat(ic, best)
    expect = [shapes_before[i] for i in expect if i != best - 1]
    R.removeinvalidshapes(pc, ic)
    assert ic.shapes == expect
    pc.enable_all()


def _ransac_via_call_sites(pc, params, seed, batched=False):
    """The reference's own loop (iterations.jl:35-162) written against the API mirrors, with ONLY the three
    hot calls going to the device -- scorecandidates! (batched), refit, invalidate_indexes! -- plus the
    k-th-enabled select; sampling, fits, score statistics and candidate bookkeeping stay on the host, as in
    julia/RANSACHIP.jl's `ransac`.  batched: the iteration's minsubsetN calls of samplepointcloud4! as ONE
    rh_sample_sets launch on the same generator (instead of a select round trip per point).  Returns (extracted,
    iterations, draws)."""
    lib = R.lib()
    it = params["iteration"]
    drawN, minsubsetN, tau, itermax, prob_det = it["drawN"], it["minsubsetN"], it["τ"], it["itermax"], it["prob_det"]
    which = {"lengthC": 0, "allcand": 1, "nofminset": 2}
    rng = L.Rng()
    lib.rh_rng_seed(C.byref(rng), seed)
    rnd = lambda n: lib.rh_rng_range(C.byref(rng), n)
    candidates, levels, ic, extracted = [], [], R.IterationCandidates(), []
    cc = [0, 0, 0]
    en = pc.isenabled
    iterations = 0
    for k in range(1, itermax + 1):
        if int(en.sum()) < tau:
            break
        if batched:
            sets, ok, _lev = R.sample_sets(pc, drawN, rng, minsubsetN)
            for j in range(minsubsetN):
                if ok[j]:
                    idx = sets[j] - 1
                    R.forcefitshapes(pc.vertices[idx], pc.normals[idx], params, candidates, levels, 1, pc)
        for _ in range(0 if batched else minsubsetN):
            # samplepointcloud4! (fitting.jl:383-430), root cell
            first = rnd(pc.size)
            while not en[first - 1]:
                first = rnd(pc.size)
            n_en = int(en.sum())
            if n_en < drawN:
                continue
            sd = [first]
            for _q in range(1, drawN):
                pick = int(R.select_enabled(pc, [rnd(n_en)])[0])
                if pick == first:
                    pick = int(R.select_enabled(pc, [rnd(n_en)])[0])
                sd.append(pick)
            if len(set(sd)) != drawN:
                continue
            idx = np.asarray(sd) - 1
            R.forcefitshapes(pc.vertices[idx], pc.normals[idx], params, candidates, levels, 1, pc)
        cc[1] += len(candidates)
        R.scorecandidates(pc, ic, candidates, 1, params, levels)
        cc[2] = k * minsubsetN
        cc[0] = len(ic)
        if len(ic) > 0:
            best = R.findhighestscore(ic)["index"]
            scr = R.E(ic.scores[best - 1])
            if R.prob(scr, cc[which[str(it["extract_s"]).lstrip(":")]], pc.size, drawN) > prob_det:
                ex = R.refit(ic.shapes[best - 1], pc, params)
                R.invalidate_indexes(pc, ex.inpoints)
                en = pc.isenabled
                extracted.append(ex)
                R.deleteat(ic, best)
                R.removeinvalidshapes(pc, ic)
        iterations = k
        if R.prob(tau, cc[which[str(it["terminate_s"]).lstrip(":")]], pc.size, drawN) > prob_det:
            break
    return extracted, iterations, rng.draws


@pytest.mark.parametrize("batched", [False, True])
def test_reference_loop_with_three_call_sites_swapped(batched):
    """Drop-in at the call sites INTEGRATION.md names: the reference's loop on the host with
    scorecandidates! / refit / invalidate_indexes! (and the enabled select, or the batched samplepointcloud4! of
    rh_sample_sets) served by the library gives exactly the oracle's run -- shapes, index sets, iteration count, RNG draws."""
    xyz, nrm, truth = synth.make_cloud(9_000, ["plane", "sphere", "cylinder"], 0.1, seed=31)
    subs = synth.make_subsets(9_000, 2, seed=31)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder],
                                iteration={"minsubsetN": 12, "itermax": 25, "τ": 200, "prob_det": 0.7})
    pc = R.RANSACCloud(xyz, nrm, subs)
    got, iters, draws = _ransac_via_call_sites(pc, params, seed=5, batched=batched)
    oc = orc.Cloud(xyz, nrm, subs[0])
    exp = oc.ransac(to_orc_params(R.params_to_c(params)), seed=5)
    assert exp["rc"] == 0 and len(exp["shapes"]) >= 2
    assert iters == exp["iterations"] and draws == exp["draws"]
    assert len(got) == len(exp["shapes"])
    for g, e in zip(got, exp["shapes"]):
        assert bytes(g.shape.to_c()) == bytes(e["shape"])
        assert np.array_equal(g.inpoints, e["inpoints"])
    assert np.array_equal(pc.enabled_chunks(), oc.get_enabled())


@pytest.mark.parametrize("drawN,frac,inject", [(3, 1.0, False), (3, 0.4, True), (4, 0.02, False), (2, 0.5, True), (5, 0.0005, False), (3, 0.0005, False)])
def test_sample_sets_equals_sequential_calls(small_scene, drawN, frac, inject):
    """rh_sample_sets = samplepointcloud4! k times in a row (fitting.jl:383-430) as one launch: the same sets, the same
    accept / reject flags and the same number of draws as the per-point calls (rh_rng_range + rh_select_enabled) on the same
    generator -- with few enabled points (long rejection runs for the first point, redraws, duplicate sets), fewer enabled
    points than drawN, and an injected stream that runs out half way (the generator takes over, as in rh_rng_range)."""
    pc, oc, truth = small_scene
    lib = R.lib()
    n = pc.size
    rs = np.random.default_rng(int(1000 * frac) + drawN)
    en = rs.random(n) < frac
    if frac < 0.001:
        en[:] = False
        en[rs.choice(n, size=3, replace=False)] = True      # fewer enabled points than drawN = 5: every call fails after its first point
    pc.set_enabled(en)
    k = 300
    stream = rs.integers(0, 2**64, size=400, dtype=np.uint64) if inject else None

    def make_rng():
        r = L.Rng()
        lib.rh_rng_seed(C.byref(r), 99)
        if stream is not None:
            r.stream = stream.ctypes.data_as(C.POINTER(C.c_uint64))
            r.stream_len = stream.size
        return r
    rng_a, rng_b = make_rng(), make_rng()
    sets, ok, lev = R.sample_sets(pc, drawN, rng_a, k)
    n_en = int(en.sum())
    n_same = 0
    for j in range(k):
        first = lib.rh_rng_range(C.byref(rng_b), n)
        while not en[first - 1]:
            first = lib.rh_rng_range(C.byref(rng_b), n)
        if n_en < drawN:
            assert not ok[j] and lev[j] == 0
            continue
        sd = [first]
        for _q in range(1, drawN):
            pick = int(R.select_enabled(pc, [lib.rh_rng_range(C.byref(rng_b), n_en)])[0])
            if pick == first:
                pick = int(R.select_enabled(pc, [lib.rh_rng_range(C.byref(rng_b), n_en)])[0])
            sd.append(pick)
        assert list(sets[j]) == sd, j
        # (level 0 with ok = 0 also for a set that is not all different, where the reference's second return value is 1,
        # fitting.jl:427: the deviation ransac_hip.h states)
        assert bool(ok[j]) == (len(set(sd)) == drawN) and lev[j] == int(ok[j])
        n_same += not ok[j]
    assert rng_a.draws == rng_b.draws and rng_a.stream_pos == rng_b.stream_pos
    assert [rng_a.s[i] for i in range(4)] == [rng_b.s[i] for i in range(4)]
    if frac >= 0.02:
        assert ok.sum() > 250
    if n_en == drawN:     # three enabled points, sets of three: most sets repeat a point -- the case the deviation is about occurs
        assert n_same >= 50 and ok.sum() >= 20
    pc.enable_all()


def test_reference_loop_with_call_sites_swapped_at_cfg3_scale(score_path, monkeypatch):
    """The drop-in a RANSAC.jl maintainer would try first, at BASELINE configs[2] scale (tools/callsite_loop.py): the reference's
    own loop on the host with scorecandidates! / refit / invalidate_indexes! served by the library and every iteration's 4096
    minimal sets drawn by ONE rh_sample_sets launch and fitted by ONE rh_fit_sets call.  (With a select round trip per point
    -- round 4 -- this loop ran at 1.6 shapes/s.)  All 40 primitives come out; the throughput is printed and held above a floor
    that leaves room for a slow box."""
    if score_path != "groups":
        pytest.skip("one pass is enough for a throughput figure")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import callsite_loop
    monkeypatch.setenv("MINSUBSET", "4096")
    monkeypatch.setenv("ITERMAX", "300")
    st = callsite_loop.main(quiet=True)
    sys.stderr.write("\n[call-site loop, cfg3 scale] %d shapes in %.3f s = %.1f shapes/s (sampling %.3f, fits %.3f, scoring %.3f, extractions %.3f s)\n"
                     % (st["shapes"], st["seconds"], st["shapes"] / st["seconds"], st["sample_s"], st["fit_s"], st["score_s"], st["extract_s"]))
    assert st["shapes"] == 40 and st["inliers"] > 6_500_000
    assert st["shapes"] / st["seconds"] > 40.0
