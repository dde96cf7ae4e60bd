"""rh_shape_extents / rh_result_extents on the device against the numpy twin of tests/test_extents_host.py.
Steps 4 to 6 of the header's definition are exact given the frame, so lo, hi and dist_maxabs are compared bit for bit with
numpy's recomputation from the returned origin and frame; what goes through sums or the eigen-solver (frame, centroid,
lambda, dist_rms) is compared with the twin's own value within the stated tolerance, on inputs with a clear direction."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from test_extents_host import (EXT_EMPTY, EXT_NO_DIRECTION, box_and_distance, cone_frustum, cylinder_part, fallback_u,
                               rectangle, ref_extents, sphere_patch)

pytestmark = pytest.mark.gpu

KINDS = (L.PLANE, L.SPHERE, L.CYLINDER, L.CONE)
LENGTHS = [1, 2, 63, 64, 65] + [(1 << k) + d for k in range(7, 14) for d in (-1, 0, 1)]
PER_KIND = 1000
NOISE = 0.02


def _noisy(p, rng):
    return p + rng.normal(0, NOISE, size=p.shape)


def _scene():
    """4 x 1000 points, one primitive of every kind, a little noise so that distances are not all zero; every primitive
    has a clear principal direction (rectangle 2 : 1, elongated sphere patch, half cylinder, half cone)"""
    rng = np.random.default_rng(11)
    parts = {L.PLANE: rectangle(PER_KIND, rng), L.SPHERE: sphere_patch(PER_KIND, rng, lon=(-1.0, 1.0), lat=(-0.3, 0.4)),
             L.CYLINDER: cylinder_part(PER_KIND, rng, arc=(0.0, np.pi)), L.CONE: cone_frustum(PER_KIND, rng, arc=(0.0, np.pi))}
    xyz = np.ascontiguousarray(np.concatenate([_noisy(parts[k][0], rng) for k in KINDS]))
    nrm = rng.normal(size=xyz.shape)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    shapes = {k: parts[k][1] for k in KINDS}
    pool = {k: np.arange(i * PER_KIND, (i + 1) * PER_KIND, dtype=np.int64) + 1 for i, k in enumerate(KINDS)}
    return xyz, nrm, shapes, pool


XYZ, NRM, SHAPES, POOL = _scene()
_CLOUDS = {}


def cloud(f32=False):
    if f32 not in _CLOUDS:
        subs = synth.make_subsets(len(XYZ), 2, seed=1)
        _CLOUDS[f32] = R.RANSACCloud(XYZ, NRM, subs, force_eltype=np.float32) if f32 else R.RANSACCloud(XYZ, NRM, subs)
    return _CLOUDS[f32]


def _draw(kind, n, rng):
    pool = POOL[kind]
    return rng.choice(pool, size=n, replace=n > len(pool))


def _bytes(e):
    return bytes(e.c)


def check_exact(xyz, shape, idx, e):
    """what is exact whatever the list: n, flags, w, orthonormality, and steps 4 + 5 from the returned origin and frame"""
    ref = ref_extents(xyz, shape, idx, frame=e.frame)
    own = ref_extents(xyz, shape, idx)
    assert e.n == len(idx) and e.kind == shape.kind
    assert e.flags == own["flags"], (e.flags, own["flags"], len(idx))
    assert np.array_equal(e.origin, ref["origin"])
    assert e.lo.tobytes() == ref["lo"].tobytes() and e.hi.tobytes() == ref["hi"].tobytes(), (len(idx), e.lo, ref["lo"], e.hi, ref["hi"])
    assert e.dist_maxabs == ref["dist_maxabs"], (len(idx), e.dist_maxabs, ref["dist_maxabs"])
    # against the twin's OWN frame the distance is the same number up to rounding: a plane's e = tw does not involve u, v
    # at all; the others' sqrt(tu^2 + tv^2 (+ tw^2)) is the length of the same vector in another orthonormal basis --
    # a few ulp of |d|, bounded here by 1e-12 (|d| + r)
    d = np.abs(xyz[np.asarray(idx) - 1] - e.origin).sum(axis=1).max() + abs(shape.v[3]) + abs(shape.v[6])
    if shape.kind == L.PLANE:
        assert e.dist_maxabs == own["dist_maxabs"]
    else:
        assert abs(e.dist_maxabs - own["dist_maxabs"]) <= 1e-12 * d
    assert abs(e.dist_rms - ref["dist_rms"]) <= 1e-12 * max(ref["dist_rms"], 1e-300)
    if shape.kind != L.SPHERE:
        assert e.frame[2].tobytes() == own["frame"][2].tobytes()
    assert np.abs(e.frame @ e.frame.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(e.frame) - 1.0) <= 1e-12
    return own


@pytest.mark.parametrize("kind", KINDS)
def test_exact_part_at_every_boundary(kind):
    """lists of every length around the wave, block and chunk sizes, all in one call"""
    rng = np.random.default_rng(100 + kind)
    pc = cloud()
    lists = [_draw(kind, n, rng) for n in LENGTHS]
    got = R.shape_extents(pc, [(SHAPES[kind], i) for i in lists])
    assert len(got) == len(LENGTHS)
    for idx, e in zip(lists, got):
        check_exact(XYZ, SHAPES[kind], idx, e)
    assert got[0].flags == EXT_NO_DIRECTION and all(e.flags == 0 for e in got[1:])


def test_frame_and_sums_against_the_twin():
    rng = np.random.default_rng(7)
    pc = cloud()
    cases = [(k, _draw(k, n, rng)) for k in KINDS for n in (700, 1000, 3000)]
    got = R.shape_extents(pc, [(SHAPES[k], i) for k, i in cases])
    for (k, idx), e in zip(cases, got):
        own = check_exact(XYZ, SHAPES[k], idx, e)
        lam = own["lam"]
        assert (lam[0] - lam[1]) / lam[0] >= 1e-3, (k, lam)
        if k == L.SPHERE:
            assert (lam[1] - lam[2]) / lam[0] >= 1e-3, lam      # v is an eigenvector of its own there
        assert np.abs(e.frame[:2] - own["frame"][:2]).max() <= 1e-9, (k, e.frame, own["frame"])
        assert np.allclose(e.centroid, own["centroid"], rtol=1e-12, atol=0)
        assert np.allclose(e.lam, own["lam"], rtol=1e-12, atol=0), (k, e.lam, own["lam"])
        assert np.isclose(e.dist_rms, own["dist_rms"], rtol=1e-12, atol=0)


def test_segments_are_independent_and_runs_repeat():
    rng = np.random.default_rng(8)
    pc = cloud()
    shared = np.concatenate([POOL[L.PLANE][:300], POOL[L.CYLINDER][:300]])
    dup = np.concatenate([_draw(L.SPHERE, 1500, rng), POOL[L.SPHERE][:40], POOL[L.SPHERE][:40]])[rng.permutation(1580)]
    items = [(SHAPES[L.CONE], np.zeros(0, dtype=np.int64)), (SHAPES[L.PLANE], shared[rng.permutation(600)]),
             (SHAPES[L.SPHERE], dup), (SHAPES[L.CYLINDER], np.zeros(0, dtype=np.int64)), (SHAPES[L.CYLINDER], shared),
             (SHAPES[L.CONE], _draw(L.CONE, 2500, rng)), (SHAPES[L.PLANE], np.zeros(0, dtype=np.int64))]
    assert len(items) == 7
    got = R.shape_extents(pc, items)
    again = R.shape_extents(pc, items)
    for (shape, idx), e, e2 in zip(items, got, again):
        alone = R.shape_extents(pc, [(shape, idx)])[0]
        assert _bytes(e) == _bytes(alone) == _bytes(e2)
        if len(idx) == 0:
            z = L.Extent(kind=shape.kind, flags=EXT_EMPTY)
            z.origin[:] = list(ref_extents(XYZ, shape, idx)["origin"])
            assert _bytes(e) == bytes(z)
        else:
            check_exact(XYZ, shape, idx, e)
    assert R.shape_extents(pc, []) == []


def test_fallback_frame():
    pc = cloud()
    for kind in KINDS:
        k = int(POOL[kind][17])
        for idx in (np.array([k]), np.full(500, k)):
            e = R.shape_extents(pc, [(SHAPES[kind], idx)])[0]
            own = check_exact(XYZ, SHAPES[kind], idx, e)
            assert e.flags == EXT_NO_DIRECTION and np.array_equal(e.lo, e.hi) and np.array_equal(e.centroid, XYZ[k - 1])
            if kind == L.SPHERE:
                assert np.array_equal(e.frame, np.eye(3))
            else:
                # e_k - w (w . e_k), normalised: three roundings of numbers of magnitude <= 1
                assert np.abs(e.frame[0] - fallback_u(e.frame[2])).max() <= 1e-15
                assert np.abs(e.frame - own["frame"]).max() <= 1e-15


def test_float32_cloud_is_the_float64_cloud_of_the_widened_points():
    rng = np.random.default_rng(9)
    wide = np.ascontiguousarray(XYZ.astype(np.float32).astype(np.float64))
    pc64 = R.RANSACCloud(wide, NRM, synth.make_subsets(len(XYZ), 2, seed=1))
    items = [(SHAPES[k], _draw(k, n, rng)) for k in KINDS for n in (1, 1025)]
    a, b = R.shape_extents(cloud(f32=True), items), R.shape_extents(pc64, items)
    assert [_bytes(x) for x in a] == [_bytes(y) for y in b]
    for (shape, idx), e in zip(items, a):
        check_exact(wide, shape, idx, e)


def _raw(pc, shapes, offsets, idx):
    arr = (L.Shape * len(shapes))(*shapes)
    off, ix = np.asarray(offsets, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    out = (L.Extent * len(shapes))()
    return R.lib().rh_shape_extents(pc._h, arr, len(shapes), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                    ix.ctypes.data_as(C.POINTER(C.c_int64)), out), out


def test_errors_leave_the_cloud_usable_and_untouched():
    pc = cloud()
    n = len(XYZ)
    good = POOL[L.PLANE][:100]
    plane, cyl = SHAPES[L.PLANE], SHAPES[L.CYLINDER]
    before = pc.enabled_chunks().copy()
    want = _bytes(R.shape_extents(pc, [(plane, good)])[0])

    def still_fine():
        assert _bytes(R.shape_extents(pc, [(plane, good)])[0]) == want
        assert np.array_equal(pc.enabled_chunks(), before)

    for bad in (0, n + 1, -5, -(1 << 63), (1 << 62)):
        for pos in (0, 57, 99):       # the first entry is the moments' shift: a path of its own
            idx = good.copy()
            idx[pos] = bad
            with pytest.raises(R.RansacHipError) as e:
                R.shape_extents(pc, [(cyl, POOL[L.CYLINDER][:1500]), (plane, idx)])
            assert e.value.code == L.RH_E_INVALID
            still_fine()
    for offsets in ([1, 100], [0, 60, 40, 100]):
        rc, _ = _raw(pc, [plane] * (len(offsets) - 1), offsets, good)
        assert rc == L.RH_E_INVALID
        still_fine()
    for zero in (R.FittedPlane([1, 2, 3], [0, 0, 0]).to_c(), R.FittedCylinder([0, 0, 0], [1, 2, 3], 2.0, True).to_c(),
                 R.FittedCone([1, 2, 3], [0.0, np.inf, 0], 0.5, True).to_c()):
        with pytest.raises(R.RansacHipError) as e:
            R.shape_extents(pc, [(plane, good), (zero, good)])
        assert e.value.code == L.RH_E_INVALID
        still_fine()
    assert _raw(pc, [], [0], [1])[0] == L.RH_OK
    # a listed point with a NaN coordinate; the same cloud serves lists that leave it out
    xyz = XYZ[:500].copy()
    xyz[123, 1] = np.nan
    pcn = R.RANSACCloud(xyz, NRM[:500], synth.make_subsets(500, 2, seed=1))
    idx = np.arange(100, 200, dtype=np.int64)
    for lst in (idx, np.concatenate([[124], idx[:50]])):
        with pytest.raises(R.RansacHipError) as e:
            R.shape_extents(pcn, [(plane, lst)])
        assert e.value.code == L.RH_E_INVALID
    ok = idx[idx != 124]
    check_exact(xyz, plane, ok, R.shape_extents(pcn, [(plane, ok)])[0])


def test_device_entry_checks_what_the_host_cannot_see():
    """rh_shape_extents_dev: everything resident; the offsets are checked by the kernels, which mark every record"""
    pc = cloud()
    rng = np.random.default_rng(10)
    items = [(SHAPES[L.PLANE], _draw(L.PLANE, 1500, rng)), (SHAPES[L.CONE], _draw(L.CONE, 700, rng))]
    want = [_bytes(e) for e in R.shape_extents(pc, items)]
    lib = R.lib()
    arr = (L.Shape * 2)(*[s for s, _ in items])
    idx = np.concatenate([i for _, i in items])

    def run(offsets):
        off = np.asarray(offsets, dtype=np.int64)
        out = (L.Extent * 2)()
        bufs = []
        for src, nbytes in ((arr, C.sizeof(arr)), (off.ctypes.data_as(C.c_void_p), off.nbytes), (idx.ctypes.data_as(C.c_void_p), idx.nbytes),
                            (None, C.sizeof(out))):
            d = C.c_void_p()
            L.check(lib.rh_dev_alloc(pc._h, nbytes, C.byref(d)))
            if src is not None:
                L.check(lib.rh_dev_upload(pc._h, d, C.cast(src, C.c_void_p), nbytes))
            bufs.append(d)
        L.check(lib.rh_shape_extents_dev(pc._h, bufs[0], 2, bufs[1], bufs[2], idx.size, bufs[3]))
        L.check(lib.rh_dev_download(pc._h, C.cast(out, C.c_void_p), bufs[3], C.sizeof(out)))
        for d in bufs:
            L.check(lib.rh_dev_free(pc._h, d))
        return out

    assert [bytes(e) for e in run([0, 1500, 2200])] == want
    for offsets in ([0, 1600, 1500], [3, 1500, 2200], [0, 1500, 2100], [-7, 1 << 40, 2200]):
        assert all(e.flags & L.EXT_INVALID for e in run(offsets)), offsets
    assert [bytes(e) for e in run([0, 1500, 2200])] == want


def _generator_truth(n_total, kinds, outlier_frac, seed):
    """synth.make_cloud's primitives with the generator's private sizes (the public truth leaves them out): the same draws"""
    rng = np.random.default_rng(seed)
    m = (n_total - int(round(n_total * outlier_frac))) // len(kinds)
    out = []
    for kind in kinds:
        t = synth._PARAMS[kind](rng)
        synth._POINTS[kind](t, m, rng)
        out.append(t)
    return out


def _dist(t, p):
    if t["kind"] == "plane":
        return np.abs((p - t["point"]) @ t["normal"])
    if t["kind"] == "sphere":
        return np.abs(np.linalg.norm(p - t["center"], axis=1) - t["radius"])
    v = p - (t["center"] if t["kind"] == "cylinder" else t["apex"])
    ax = v @ t["axis"]
    rad = np.linalg.norm(v - np.outer(ax, t["axis"]), axis=1)
    if t["kind"] == "cylinder":
        return np.abs(rad - t["radius"])
    return np.abs(rad * np.cos(t["opang"] / 2) - ax * np.sin(t["opang"] / 2))


def _covers(g, t, xyz):
    """an extracted shape whose inpoints lie on the truth primitive (median distance < 0.05), as test_normals_gpu.py has it"""
    pts = xyz[np.asarray(g.inpoints) - 1]
    return len(pts) > 1000 and np.median(_dist(t, pts)) < 0.05


def test_through_ransac():
    kinds = ["plane", "sphere", "cylinder", "cone"]
    xyz, nrm, truth = synth.make_cloud(200_000, kinds, 0.1, seed=9)
    gen = _generator_truth(200_000, kinds, 0.1, 9)
    for t, g in zip(truth, gen):
        assert all(np.array_equal(t[k], g[k]) for k in t if k != "n_points")
    subs = synth.make_subsets(200_000, 8, seed=9)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone],
                                iteration={"minsubsetN": 200, "itermax": 200, "τ": 2000, "prob_det": 0.9})
    cp = R.params_to_c(params, score_mode=L.SCORE_F64)
    pc = R.RANSACCloud(xyz, nrm, subs)
    plain, _ = R.ransac(pc, cp, seed=1234)
    pc.enable_all()
    got, _ = R.ransac(pc, cp, seed=1234, extents=True)
    assert len(got) == len(plain) >= 4
    for a, b in zip(plain, got):
        assert bytes(a.c_shape) == bytes(b.c_shape) and np.array_equal(a.inpoints, b.inpoints) and not hasattr(a, "extent")
    for es in got:
        assert _bytes(es.extent) == _bytes(R.shape_extents(pc, [es])[0])
        check_exact(xyz, es.c_shape, es.inpoints, es.extent)
    code = {"plane": L.PLANE, "sphere": L.SPHERE, "cylinder": L.CYLINDER, "cone": L.CONE}
    for t, g in zip(truth, gen):
        mine = [es for es in got if es.c_shape.kind == code[t["kind"]] and _covers(es, t, xyz)]
        assert len(mine) == 1, (t["kind"], len(mine))
        e = mine[0].extent
        size = e.hi - e.lo
        if t["kind"] == "plane":
            # the generator's patch is a SQUARE: no principal direction, so its box is the square's only up to the in-plane
            # rotation (side .. side * sqrt 2); the rotation-free measure of a uniform rectangle's sides is sqrt(12 lambda)
            assert np.allclose(np.sqrt(12 * e.lam[:2]), g["_size"], rtol=0.05), (e.lam, g["_size"])
            assert (size[:2] >= 0.95 * g["_size"]).all() and (size[:2] <= 1.05 * np.sqrt(2) * g["_size"]).all()
        elif t["kind"] == "sphere":
            assert np.allclose(size, 2 * t["radius"], rtol=0.05), (size, t["radius"])
        elif t["kind"] == "cylinder":
            assert np.isclose(size[2], g["_h"], rtol=0.05), (size, g["_h"])
        else:
            assert np.isclose(size[2], (g["_h1"] - g["_h0"]) * np.cos(t["opang"] / 2), rtol=0.05), (size, g["_h0"], g["_h1"])
        assert 0 < e.dist_rms <= e.dist_maxabs <= 0.3      # every inpoint lies within the shape's eps (0.3, the default)


def test_one_run_at_cfg2():
    c = synth.config("cfg2")
    xyz = c["xyz"]
    pc = R.RANSACCloud(xyz, c["nrm"], synth.make_subsets(len(xyz), c["r"], c["seed"]))
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    rp = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 200, "τ": 900, "prob_det": 0.9})
    cp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    got, _ = R.ransac(pc, cp, seed=1234, extents=True)
    assert len(got) >= 6 and sum(es.inpoints.size for es in got) > 900_000
    again = R.shape_extents(pc, got)            # all shapes in one call through the other host entry
    for es, e in zip(got, again):
        assert _bytes(e) == _bytes(es.extent)
        check_exact(xyz, es.c_shape, es.inpoints, e)
