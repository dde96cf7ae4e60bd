"""Point normals for clouds without them (rh_estimate_normals) on the GPU, held to the numpy reference of
tests/test_normals_host.py: flags exactly, normals and curvature within the eigen solver's tolerance, Float32, run-to-run
bits, orientation, analytic surfaces, ransac() on estimated normals, errors and the 10M-point scene."""
import ctypes as C
import time

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
from test_normals_host import ref_neighbours, ref_normals

pytestmark = pytest.mark.gpu


def _datasets():
    rng = np.random.default_rng(11)
    out = {"uniform": rng.uniform(0, 10, size=(3000, 3)),
           "lattice": rng.integers(0, 8, size=(2000, 3)).astype(np.float64)}   # 512 sites: duplicates and ties
    out["plane"] = synth.plane_patch(3000, rng, size=20.0)[0]
    out["sphere"] = synth.sphere(3000, rng, radius=8.0)[0]
    out["cylinder"] = synth.cylinder(3000, rng)[0]
    return out


DATA = _datasets()
_NB = {}


def _nb(name):
    if name not in _NB:
        _NB[name] = ref_neighbours(DATA[name], 64)
    return _NB[name]


def _close(got, exp, gap):
    """Where (l1 - l0) / l2 >= 1e-6: within 1e-9 per component, and the same signs (components clear of 0).  With the
    canonical sign (orient = 0), a normal whose two largest magnitudes are within 1e-9 (45-degree normals of the lattice) has its
    sign decided by the last bits of two eigen solvers: there it is compared up to sign."""
    ok = gap >= 1e-6
    g, e = got[ok], exp[ok]
    d = np.abs(g - e)
    top = np.sort(np.abs(e), axis=1)
    tie = top[:, 2] - top[:, 1] < 1e-9
    d[tie] = np.minimum(d[tie], np.abs(g[tie] + e[tie]))
    g, e, d = g[~tie], e[~tie], np.concatenate([d[~tie], d[tie]])
    assert d.max(initial=0.0) <= 1e-9, d.max()
    sig = np.abs(e) > 1e-6
    assert np.array_equal(np.sign(g[sig]), np.sign(e[sig]))


@pytest.mark.parametrize("name", sorted(DATA))
@pytest.mark.parametrize("k", [3, 8, 16, 64])
@pytest.mark.parametrize("with_radius", [False, True])
def test_against_the_reference(name, k, with_radius):
    xyz = DATA[name]
    nb = _nb(name)
    radius = float(np.sqrt(np.median(nb[1][:, k - 1]))) if with_radius else 0.0
    nrm, curv, flags = R.estimatenormals(xyz, k=k, radius=radius, return_curvature=True, return_flags=True)
    en, ec, ef, gap = ref_normals(xyz, k, radius=radius, nb=nb)
    assert np.array_equal(flags, ef), np.flatnonzero(flags != ef)[:10]
    assert not np.isnan(nrm).any() and not np.isnan(curv).any()
    assert np.array_equal(nrm[ef == 1], np.zeros(((ef == 1).sum(), 3))) and not curv[ef == 1].any()
    ok = gap >= 1e-6
    assert name == "lattice" or ok.mean() > 0.4      # (k = 3 with a radius: about half keep fewer than 3)
    _close(nrm, en, gap)
    assert np.abs(curv[ok] - ec[ok]).max(initial=0.0) <= 1e-12


def test_float32_is_the_double_result_rounded():
    for name in ("uniform", "sphere", "cylinder"):
        x32 = DATA[name].astype(np.float32)
        n32, c32, f32 = R.estimatenormals(x32, k=16, return_curvature=True, return_flags=True)
        assert n32.dtype == np.float32 and c32.dtype == np.float32
        n64, c64, f64 = R.estimatenormals(x32.astype(np.float64), k=16, return_curvature=True, return_flags=True)
        assert np.array_equal(f32, f64)
        r = n64.astype(np.float32)
        assert (np.abs(n32 - r) <= np.spacing(np.abs(r))).all()
        _, _, _, gap = ref_normals(x32.astype(np.float64), 16)
        ok = gap >= 1e-6
        assert np.abs(n64[ok] - ref_normals(x32.astype(np.float64), 16)[0][ok]).max() <= 1e-9


def test_determinism_and_orientation():
    xyz = DATA["sphere"]
    a = R.estimatenormals(xyz, k=16)
    b = R.estimatenormals(xyz, k=16)
    assert a.tobytes() == b.tobytes()
    v = np.array([-30.0, 50.0, 20.0])
    nv, fv = R.estimatenormals(xyz, k=16, viewpoint=v, return_flags=True)
    assert ((nv * (v - xyz)).sum(axis=1)[fv == 0] >= 0).all()
    rng = np.random.default_rng(3)
    h = rng.normal(size=xyz.shape)
    nh, fh = R.estimatenormals(xyz, k=16, hints=h, return_flags=True)
    assert ((nh * h).sum(axis=1)[fh == 0] >= 0).all()
    en = ref_normals(xyz, 16, hints=h, nb=_nb("sphere"))
    ok = en[3] >= 1e-6
    assert np.abs(nh[ok] - en[0][ok]).max() <= 1e-9
    ev = ref_normals(xyz, 16, viewpoint=v, nb=_nb("sphere"))
    assert np.abs(nv[ok] - ev[0][ok]).max() <= 1e-9


def _angle_ok(nrm, truth):
    c = np.abs((nrm * truth).sum(axis=1))
    return np.mean(c >= np.cos(np.radians(1.0)))


def test_analytic_surfaces():
    rng = np.random.default_rng(5)
    n = 1_000_000
    # plane z = 3 in a 100 x 100 square, tilted
    uv = rng.uniform(-50, 50, size=(n, 2))
    a, b = np.array([1.0, 0.0, 0.3]) / np.linalg.norm([1.0, 0.0, 0.3]), np.array([0.0, 1.0, 0.0])
    nz = np.cross(a, b)
    p = uv[:, :1] * a + uv[:, 1:] * b + 3.0
    inner = (np.abs(uv) < 48).all(axis=1)
    assert _angle_ok(R.estimatenormals(p, k=16)[inner], nz) >= 0.999
    # sphere, radius 10
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    s = 10.0 * d + [50.0, 40.0, 30.0]
    assert _angle_ok(R.estimatenormals(s, k=16), d) >= 0.999
    # cylinder, radius 5, axis z, height 60 (the ends are borders)
    th = rng.uniform(0, 2 * np.pi, n)
    z = rng.uniform(0, 60, n)
    radial = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
    cy = 5.0 * radial + np.stack([np.zeros(n), np.zeros(n), z], axis=1)
    inner = (z > 2) & (z < 58)
    assert _angle_ok(R.estimatenormals(cy, k=16)[inner], radial[inner]) >= 0.999


def test_ransac_on_estimated_normals_finds_every_primitive():
    xyz, nrm, truth = synth.make_cloud(200_000, ["plane", "sphere", "cylinder", "cone"], 0.1, seed=9)
    est, flags = R.estimatenormals(xyz, k=16, hints=nrm, return_flags=True)
    assert flags.mean() < 1e-3
    subs = synth.make_subsets(200_000, 8, seed=9)
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone],
                                iteration={"minsubsetN": 200, "itermax": 200, "τ": 2000, "prob_det": 0.9})
    cp = R.params_to_c(params, score_mode=L.SCORE_F64)
    kinds = {"plane": L.PLANE, "sphere": L.SPHERE, "cylinder": L.CYLINDER, "cone": L.CONE}

    def found(normals):
        pc = R.RANSACCloud(xyz, normals, subs)
        got, _ = R.ransac(pc, cp, seed=1234)
        res = set()
        for ti, t in enumerate(truth):
            # found: an extracted shape of the primitive's kind whose inpoints lie on it (median distance < 0.05)
            for g in got:
                if g.c_shape.kind == kinds[t["kind"]] and _covers(g, t, xyz):
                    res.add(ti)
        return res, got

    f_est, got_est = found(est)
    f_gen, got_gen = found(nrm)
    assert f_est == set(range(len(truth))), ([R.strt(g.shape) for g in got_est], f_est)
    assert f_gen == f_est, ([R.strt(g.shape) for g in got_gen], f_gen)


def _dist(t, p):
    if t["kind"] == "plane":
        return np.abs((p - t["point"]) @ t["normal"])
    if t["kind"] == "sphere":
        return np.abs(np.linalg.norm(p - t["center"], axis=1) - t["radius"])
    if t["kind"] == "cylinder":
        v = p - t["center"]
        return np.abs(np.linalg.norm(v - np.outer(v @ t["axis"], t["axis"]), axis=1) - t["radius"])
    v = p - t["apex"]
    ax = v @ t["axis"]
    rad = np.linalg.norm(v - np.outer(ax, t["axis"]), axis=1)
    h = t["opang"] / 2
    return np.abs(rad * np.cos(h) - ax * np.sin(h))


def _covers(g, t, xyz):
    pts = xyz[np.asarray(g.inpoints) - 1]
    return len(pts) > 1000 and np.median(_dist(t, pts)) < 0.05


def test_errors_and_degenerate_inputs():
    xyz = DATA["uniform"][:100].copy()
    for kw in (dict(k=2), dict(k=65), dict(radius=-0.5)):
        with pytest.raises(R.RansacHipError):
            R.estimatenormals(xyz, **kw)
    p = L.NormalsParams(k=8, orient=2)
    out = np.zeros((100, 3))
    assert R.lib().rh_estimate_normals(xyz.ctypes.data_as(C.POINTER(C.c_double)), 100, C.byref(p), None, 0,
                                       out.ctypes.data_as(C.POINTER(C.c_double)), None, None) == L.RH_E_INVALID
    bad = xyz.copy()
    bad[37, 1] = np.nan
    with pytest.raises(R.RansacHipError) as e:
        R.estimatenormals(bad)
    assert e.value.code == L.RH_E_INVALID
    for n in (1, 2):
        nrm, curv, flags = R.estimatenormals(xyz[:n], k=16, return_curvature=True, return_flags=True)
        assert not nrm.any() and not curv.any() and (flags == 1).all()
    # isolated points far from a dense cluster end, and end exact
    rng = np.random.default_rng(2)
    far = np.concatenate([rng.normal(size=(5000, 3)) * 0.1, [[1e3, 0, 0], [0, -2e3, 5e2], [1e3, 1.0, 0.5]]])
    nrm, flags = R.estimatenormals(far, k=8, return_flags=True)
    en, _, ef, gap = ref_normals(far, 8)
    assert np.array_equal(flags, ef)
    ok = gap >= 1e-6
    assert np.abs(nrm[ok] - en[ok]).max() <= 1e-9


def test_cfg3_full_size():
    c = synth.config("cfg3")
    xyz = c["xyz"]
    R.estimatenormals(xyz[:100_000], k=16)            # warm-up: code objects, allocator
    t0 = time.perf_counter()
    nrm, flags = R.estimatenormals(xyz, k=16, return_flags=True)
    secs = time.perf_counter() - t0
    assert secs < 2.0, secs
    near = np.zeros(len(xyz), dtype=bool)
    for t in c["truth"]:
        near |= _dist(t, xyz) < 0.1
    assert near.sum() > 5_000_000
    assert flags[near].mean() < 1e-3
    assert not np.isnan(nrm).any()
