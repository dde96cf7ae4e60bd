"""The least-squares refit's specification twin (orc_refit_lsq) against tests/lsq_reference.py, on the CPU: one
Gauss-Newton step, the rms, the count and the gradient of the converged result, on the cases that tests/test_lsq_gpu.py
runs on the device.  The constants of the one-step bound are measured here, on the oracle, and never on the GPU.

The one-step bound, u = 2^-53:

    |p_out - p_ref|_inf <= c n_sel u kappa |x_ref|_inf + 8 u |p|_inf

(first-order perturbation of normal equations whose entries are sums of n_sel products; kappa = the condition number of
the diagonally scaled matrix; the last term is the rounding of the output fields themselves).  For a plane, x_ref is
the change of (point, normal) and kappa = lambda_max / (lambda_mid - lambda_min) of the centred scatter.

Measured on the oracle (sequential sums, the worst order), c = 1:

    case kind      n_sel   kappa   |x|_inf  bound      bound/|x|  error     error/bound  rms rel.err  iters  |J'r|/(|J||r|)
    S    plane       821    1.19    0.733   1.45e-13   2.0e-13    2.18e-15  0.0150       1.7e-12      -      -
    S    sphere      680    1.19    0.828   1.52e-13   1.8e-13    6.17e-15  0.0406       2.2e-16      5      7.81e-14
    S    cylinder    819    1.24    0.173   8.02e-14   4.6e-13    6.40e-15  0.0798       1.9e-16      4      1.56e-14
    S    cone        521    290     0.498   8.41e-12   1.7e-11    1.75e-14  0.0021       1.8e-16      5      8.86e-14
    S/2  cone        260    278     0.492   4.01e-12   8.2e-12    2.03e-14  0.0051       1.9e-16      -      -
    L    plane     60001    1.00    0.460   3.14e-12   6.8e-12    6.05e-15  0.0019       6.6e-10      -      -
    L    sphere    60000    1.11    0.288   2.15e-12   7.5e-12    7.72e-16  0.0004       5.8e-16      4      1.73e-14
    L    cylinder  60001    1.05    0.162   1.17e-12   7.2e-12    3.06e-15  0.0026       8.0e-16      4      8.42e-15
    L    cone      46670    133     0.497   3.41e-10   6.9e-10    1.71e-13  0.0005       5.1e-15      5      4.29e-14
    L/2  cylinder  30000    1.06    0.162   6.11e-13   3.8e-12    1.30e-15  0.0021       3.4e-15      -      -
    T8   sphere        8    72.3    0.0827  4.98e-14   6.0e-13    4.61e-15  0.0926       7.5e-16      -      -
    F    plane       128    1.30    0.581   7.70e-14   1.3e-13    3.89e-15  0.0505       (rms 0 against 4.4e-15)
    Lmov plane     60001    1.00    0.460   7.23e-06   1.6e-05    4.57e-09  0.0006       5.4e-4 (rms^2: 4.3e-7 of the bound 2.7e-3)

(S/2, L/2: every second selected point disabled; Lmov: the plane's point moved by 100 x the extent, bound x (D / sigma)^2
= 7.6e5.)  The largest ratio is 0.0926 (0.0798 among S and L), not below 1/64: where n_sel is small the bound is mostly
its 8 u |p| term and the error the rounding of coordinates of size 50, one or two units in the last place.  So c stays
the a-priori 1:  C_STEP = 1.  The largest gradient ratio of a converged oracle run is 8.86e-14 (it is what one unit in
the last place of the result's fields leaves): TOL_G = 16 x 8.86e-14 = 1.42e-12.  Every case satisfies bound <= 1e-3
|x_ref|_inf (at most 1.6e-5) and |x_ref|_inf >= 1e-3 of the shape's size; the tests assert both.
"""
import functools

import numpy as np
import pytest

import lsq_reference as ref
from oracle import oracle as orc
from ransac_jl_amd import synth

U = 2.0 ** -53
KINDS = ["plane", "sphere", "cylinder", "cone"]
CASES = {"S": (4097, 21), "L": (300_001, 22)}     # name -> (points, seed of the cloud, the subsets and the jitter)
C_STEP = 1.0
TOL_G = 16 * 8.86e-14
MAX_ITER = 12


@functools.lru_cache(maxsize=None)
def scene(case):
    """-> xyz, nrm, subsets, {kind: (name, outwards, v)}: one primitive of every kind + 20 % outliers, 1 %-jittered
    candidates with the normals pointing outwards as the synthetic primitives' do"""
    n, seed = CASES[case]
    xyz, nrm, truth = synth.make_cloud(n, KINDS, 0.2, seed)
    subs = synth.make_subsets(n, 3, seed)
    cands = {}
    for name, _, v in synth.jittered_candidates(truth, 4, seed=seed):
        cands[name] = (name, name != "plane", np.asarray(v, dtype=np.float64))
    for a in (xyz, nrm):
        a.setflags(write=False)
    return xyz, nrm, subs, cands, truth


@functools.lru_cache(maxsize=None)
def ref_step(case, kind):
    """the reference's step of the case's candidate on the fully enabled cloud: computed once, shared, not modified"""
    xyz, nrm, _, cands, _ = scene(case)
    return ref.one_step(cands[kind], xyz, nrm, None, orc.default_params())


def shape_size(shape, truth=None):
    """the length a step is measured against: the radius; the cone's radius 10 along its axis; the plane's patch 20"""
    name, _, v = shape
    return {"plane": lambda: 20.0, "sphere": lambda: v[3], "cylinder": lambda: v[6],
            "cone": lambda: 10.0 * np.tan(v[6] / 2)}[name]()


def to_orc(shape):
    name, outw, v = shape
    return orc.make_shape(ref.KIND[name], outw, np.asarray(v, dtype=np.float64)[:ref.NPAR[name]])


def from_c(name, cshape, outw):
    return (name, outw, np.array(list(cshape.v), dtype=np.float64)[:ref.NPAR[name]])


def step_error(name, v_out, st):
    return float(np.abs(np.asarray(v_out, dtype=ref.LD)[:ref.NPAR[name]] - st.v).max())


def check_conditions(shape, st, bound):
    """the bound hides no wrong Jacobian entry: it is <= 1e-3 of the step, and the step is >= 1e-3 of the shape's size"""
    xinf = float(np.abs(st.x).max())
    assert xinf >= 1e-3 * shape_size(shape), (shape[0], xinf, shape_size(shape))
    assert bound <= 1e-3 * xinf, (shape[0], bound, xinf)


def check_one_step(shape, got, n_used, rms, st, c=None, scale=1.0):
    """got: the fields of the implementation's shape after one step from `shape`; st: the reference's Step"""
    name = shape[0]
    bound = ref.one_step_bound(C_STEP if c is None else c, st, shape[2], name) * scale
    check_conditions(shape, st, bound)
    err = step_error(name, got, st)
    assert n_used == st.n_sel, (name, n_used, st.n_sel)
    assert err <= bound, (name, err, bound, err / bound)
    return err / bound


def check_rms(rms, st):
    assert abs(rms - float(st.rms)) <= 1e-12 + 1e-9 * float(st.rms), (rms, float(st.rms))


def gradient_ratio(shape_out, xyz, sel):
    g, jr = ref.gradient(shape_out, xyz[sel])
    return g / jr


@pytest.fixture(scope="module")
def oracle_clouds():
    out = {}
    for case in CASES:
        xyz, nrm, subs, _, _ = scene(case)
        out[case] = orc.Cloud(xyz, nrm, subs[0])
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_one_step_equals_reference(oracle_clouds, case, kind):
    xyz, nrm, _, cands, _ = scene(case)
    oc, op = oracle_clouds[case], orc.default_params()
    shape = cands[kind]
    st = ref_step(case, kind)
    out, n, rms, it = oc.refit_lsq(to_orc(shape), op, max_iter=1)
    assert it == 1
    check_one_step(shape, list(out.v), n, rms, st)
    check_rms(rms, st)
    assert n >= 150, (case, kind, n)          # the candidate really sits on its primitive


@pytest.mark.parametrize("kind", KINDS[1:])
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_converged_result_has_zero_gradient(oracle_clouds, case, kind):
    xyz, nrm, _, cands, _ = scene(case)
    oc, op = oracle_clouds[case], orc.default_params()
    shape = cands[kind]
    out, n, rms, it = oc.refit_lsq(to_orc(shape), op, max_iter=MAX_ITER)
    assert it < MAX_ITER
    assert gradient_ratio(from_c(kind, out, True), xyz, ref_step(case, kind).sel) <= TOL_G


# ---- the small cases -------------------------------------------------------------------------------------------------
def tiny_sphere(k):
    """200 points: k on a sphere (radius 10, noise 0.02, outward normals) at scattered indices, the rest far outside the
    3 eps band; the candidate is the sphere moved by ~0.15 and shrunk by 0.05"""
    rng = np.random.default_rng(5)
    n, centre, radius = 200, np.array([50.0, 50.0, 50.0]), 10.0
    xyz = rng.uniform(0.0, 20.0, size=(n, 3))                 # >= 52 from the centre
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    at = np.sort(rng.permutation(n)[:8])[:k]                  # the same places for k = 8 and k = 7
    d = rng.normal(size=(8, 3))[:k]
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz[at] = centre + (radius + rng.normal(0, 0.02, size=(k, 1))) * d
    nrm[at] = d
    shape = ("sphere", True, np.array([50.1, 49.92, 50.07, 9.95]))
    return np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), synth.make_subsets(n, 3, 5), shape


def flat_plane():
    """128 points exactly (to rounding) on a plane in general position, no outliers, exact normals: both 64-point words
    are fully selected.  The candidate is offset by 0.3 along the normal and tilted by 0.5 degrees."""
    rng = np.random.default_rng(6)
    t = synth.plane_params(rng, size=20.0)
    uv = rng.uniform(-10.0, 10.0, size=(128, 2))
    xyz = np.ascontiguousarray(t["point"] + uv[:, :1] * t["_x"] + uv[:, 1:] * t["_y"])
    nrm = np.ascontiguousarray(np.repeat(t["normal"][None], 128, 0))
    tilt = np.radians(0.5)
    normal = np.cos(tilt) * t["normal"] + np.sin(tilt) * t["_x"]
    shape = ("plane", False, np.concatenate([t["point"] + 0.3 * t["normal"], normal / np.linalg.norm(normal)]))
    return xyz, nrm, synth.make_subsets(128, 3, 6), shape


def rms2_bound(st, D):
    """The implementations take the plane's rms^2 as lambda_min / N of a scatter formed as M - s s' / N about the
    caller's point, at the distance D from the centroid.  An entry of M is a sum of n_sel products of size <= D^2 + 3
    sigma^2 (sigma^2 = lambda_max / N), so its error is <= n_sel u N (D^2 + 3 sigma^2); s s' / N, the subtraction and the
    eigen-solver each add at most as much again (in fact ~u of it): |rms^2 - rms_ref^2| <= 4 n_sel u (D^2 + 3 sigma^2)."""
    return 4 * st.n_sel * U * (D * D + 3 * st.sigma2)


def moved_plane(case):
    """the case's plane candidate with its point moved along the plane by 100 x the cloud's extent, and that distance"""
    name, outw, v = scene(case)[3]["plane"]
    e1, _ = ref.frame(v[3:6])
    D = 100.0 * synth.BOX
    return (name, outw, np.concatenate([v[0:3] + D * e1.astype(np.float64), v[3:6]])), D


def check_moved_plane(case, got, n_used, rms):
    """The scatter about a point at the distance D from the centroid: the entries of M = sum d d' grow to N D^2 while the
    centred scatter S = M - s s' / N stays N sigma^2, so the rounding errors of M, relative to S, are (D / sigma)^2
    times those of a sum about the centroid; the one-step bound of the unmoved candidate (the same points, the same
    fitted plane) is multiplied by that factor.  rms: rms2_bound with this D."""
    shape, D = moved_plane(case)
    xyz, nrm, _, cands, _ = scene(case)
    st0 = ref_step(case, "plane")
    st = ref.one_step(shape, xyz, nrm, None, orc.default_params())
    assert st.n_sel == st0.n_sel == n_used
    loss = D * D / st0.sigma2
    bound = ref.one_step_bound(C_STEP, st0, shape[2], "plane") * loss
    check_conditions(cands["plane"], st0, bound)
    err = step_error("plane", got, st)
    assert err <= bound, (err, bound)
    assert abs(rms * rms - float(st.rms) ** 2) <= rms2_bound(st, D), (rms, float(st.rms))
    return err / bound


def half_disabled(case, kind):
    """-> the 1-based indices of every second selected point of the case's candidate of that kind, the enabled mask"""
    sel = np.nonzero(ref_step(case, kind).sel)[0]
    off = sel[::2]
    en = np.ones(CASES[case][0], dtype=bool)
    en[off] = False
    return off + 1, en


DISABLED = {"S": "cone", "L": "cylinder"}


def test_oracle_eight_points_fit_seven_refuse():
    op = orc.default_params()
    xyz, nrm, subs, shape = tiny_sphere(8)
    st = ref.one_step(shape, xyz, nrm, None, op)
    assert st.n_sel == 8
    out, n, rms, it = orc.Cloud(xyz, nrm, subs[0]).refit_lsq(to_orc(shape), op, max_iter=1)
    check_one_step(shape, list(out.v), n, rms, st, c=1.0)
    check_rms(rms, st)
    xyz, nrm, subs, shape = tiny_sphere(7)
    assert ref.select(shape, xyz, nrm, None, op).sum() == 7
    with pytest.raises(RuntimeError):
        orc.Cloud(xyz, nrm, subs[0]).refit_lsq(to_orc(shape), op, max_iter=1)


def test_oracle_noise_free_plane():
    op = orc.default_params()
    xyz, nrm, subs, shape = flat_plane()
    st = ref.one_step(shape, xyz, nrm, None, op)
    assert st.n_sel == 128
    out, n, rms, it = orc.Cloud(xyz, nrm, subs[0]).refit_lsq(to_orc(shape), op, max_iter=1)
    check_one_step(shape, list(out.v), n, rms, st, c=1.0)
    D = float(np.linalg.norm((st.v[0:3] - shape[2][0:3]).astype(np.float64)))
    assert float(st.rms) < 1e-13 and rms * rms <= rms2_bound(st, D), (rms, float(st.rms))


def test_oracle_far_reference_point_of_a_plane(oracle_clouds):
    shape, D = moved_plane("L")
    out, n, rms, it = oracle_clouds["L"].refit_lsq(to_orc(shape), orc.default_params(), max_iter=1)
    check_moved_plane("L", list(out.v), n, rms)


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_leaves_disabled_points_out(case):
    xyz, nrm, subs, cands, _ = scene(case)
    op, kind = orc.default_params(), DISABLED[case]
    off, en = half_disabled(case, kind)
    oc = orc.Cloud(xyz, nrm, subs[0])
    oc.invalidate(off)
    st = ref.one_step(cands[kind], xyz, nrm, en, op)
    assert st.n_sel == ref_step(case, kind).n_sel // 2
    out, n, rms, it = oc.refit_lsq(to_orc(cands[kind]), op, max_iter=1)
    check_one_step(cands[kind], list(out.v), n, rms, st)
    check_rms(rms, st)


@pytest.mark.parametrize("max_iter", [0, -3])
def test_oracle_max_iter_below_one_means_one(oracle_clouds, max_iter):
    op, shape = orc.default_params(), to_orc(scene("S")[3]["cone"])
    one = oracle_clouds["S"].refit_lsq(shape, op, max_iter=1)
    got = oracle_clouds["S"].refit_lsq(shape, op, max_iter=max_iter)
    assert bytes(got[0]) == bytes(one[0]) and got[1:] == one[1:]
