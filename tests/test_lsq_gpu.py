"""rh_refit_lsq on the device against tests/lsq_reference.py: single Gauss-Newton steps (the Jacobian, the MFMA tile, the
update formulas), a cloud large enough for every wave to take a second and a third 64-point word (the accumulator
carried across words, the wave's LDS rows reused), the threshold of 8 points, fully selected words, disabled points,
same bits on every call and under either selection scan, and a cloud left as it was.  Cases, bounds and constants are
those of tests/test_lsq_host.py, where they are measured on the oracle."""
import numpy as np
import pytest

import lsq_reference as ref
import ransac_jl_amd as R
from oracle import oracle as orc
from test_lsq_host import (C_STEP, CASES, DISABLED, KINDS, MAX_ITER, TOL_G, check_moved_plane, check_one_step, check_rms,
                           flat_plane, gradient_ratio, half_disabled, moved_plane, ref_step, rms2_bound, scene,
                           step_error, tiny_sphere, to_orc)

pytestmark = pytest.mark.gpu

CASE_KIND = [(c, k) for c in CASES for k in KINDS]


def params():
    cp = R.params_to_c(R.ransacparameters())
    op = orc.default_params()
    assert list(cp.eps) == list(op.eps) and list(cp.cos_alpha) == list(op.cos_alpha)   # what ref_step selected with
    return cp


def to_R(shape):
    name, outw, v = shape
    if name == "plane":
        return R.FittedPlane(v[0:3], v[3:6])
    if name == "sphere":
        return R.FittedSphere(v[0:3], v[3], outw)
    if name == "cylinder":
        return R.FittedCylinder(v[0:3], v[3:6], v[6], outw)
    return R.FittedCone(v[0:3], v[3:6], v[6], outw)


def run(shape, pc, cp, max_iter):
    """-> fields of the result, n_used, rms, iters_done, and all of it as bytes"""
    got, n, rms, it = R.refit_lsq(to_R(shape), pc, cp, max_iter=max_iter)
    c = got.to_c()
    return list(c.v), n, rms, it, (bytes(c), n, np.float64(rms).tobytes(), it)


_CLOUDS = {}


def cloud(case):
    if case not in _CLOUDS:
        xyz, nrm, subs, _, _ = scene(case)
        _CLOUDS[case] = R.RANSACCloud(xyz, nrm, subs)
    return _CLOUDS[case]


@pytest.mark.parametrize("case,kind", CASE_KIND)
def test_one_step_equals_reference(case, kind):
    pc, cp, shape = cloud(case), params(), scene(case)[3][kind]
    st = ref_step(case, kind)
    v, n, rms, it, raw = run(shape, pc, cp, 1)
    ratio = check_one_step(shape, v, n, rms, st)
    print("one step %s %-8s n_used %6d error / bound %.4f" % (case, kind, n, ratio))
    check_rms(rms, st)
    assert it == 1
    for max_iter in (0, -3):                                   # max_iter < 1 means 1
        assert run(shape, pc, cp, max_iter)[4] == raw


@pytest.mark.parametrize("case,kind", CASE_KIND)
def test_second_step_equals_reference(case, kind):
    """from the device's own one-step result: another selection, another frame, and the update formulas (unit-length
    axis, opang = 2 phi) enter the input.  The step is small now, so of the two conditions only bound <= 1e-3 |x| is
    asserted; not for the plane, whose fit is done after one step: its second step is zero up to the points that the new
    selection adds, and the comparison says that a fitted plane is refitted to itself within 8 u |p|."""
    pc, cp, shape = cloud(case), params(), scene(case)[3][kind]
    xyz, nrm = scene(case)[:2]
    v1 = run(shape, pc, cp, 1)[0]
    shape1 = (kind, shape[1], np.array(v1[:ref.NPAR[kind]]))
    st = ref.one_step(shape1, xyz, nrm, None, cp)
    v2, n, rms, it, _ = run(shape1, pc, cp, 1)
    bound = ref.one_step_bound(C_STEP, st, shape1[2], kind)
    err = step_error(kind, v2, st)
    print("second step %s %-8s n_used %6d |x| %.3g error / bound %.4f" % (case, kind, n, np.abs(st.x).max(), err / bound))
    assert n == st.n_sel
    assert kind == "plane" or bound <= 1e-3 * float(np.abs(st.x).max())
    assert err <= bound, (err, bound)
    check_rms(rms, st)


@pytest.mark.parametrize("case,kind", CASE_KIND)
def test_converged_fit(case, kind):
    pc, cp, shape = cloud(case), params(), scene(case)[3][kind]
    xyz, nrm, subs = scene(case)[:3]
    v, n, rms, it, _ = run(shape, pc, cp, MAX_ITER)
    exp, on, orms, oit = orc.Cloud(xyz, nrm, subs[0]).refit_lsq(to_orc(shape), orc.default_params(), max_iter=MAX_ITER)
    assert it < MAX_ITER and abs(it - oit) <= 1, (it, oit)
    assert n == on == ref_step(case, kind).n_sel
    assert np.allclose(np.array(v), np.array(list(exp.v)), rtol=1e-8, atol=1e-9), (v, list(exp.v))
    assert abs(rms - orms) <= 1e-9 + 1e-6 * orms
    if kind != "plane":
        g = gradient_ratio((kind, True, np.array(v[:ref.NPAR[kind]])), xyz, ref_step(case, kind).sel)
        print("converged %s %-8s iterations %d (oracle %d) |J'r| / (|J| |r|) %.3g" % (case, kind, it, oit, g))
        assert g <= TOL_G


@pytest.mark.parametrize("case,kind", CASE_KIND)
def test_same_bits_on_every_call_and_selection_scan(case, kind):
    pc, cp, shape = cloud(case), params(), scene(case)[3][kind]
    first = run(shape, pc, cp, 3)[4]
    assert run(shape, pc, cp, 3)[4] == first
    by_path = {}
    for path in ("scan", "culled"):
        with R.option("refit_path", path, cloud=pc):
            by_path[path] = run(shape, pc, cp, 3)[4]
    assert by_path["scan"] == by_path["culled"] == first


@pytest.mark.parametrize("case", list(CASES))
def test_disabled_points_stay_out(case):
    pc, cp, kind = cloud(case), params(), DISABLED[case]
    xyz, nrm, subs, cands, _ = scene(case)
    off, en = half_disabled(case, kind)
    try:
        R.invalidate_indexes(pc, off)
        st = ref.one_step(cands[kind], xyz, nrm, en, cp)
        assert st.n_sel == ref_step(case, kind).n_sel // 2
        v, n, rms, it, _ = run(cands[kind], pc, cp, 1)
        check_one_step(cands[kind], v, n, rms, st)
        check_rms(rms, st)
    finally:
        pc.enable_all()


@pytest.mark.parametrize("case", list(CASES))
def test_cloud_is_left_as_it_was(case):
    xyz, nrm, subs, cands, _ = scene(case)
    cp = params()
    small = R.params_to_c(R.ransacparameters(iteration={"minsubsetN": 40, "τ": 200, "itermax": 25, "prob_det": 0.5}))
    used, fresh = R.RANSACCloud(xyz, nrm, subs), R.RANSACCloud(xyz, nrm, subs)
    off, _ = half_disabled(case, "sphere")
    for pc in (used, fresh):
        R.invalidate_indexes(pc, off)
    before = used.count_enabled()
    chunks = used.enabled_chunks()
    for kind in KINDS:
        run(cands[kind], used, cp, MAX_ITER)
    assert used.count_enabled() == before == fresh.count_enabled()
    assert np.array_equal(used.enabled_chunks(), chunks)
    for kind in KINDS:
        assert np.array_equal(R.refit(to_R(cands[kind]), used, cp).inpoints, R.refit(to_R(cands[kind]), fresh, cp).inpoints)
    a, b = R.ransac(used, small, seed=9)[0], R.ransac(fresh, small, seed=9)[0]
    assert len(a) == len(b) >= 1
    for g, e in zip(a, b):
        assert bytes(g.c_shape) == bytes(e.c_shape) and np.array_equal(g.inpoints, e.inpoints)


def test_far_reference_point_of_a_plane():
    shape, D = moved_plane("L")
    v, n, rms, it, _ = run(shape, cloud("L"), params(), 1)
    print("moved plane error / bound %.3g" % check_moved_plane("L", v, n, rms))


def test_eight_points_fit_seven_refuse():
    cp = params()
    xyz, nrm, subs, shape = tiny_sphere(8)
    st = ref.one_step(shape, xyz, nrm, None, cp)
    v, n, rms, it, _ = run(shape, R.RANSACCloud(xyz, nrm, subs), cp, 1)
    assert n == 8
    check_one_step(shape, v, n, rms, st, c=1.0)
    check_rms(rms, st)
    xyz, nrm, subs, shape = tiny_sphere(7)
    with pytest.raises(R.RansacHipError):                      # a clean error return, taken before any accumulation
        R.refit_lsq(to_R(shape), R.RANSACCloud(xyz, nrm, subs), cp, max_iter=1)


def test_noise_free_plane_with_full_words():
    cp = params()
    xyz, nrm, subs, shape = flat_plane()
    st = ref.one_step(shape, xyz, nrm, None, cp)
    v, n, rms, it, _ = run(shape, R.RANSACCloud(xyz, nrm, subs), cp, 1)
    assert n == 128
    check_one_step(shape, v, n, rms, st, c=1.0)
    D = float(np.linalg.norm((st.v[0:3] - shape[2][0:3]).astype(np.float64)))
    assert rms * rms <= rms2_bound(st, D), (rms, float(st.rms))
