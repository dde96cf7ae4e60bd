"""Rigid registration (rh_register, include/ransac_hip.h), CPU side: the numpy twin of tests/register_reference.py pinned
by hand-derived cases, the scheme's basin tried on the twin (an exact copy; disjoint noisy samples with outliers), the
argument checks and the ABI declarations.  tests/test_register_gpu.py holds the library to the twin, byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
import register_reference as RR
from register_reference import ref_register
from test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMS = ["plane", "plane", "plane", "sphere", "cylinder"]
IDENT = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


# ------------------------------------------------------------------ the twin, pinned by hand ----
def _lattice():
    """64 points at -15, -5, 5, 15 around (100, 200, 300): symmetric about the box centre, spacing 10"""
    g = np.array([-15.0, -5.0, 5.0, 15.0])
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([100.0, 200.0, 300.0])


def test_a_pure_translation_is_recovered_in_one_step():
    """Queries = the reference shifted by 0.25 along x, far less than the spacing: the correspondences are the identity.
    With c = (100, 200, 300) every y', e and leaf is a small dyadic number and every sum exact: Y = (16, 0, 0), g =
    (0, 0, 0, -16, 0, 0), H_33 = 64, L_33 = 8, the couplings H_15 = -16 and H_24 = 16 meet only zeros of z and x, so
    x_3 = (-16 / 8) / 8 = -0.25 and every other x_k is a zero; the Cayley step of a = 0 is the identity exactly."""
    ref = _lattice()
    qry = ref + np.array([0.25, 0.0, 0.0])
    want = IDENT.copy()
    want[0, 3] = -0.25
    one = ref_register(ref, qry, max_iter=1)
    assert (one["transform"] + 0.0).tobytes() == want.tobytes()          # (+ 0.0: a zero of either sign)
    assert (one["status"], one["iterations"], one["n_valid"], one["rms"]) == (RR.MAX_ITER, 1, 64, 0.25)
    more = ref_register(ref, qry, max_iter=5)
    assert (more["transform"] + 0.0).tobytes() == want.tobytes()
    assert (more["status"], more["iterations"]) == (RR.CONVERGED, 2)      # the second iteration finds nothing left to do
    assert more["n_valid_it"].tolist() == [64, 64, 0, 0, 0] and more["rms_it"].tolist() == [0.25, 0.0, 0.0, 0.0, 0.0]
    # an init that already holds the answer: one iteration, a zero step
    held = ref_register(ref, qry, max_iter=5, init=want)
    assert (held["transform"] + 0.0).tobytes() == want.tobytes() and (held["status"], held["iterations"]) == (RR.CONVERGED, 1)


def test_a_planar_reference_under_the_plane_metric_is_degenerate():
    """z = 0 and normals (0, 0, 1) exactly: a = (y'_1, -y'_0, 0, 0, 0, 1) -- rows and columns 2 (w_z), 3 and 4 (tau_x, tau_y)
    of H are exactly 0, so pivot 2 is 0 - 0 - 0 = 0 and is refused at the first solve."""
    rng = np.random.default_rng(1)
    ref = np.zeros((400, 3))
    ref[:, :2] = rng.uniform(0.0, 20.0, size=(400, 2))
    nrm = np.tile([0.0, 0.0, 1.0], (400, 1))
    qry = ref[:150] + np.array([0.01, -0.02, 0.3])
    r = ref_register(ref, qry, normals=nrm)
    assert (r["status"], r["iterations"], r["n_valid"]) == (RR.DEGENERATE, 1, 150)
    assert (r["transform"] + 0.0).tobytes() == IDENT.tobytes()            # the transform reached so far: the start
    assert r["rms"] > 0.0 and r["n_valid_it"][:2].tolist() == [150, 0]
    # the point metric has no such null space
    assert ref_register(ref, qry, max_iter=40)["status"] == RR.CONVERGED


def test_fewer_than_six_valid_queries_end_the_call():
    ref = _lattice()
    qry = ref[:9] + np.array([0.25, 0.0, 0.0])
    qry[5:] += 3.0                                                         # four of the nine farther than the radius
    r = ref_register(ref, qry, radius=1.0)
    assert (r["status"], r["iterations"], r["n_valid"]) == (RR.TOO_FEW, 1, 5)
    assert (r["transform"] + 0.0).tobytes() == IDENT.tobytes() and r["rms"] == 0.25
    assert ref_register(ref, qry[:5])["status"] == RR.TOO_FEW             # m < 6
    none = ref_register(ref, qry + 1000.0, radius=1.0)
    assert (none["status"], none["n_valid"], none["rms"]) == (RR.TOO_FEW, 0, 0.0)


def test_cholesky_and_cayley_by_hand():
    H = [[4.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    H[0][1] = H[1][0] = 2.0                                                # L00 = 2, L10 = 1, L11 = sqrt(4 - 1)
    x = RR.ref_cholesky_solve(H, [2.0, 4.0, 4.0, 8.0, -4.0, 0.0])
    s3 = np.sqrt(3.0)
    z1 = (4.0 - 1.0 * 1.0) / s3
    x1 = z1 / s3
    assert x == [(1.0 - 1.0 * x1) / 2.0, x1, 1.0, 2.0, -1.0, 0.0]
    H[2][2] = 0.0
    assert RR.ref_cholesky_solve(H, [0.0] * 6) is None                     # a pivot of 0 is refused
    H[2][2] = 1e-300                                                       # the test is relative to H_ii: units do not matter
    assert RR.ref_cholesky_solve(H, [0.0] * 6) is not None
    H[2][2], H[0][2], H[2][0] = 1.0, 2.0, 2.0                              # pivot 2 = (1 - 1*1) - L21*L21 < 0 after elimination
    assert RR.ref_cholesky_solve(H, [0.0] * 6) is None
    # the Cayley map of a = (0, 0, 1) is a quarter turn about z: ((1 - 1) I + 2 a a^T + 2 [a]x) / 2
    Rn, tn = RR.ref_cayley_update([0.0, 0.0, 2.0, 1.0, 2.0, 3.0], [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], [1.0, 0.0, 0.0])
    assert (np.array(Rn) + 0.0).tolist() == [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    assert (np.array(tn) + 0.0).tolist() == [1.0, 3.0, 3.0]


# ------------------------------------------------------------------------- the scheme's basin ----
MOTIONS = [(2.0, 0.5), (5.0, 2.0), (10.0, 3.0)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_an_exact_copy_is_brought_back(seed, metric):
    """1300 points of the reference itself, moved by a known motion: converged within 60 iterations, every point within
    1e-9 of its original (the stopping tolerance of 1e-10 at coordinates up to 100), R orthogonal to 1e-13.
    Measured on the twin, seeds 0 .. 3: plane 4 - 6 iterations, point 5 - 20; the largest point error 4.3e-14, the largest
    |R^T R - I| 1.4e-15."""
    xyz, nrm, _ = synth.make_cloud(3000, PRIMS, seed=seed)
    pick = np.random.default_rng(100 + seed).choice(3000, 1300, replace=False)
    for deg, shift in MOTIONS:
        q = RR.apply(RR.rigid(deg, shift, seed, xyz.mean(axis=0)), xyz[pick])
        r = ref_register(xyz, q, normals=nrm if metric == "plane" else None, metric=metric, max_iter=60, rot_tol=1e-10,
                         trans_tol=1e-10)
        err = np.abs(RR.apply(r["transform"], q) - xyz[pick]).max()
        Rm = r["transform"][:, :3]
        orth = np.abs(Rm.T @ Rm - np.eye(3)).max()
        print("seed %d %s %g deg / %g: %s after %d, error %.3g, |RtR - I| %.3g" % (seed, metric, deg, shift, RR.STATUS[r["status"]],
                                                                                  r["iterations"], err, orth))
        assert r["status"] == RR.CONVERGED and r["iterations"] <= 60
        assert err <= 1e-9 and orth <= 1e-13


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", ["plane", "point"])
def test_disjoint_noisy_samples_with_outliers(seed, metric):
    """Reference: the first 3000 points of a 4600-point cloud; queries: the next 1300 and 300 uniform outliers, moved.  No
    query has its original in the reference.  The largest error over the 1300 true points stays within 0.5 (plane) and 1.5
    (point) point spacings.  Measured on the twin, seeds 0 .. 3, in spacings: plane at most 0.22 (cap 0.5), point at most 0.88 (cap
    1.5).  CONVERGED is not required: under a radius the iteration can cycle between two correspondence sets (seed 2, point
    metric, 4 degrees ends at max_iter = 50 with an error of 0.49 spacings)."""
    xyz, nrm, _ = synth.make_cloud(4600, PRIMS, seed=seed)
    ref, rn = np.ascontiguousarray(xyz[:3000]), np.ascontiguousarray(nrm[:3000])
    true = xyz[3000:4300]
    out = np.random.default_rng(200 + seed).uniform(xyz.min(axis=0), xyz.max(axis=0), size=(300, 3))
    spacing = synth.median_nn_distance(ref)
    for deg, shift in ((2.0, 0.5), (4.0, 1.0)):
        q = RR.apply(RR.rigid(deg, shift, seed, xyz.mean(axis=0)), np.concatenate([true, out]))
        r = ref_register(ref, q, normals=rn if metric == "plane" else None, metric=metric, radius=4.0 * spacing, max_iter=50,
                         rot_tol=1e-7, trans_tol=1e-7)
        err = np.linalg.norm(RR.apply(r["transform"], q[:1300]) - true, axis=1).max() / spacing
        print("seed %d %s %g deg / %g: %s after %d, error %.3f spacings (%.3f), n_valid %d" % (
            seed, metric, deg, shift, RR.STATUS[r["status"]], r["iterations"], err, spacing, r["n_valid"]))
        assert r["status"] in (RR.CONVERGED, RR.MAX_ITER)
        assert err <= (0.5 if metric == "plane" else 1.5)


# ------------------------------------------------------------------------------ bookkeeping ----
def test_header_declares_the_entry_points_and_the_structs():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_register", "rh_register_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES and hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_register_params\s*;", src) and re.search(r"}\s*rh_register_result\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 119
    assert R.lib().rh_version() >= 119
    assert re.search(r"RH_REG_CONVERGED\s*=\s*0\s*,\s*RH_REG_MAX_ITER\s*=\s*1\s*,\s*RH_REG_DEGENERATE\s*=\s*2\s*,\s*RH_REG_TOO_FEW\s*=\s*3", src)
    assert (L.REG_CONVERGED, L.REG_MAX_ITER, L.REG_DEGENERATE, L.REG_TOO_FEW) == (RR.CONVERGED, RR.MAX_ITER, RR.DEGENERATE, RR.TOO_FEW)
    assert int(re.search(r"#define\s+RH_REG_MAX_ITERATIONS\s+(\d+)", src).group(1)) == L.REG_MAX_ITERATIONS == 1000
    assert header_symbols() == sorted(L.SIGNATURES)


def test_ctypes_structs_have_the_header_layout(tmp_path):
    pf = ["radius", "rot_tol", "trans_tol", "metric", "max_iter"]
    sf = ["status", "iterations", "n_valid", "rms"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\nint main(void) {\n'
                    '    printf("%zu %zu", sizeof(rh_register_params), sizeof(rh_register_result));\n'
                    + "".join('    printf(" %%zu", offsetof(rh_register_params, %s));\n' % f for f in pf)
                    + "".join('    printf(" %%zu", offsetof(rh_register_result, %s));\n' % f for f in sf)
                    + '    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    mine = [C.sizeof(L.RegisterParams), C.sizeof(L.RegisterResult)]
    mine += [getattr(L.RegisterParams, f).offset for f in pf] + [getattr(L.RegisterResult, f).offset for f in sf]
    assert got == mine
    assert [f for f, _ in L.RegisterParams._fields_] == pf and [f for f, _ in L.RegisterResult._fields_] == sf


def test_python_entries_are_exported_and_the_transforms_apply():
    for name in ("register", "transform_points", "transform_normals"):
        assert callable(getattr(R, name)) and name in R.__all__
    with pytest.raises(ValueError):
        R.register(np.zeros((8, 3)), np.zeros((4, 3)), metric="chamfer")
    with pytest.raises(ValueError):
        R.register(np.zeros((8, 3)), np.zeros((4, 3)), normals=np.zeros((7, 3)))
    with pytest.raises(ValueError):
        R.register(np.zeros((8, 3)), np.zeros((4, 3)), init=np.eye(3))
    with pytest.raises(ValueError):
        R.transform_points(np.eye(3), np.zeros((4, 3)))
    T = RR.rigid(30.0, 2.0, 5, np.array([1.0, 2.0, 3.0]))
    pts = np.random.default_rng(5).uniform(-5.0, 5.0, size=(50, 3))
    T4 = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
    assert R.transform_points(T, pts).tobytes() == RR.apply(T, pts).tobytes() == R.transform_points(T4, pts).tobytes()
    assert np.allclose(R.transform_points(T, pts), pts @ T[:, :3].T + T[:, 3], rtol=0, atol=1e-13)
    nr = R.transform_normals(T4, pts)
    assert np.allclose(nr, pts @ T[:, :3].T, rtol=0, atol=1e-13)
    assert np.allclose(np.linalg.norm(nr, axis=1), np.linalg.norm(pts, axis=1), rtol=1e-13)   # directions turn, lengths stay
    assert R.transform_points(T, pts.astype(np.float32)).dtype == np.float64


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """Every case below is RH_E_INVALID with or without a GPU: the checks come first."""
    ref, qry, nrm = np.zeros((8, 3)), np.ones((7, 3)), np.tile([0.0, 0.0, 1.0], (8, 1))
    bad_init = np.eye(4)
    bad_init[1, 3] = np.inf
    nan_init = np.eye(4)
    nan_init[2, 0] = np.nan
    for dt in (np.float64, np.float32):
        r, q, nr = ref.astype(dt), qry.astype(dt), nrm.astype(dt)
        for kw in (dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(rot_tol=-1e-9),
                   dict(rot_tol=float("nan")), dict(trans_tol=-1.0), dict(trans_tol=float("nan")), dict(max_iter=0),
                   dict(max_iter=-4), dict(max_iter=1001), dict(metric=2), dict(metric=-1), dict(metric="plane"),
                   dict(init=bad_init), dict(init=nan_init), dict(init=nan_init[:3])):
            with pytest.raises(R.RansacHipError) as e:
                R.register(r, q, **kw)
            assert e.value.code == L.RH_E_INVALID, kw
        for a, b in ((r[:0], q), (r, q[:0])):
            with pytest.raises(R.RansacHipError) as e:
                R.register(a, b)
            assert e.value.code == L.RH_E_INVALID
        with pytest.raises(R.RansacHipError) as e:                        # valid otherwise: the plane metric with a bad radius
            R.register(r, q, normals=nr, radius=-2.0)
        assert e.value.code == L.RH_E_INVALID
    lib = R.lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pr, pq = ref.ctypes.data_as(dp), qry.ctypes.data_as(dp)
    out, res = np.full((3, 4), -7.0), L.RegisterResult(status=-7, iterations=-7, n_valid=-7)
    nv, rms = np.full(10, -7, dtype=np.int32), np.full(10, -7.0)
    po, pn, prms = out.ctypes.data_as(dp), nv.ctypes.data_as(i32p), rms.ctypes.data_as(dp)
    prm = L.RegisterParams(radius=0.0, rot_tol=1e-9, trans_tol=1e-9, metric=L.DIST_POINT, max_iter=10)
    fn = lib.rh_register
    assert fn(None, None, 8, pq, 7, C.byref(prm), None, 0, po, C.byref(res), pn, prms) == L.RH_E_INVALID
    assert fn(pr, None, 8, None, 7, C.byref(prm), None, 0, po, C.byref(res), pn, prms) == L.RH_E_INVALID
    assert fn(pr, None, 8, pq, 7, None, None, 0, po, C.byref(res), pn, prms) == L.RH_E_INVALID
    assert fn(pr, None, 8, pq, 7, C.byref(prm), None, 0, None, C.byref(res), pn, prms) == L.RH_E_INVALID
    for n, m in ((0, 7), (-1, 7), (2 ** 31 - 1, 7), (2 ** 40, 7), (8, 0), (8, -1), (8, 2 ** 31), (8, 2 ** 40)):
        assert fn(pr, None, n, pq, m, C.byref(prm), None, 0, po, C.byref(res), pn, prms) == L.RH_E_INVALID, (n, m)
    plane = L.RegisterParams(radius=0.0, rot_tol=1e-9, trans_tol=1e-9, metric=L.DIST_PLANE, max_iter=10)
    assert fn(pr, None, 8, pq, 7, C.byref(plane), None, 0, po, C.byref(res), pn, prms) == L.RH_E_INVALID
    assert b"rh_register" in lib.rh_last_error()
    assert (out == -7.0).all() and (nv == -7).all() and (rms == -7.0).all()                # nothing was written
    assert (res.status, res.iterations, res.n_valid) == (-7, -7, -7)
