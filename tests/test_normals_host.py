"""Point normals for clouds without them (rh_estimate_normals, include/ransac_hip.h), CPU side: a numpy reference of the
definition, pinned by hand-derived cases, and the ABI declarations.  tests/test_normals_gpu.py holds the library to it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_neighbours(xyz, kmax):
    """The first kmax points of every point's order: itself, then the others by d^2 = (dx*dx + dy*dy) + dz*dz,
    ties to the smaller index.  Returns (idx[n, kmax], d2[n, kmax]); -1 / inf past the end when n < kmax."""
    n = xyz.shape[0]
    kk = min(kmax, n)
    idx = np.full((n, kmax), -1, dtype=np.int64)
    d2 = np.full((n, kmax), np.inf)
    for lo in range(0, n, 512):
        p = xyz[lo:lo + 512]
        dx = xyz[None, :, 0] - p[:, None, 0]
        dy = xyz[None, :, 1] - p[:, None, 1]
        dz = xyz[None, :, 2] - p[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        key = d.copy()
        key[np.arange(p.shape[0]), lo + np.arange(p.shape[0])] = -1.0     # the point itself first
        order = np.argsort(key, axis=1, kind="stable")[:, :kk]            # stable: equal d^2 keep index order
        idx[lo:lo + p.shape[0], :kk] = order
        d2[lo:lo + p.shape[0], :kk] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def ref_normals(xyz, k, radius=0.0, viewpoint=None, hints=None, nb=None):
    """The definition, step by step.  Returns (normals, curvature, flags, gap) with gap = (l1 - l0) / l2 (0 when
    degenerate).  nb: ref_neighbours(xyz, >= k), to share one neighbour search between calls."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = xyz.shape[0]
    idx, d2 = nb if nb is not None else ref_neighbours(xyz, k)
    idx, d2 = idx[:, :k], d2[:, :k]
    use = idx >= 0
    if radius > 0:
        use &= d2 <= radius * radius
    m = use.sum(axis=1)
    q = xyz[np.where(use, idx, 0)] * use[:, :, None]
    c = q.sum(axis=1) / m[:, None]
    e = (q - c[:, None, :]) * use[:, :, None]
    cov = np.einsum("nki,nkj->nij", e, e) / m[:, None, None]
    lam, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0].copy()
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = l0 / (l0 + l1 + l2)
        gap = (l1 - l0) / l2
    deg = (m < 3) | (l2 == 0) | (l1 <= 1e-12 * l2)
    im = np.argmax(np.abs(nrm), axis=1)                 # argmax: the first on a tie
    nrm *= np.where(nrm[np.arange(n), im] < 0, -1.0, 1.0)[:, None]
    if viewpoint is not None:
        dot = (nrm * (np.asarray(viewpoint, dtype=np.float64)[None] - xyz)).sum(axis=1)
        nrm *= np.where(dot < 0, -1.0, 1.0)[:, None]
    elif hints is not None:
        dot = (nrm * np.asarray(hints, dtype=np.float64)).sum(axis=1)
        nrm *= np.where(dot < 0, -1.0, 1.0)[:, None]
    nrm[deg] = 0.0
    curv = np.where(deg, 0.0, curv)
    gap = np.where(deg, 0.0, gap)
    return nrm, curv, deg.astype(np.int32), gap


# ------------------------------------------------------------ the reference, pinned by hand ----
def test_square_corners_give_the_z_axis():
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    nrm, curv, flags, _ = ref_normals(sq, k=4)
    assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (4, 1)))
    assert np.array_equal(curv, np.zeros(4)) and np.array_equal(flags, np.zeros(4, np.int32))


def test_collinear_points_are_flagged():
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], dtype=np.float64)
    nrm, curv, flags, _ = ref_normals(line, k=3)
    assert np.array_equal(flags, np.ones(3, np.int32))
    assert np.array_equal(nrm, np.zeros((3, 3))) and np.array_equal(curv, np.zeros(3))


def test_fewer_than_three_neighbours_are_flagged():
    for pts in ([[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]):
        nrm, _, flags, _ = ref_normals(np.array(pts), k=8)
        assert np.array_equal(flags, np.ones(len(pts), np.int32)) and not nrm.any()


def test_ties_go_to_the_smaller_index():
    # point 0 at the origin, 4 a duplicate of it; 1, 2, 3 at distance 1 on z, x, y.  Order of 0: 0, 4 (d^2 = 0), 1, 2, 3.
    pts = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    idx, d2 = ref_neighbours(pts, 5)
    assert idx[0].tolist() == [0, 4, 1, 2, 3] and idx[4].tolist() == [4, 0, 1, 2, 3]
    nrm, _, flags, _ = ref_normals(pts, k=4)
    # {0, 4, 1, 2} span the plane y = 0 (taking 3 before 2 would give x = 0)
    assert flags[0] == 0 and np.allclose(nrm[0], [0, 1, 0], atol=1e-15) and np.allclose(nrm[4], [0, 1, 0], atol=1e-15)
    _, _, flags3, _ = ref_normals(pts, k=3)   # {0, 4, 1}: two coincident points and one more -> collinear
    assert flags3[0] == 1 and flags3[4] == 1


def test_lattice_with_duplicates_tie_rule():
    g = np.array([[x, y, 0.0] for y in range(3) for x in range(3)])           # 3 x 3 lattice in z = 0
    pts = np.concatenate([g, g[4:5] + [0, 0, 1]])                             # and one point above the centre
    idx, d2 = ref_neighbours(pts, 10)
    # the centre (index 4): itself, then the four at distance 1 in index order 1, 3, 5, 7, then 9 (above), then corners
    assert idx[4].tolist()[:6] == [4, 1, 3, 5, 7, 9]
    nrm, _, flags, _ = ref_normals(pts, k=5)
    assert flags[4] == 0 and np.allclose(nrm[4], [0, 0, 1], atol=1e-15)       # the lattice neighbours only
    dup = np.concatenate([pts, pts[1:2]])                                      # index 10 duplicates point 1
    idx2, _ = ref_neighbours(dup, 11)
    assert idx2[4].tolist()[:7] == [4, 1, 3, 5, 7, 9, 10] and idx2[10].tolist()[:2] == [10, 1]


def test_orientation_modes():
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    down = np.tile([0.0, 0.0, -1.0], (4, 1))
    assert np.array_equal(ref_normals(sq, 4, viewpoint=[0.5, 0.5, -5.0])[0], down)
    assert np.array_equal(ref_normals(sq, 4, viewpoint=[0.5, 0.5, 5.0])[0], -down)
    assert np.array_equal(ref_normals(sq, 4, hints=down)[0], down)
    side = np.tile([1.0, 0.0, 0.0], (4, 1))              # dot exactly 0: the canonical sign stays
    assert np.array_equal(ref_normals(sq, 4, hints=side)[0], -down)
    # canonical: the largest component positive, the first one on a tie
    tilted = np.array([[0, 0, 0], [1, 0, -1], [0, 1, 0], [1, 1, -1]], dtype=np.float64)   # plane x + z = 0
    n = ref_normals(tilted, 4)[0]
    assert np.allclose(n, np.tile([np.sqrt(0.5), 0, np.sqrt(0.5)], (4, 1)), atol=1e-15) and (n[:, 0] > 0).all()


def test_radius_drops_far_neighbours():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float64)
    _, _, flags, _ = ref_normals(pts, k=4, radius=1.5)
    assert flags[3] == 1 and flags[0] == 0                # (5, 5, 5) keeps only itself


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_struct():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_estimate_normals", "rh_estimate_normals_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
    assert re.search(r"}\s*rh_normals_params\s*;", src)


def test_ctypes_struct_has_the_header_size(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\n'
                    'int main(void) { printf("%zu %zu %zu\\n", sizeof(rh_normals_params), '
                    'offsetof(rh_normals_params, radius), offsetof(rh_normals_params, viewpoint)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    size, off_r, off_v = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert (C.sizeof(L.NormalsParams), L.NormalsParams.radius.offset, L.NormalsParams.viewpoint.offset) == (size, off_r, off_v)


def test_estimatenormals_is_exported_and_checks_its_arguments():
    assert callable(R.estimatenormals) and "estimatenormals" in R.__all__
    xyz = np.zeros((8, 3))
    for kw in (dict(k=2), dict(k=65), dict(radius=-1.0), dict(radius=float("inf"))):
        with pytest.raises(R.RansacHipError) as e:
            R.estimatenormals(xyz, **kw)
        assert e.value.code == L.RH_E_INVALID, kw
    p = L.NormalsParams(k=8, orient=2)
    out = np.zeros((8, 3))
    rc = R.lib().rh_estimate_normals(xyz.ctypes.data_as(C.POINTER(C.c_double)), 8, C.byref(p), None, 0,
                                     out.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == L.RH_E_INVALID                           # orient = 2 without hints
    with pytest.raises(R.RansacHipError):
        R.estimatenormals(np.zeros((0, 3)))
