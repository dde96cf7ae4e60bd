"""The normal-cell mask of a plane candidate (csrc/score4_device.h: nsig_cand_mask inside cls_make, fields 5-7 of the culling
record) as the HOST builds it, against a brute-force statement in numpy.  The score kernel skips a (plane, group) pair when no
point of the group has its normal's cell in the candidate's mask, so the mask must hold the cell of EVERY direction d that a
point's normal may have when the exact test accepts it:  n . (l d) >= cos(alpha) - margin  for some length l <= L, margin being the
classifier's own margin on the normal half (mN of cls_make) and L the largest normal length of the cloud.  rh_dbg_nsig (diag
build, no GPU) hands out the mask and the library's one cell function."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

NDIR = 200_000
ALPHAS = [5.0, 60.0, 95.0]
U = 2.0 ** -24


def _params(alpha_deg):
    params = R.ransacparameters([R.FittedPlane])
    params["plane"]["ϵ"] = 0.3
    params["plane"]["α"] = float(np.radians(alpha_deg))
    return R.params_to_c(params)


def _shape(n, p0=(1.0, 2.0, 3.0)):
    s = L.Shape()
    s.kind, s.outwards = L.PLANE, 0
    for i, v in enumerate(list(p0) + list(n)):
        s.v[i] = float(v)
    return s


def _mask(n, cp, M=100.0, Nm=1.0, Ln=1.0, f32=0, p0=(1.0, 2.0, 3.0)):
    out = (C.c_uint32 * 3)()
    s = _shape(n, p0)
    L.check(L.lib("diag").rh_dbg_nsig(C.byref(s), C.byref(cp), M, Nm, Ln, f32, out, None, 0, None))
    return int(out[0]) | (int(out[1]) << 32) | (int(out[2]) << 64)


def _cells(dirs):
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    out = np.zeros(len(dirs), dtype=np.int32)
    L.check(L.lib("diag").rh_dbg_nsig(None, C.byref(_params(5.0)), 0.0, 0.0, 0.0, 0, None, dirs.ctypes.data_as(C.POINTER(C.c_double)),
                                      len(dirs), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


ALL = (1 << 96) - 1
BORDER = [(1, 1, 0), (1, 1, 1), (1, 0.5, 0), (1, 0, 0), (1, 0.5, 0.5), (1, -0.5, 0), (1, 1, 0.5), (1, -1, -1), (1, 0, 0.5)]


def _border_dirs():
    """directions exactly on face edges, cube corners and the 4 x 4 cell borders, in every axis order and sign"""
    out = []
    for b in BORDER:
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
            for sg in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1)):
                out.append([sg[k] * b[perm[k]] for k in range(3)])
    return np.unique(np.array(out, dtype=np.float64), axis=0)


@pytest.fixture(scope="module")
def dirs():
    """2 x 10^5 unit directions: random ones, the border directions (normalised: the rounding moves them to either side of
    their border) and, un-normalised, the border directions themselves (exactly ON it)"""
    rng = np.random.default_rng(7)
    bd = _border_dirs()
    d = rng.normal(size=(NDIR - len(bd), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    unit = np.vstack([d, bd / np.linalg.norm(bd, axis=1, keepdims=True)])
    return unit, _cells(unit), bd, _cells(bd)


def _numpy_cell(d):
    """the cell of score4_device.h stated independently: face = largest |component| (x before y before z on ties) with its
    sign, the two others (cyclic order) divided by that magnitude and cut at -1/2, 0, 1/2; and the distance of either quotient
    to a cut or of the face choice to a tie"""
    a = np.abs(d)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    idx = np.arange(len(d))
    m = d[idx, axis]
    qa, qb = d[idx, (axis + 1) % 3] / np.abs(m), d[idx, (axis + 2) % 3] / np.abs(m)
    i = (qa >= -0.5).astype(int) + (qa >= 0).astype(int) + (qa >= 0.5).astype(int)
    j = (qb >= -0.5).astype(int) + (qb >= 0).astype(int) + (qb >= 0.5).astype(int)
    cuts = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    gap = np.minimum(np.abs(qa[:, None] - cuts).min(axis=1), np.abs(qb[:, None] - cuts).min(axis=1))
    return (axis * 2 + (m < 0)) * 16 + i * 4 + j, gap


def test_cell_function_is_the_cube_map(dirs):
    unit, cells, bd, bcells = dirs
    want, gap = _numpy_cell(unit)
    clear = gap > 1e-9
    assert clear.sum() > NDIR * 0.99
    assert np.array_equal(cells[clear], want[clear])
    assert cells.min() >= 0 and cells.max() <= 95 and len(np.unique(cells)) == 96
    # exactly on a border: one of the cells that meet there, and the comparisons (>=) say which
    wb, gb = _numpy_cell(bd)
    assert (gb == 0).all() and np.array_equal(bcells, wb)
    # what sets no bit / every bit
    odd = np.array([[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [1.0, np.inf, 0.0], [-np.inf, 0.0, 0.0], [np.nan, np.inf, 0.0], [1e-300, 0.0, 0.0],
                    [0.0, -3e200, 1e200]])
    assert _cells(odd).tolist() == [-1, -1, -2, -2, -2, 0 * 16 + 2 * 4 + 2, (1 * 2 + 1) * 16 + 2 * 4 + 2]


def _candidate_normals():
    rng = np.random.default_rng(11)
    truth = rng.normal(size=(6, 3))
    truth /= np.linalg.norm(truth, axis=1, keepdims=True)
    bd = _border_dirs()
    rnd = rng.normal(size=(200, 3))
    rnd *= (rng.uniform(0.3, 3.0, size=200) / np.linalg.norm(rnd, axis=1))[:, None]     # candidates' normals need not be unit vectors
    named = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.5, 0.0], [1.0, 0.0, 0.0]])
    named = np.vstack([named, named / np.linalg.norm(named, axis=1, keepdims=True)])
    return truth, np.vstack([truth, -truth, named, bd[::7], bd[::7] / np.linalg.norm(bd[::7], axis=1, keepdims=True), rnd])


def _margin(n, cosa, Nm, f32):
    S = 6.0 if f32 else 2.0
    return S * U * (5.05 * (np.abs(n).sum() * Nm) + 4.1 * (abs(cosa) + 1e-3)) + 1e-30


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_mask_holds_every_direction_the_test_can_accept(dirs, alpha, f32):
    unit, cells, bd, bcells = dirs
    truth, normals = _candidate_normals()
    # from the inputs alone: flipped normals, border normals, wide cones and border directions all occur
    assert any(np.array_equal(normals[i], -normals[j]) for i in range(6) for j in range(6, 12))
    assert any(np.array_equal(n, [1.0, 1.0, 0.0]) for n in normals) and any(np.array_equal(n, [1.0, 1.0, 1.0]) for n in normals)
    assert (_numpy_cell(bd)[1] == 0).all() and len(bd) >= 80
    assert max(ALPHAS) > 90.0 and 60.0 in ALPHAS
    cp = _params(alpha)
    cosa = float(cp.cos_alpha[L.PLANE])
    pops = []
    for n in normals:
        # (unit normals in the cloud, their length known; twice and three times as long with the bound the cloud's largest
        # component gives; lengths between 0.5 and 3 with the largest known)
        for Nm, Ln, lens in ((1.0, 1.0, (1.0,)), (2.0, 0.0, (2.0, 2.0 * np.sqrt(3.0))), (3.0, 3.0, (0.5, 3.0))):
            m = _mask(n, cp, Nm=Nm, Ln=Ln, f32=f32)
            thr = cosa - _margin(n, cosa, Nm, f32)
            if thr <= 0.0:
                assert m == ALL
                continue
            for dd, cc in ((unit, cells), (bd / np.linalg.norm(bd, axis=1, keepdims=True), _cells(bd))):
                ok = np.zeros(len(dd), dtype=bool)
                for ln in lens:
                    ok |= (dd @ n) * ln >= thr
                hit = np.unique(cc[ok])
                assert all((m >> int(k)) & 1 for k in hit), (n, alpha, Nm, Ln, [int(k) for k in hit if not (m >> int(k)) & 1])
            if Ln == 1.0 and abs(np.linalg.norm(n) - 1.0) < 1e-12:
                pops.append(bin(m).count("1"))
    if alpha == 5.0:
        # the mask is worth having: a 5-degree cone about a unit normal reaches the centres within 5 + 19.5 degrees (the largest
        # cell radius) of it -- a cap of 0.56 sr, where the smallest cells (0.08 sr) have at most a dozen centres
        assert max(pops) <= 12 and min(pops) >= 1
    if alpha == 95.0:
        assert not pops or min(pops) == 96


def test_all_ones_where_nothing_may_be_skipped():
    cp5, cp90, cp95 = _params(5.0), _params(90.0), _params(95.0)
    n = np.array([0.6, 0.0, 0.8])
    assert _mask(n, cp5) != ALL
    assert _mask(n, cp95) == ALL and _mask(n, cp90) == ALL                      # cos(alpha) - margin <= 0: a cone of 90 degrees or more
    for bad in ([np.nan, 0.0, 1.0], [np.inf, 0.0, 1.0], [0.0, 0.0, 0.0], [3e6, 0.0, 1.0]):   # exact-only candidates
        assert _mask(np.array(bad), cp5) == ALL
    assert _mask(n, cp5, p0=(np.nan, 0.0, 0.0)) == ALL and _mask(n, cp5, p0=(2e6, 0.0, 0.0)) == ALL
    for kw in ({"Nm": np.inf}, {"Nm": np.nan}, {"M": np.nan}, {"M": 4e6}, {"Nm": 4e6}, {"Nm": 0.0, "Ln": 0.0}):
        assert _mask(n, cp5, **kw) == ALL, kw
    # a length that is not a number is no bound: the component bound takes over
    assert _mask(n, cp5, Ln=np.nan) == _mask(n, cp5, Ln=0.0) == _mask(n, cp5, Ln=-1.0) != ALL
    # a cloud whose normals are a thousand times too long: the cone is all but a half space
    wide = _mask(n, cp5, Nm=1000.0, Ln=0.0)
    assert bin(wide).count("1") >= 48
