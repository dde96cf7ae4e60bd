"""Voxel-grid downsampling (rh_voxel_downsample, include/ransac_hip.h), CPU side: the numpy twin of the definition, pinned
by hand-derived cases, the ABI declarations, the argument checks that come before the first device call, and
expand_inpoints.  tests/test_voxel_gpu.py holds the library to the twin bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO32 = 4294967296.0


def ref_voxel(xyz, nrm, beta, mode, align=False):
    """The definition, step by step, float64 throughout.  mode: "first" or "centroid".
    Returns (xyz_out, nrm_out or None, first (1-based), count, row_of_point, n_dropped); ValueError where the library
    returns RH_E_INVALID."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    if nrm is not None:
        nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    if not (n >= 1 and np.isfinite(beta) and beta > 0):
        raise ValueError("bad arguments")
    keep = np.isfinite(xyz).all(axis=1)
    if nrm is not None:
        with np.errstate(invalid="ignore"):
            keep &= (np.abs(nrm) <= 2.0).all(axis=1)        # (false for NaN and infinities)
    idx = np.flatnonzero(keep)
    rowof = np.zeros(n, dtype=np.int32)
    empty = (np.zeros((0, 3)), None if nrm is None else np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int32))
    if idx.size == 0:
        return empty + (rowof, n)
    p = xyz[idx]
    o = p.min(axis=0)
    with np.errstate(over="ignore"):
        if not (np.floor((p.max(axis=0) - o) / beta) < 1048576.0).all():
            raise ValueError("more than 2^20 cells along an axis")
    a = (p - o) / beta
    fl = np.floor(a)
    c = fl.astype(np.int64)
    f = np.floor((a - fl) * TWO32).astype(np.uint64)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    ukey, ufirst, inv = np.unique(key, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(ufirst, kind="stable")              # rows by the smallest point index they hold
    rank = np.empty(len(ukey), dtype=np.int64)
    rank[order] = np.arange(len(ukey))
    row = rank[inv]                                        # 0-based row of every kept point
    M = len(ukey)
    firstk = ufirst[order]                                 # position in idx of every row's first point
    first = idx[firstk].astype(np.int64) + 1
    count = np.bincount(row, minlength=M).astype(np.int32)
    rowof[idx] = (row + 1).astype(np.int32)
    q = None if nrm is None else nrm[idx]
    if mode == "first":
        return p[firstk].copy(), None if q is None else q[firstk].copy(), first, count, rowof, n - idx.size
    assert mode == "centroid"
    S = np.zeros((M, 3), dtype=np.uint64)
    for ax in range(3):
        np.add.at(S[:, ax], row, f[:, ax])
    num = (S >> np.uint64(32)).astype(np.float64) * TWO32 + (S & np.uint64(0xFFFFFFFF)).astype(np.float64)
    m = (num / count.astype(np.float64)[:, None]) * (1.0 / TWO32)
    out = o + (c[firstk].astype(np.float64) + m) * beta
    nout = None
    if q is not None:
        g = np.rint(q * 1048576.0).astype(np.int64)
        if align:
            r = q[firstk][row]
            g[(q[:, 0] * r[:, 0] + q[:, 1] * r[:, 1]) + q[:, 2] * r[:, 2] < 0] *= -1
        G = np.zeros((M, 3), dtype=np.int64)
        for ax in range(3):
            np.add.at(G[:, ax], row, g[:, ax])
        G = G.astype(np.float64)
        ln = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            nout = np.where(ln[:, None] == 0.0, 0.0, G / ln[:, None])
    return out, nout, first, count, rowof, n - idx.size


# ------------------------------------------------------------------ the twin, pinned by hand ----
def test_two_points_in_one_unit_cell_give_their_exact_midpoint():
    pts = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.75]])
    out, _, first, count, rowof, nd = ref_voxel(pts, None, 1.0, "centroid")
    assert np.array_equal(out, [[0.25, 0.125, 0.375]]) and first.tolist() == [1] and count.tolist() == [2]
    assert rowof.tolist() == [1, 1] and nd == 0
    out, _, first, _, _, _ = ref_voxel(pts[::-1], None, 1.0, "first")
    assert np.array_equal(out, [[0.5, 0.25, 0.75]]) and first.tolist() == [1]


def test_points_on_cell_faces_go_to_the_upper_cell_and_the_maximum_has_its_own():
    pts = np.array([[0.0, 0.0, 0.0], [0.999, 0.0, 0.0], [1.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, 0.0, 0.0]])
    out, _, first, count, rowof, _ = ref_voxel(pts, None, 1.0, "centroid")
    assert rowof.tolist() == [1, 1, 2, 2, 3] and first.tolist() == [1, 3, 5] and count.tolist() == [2, 2, 1]
    assert np.array_equal(out[1], [1.25, 0.0, 0.0])
    assert np.array_equal(out[2], [2.0, 0.0, 0.0])           # the point at the maximum: a cell of its own


def test_rows_are_in_first_appearance_order():
    pts = np.array([[5.5, 0, 0], [0.5, 0, 0], [5.6, 0, 0], [3.5, 0, 0], [0.6, 0, 0]], dtype=np.float64)
    _, _, first, count, rowof, _ = ref_voxel(pts, None, 1.0, "centroid")
    assert rowof.tolist() == [1, 2, 1, 3, 2] and first.tolist() == [1, 2, 4] and count.tolist() == [2, 2, 1]
    assert (np.diff(first) > 0).all()


def test_negative_coordinates_and_an_offset_of_1e6():
    base = np.array([[-3.0, -2.0, -1.0], [-2.5, -1.5, -0.5], [-1.0, 0.0, 1.0]])
    for off in (0.0, 1e6):
        out, _, _, count, rowof, _ = ref_voxel(base + off, None, 2.0, "centroid")
        # o = (-3, -2, -1) + off; the first two share cell (0, 0, 0), the third sits exactly on the face of cell (1, 1, 1)
        assert rowof.tolist() == [1, 1, 2] and count.tolist() == [2, 1]
        assert np.array_equal(out, np.array([[-2.75, -1.75, -0.75], [-1.0, 0.0, 1.0]]) + off)


def test_nan_rows_are_dropped_and_map_to_zero():
    pts = np.array([[np.nan, 0, 0], [0.25, 0.25, 0.25], [0.5, np.inf, 0.125], [0.75, 0.75, 0.75], [0, 0, -np.inf]])
    out, _, first, count, rowof, nd = ref_voxel(pts, None, 1.0, "centroid")
    assert rowof.tolist() == [0, 1, 0, 1, 0] and nd == 3 and first.tolist() == [2] and count.tolist() == [2]
    assert np.array_equal(out, [[0.5, 0.5, 0.5]])             # o = 0.25: offsets 0 and 0.5 of the cell
    nrm = np.tile([0.0, 0.0, 1.0], (5, 1))
    nrm[1] = [0.0, 2.5, 0.0]                                 # a normal component above 2: dropped too
    nrm[3, 0] = np.nan
    out, nout, first, count, rowof, nd = ref_voxel(np.abs(np.nan_to_num(pts, posinf=0.3, neginf=0.3)), nrm, 1.0, "centroid")
    assert rowof.tolist() == [1, 0, 1, 0, 1] and nd == 2 and count.tolist() == [3]
    assert np.array_equal(nout, [[0.0, 0.0, 1.0]])
    allbad = ref_voxel(np.full((3, 3), np.nan), None, 1.0, "first")
    assert allbad[0].shape == (0, 3) and allbad[4].tolist() == [0, 0, 0] and allbad[5] == 3


def test_align_turns_a_flipped_normal():
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]])
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    _, plain, _, _, _, _ = ref_voxel(pts, nrm, 1.0, "centroid", align=False)
    _, turned, _, _, _, _ = ref_voxel(pts, nrm, 1.0, "centroid", align=True)
    assert np.array_equal(plain, [[0.0, 0.0, 1.0]]) and np.array_equal(turned, [[0.0, 0.0, 1.0]])
    _, cancel, _, _, _, _ = ref_voxel(pts[:2], nrm[:2], 1.0, "centroid", align=False)
    _, kept, _, _, _, _ = ref_voxel(pts[:2], nrm[:2], 1.0, "centroid", align=True)
    assert np.array_equal(cancel, [[0.0, 0.0, 0.0]]) and np.array_equal(kept, [[0.0, 0.0, 1.0]])
    _, fn, _, _, _, _ = ref_voxel(pts[1:], nrm[1:], 1.0, "first")
    assert np.array_equal(fn, [[0.0, 0.0, -1.0]])            # first mode copies


def test_the_twin_refuses_what_the_library_refuses():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for beta in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -21):
        with pytest.raises(ValueError):
            ref_voxel(pts, None, beta, "centroid")
    assert len(ref_voxel(pts, None, 2.0 ** -19, "centroid")[2]) == 2


# ------------------------------------------------------------------------------------- ABI ----
def test_header_declares_the_entry_points_and_the_struct():
    src = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_voxel_downsample", "rh_voxel_downsample_f32"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(R.lib(), name)
    assert re.search(r"}\s*rh_voxel_params\s*;", src)
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", src).group(1)) >= 113
    assert R.lib().rh_version() >= 113


def test_ctypes_struct_has_the_header_size(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ransac_hip.h"\n'
                    'int main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(rh_voxel_params), '
                    'offsetof(rh_voxel_params, beta), offsetof(rh_voxel_params, mode), offsetof(rh_voxel_params, flags), '
                    '(int)RH_VOX_FIRST, (int)RH_VOX_CENTROID, (int)RH_VOX_ALIGN_NORMALS); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    size, off_b, off_m, off_f, k_first, k_cen, k_align = map(int, subprocess.check_output([str(exe)], text=True).split())
    V = L.VoxelParams
    assert (C.sizeof(V), V.beta.offset, V.mode.offset, V.flags.offset) == (size, off_b, off_m, off_f)
    assert (L.VOX_FIRST, L.VOX_CENTROID, L.VOX_ALIGN_NORMALS) == (k_first, k_cen, k_align)


def test_voxeldownsample_is_exported_and_checks_its_arguments():
    assert callable(R.voxeldownsample) and "voxeldownsample" in R.__all__ and "expand_inpoints" in R.__all__
    xyz = np.zeros((8, 3))
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(R.RansacHipError) as e:
            R.voxeldownsample(xyz, beta)
        assert e.value.code == L.RH_E_INVALID, beta
    for mode in (-1, 2):
        with pytest.raises(R.RansacHipError) as e:
            R.voxeldownsample(xyz, 1.0, mode=mode)
        assert e.value.code == L.RH_E_INVALID, mode
    with pytest.raises(ValueError):
        R.voxeldownsample(xyz, 1.0, mode="median")
    with pytest.raises(R.RansacHipError) as e:
        R.voxeldownsample(np.zeros((0, 3)), 1.0)                                  # n = 0
    assert e.value.code == L.RH_E_INVALID
    dp = C.POINTER(C.c_double)
    out, nout, m = np.zeros((8, 3)), np.zeros((8, 3)), C.c_int64(-1)
    p = L.VoxelParams(beta=1.0, mode=L.VOX_CENTROID, flags=0)
    fn = R.lib().rh_voxel_downsample
    rc = fn(xyz.ctypes.data_as(dp), None, 8, C.byref(p), 0, out.ctypes.data_as(dp), nout.ctypes.data_as(dp), None, None, 8, None,
            C.byref(m), None)
    assert rc == L.RH_E_INVALID and b"normals" in R.lib().rh_last_error()       # normals out without normals in
    assert fn(None, None, 8, C.byref(p), 0, out.ctypes.data_as(dp), None, None, None, 8, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(xyz.ctypes.data_as(dp), None, 8, None, 0, out.ctypes.data_as(dp), None, None, None, 8, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(xyz.ctypes.data_as(dp), None, 8, C.byref(p), 0, out.ctypes.data_as(dp), None, None, None, 8, None, None, None) == L.RH_E_INVALID
    assert fn(xyz.ctypes.data_as(dp), None, 8, C.byref(p), 0, None, None, None, None, 8, None, C.byref(m), None) == L.RH_E_INVALID
    assert fn(xyz.ctypes.data_as(dp), None, 1 << 31, C.byref(p), 0, out.ctypes.data_as(dp), None, None, None, 8, None, C.byref(m), None) == L.RH_E_INVALID
    p.flags = 2
    assert fn(xyz.ctypes.data_as(dp), None, 8, C.byref(p), 0, out.ctypes.data_as(dp), None, None, None, 8, None, C.byref(m), None) == L.RH_E_INVALID
    x32 = np.zeros((8, 3), dtype=np.float32)
    with pytest.raises(R.RansacHipError) as e:
        R.voxeldownsample(x32, 0.0)
    assert e.value.code == L.RH_E_INVALID


def test_expand_inpoints():
    rowof = np.array([1, 2, 0, 1, 3, 2, 0, 4, 1], dtype=np.int32)
    assert R.expand_inpoints([1], rowof).tolist() == [1, 4, 9]
    assert R.expand_inpoints([3, 2], rowof).tolist() == [2, 5, 6]
    assert R.expand_inpoints(np.array([4, 1, 4]), rowof).tolist() == [1, 4, 8, 9]
    assert R.expand_inpoints([], rowof).tolist() == [] and R.expand_inpoints([], rowof).dtype == np.int64
    with pytest.raises(ValueError):
        R.expand_inpoints([5], rowof)
    with pytest.raises(ValueError):
        R.expand_inpoints([0], rowof)
