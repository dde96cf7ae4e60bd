"""The entry points on raw host arrays own their device buffers and their stream for the length of the call
(csrc/call_scope.h) and give them back on every way out: a normal end, RH_E_CAPACITY where the entry has a capacity, and
RH_E_INVALID for a device that is not there.

What is compared is the device's free memory (torch.cuda.mem_get_info) after one warm-up round and after twenty more
rounds of all three ways out.  Measured on an MI355X, free memory after every single round, eight entries, thirty rounds,
four processes on the code before call_scope.h and four on this code: the figure moves in an entry's FIRST round only
(150 MiB for the first entry of a process, 0, 2 or 4 MiB for a later one: the runtime's start and the entry's code
objects) and by exactly 0 bytes from the second round on, in every process.  So 0 is what is allowed.
The figure is the whole device's, in steps of 2 MiB, and other processes may share the device: a step that is no leak
of this library can fall into the window.  A leak grows with the rounds and shows in every window, a step from outside
does not: the window is repeated, three times at the most, and one of them must show 0.  The arrays are large enough for
the smallest per-point buffer (one byte per point or pixel) lost once a round to come to 4 MB a window, two steps of
the figure; a lost scalar buffer or stream is below what this figure can show."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

N = 200_000
RNG = np.random.default_rng(21)
XYZ = np.ascontiguousarray(RNG.uniform(0, 16, size=(N, 3)))
NRM = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (N, 1)))
XS, YS = 512, 400
BITMAP = np.ascontiguousarray((RNG.random(XS * YS) < 0.7).astype(np.uint8))


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _cc(device, small):
    out, n = np.zeros(BITMAP.size, dtype=np.int64), C.c_int64()
    return R.lib().rh_largestconncomp(_p(BITMAP, C.c_uint8), XS, YS, 1, device, _p(out, C.c_int64), 3 if small else out.size, C.byref(n))


def _voxel(device, small):
    cap = 2 if small else N
    xo, no = np.zeros((N, 3)), np.zeros((N, 3))
    first, count, rowof = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    m, nd = C.c_int64(), C.c_int64()
    prm = L.VoxelParams(beta=0.5, mode=L.VOX_CENTROID, flags=0)
    return R.lib().rh_voxel_downsample(_p(XYZ, C.c_double), _p(NRM, C.c_double), N, C.byref(prm), device, _p(xo, C.c_double),
                                       _p(no, C.c_double), _p(first, C.c_int64), _p(count, C.c_int32), cap, _p(rowof, C.c_int32),
                                       C.byref(m), C.byref(nd))


def _voxel_f32(device, small):
    x32, xo = XYZ.astype(np.float32), np.zeros((N, 3), dtype=np.float32)
    m = C.c_int64()
    prm = L.VoxelParams(beta=0.5, mode=L.VOX_FIRST, flags=0)
    return R.lib().rh_voxel_downsample_f32(_p(x32, C.c_float), None, N, C.byref(prm), device, _p(xo, C.c_float), None, None, None,
                                           2 if small else N, None, C.byref(m), None)


def _assign(device, small):
    shapes = (L.Shape * 2)(R.FittedPlane([0.0, 0.0, 1.0], [0.0, 0.0, 1.0]).to_c(), R.FittedSphere([2.0, 2.0, 2.0], 1.0, True).to_c())
    prm = R.params_to_c(R.ransacparameters([R.FittedPlane, R.FittedSphere]))
    labels, dist = np.zeros(N, dtype=np.int32), np.zeros(N)
    counts, offsets, idx = np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(N, dtype=np.int64)
    return R.lib().rh_assign_points(_p(XYZ, C.c_double), _p(NRM, C.c_double), N, shapes, 2, C.byref(prm), 0, device, _p(labels, C.c_int32),
                                    _p(dist, C.c_double), _p(counts, C.c_int64), _p(offsets, C.c_int64), _p(idx, C.c_int64))


def _knn(device, small):
    idx, d2, cnt = np.zeros((N, 8), dtype=np.int32), np.zeros((N, 8)), np.zeros(N, dtype=np.int32)
    return R.lib().rh_knn(_p(XYZ, C.c_double), N, 8, 0.0, device, _p(idx, C.c_int32), _p(d2, C.c_double), _p(cnt, C.c_int32))


def _knn_f32(device, small):
    x32, idx = XYZ.astype(np.float32), np.zeros((N, 8), dtype=np.int32)
    return R.lib().rh_knn_f32(_p(x32, C.c_float), N, 8, 0.0, device, _p(idx, C.c_int32), None, None)


def _outliers(device, small):
    keep, kept, nk = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.int32), C.c_int64()
    prm = L.OutlierParams(k=8, mode=L.OUT_STATISTICAL, std_mul=2.0)
    return R.lib().rh_remove_outliers(_p(XYZ, C.c_double), N, C.byref(prm), device, _p(keep, C.c_uint8), _p(kept, C.c_int32),
                                      5 if small else N, C.byref(nk), None, None)


def _normals(device, small):
    out, curv, flags = np.zeros((N, 3)), np.zeros(N), np.zeros(N, dtype=np.int32)
    prm = L.NormalsParams(k=12, orient=2, radius=0.0)
    return R.lib().rh_estimate_normals(_p(XYZ, C.c_double), N, C.byref(prm), _p(NRM, C.c_double), device, _p(out, C.c_double),
                                       _p(curv, C.c_double), _p(flags, C.c_int32))


# entry -> (call, has a capacity)
ENTRIES = {"largestconncomp": (_cc, True), "voxel": (_voxel, True), "voxel_f32": (_voxel_f32, True), "assign": (_assign, False),
           "knn": (_knn, False), "knn_f32": (_knn_f32, False), "remove_outliers": (_outliers, True), "normals": (_normals, False)}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_way_out_releases(name):
    call, has_cap = ENTRIES[name]
    ndev = C.c_int()
    L.check(R.lib().rh_device_count(C.byref(ndev)))

    def one_round():
        assert call(0, False) == L.RH_OK, R.lib().rh_last_error()
        if has_cap:
            assert call(0, True) == L.RH_E_CAPACITY
        assert call(ndev.value, False) == L.RH_E_INVALID

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    one_round()
    seen = []
    for _ in range(3):
        warm = free_bytes()
        for _ in range(20):
            one_round()
        seen.append(warm - free_bytes())
        print("%s: free before the window %d, after its 20 rounds %d bytes less" % (name, warm, seen[-1]))
        if seen[-1] == 0:
            break
    assert 0 in seen, seen
