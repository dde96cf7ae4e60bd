"""The census of the box tests on the hostile batch of test_cylbox_gpu.py (diag build: rh_dbg_cls_soundness / _tiles,
csrc/score4_diag.hip sound_one): no pair that a group's, a tile's or a super-tile's box rules out holds an exact inlier, for any kind;
and the cylinder's box test skips no fewer pairs than its two ball clauses alone, counted on the host with the kernel's own
function (rh_dbg_cylbox) over the library's group boxes (rh_dbg_group_boxes)."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import test_cylbox_gpu as T

pytestmark = [pytest.mark.gpu, pytest.mark.diag]


def _group_boxes(pc):
    n = C.c_int64()
    L.check(R.lib().rh_dbg_group_boxes(pc._h, None, 0, C.byref(n)))
    out = np.zeros((n.value, 6), dtype=np.float64)
    L.check(R.lib().rh_dbg_group_boxes(pc._h, out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
    return out


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_boxes_skip_pairs_and_never_an_inlier(f32):
    sc = T._scene(f32)
    lib = R.lib()
    snd = np.zeros(56, dtype=np.uint64)
    L.check(lib.rh_dbg_cls_soundness(sc.pc._h, sc.arr, T.B, C.byref(sc.cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    snt = np.zeros(8, dtype=np.uint64)
    L.check(lib.rh_dbg_cls_soundness_tiles(sc.pc._h, sc.arr, T.B, C.byref(sc.cp), snt.ctypes.data_as(C.POINTER(C.c_uint64))))
    ngroups = (T.N + 63) // 64
    for k, name in enumerate(("plane", "sphere", "cylinder")):
        s10 = snd[10 * k:10 * k + 10]
        assert int(s10[0]) == sum(x == name for x in sc.kinds) * ngroups
        assert int(s10[2] + s10[6] + s10[7] + s10[9]) == 0, (name, "group level", [int(v) for v in s10])
        assert int(snd[52 + k]) == 0, (name, "super-tile level")
        assert int(snt[4 + k]) == 0, (name, "tile level")
    pairs, skips = int(snd[20]), int(snd[21])
    # (not against the census's band pairs, out[40 + k]: it counts every pair of an exact-only candidate -- the cylinders with
    # R < eps here -- as one, and their boxes are skipped like any other's)
    assert int(snd[44 + 2]) > 0 and 0 < skips <= pairs - int(snd[44 + 2])
    # the same pairs on the host, with the kernel's own function over the library's group boxes
    gb = _group_boxes(sc.pc)
    assert gb.shape == (ngroups, 6)
    M = float(np.abs(sc.xyz.astype(np.float64)).max())
    host_skip = host_ball = 0
    for i, kind in enumerate(sc.kinds):
        if kind != "cylinder":
            continue
        skip, ball = np.zeros(ngroups, dtype=np.uint8), np.zeros(ngroups, dtype=np.uint8)
        L.check(lib.rh_dbg_cylbox(C.byref(sc.arr[i]), C.byref(sc.cp), M, 1.0, int(f32), gb.ctypes.data_as(C.POINTER(C.c_double)), ngroups,
                                  skip.ctypes.data_as(C.POINTER(C.c_uint8)), ball.ctypes.data_as(C.POINTER(C.c_uint8)), None))
        assert not (ball & ~skip).any()
        host_skip += int(skip.sum())
        host_ball += int(ball.sum())
    print("f32 %d: cylinder pairs %d, the box test skips %d (host, M as the largest coordinate: %d), the ball clauses alone %d; super-tile level %d, tile level %d"
          % (f32, pairs, skips, host_skip, host_ball, int(snd[48 + 2]), int(snt[2])))
    assert host_ball > 0
    assert skips >= host_ball
