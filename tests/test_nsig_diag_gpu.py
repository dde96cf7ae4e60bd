"""The census of the normal-cell masks (diag build: rh_dbg_cls_soundness_nsig, csrc/score4_diag.hip sound_one): over every (plane
candidate, 64-point group) pair of the hostile batch of test_nsig_gpu.py, the pairs that the group's mask and the super-tile's
mask rule out, and of those the pairs that hold an exact inlier -- the masks must skip something, and never an inlier."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import test_nsig_gpu as T

pytestmark = [pytest.mark.gpu, pytest.mark.diag]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("alpha", T.ALPHAS)
def test_masks_skip_pairs_and_never_an_inlier(alpha, f32):
    sc = T._scene("mixed", f32)
    arr, cp, ref_c, _, kinds = sc.cases[alpha]
    out = np.zeros(4, dtype=np.uint64)
    L.check(R.lib().rh_dbg_cls_soundness_nsig(sc.pc._h, arr, T.B, C.byref(cp), out.ctypes.data_as(C.POINTER(C.c_uint64))))
    snd = np.zeros(56, dtype=np.uint64)
    L.check(R.lib().rh_dbg_cls_soundness(sc.pc._h, arr, T.B, C.byref(cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    g_skips, g_viol, st_skips, st_viol = (int(v) for v in out)
    pairs = int(snd[0])
    print("alpha %g f32 %d: plane pairs %d, group-mask skips %d (violations %d), super-tile-mask skips %d (violations %d), pairs with an exact inlier %d"
          % (alpha, f32, pairs, g_skips, g_viol, st_skips, st_viol, int(snd[44])))
    assert pairs == sum(k == "plane" for k in kinds) * ((T.N + 63) // 64) and int(snd[44]) > 0
    assert g_viol == 0 and st_viol == 0
    assert st_skips <= g_skips <= pairs - int(snd[44])
    if alpha < 90.0:
        assert g_skips > 0        # (a super-tile of 1024 points with 30 % outliers holds every cell: its mask may well skip nothing here)
    else:
        assert g_skips == 0 and st_skips == 0        # cos(alpha) < 0: every mask is all ones
