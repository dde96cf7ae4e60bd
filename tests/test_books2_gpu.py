"""The culled score kernel with the two-bit books (csrc/score4_device.h, "Two-bit books"; score4.hip, score4_batch): the point
loops keep the top two bits of u' = 2 u per point, and the pairs with an undecided point hand those points to the exact test
straight from the owning lane's books -- no second evaluation of the classifier.  That changes how the undecided points are found,
never what a candidate counts: counts AND dense masks equal the oracle's bit for bit on the scene of books2_scene.py (8262
points: 129 full groups and a last one with 6 valid points; 192 candidates) -- points on both thresholds of every kind, groups whose 64
points are all undecided (exact-only candidates; a tile with an infinite coordinate), far more than 64 undecided points per
batch, a third of the points disabled -- with the super-tile lists on and off, one and three batches in flight, on a Float64 and
on a Float32 cloud."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist

import books2_scene as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_scene_holds_what_it_is_meant_to_hold(f32):
    sc = S.scene(f32)
    assert S.N // 64 == 129 and S.N % 64 == 6 and S.B == 192
    assert 0.3 < 1.0 - sc.en.mean() < 0.37 and sc.en[sc.i_inf]
    c = sc.ref_c
    # the exact copies hold their shapes' points in both orientations; the exact-only candidates with R <= eps nothing; the
    # plane given by a point 2^21 away holds points of the plane all the same; most of the jitters hold points
    assert min(c[0], c[2], c[4]) > 300 and min(c[1], c[3], c[5]) > 50, c[:14]
    assert c[6] == 0 and c[7] == 0 and c[8] == 0 and c[9] > 100, c[:14]
    assert (c[14:] > 0).sum() > 150


@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("lists", [1, 2], ids=["lists-on", "lists-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counts_and_masks_equal_the_oracle(f32, lists, in_flight):
    import torch
    sc = S.scene(f32)
    lib = R.lib()
    w = sc.ref_m.shape[1]
    batch = rdist.DeviceBatch(sc.pc, sc.arr, S.B)
    try:
        with R.option("st_cull", lists, cloud=sc.pc), R.option("batches_in_flight", in_flight, cloud=sc.pc):
            got_c, got_m = R.score_batch(sc.pc, sc.arr, sc.cp, want_masks=True)
            assert np.array_equal(got_c, sc.ref_c), (np.flatnonzero(got_c != sc.ref_c)[:8], got_c[got_c != sc.ref_c][:8], sc.ref_c[got_c != sc.ref_c][:8])
            assert np.array_equal(got_m, sc.ref_m)
            assert np.array_equal(R.score_batch(sc.pc, sc.arr, sc.cp), sc.ref_c)
            # the step bench.py times: device buffers, counts-only and mask batches taking turns, in_flight of them without a wait
            cn = [torch.full((S.B,), 7, dtype=torch.int32, device="cuda") for _ in range(2 * in_flight)]
            mk = [torch.zeros(S.B * w, dtype=torch.int64, device="cuda") for _ in range(in_flight)]
            torch.cuda.synchronize()
            for j in range(in_flight):
                L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), S.B, C.byref(sc.cp), C.c_void_p(cn[j].data_ptr()), None))
            L.check(lib.rh_cloud_sync(sc.pc._h))
            info = (C.c_int32 * 4)()
            L.check(lib.rh_score_launch_info(sc.pc._h, info))
            assert info[0] > 0 and info[1] == (1 if lists == 1 else 0) and info[3] == (S.N + 255) // 256, list(info)
            for j in range(in_flight):
                L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), S.B, C.byref(sc.cp), C.c_void_p(cn[in_flight + j].data_ptr()),
                                               C.c_void_p(mk[j].data_ptr())))
            L.check(lib.rh_cloud_sync(sc.pc._h))
            for j in range(2 * in_flight):
                assert np.array_equal(cn[j].cpu().numpy(), sc.ref_c), j
            for j in range(in_flight):
                assert np.array_equal(mk[j].cpu().numpy().view(np.uint64).reshape(S.B, w), sc.ref_m), j
    finally:
        batch.free()
