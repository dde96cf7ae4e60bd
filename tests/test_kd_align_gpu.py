"""The aligned shape of the position tree of subset 1 (rh_set_option "kd_align"; csrc/rh_internal.h: kd_left_count, DESIGN.md
section 3): a node of more than 1024 points gives its left child a multiple of 1024 points, so the super-tiles of the candidate
lists and the blocks of the plane order are nodes of the tree.  The order of the points changes, what is computed must not: on
a cloud created with "kd_align" = 1 counts and masks equal the oracle's bit for bit -- with super-tile lists on and off, with the
plane order on and off, for rows of 2 / 4 / 16 chunks, with three batches in flight, after rh_invalidate has cleared a third of
the bits, and through rh_refit -- on a Float64 and a Float32 cloud; a cloud created with "kd_align" = 2 or by size (today's
shape at this size) gives the oracle's counts too.  Scene: kd_align_scene.py (9421 points, all four kinds)."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist

import kd_align_scene as S

pytestmark = pytest.mark.gpu


def _counts(s, batch, n=S.B, out=None):
    import torch
    out = torch.full((S.B,), -5, dtype=torch.int32, device="cuda") if out is None else out
    L.check(R.lib().rh_score_batch_dev(s.pc._h, batch.slice_ptr(0), n, C.byref(s.cp), C.c_void_p(out.data_ptr()), None))
    return out


def _read(s, out):
    L.check(R.lib().rh_cloud_sync(s.pc._h))
    return out.cpu().numpy()


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def sc(request):
    s = S.scene(request.param, 1)
    s.pc.enable_all()
    batch = rdist.DeviceBatch(s.pc, s.arr, S.B)
    yield s, batch
    batch.free()
    s.pc.enable_all()


def test_the_scene_is_what_the_tests_need(sc):
    s, _ = sc
    assert S.N == 9 * 1024 + 205 and 205 % 64 == 13
    kinds = [c[0] for c in s.cands]
    ref = np.asarray(s.ref_all)
    for k in S.KINDS:
        assert kinds.count(k) >= 24, k
        assert max(int(ref[i]) for i in range(S.B) if kinds[i] == k) > 300, k
    assert np.isnan(s.nrm[s.i_nan]).any()
    assert (np.asarray(s.ref_cut) <= ref).all() and int(np.asarray(s.ref_cut).sum()) < int(ref.sum())
    # exact-only planes of the batch: they count what an exact test of every point counts
    assert ref[12] > 300 and ref[13] > 300
    # the option is the process's, read at creation; a cloud refuses it
    assert R.get_option("kd_align") is None
    with pytest.raises(Exception):
        R.set_option("kd_align", 1, cloud=s.pc)


@pytest.mark.parametrize("plane_order", [1, 2], ids=["plane-order-on", "plane-order-off"])
def test_counts_equal_the_oracle_for_every_launch_form(sc, plane_order):
    s, batch = sc
    s.pc.enable_all()
    lib = R.lib()
    info = (C.c_int32 * 4)()
    with R.option("plane_order", plane_order, cloud=s.pc):
        for lists in (1, 2):
            for rows in (2, 4, 16):
                with R.option("st_cull", lists, cloud=s.pc), R.option("s4_rows", rows, cloud=s.pc):
                    got = _read(s, _counts(s, batch))
                    L.check(lib.rh_score_launch_info(s.pc._h, info))
                assert info[0] == rows and info[1] == (1 if lists == 1 else 0), (list(info), rows, lists)
                assert np.array_equal(got, s.ref_all), (plane_order, lists, rows, np.flatnonzero(got != s.ref_all)[:8])
        for n in (131, 1):          # a batch that ends inside a chunk, and one of a single candidate
            got = _read(s, _counts(s, batch, n))
            assert np.array_equal(got[:n], s.ref_all[:n]) and (got[n:] == -5).all(), n


@pytest.mark.parametrize("plane_order", [1, 2], ids=["plane-order-on", "plane-order-off"])
def test_counts_with_three_batches_in_flight(sc, plane_order):
    import torch
    s, batch = sc
    s.pc.enable_all()
    lib = R.lib()
    with R.option("batches_in_flight", 3, cloud=s.pc), R.option("st_cull", 1, cloud=s.pc), R.option("plane_order", plane_order, cloud=s.pc):
        ring = [torch.full((S.B,), -5, dtype=torch.int32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        sizes = [S.B, 131, S.B, 64, S.B, S.B, 77]
        for k, n in enumerate(sizes):
            _counts(s, batch, n, ring[k % 3])
        L.check(lib.rh_cloud_sync(s.pc._h))
        for k in range(len(sizes) - 3, len(sizes)):
            assert np.array_equal(ring[k % 3].cpu().numpy()[:sizes[k]], s.ref_all[:sizes[k]]), k


def test_counts_and_masks_after_invalidate_cleared_a_third_of_the_bits(sc):
    import torch
    s, batch = sc
    s.pc.enable_all()
    lib = R.lib()
    with R.option("batches_in_flight", 3, cloud=s.pc), R.option("plane_order", 1, cloud=s.pc):
        ring = [torch.full((S.B,), -5, dtype=torch.int32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for k in range(3):      # batches against every point, in flight when the bits go
            _counts(s, batch, S.B, ring[k])
        R.invalidate_indexes(s.pc, s.gone)
        L.check(lib.rh_cloud_sync(s.pc._h))
        for k in range(3):
            assert np.array_equal(ring[k].cpu().numpy(), s.ref_all), k
        for lists in (1, 2):
            with R.option("st_cull", lists, cloud=s.pc):
                for k in range(3):
                    _counts(s, batch, S.B, ring[k])
                L.check(lib.rh_cloud_sync(s.pc._h))
                for k in range(3):
                    assert np.array_equal(ring[k].cpu().numpy(), s.ref_cut), (lists, k)
    for plane_order in (1, 2):
        with R.option("plane_order", plane_order, cloud=s.pc):
            assert np.array_equal(_read(s, _counts(s, batch)), s.ref_cut), plane_order
            counts, masks = R.score_batch(s.pc, s.arr, s.cp, want_masks=True)
        assert np.array_equal(counts, s.ref_cut) and np.array_equal(masks, s.ref_cut_m), plane_order
    s.pc.enable_all()
    assert np.array_equal(_read(s, _counts(s, batch)), s.ref_all)


def test_mask_launches_return_what_the_oracle_returns(sc):
    s, _ = sc
    s.pc.enable_all()
    for lists in (1, 2):
        with R.option("st_cull", lists, cloud=s.pc):
            counts, masks = R.score_batch(s.pc, s.arr, s.cp, want_masks=True)
        assert np.array_equal(counts, s.ref_all), lists
        assert np.array_equal(masks, s.ref_all_m), lists


def test_refit_returns_the_oracle_s_points(sc):
    s, _ = sc
    s.pc.enable_all()
    for cut in (False, True):
        if cut:
            R.invalidate_indexes(s.pc, s.gone)
            s.oc.invalidate(s.gone)
        try:
            for i in (0, 6, 8, 10, 12, 57):          # a plane, the sphere, the cylinder, the cone, an exact-only plane, a jitter
                ex = R.refit(s.arr[i], s.pc, s.cp)
                assert np.array_equal(ex.inpoints, s.oc.refit(s.osh[i], s.op)), (cut, i)
                assert len(ex.inpoints) > 300
        finally:
            s.oc.enable_all()
            s.pc.enable_all()


@pytest.mark.parametrize("mode", [2, 0], ids=["never", "by-size"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_today_s_shape_and_the_default_give_the_oracle_s_counts(f32, mode):
    s = S.scene(f32, mode)
    s.pc.enable_all()
    batch = rdist.DeviceBatch(s.pc, s.arr, S.B)
    try:
        for lists in (1, 2):
            with R.option("st_cull", lists, cloud=s.pc), R.option("plane_order", 1, cloud=s.pc):
                assert np.array_equal(_read(s, _counts(s, batch)), s.ref_all), lists
        counts, masks = R.score_batch(s.pc, s.arr, s.cp, want_masks=True)
        assert np.array_equal(counts, s.ref_all) and np.array_equal(masks, s.ref_all_m)
    finally:
        batch.free()
