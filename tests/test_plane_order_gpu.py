"""The plane order (csrc/kdorder.hip; rh_set_option "plane_order"): counts-only launches of the culled score
kernel walk their plane candidates over a second internal order of subset 1.  The culling rules hold for any grouping of the
points and a count is a sum over points, so the counts must be the oracle's bit for bit with the order on (1: whenever possible;
the scene is below the size from which the default takes it), off (2) and by size (0) -- with and without super-tile lists, for every row length, on a Float64 and a Float32 cloud, with three batches in flight, and after
rh_invalidate has cleared a third of the bits (the enabled words reach the plane order through a gather).  Launches that write
masks never take the order: they return what the oracle returns.  Scene: plane_order_scene.py."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist

import plane_order_scene as S

pytestmark = pytest.mark.gpu


def _counts(sc, batch, n=S.B, out=None):
    import torch
    out = torch.full((S.B,), -5, dtype=torch.int32, device="cuda") if out is None else out
    L.check(R.lib().rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), n, C.byref(sc.cp), C.c_void_p(out.data_ptr()), None))
    return out


def _read(sc, out):
    """the counts a launch left in `out` (the launches run on the cloud's own stream: wait for it first)"""
    L.check(R.lib().rh_cloud_sync(sc.pc._h))
    return out.cpu().numpy()


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def sc(request):
    s = S.scene(request.param)
    s.pc.enable_all()
    batch = rdist.DeviceBatch(s.pc, s.arr, S.B)
    yield s, batch
    batch.free()
    s.pc.enable_all()


def test_the_scene_is_what_the_tests_need(sc):
    s, _ = sc
    kinds = [c[0] for c in s.cands]
    assert kinds.count("plane") >= 64 and kinds.count("sphere") >= 32 and kinds.count("cylinder") >= 32
    ref = np.asarray(s.ref_all)
    for k in S.KINDS:
        assert max(int(ref[i]) for i in range(S.B) if kinds[i] == k) > 300, k
    assert np.isnan(s.nrm[s.i_nan]).any()
    assert (np.asarray(s.ref_cut) <= ref).all() and int(np.asarray(s.ref_cut).sum()) < int(ref.sum())
    if not s.f32:   # the oracle's batch entry is its orc_scorecandidate, candidate by candidate
        osh = S.orc_shapes(s.arr, S.B)
        for i in (0, 1, 6, 8, 10, 11, 57):
            assert s.oc.scorecandidate(osh[i], s.op)[0] == ref[i]


@pytest.mark.parametrize("plane_order", [1, 2, 0], ids=["order-on", "order-off", "order-by-size"])
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
        # a batch that ends inside a chunk, and one of a single candidate
        for n in (131, 1):
            got = _read(s, _counts(s, batch, n))
            assert np.array_equal(got[:n], s.ref_all[:n]) and (got[n:] == -5).all(), n


def test_counts_with_three_batches_in_flight(sc):
    import torch
    s, batch = sc
    s.pc.enable_all()
    lib = R.lib()
    with R.option("batches_in_flight", 3, cloud=s.pc), R.option("st_cull", 1, cloud=s.pc), R.option("plane_order", 1, cloud=s.pc):
        ring = [torch.full((S.B,), -5, dtype=torch.int32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        sizes = [S.B, 131, S.B, 64, S.B, S.B, 77]
        for k, n in enumerate(sizes):
            _counts(s, batch, n, ring[k % 3])
        L.check(lib.rh_cloud_sync(s.pc._h))
        for k in range(len(sizes) - 3, len(sizes)):
            assert np.array_equal(ring[k % 3].cpu().numpy()[:sizes[k]], s.ref_all[:sizes[k]]), k


@pytest.mark.parametrize("in_flight", [1, 3])
def test_counts_after_invalidate_cleared_a_third_of_the_bits(sc, in_flight):
    import torch
    s, batch = sc
    s.pc.enable_all()
    lib = R.lib()
    with R.option("batches_in_flight", in_flight, cloud=s.pc), R.option("plane_order", 1, cloud=s.pc):
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
        for other in (2, 0):
            R.set_option("plane_order", other, cloud=s.pc)
            assert np.array_equal(_read(s, _counts(s, batch)), s.ref_cut), other
    s.pc.enable_all()
    assert np.array_equal(_read(s, _counts(s, batch)), s.ref_all)


@pytest.mark.parametrize("cut", [False, True], ids=["all-enabled", "a-third-cleared"])
def test_mask_launches_return_what_the_oracle_returns(sc, cut):
    s, _ = sc
    s.pc.enable_all()
    if cut:
        R.invalidate_indexes(s.pc, s.gone)
    ref_c, ref_m = (s.ref_cut, s.ref_cut_m) if cut else (s.ref_all, s.ref_all_m)
    for plane_order in (1, 2):
        with R.option("plane_order", plane_order, cloud=s.pc):
            counts, masks = R.score_batch(s.pc, s.arr, s.cp, want_masks=True)
        assert np.array_equal(counts, ref_c), plane_order
        assert np.array_equal(masks, ref_m), plane_order
    s.pc.enable_all()
