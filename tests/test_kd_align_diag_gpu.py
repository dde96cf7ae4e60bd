"""The aligned position tree as the cloud holds it (diag build; "kd_align" = 1; scene: kd_align_scene.py, 9421 points: nine nodes
of 1024 points and one of 205).

  - rh_dbg_plane_order's table: every plane-order position in [1024 k, 1024 k + 1024) comes from a leaf-order position of the same
    range -- the plane order's blocks are the super-tiles, so super-tile k of both orders is one point set.  (With today's shape
    the same scene's table crosses those borders: the test would see it.)
  - rh_dbg_cls_soundness and its tile, super-tile and normal-cell twins count no violation, with the plane order on and off.
  - The order made on the host (RH_KD_HOST=1: the nth_element recursion of cloud.hip takes its splits from the same
    kd_left_count) gives the same counts and culls alike: the share of (candidate, group) pairs the box tests skip within
    0.02 of the device order's, the bound tests/test_parity_gpu.py holds the two to.

No constants on pair counts: on ten super-tiles alignment need not shorten anything."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import kd_align_scene as S
import plane_order_scene as P

pytestmark = [pytest.mark.gpu, pytest.mark.diag]
U64P = C.POINTER(C.c_uint64)


def _census(s, plane_order):
    lib = R.lib()
    snd, tiles, nsig = np.zeros(56, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    with R.option("plane_order", plane_order, cloud=s.pc):
        L.check(lib.rh_dbg_cls_soundness(s.pc._h, s.arr, S.B, C.byref(s.cp), snd.ctypes.data_as(U64P)))
        L.check(lib.rh_dbg_cls_soundness_tiles(s.pc._h, s.arr, S.B, C.byref(s.cp), tiles.ctypes.data_as(U64P)))
        L.check(lib.rh_dbg_cls_soundness_nsig(s.pc._h, s.arr, S.B, C.byref(s.cp), nsig.ctypes.data_as(U64P)))
    return snd.astype(np.int64), tiles.astype(np.int64), nsig.astype(np.int64)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_super_tile_k_of_both_orders_is_one_point_set(f32):
    s = S.scene(f32, 1)
    po = P.plane_order(s.pc)
    src = po["src"]
    assert po["s"] == S.N and po["nst"] == 10 and po["ngroups"] == 148
    assert np.array_equal(src // 1024, np.arange(S.N) // 1024)
    for k in range(10):
        lo, hi = 1024 * k, min(S.N, 1024 * k + 1024)
        assert np.array_equal(np.sort(src[lo:hi]), np.arange(lo, hi)), k
    assert not np.array_equal(src, np.arange(S.N))
    assert np.array_equal(po["sub"][:, src].view(np.uint64), po["pl"].view(np.uint64))
    assert np.array_equal(np.sort(po["sub"][0]), np.sort(s.xyz[:, 0].astype(np.float64)))
    # today's shape on the same points: its nodes are not the super-tiles, and the table shows it
    old = P.plane_order(S.scene(f32, 2).pc)["src"]
    assert not np.array_equal(old // 1024, np.arange(S.N) // 1024)
    for lo, hi in P.tree_nodes(S.N):
        assert np.array_equal(np.sort(old[lo:hi]), np.arange(lo, hi)), (lo, hi)


@pytest.mark.parametrize("plane_order", [1, 2], ids=["plane-order-on", "plane-order-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_shows_no_violation(f32, plane_order):
    s = S.scene(f32, 1)
    s.pc.enable_all()
    snd, tiles, nsig = _census(s, plane_order)
    for k, kind in enumerate(S.KINDS):
        s10 = snd[10 * k:10 * k + 10]
        nk = sum(1 for c in s.cands if c[0] == kind)
        print("census", "f32" if f32 else "f64", kind, s10.tolist(), "tiles", int(tiles[k]), int(tiles[4 + k]), "st", int(snd[48 + k]), int(snd[52 + k]))
        assert s10[0] == ((S.N + 63) // 64) * nk and s10[3] == S.N * nk
        assert s10[2] == 0 and s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
        assert s10[8] > 300 and s10[1] > 0
        assert snd[52 + k] == 0 and tiles[4 + k] == 0
    print("nsig", nsig.tolist())
    assert nsig[0] > 0 and nsig[1] == 0 and nsig[3] == 0


def test_the_host_s_order_gives_the_same_counts_and_culls_alike(monkeypatch):
    dev = S.scene(False, 1)
    dev.pc.enable_all()
    monkeypatch.setenv("RH_KD_HOST", "1")
    host = S.Scene(False, 1)
    monkeypatch.delenv("RH_KD_HOST")
    share = {}
    for name, s in (("device", dev), ("host", host)):
        counts, masks = R.score_batch(s.pc, s.arr, s.cp, want_masks=True)
        assert np.array_equal(counts, dev.ref_all) and np.array_equal(masks, dev.ref_all_m), name
        snd, tiles, nsig = _census(s, 1)
        out = snd[:40].reshape(4, 10)
        assert out[:, [2, 6, 7, 9]].sum() == 0 and snd[52:56].sum() == 0 and tiles[4:8].sum() == 0 and nsig[1] == 0 and nsig[3] == 0, name
        share[name] = out[:, 1].sum() / out[:, 0].sum()
    print("share of pairs the box tests skip", share)
    # the host's tree has the aligned shape too: its plane-order blocks are the super-tiles
    src = P.plane_order(host.pc)["src"]
    assert np.array_equal(src // 1024, np.arange(S.N) // 1024)
    assert abs(share["host"] - share["device"]) < 0.02, share
