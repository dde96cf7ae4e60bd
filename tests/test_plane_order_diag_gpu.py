"""The plane order as the cloud holds it, the census of the score kernel's decisions over it, and the pairs the launch walks
(diag build; csrc/kdorder.hip; scene: plane_order_scene.py).

  - The order is a bijection inside every node of the position tree with at most 1024 points and the identity across them (the
    last node, with a partial group, permutes only its valid points); the table inverts it; the plane-order copy of the points
    is the leaf order read through the table.
  - Every plane-order group's binary32 box holds its points, every group's normal-cell mask holds its points' cells; the enabled
    words in plane order are the leaf order's bits read through the table.
  - rh_dbg_cls_soundness and its tile / normal-cell twins, which walk the plane candidates over the plane-order groups, show no
    violation.
  - The plane pairs that survive stage 1 of a counts-only launch are no more than with the parent commit's library; by size
    (the default: the scene is far below the 256 tiles from which the order is taken) the launch walks what the parent walked.
The order is forced on with "plane_order" = 1.

PARENT_PLANE_PAIRS: counter 7 of the plane kind (rh_dbg_s4_stats: surviving pairs) of ONE counts-only launch of the scene's batch
on the Float64 / Float32 cloud, super-tile lists on / off, measured once with the diag library of the commit before the plane
order on an MI355X (loaded through RH_LIB_PATH; also in profiles/r13/experiments.txt)."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist

import plane_order_scene as S

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

PARENT_PLANE_PAIRS = {(False, 1): 4634, (False, 2): 4634, (True, 1): 4634, (True, 2): 4634}


def surviving_pairs(sc, lists):
    """{kind: surviving pairs} of one counts-only launch of the scene's batch (every point enabled); its counts are checked"""
    import torch
    lib = R.lib()
    sc.pc.enable_all()
    batch = rdist.DeviceBatch(sc.pc, sc.arr, S.B)
    counts = torch.zeros(S.B, dtype=torch.int32, device="cuda")
    st = np.zeros(128, dtype=np.uint64)
    try:
        with R.option("st_cull", lists, cloud=sc.pc):
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 1, None))
            L.check(lib.rh_score_batch_dev(sc.pc._h, batch.slice_ptr(0), S.B, C.byref(sc.cp), C.c_void_p(counts.data_ptr()), None))
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 0, st.ctypes.data_as(C.POINTER(C.c_uint64))))
            L.check(lib.rh_dbg_s4_stats(sc.pc._h, 2, None))
    finally:
        batch.free()
    assert np.array_equal(counts.cpu().numpy(), sc.ref_all)
    return {name: int(st[24 * k + 7]) for k, name in enumerate(S.KINDS)}, {name: int(st[24 * k + 14]) for k, name in enumerate(S.KINDS)}


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_order_its_boxes_masks_and_enabled_words(f32):
    sc = S.scene(f32)
    sc.pc.enable_all()
    R.invalidate_indexes(sc.pc, sc.gone)          # so that the enabled words are not all ones
    po = S.plane_order(sc.pc)
    sc.pc.enable_all()
    s, src = po["s"], po["src"]
    assert s == S.N and po["ngroups"] == (S.N + 63) // 64 and po["nst"] == (S.N + 1023) // 1024 == 9
    # a bijection inside every node of the position tree, the identity across them
    nodes = S.tree_nodes(s)
    assert len(nodes) == 10 and nodes[0][0] == 0 and nodes[-1][1] == s and all(lo % 64 == 0 and 0 < hi - lo <= 1024 for lo, hi in nodes)
    assert (nodes[-1][1] - nodes[-1][0]) % 64 == 44
    for lo, hi in nodes:
        assert np.array_equal(np.sort(src[lo:hi]), np.arange(lo, hi)), (lo, hi)
    # the table inverts the order: reading the leaf order through it gives the plane-order copy, bit for bit (NaN included)
    assert np.array_equal(po["sub"][:, src].view(np.uint64), po["pl"].view(np.uint64))
    inv = np.empty(s, dtype=np.int64); inv[src] = np.arange(s)
    assert np.array_equal(po["pl"][:, inv].view(np.uint64), po["sub"].view(np.uint64))
    # the leaf order holds the cloud's points
    assert np.array_equal(np.sort(po["sub"][0]), np.sort(sc.xyz[:, 0].astype(np.float64)))
    assert not np.array_equal(src, np.arange(s))
    # every group's box holds its points: |p - c| <= h in binary64 on the binary32 numbers
    gb = po["gb32"].astype(np.float64)
    g = np.arange(s) // 64
    for k in range(3):
        assert (np.abs(po["pl"][k] - gb[g, k]) <= gb[g, 3 + k]).all(), k
    assert (gb[:, 3:6] >= 0).all() and np.isfinite(gb[:, :7]).all()
    # every group's mask holds its points' cells (the cell function is the library's own, rh_dbg_nsig; the NaN normal sets none)
    cells = np.zeros(s, dtype=np.int32)
    dirs = np.ascontiguousarray(po["pl"][3:6].T)
    L.check(R.lib().rh_dbg_nsig(None, C.byref(sc.cp), 0.0, 0.0, 0.0, 0, None, dirs.ctypes.data_as(C.POINTER(C.c_double)), s,
                                cells.ctypes.data_as(C.POINTER(C.c_int32))))
    assert (cells == -1).sum() == 1 and (cells >= -1).all()
    ok = cells >= 0
    word = po["gm32"][g[ok], cells[ok] >> 5]
    assert ((word >> (cells[ok] & 31).astype(np.uint32)) & 1).all()
    # ... and nothing else: the masks are exactly the OR of the cells
    want = np.zeros_like(po["gm32"])
    np.bitwise_or.at(want, (g[ok], cells[ok] >> 5), (np.uint32(1) << (cells[ok] & 31).astype(np.uint32)))
    assert np.array_equal(want, po["gm32"])
    # grouped by normals: fewer cells per group than the leaf order's groups have
    def cells_per_group(pts):
        c = np.zeros(s, dtype=np.int32)
        d = np.ascontiguousarray(pts[3:6].T)
        L.check(R.lib().rh_dbg_nsig(None, C.byref(sc.cp), 0.0, 0.0, 0.0, 0, None, d.ctypes.data_as(C.POINTER(C.c_double)), s,
                                    c.ctypes.data_as(C.POINTER(C.c_int32))))
        return np.mean([len(set(c[i:i + 64][c[i:i + 64] >= 0])) for i in range(0, s, 64)])
    cl, cp = cells_per_group(po["sub"]), cells_per_group(po["pl"])
    print("cells per group: leaf order %.2f, plane order %.2f" % (cl, cp))
    assert cp < cl
    # the enabled words went through the gather
    def bits(w):
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:s]
    bl, bp = bits(po["en_leaf"]), bits(po["en_plane"])
    assert 0.3 < 1.0 - bl.mean() < 0.37
    assert np.array_equal(bl[src], bp)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_in_plane_order_shows_no_violation(f32):
    sc = S.scene(f32)
    sc.pc.enable_all()
    lib = R.lib()
    u64p = C.POINTER(C.c_uint64)
    snd, tiles, nsig = np.zeros(56, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    with R.option("plane_order", 1, cloud=sc.pc):
        L.check(lib.rh_dbg_cls_soundness(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), snd.ctypes.data_as(u64p)))
        L.check(lib.rh_dbg_cls_soundness_tiles(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), tiles.ctypes.data_as(u64p)))
        L.check(lib.rh_dbg_cls_soundness_nsig(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), nsig.ctypes.data_as(u64p)))
    for k, kind in enumerate(S.KINDS):
        s10 = snd[10 * k:10 * k + 10].astype(np.int64)
        print("census", "f32" if f32 else "f64", kind, s10.tolist(), "tiles", int(tiles[k]), int(tiles[4 + k]))
        assert s10[0] == ((S.N + 63) // 64) * sum(1 for c in sc.cands if c[0] == kind)
        assert s10[3] == S.N * sum(1 for c in sc.cands if c[0] == kind)
        assert s10[2] == 0 and s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
        assert s10[8] > 1000 and s10[4] > 0 and s10[5] > 0 and s10[1] > 0
        assert snd[52 + k] == 0 and tiles[4 + k] == 0
    print("nsig", nsig.tolist())
    # (a super-tile of this scene holds 300 random normals: its mask is full and rules nothing out)
    assert nsig[0] > 0 and nsig[1] == 0 and nsig[3] == 0
    # the same census over the leaf order: the exact inliers are the same points, only grouped differently
    with R.option("plane_order", 2, cloud=sc.pc):
        leaf = np.zeros(56, dtype=np.uint64)
        L.check(lib.rh_dbg_cls_soundness(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), leaf.ctypes.data_as(u64p)))
    assert leaf[8] == snd[8] and leaf[3] == snd[3] and leaf[2] == 0
    assert np.array_equal(leaf[10:40], snd[10:40])          # the other kinds: untouched
    assert leaf[1] != snd[1]          # the planes did meet other groups
    bysize = np.zeros(56, dtype=np.uint64)
    L.check(lib.rh_dbg_cls_soundness(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), bysize.ctypes.data_as(u64p)))
    assert np.array_equal(bysize, leaf)


@pytest.mark.parametrize("lists", [1, 2], ids=["lists-on", "lists-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_plane_pairs_are_no_more_than_the_parent_s(f32, lists):
    sc = S.scene(f32)
    with R.option("plane_order", 1, cloud=sc.pc):
        pairs, with_count = surviving_pairs(sc, lists)
    with R.option("plane_order", 2, cloud=sc.pc):
        off, off_count = surviving_pairs(sc, lists)
    bysize, _ = surviving_pairs(sc, lists)
    assert bysize == off
    print("surviving pairs", "f32" if f32 else "f64", "lists", lists, pairs, "with a count", with_count, "order off", off, off_count,
          "parent", PARENT_PLANE_PAIRS[(f32, lists)])
    assert pairs["plane"] <= PARENT_PLANE_PAIRS[(f32, lists)]
    assert off["plane"] == PARENT_PLANE_PAIRS[(f32, lists)]          # "plane_order" = 2 is the parent's walk
    assert pairs["sphere"] == off["sphere"] and pairs["cylinder"] == off["cylinder"]
