"""The undecided points of a pair read from the books in place (csrc/score4_device.h, "Books in place"; score4.hip,
score4_batch): the counts-only launches no longer bring the undecided bits of a pair into point order -- the pair's 64-bit word
keeps the books' own bit order and the lane that stands for bit L queues point pi(L).  That changes the order of the ring's
entries, never which points are undecided nor what a candidate counts.

The scene is the one of books2_scene.py (threshold points of every kind, groups whose enabled points are all undecided, far more
than 64 undecided points per batch, a third of the points disabled, a last group of 6 valid points) with two additions: the last
candidate is replaced by one more exact-only one (a sphere with R = eps / 2: cls_make flags its record with a NaN), and a second
cloud over the same points whose subset stops 41 points early, so that its last group holds 29 points.

Counts equal the oracle's with the lists on and off, rows of 2 and 16 chunks, one and three batches in flight, on a Float64 and
a Float32 cloud.  In the diag build the launch's event counters are EQUAL to the parent commit's: nothing in the change may alter
which points are undecided, how many pairs hold one, what the exact test accepts or how many pairs end with a count.

PARENT: measured once with the parent commit's diag library on this very scene and batch, on an MI355X, before the kernel was
changed (one counts-only launch; the same with the super-tile lists on and off, and from launch to launch): (Float32 cloud, kind)
-> second-pass pairs, undecided points, points the exact test accepted, pairs with a count.  Also in profiles/r16/experiments.txt.

The number of ring drains is NOT a constant of the scene, in the parent either: a batch with U undecided points drains its ring
ceil(U / 64) times, and which pairs share a batch follows the order in which the block's waves append their survivors to the pair
list (an atomic add per chunk), which differs from launch to launch.  Measured with the parent's library, four launches each
(full + final): plane 246 / 245 / 245 / 245 (Float32 cloud 257 / 255 / 255 / 255), sphere 159 / 158 / 158 / 158 (166 / 167 / 167 / 167),
cylinder 230 / 228 / 228 / 228 (231 / 230 / 230 / 230).  What holds for every order is held here instead: with U the kind's undecided
points and b its batches, ceil(U / 64) <= full + final <= floor(U / 64) + b, and full drains do happen."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist
from oracle import oracle as orc

import books2_scene as S

SHORT = S.N - 41          # 128 full groups and a last one of 29 points
FIELDS = {"batches": 8, "second_pass_pairs": 9, "undecided_points": 10, "ring_drains_full": 11, "ring_drains_final": 12, "exact_accepted": 13,
          "pairs_with_count": 14}

PARENT = {(False, "plane"): (340, 14405, 820, 2229), (False, "sphere"): (170, 9066, 405, 1545), (False, "cylinder"): (391, 12820, 1648, 1711),
          (True, "plane"): (364, 14429, 805, 2222), (True, "sphere"): (210, 9106, 431, 1545), (True, "cylinder"): (552, 13013, 1748, 1709)}


class Ext:
    """the scene with the extra exact-only candidate, and its twin over the short subset; the references once per scene"""

    def __init__(self, f32):
        import bench
        sc = S.scene(f32)
        self.sc, self.f32, self.cp, self.op = sc, f32, sc.cp, sc.op
        self.cands = list(sc.cands)
        self.cands[-1] = ("sphere", True, list(S.SPH["o"]) + [S.EPS / 2])
        self.arr = bench.shapes_to_c(R, L, self.cands)
        if f32:
            for i in range(S.B):
                R.lib().rh_shape_finalize_f32(C.byref(self.arr[i]))
        self.pc, self.oc = sc.pc, sc.oc          # (enabled words set by the scene)
        sub = np.arange(1, SHORT + 1, dtype=np.int64)
        bits = np.zeros(((S.N + 63) // 64) * 64, dtype=np.uint8); bits[:S.N] = sc.en
        with R.option("score_path", "groups"):
            if f32:
                self.pc2 = R.RANSACCloud(sc.pc.vertices32, sc.pc.normals32, [sub], force_eltype=np.float32)
                self.oc2 = orc.Cloud32(sc.pc.vertices32, sc.pc.normals32, sub)
            else:
                self.pc2 = R.RANSACCloud(sc.pc.vertices, sc.pc.normals, [sub])
                self.oc2 = orc.Cloud(sc.pc.vertices, sc.pc.normals, sub)
        self.pc2.set_enabled(sc.en)
        self.oc2.set_enabled(np.packbits(bits, bitorder="little").view(np.uint64))
        self.ref = self.oc.score_batch(S.orc_shapes(self.arr, S.B), self.op)
        self.ref2 = self.oc2.score_batch(S.orc_shapes(self.arr, S.B), self.op)
        for r in (self.ref, self.ref2):
            r.setflags(write=False)


_EXT = {}


def ext(f32):
    if f32 not in _EXT:
        _EXT[f32] = Ext(f32)
    return _EXT[f32]


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("rows", [2, 16])
@pytest.mark.parametrize("lists", [1, 2], ids=["lists-on", "lists-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counts_equal_the_oracle(f32, lists, rows, in_flight):
    import torch
    e = ext(f32)
    lib = R.lib()
    assert e.ref[-1] == 0 and e.ref.max() > 300 and not np.array_equal(e.ref, e.ref2)
    for pc, ref in ((e.pc, e.ref), (e.pc2, e.ref2)):
        batch = rdist.DeviceBatch(pc, e.arr, S.B)
        try:
            with R.option("st_cull", lists, cloud=pc), R.option("s4_rows", rows, cloud=pc), R.option("batches_in_flight", in_flight, cloud=pc):
                assert np.array_equal(R.score_batch(pc, e.arr, e.cp), ref)
                # the step bench.py times: device buffers, in_flight counts-only batches without a wait between them
                cn = [torch.full((S.B,), 7, dtype=torch.int32, device="cuda") for _ in range(in_flight)]
                torch.cuda.synchronize()
                for j in range(in_flight):
                    L.check(lib.rh_score_batch_dev(pc._h, batch.slice_ptr(0), S.B, C.byref(e.cp), C.c_void_p(cn[j].data_ptr()), None))
                L.check(lib.rh_cloud_sync(pc._h))
                info = (C.c_int32 * 4)()
                L.check(lib.rh_score_launch_info(pc._h, info))
                assert info[0] == rows and info[1] == (1 if lists == 1 else 0), list(info)
                for j in range(in_flight):
                    got = cn[j].cpu().numpy()
                    assert np.array_equal(got, ref), (j, np.flatnonzero(got != ref)[:8], got[got != ref][:8], ref[got != ref][:8])
        finally:
            batch.free()


def counters(e, lists):
    """the event counters (rh_dbg_s4_stats, diag build) of ONE counts-only launch on the scene: {kind: {field: n}}"""
    import torch
    lib = R.lib()
    batch = rdist.DeviceBatch(e.pc, e.arr, S.B)
    counts = torch.zeros(S.B, dtype=torch.int32, device="cuda")
    st = np.zeros(128, dtype=np.uint64)
    try:
        with R.option("st_cull", lists, cloud=e.pc):
            L.check(lib.rh_dbg_s4_stats(e.pc._h, 1, None))
            L.check(lib.rh_score_batch_dev(e.pc._h, batch.slice_ptr(0), S.B, C.byref(e.cp), C.c_void_p(counts.data_ptr()), None))
            L.check(lib.rh_dbg_s4_stats(e.pc._h, 0, st.ctypes.data_as(C.POINTER(C.c_uint64))))
            L.check(lib.rh_dbg_s4_stats(e.pc._h, 2, None))
    finally:
        batch.free()
    assert np.array_equal(counts.cpu().numpy(), e.ref)
    return {name: {f: int(st[24 * k + i]) for f, i in FIELDS.items()} for k, name in enumerate(S.KINDS)}


@pytest.mark.gpu
@pytest.mark.diag
@pytest.mark.parametrize("lists", [1, 2], ids=["lists-on", "lists-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counters_equal_the_parent_s(f32, lists):
    e = ext(f32)
    # the added candidate is exact-only by its record: the flag of what cls_make builds for it is a NaN
    rec = np.zeros(16, dtype=np.float32)
    one = np.zeros((1, 3))
    u = np.zeros(1, dtype=np.float32)
    _fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.check(R.lib().rh_dbg_cls_u2(C.byref(e.arr[S.B - 1]), C.byref(e.cp), 100.0, 1.0, int(f32), 1, one.ctypes.data_as(_dp), one.ctypes.data_as(_dp),
                                  u.ctypes.data_as(_fp), u.ctypes.data_as(_fp), rec.ctypes.data_as(_fp)))
    assert np.isnan(rec[15])
    got = counters(e, lists)
    for kind in S.KINDS:
        g = got[kind]
        mine = (g["second_pass_pairs"], g["undecided_points"], g["exact_accepted"], g["pairs_with_count"])
        print("books in place counters", "f32" if f32 else "f64", "lists", lists, kind, g, "parent", PARENT[(f32, kind)])
        assert mine == PARENT[(f32, kind)], (kind, g, PARENT[(f32, kind)])
        drains, und = g["ring_drains_full"] + g["ring_drains_final"], g["undecided_points"]
        assert (und + 63) // 64 <= drains <= und // 64 + g["batches"], (kind, g)
        assert g["ring_drains_full"] > 0, (kind, g)


@pytest.mark.gpu
@pytest.mark.diag
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_shows_no_violation(f32):
    e = ext(f32)
    snd = np.zeros(56, dtype=np.uint64)
    L.check(R.lib().rh_dbg_cls_soundness(e.pc._h, e.arr, S.B, C.byref(e.cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    for k, kind in enumerate(S.KINDS):
        s10 = snd[10 * k:10 * k + 10].astype(np.int64)
        print("census", "f32" if f32 else "f64", kind, s10.tolist())
        assert s10[3] == S.N * sum(1 for c in e.cands if c[0] == kind)
        assert s10[2] == 0 and s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
        assert snd[52 + k] == 0
