"""The event counters of the score launch (rh_dbg_s4_stats, diag build) on the scene of books2_scene.py, against the library of the
commit before the two-bit books.  The books change how the undecided points of a pair are found, not which points they are --
except that u = 1 exactly, undecided until now, is out (the margins say it is): per kind
  - the exact test accepts exactly as many points as it did (every inlier the classifier does not decide still reaches it);
  - no more undecided points than the parent's, and no fewer than the exact test accepts;
  - no more pairs in the wave-uniform loop over the pairs with an undecided point;
and full ring drains happen inside that loop (more than 64 undecided points per batch), and the census of the classifier's
decisions against the exact test (rh_dbg_cls_soundness) shows no violation.

PARENT: measured once with the parent commit's diag library on this very scene and batch, on an MI355X, before the kernel was
changed (one counts-only launch; the same with the super-tile lists on and off): (Float32 cloud, kind) -> second-pass pairs,
undecided points, points the exact test accepted.  Also in profiles/r12/experiments.txt."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import books2_scene as S

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

PARENT = {(False, "plane"): (340, 14405, 820), (False, "sphere"): (170, 9066, 405), (False, "cylinder"): (396, 13003, 1671),
          (True, "plane"): (364, 14429, 805), (True, "sphere"): (210, 9106, 431), (True, "cylinder"): (562, 13202, 1775)}


@pytest.mark.parametrize("lists", [1, 2], ids=["lists-on", "lists-off"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counters_against_the_parent_s(f32, lists):
    sc = S.scene(f32)
    got = S.counters(sc, lists)
    for kind in S.KINDS:
        g, (pairs, und, acc) = got[kind], PARENT[(f32, kind)]
        print("books2 counters", "f32" if f32 else "f64", "lists", lists, kind, g, "parent", (pairs, und, acc))
        assert g["exact_accepted"] == acc, (kind, g, acc)
        assert acc <= g["undecided_points"] <= und, (kind, g, und)
        assert g["second_pass_pairs"] <= pairs, (kind, g, pairs)
        assert g["ring_drains_full"] > 0, (kind, g)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_census_shows_no_violation(f32):
    sc = S.scene(f32)
    snd = np.zeros(56, dtype=np.uint64)
    L.check(R.lib().rh_dbg_cls_soundness(sc.pc._h, sc.arr, S.B, C.byref(sc.cp), snd.ctypes.data_as(C.POINTER(C.c_uint64))))
    for k, kind in enumerate(S.KINDS):
        s10 = snd[10 * k:10 * k + 10].astype(np.int64)
        print("census", "f32" if f32 else "f64", kind, s10.tolist())
        assert s10[3] == S.N * sum(1 for c in sc.cands if c[0] == kind)
        assert s10[2] == 0 and s10[6] == 0 and s10[7] == 0 and s10[9] == 0, s10
        assert s10[8] > 1000 and s10[4] > 0 and s10[5] > 0
        assert snd[52 + k] == 0
