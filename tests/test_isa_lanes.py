"""Build-time invariants of the score kernel's LIST instantiations, checked on the gfx950 ISA hipcc emits (no GPU needed).

A performance tripwire like test_isa_invariants.py, not a correctness test: the counts-only list launches -- the timed step -- keep
their scalar values in scalar registers.  Until round 16 their four per-kind bodies took their arguments from a by-value struct
that the compiler loaded in the prologue and kept live across all four: 37 to 52 scalar registers were spilled into the lanes of a
vector register, 30 v_writelane_b32 per wave up front and a v_readlane_b32 wherever one was used.  Each body now reads its
arguments from the kernarg segment where it starts (score4.hip, RH_S4_BODY).  Held here:
  - every counts-only list instantiation within the plain ones' bounds: at most 12 spilled scalar registers, 72 vector registers,
    2 spilled vector registers;
  - with tools/isa_account.py's region cut, rows of 16 and 12 with lists: no v_writelane_b32 in the prologue, and in each kind's
    batch region no more lane moves than the plain instantiation's same region (those that remain are the algorithm's own: the
    owner's undecided word read by the pair loop)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_invariants import ROOT, _kernels, isa   # noqa: E402,F401  (the module's fixture: the ISA, compiled once per module)

KINDS = ("plane", "sphere", "cylinder", "cone")


def test_counts_only_list_instantiations_spill_no_scalar_registers(isa):
    ks = _kernels(isa)
    for R in (2, 4, 8, 12, 16):
        for f32 in (False, True):
            v = ks[(R, False, f32, False, True)]
            print("score4_kernel<%d, false, %s, false, true>" % (R, str(f32).lower()), v)
            assert v["sgpr_spill"] <= 12 and v["vgpr"] <= 72 and v["vgpr_spill"] <= 2, (R, f32, v)
    for key, v in sorted(ks.items()):        # the mask-writing and row-walking forms: reported, bounded by test_isa_invariants.py
        if key[1] or key[3]:
            print("score4_kernel<%d, %s, %s, %s, %s>" % tuple([key[0]] + [str(b).lower() for b in key[1:]]), v)


@pytest.mark.parametrize("rows", [16, 12])
def test_list_launch_moves_no_scalars_through_lanes(isa, rows):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_account as ia

    def lane_moves(lists):
        _sym, text = ia.kernel_text(isa, rows, lists=lists)
        reg = ia.regions(ia.parse_blocks(text), rows)
        count = lambda name, ops: sum(1 for b in reg[name] for op in b.ins if op.startswith(ops))
        out = {"prologue": count("prologue", ("v_writelane_b32",))}
        for kind in KINDS:
            out["batch_" + kind] = count("batch_" + kind, ("v_readlane_b32", "v_writelane_b32"))
        return out
    plain, lst = lane_moves(False), lane_moves(True)
    print("lane moves, rows of", rows, "plain", plain, "lists", lst)
    assert lst["prologue"] == 0, lst
    for kind in KINDS:
        assert lst["batch_" + kind] <= plain["batch_" + kind], (kind, lst, plain)
