"""CPU prototype: candidate lists per TILE (256 points) instead of per SUPER-TILE (1024 points) in front of the culled score
kernel (score4.hip, st_cull_kernel).  numpy only, no GPU: the cfg3 cloud of bench.py (synth, 10M points, subset 1 of 32 =
312 500 points), the k-d leaf order of cull_proto.py, the 4096 candidates of the bench, conservative box tests in binary64
(the kernel's box_skip32 in exact arithmetic, without its binary32 slack).  It reproduces the event counters the GPU leaves
(profiles/r5/s4_stats_cfg3.json, profiles/r6/experiments.txt): 24 645 chunk visits with super-tile lists and 15 369 with tile
lists, both exactly; 1 775 390 surviving pairs against the GPU's 1 775 511.

What the score launch walks, by the level its lists are made at (R = 64-candidate chunks per block row):

                                              super-tile lists      tile lists
    list entries                                       369 328         894 071
    stage-1 chunk visits per launch                     24 645          15 369   (-37.6 %)
    blocks with work, R = 8 / 12 / 16       3613 / 2617 / 2137   2469 / 1815 / 1455
    most chunks on one tile                                 58              56
    surviving pairs (the point-loop work)            1 775 390       1 774 447

(The estimate the round started from -- another prototype of the same idea -- read 896 606 / 15 406 / 2473, 1817, 1457 and the
same pairs in both columns.  The pairs differ a little because the cylinder's test bounds a box by its circumscribed sphere,
which is not monotone under box inclusion: a tile's box can rule out a candidate that one of its groups' boxes lets through.
Either way such a pair holds no inlier.)

A candidate that a tile's box rules out has no inlier in any of the tile's groups, so the counts are the same; what goes is the
stage-1 work on candidates that cannot meet any of the block's four groups.  Built and measured in round 6 and NOT kept: the
score launch lost 6.5 % of its instructions, the two-level list launch took half of that back, and the step did not move beyond
its run-to-run spread (HISTORY.md, profiles/r6/experiments.txt).  Not part of the product or the tests: a design aid
(DESIGN.md sections 4 and 11).

    python tools/proto/tile_lists.py [points [candidates]]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ransac_jl_amd import synth
from cull_proto import kd_order

EPS = 0.3
KINDS = ("plane", "sphere", "cylinder")


def union_boxes(lo, hi, k):
    """boxes of runs of k consecutive boxes (the last run may be short)"""
    n = (lo.shape[0] + k - 1) // k
    pad = n * k - lo.shape[0]
    lo = np.vstack([lo, np.full((pad, 3), np.inf)]).reshape(n, k, 3).min(1)
    hi = np.vstack([hi, np.full((pad, 3), -np.inf)]).reshape(n, k, 3).max(1)
    return lo, hi


def keeps(kind, V, lo, hi):
    """[candidates, boxes]: the box may hold an inlier of the candidate (the negation of box_skip32)"""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    if kind == "plane":
        p0, oz = V[:, 0:3], V[:, 3:6] / np.linalg.norm(V[:, 3:6], axis=1, keepdims=True)
        d = oz @ c.T - np.einsum("ij,ij->i", oz, p0)[:, None]
        return np.abs(d) <= np.abs(oz) @ h.T + EPS
    if kind == "sphere":
        o, R = V[:, 0:3], V[:, 3][:, None]
        a = np.abs(c[None, :, :] - o[:, None, :])
        dmin2 = (np.maximum(a - h[None], 0.0) ** 2).sum(2)
        dmax2 = ((a + h[None]) ** 2).sum(2)
        return (dmin2 <= (R + EPS) ** 2) & ~((R - EPS > 0) & (dmax2 < (R - EPS) ** 2))
    ax, c0, R = V[:, 0:3], V[:, 3:6], V[:, 6][:, None]
    t = c[None, :, :] - c0[:, None, :]
    q = t - np.einsum("cbk,ck->cb", t, ax)[:, :, None] * ax[:, None, :]
    rho = np.linalg.norm(q, axis=2)
    hr = np.linalg.norm(h, axis=1)[None, :]
    return (rho <= R + EPS + hr) & ~((R - EPS - hr > 0) & (rho < R - EPS - hr))


def chunked(kind, V, lo, hi, step=128):
    return np.vstack([keeps(kind, V[i:i + step], lo, hi) for i in range(0, V.shape[0], step)]) if V.shape[0] else np.zeros((0, lo.shape[0]), bool)


def main():
    npts = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    ncand = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    t0 = time.time()
    prim = ["plane"] * 16 + ["sphere"] * 12 + ["cylinder"] * 12
    xyz, _nrm, truth = synth.make_cloud(npts, prim, 0.30, seed=3)
    subs = synth.make_subsets(npts, 32, seed=3)
    P = xyz[subs[0] - 1]
    t1 = time.time()
    P = P[kd_order(P)]
    s = P.shape[0]
    ng = (s + 63) // 64
    pad = np.vstack([P, np.repeat(P[-1:], ng * 64 - s, axis=0)]).reshape(ng, 64, 3)
    glo, ghi = pad.min(1), pad.max(1)
    tlo, thi = union_boxes(glo, ghi, 4)
    slo, shi = union_boxes(glo, ghi, 16)
    nt = tlo.shape[0]
    cands = synth.jittered_candidates(truth, ncand, seed=0)
    tile_of_group = np.arange(ng) // 4
    st_of_tile = np.arange(nt) // 4
    n_st = np.zeros((nt, 3), dtype=np.int64)     # candidates a tile's blocks walk: its super-tile's list / its own
    n_tl = np.zeros((nt, 3), dtype=np.int64)
    pairs = [0, 0]
    for k, kind in enumerate(KINDS):
        V = np.array([np.asarray(v, dtype=float) for (kk, _o, v) in cands if kk == kind])
        if V.size == 0:
            continue
        ks, kt, kg = chunked(kind, V, slo, shi), chunked(kind, V, tlo, thi), chunked(kind, V, glo, ghi)
        kt &= ks[:, st_of_tile]                  # the tile level only sees the super-tile's survivors
        n_st[:, k] = ks.sum(0)[st_of_tile]
        n_tl[:, k] = kt.sum(0)
        pairs[0] += int((kg & ks[:, st_of_tile][:, tile_of_group]).sum())
        pairs[1] += int((kg & kt[:, tile_of_group]).sum())
    rows = []
    for n in (n_st, n_tl):
        ch = (n + 63) // 64
        per_tile = ch.sum(1)
        rows.append(dict(entries=int(n[::4].sum()) if n is n_st else int(n.sum()), visits=int(ch.sum()),
                         blocks=[int(((per_tile + R - 1) // R).sum()) for R in (8, 12, 16)], most=int(per_tile.max())))
    a, b = rows
    print("%d subset points, %d groups, %d tiles, %d candidates (cloud %.0f s, lists %.0f s)" % (s, ng, nt, len(cands), t1 - t0, time.time() - t1))
    print("%-42s %20s %20s" % ("", "super-tile lists", "tile lists"))
    print("%-42s %20d %20d" % ("list entries", a["entries"], b["entries"]))
    print("%-42s %20d %20d   (%+.1f %%)" % ("stage-1 chunk visits per launch", a["visits"], b["visits"], 100.0 * (b["visits"] - a["visits"]) / max(1, a["visits"])))
    print("%-42s %20s %20s" % ("blocks with work, R = 8 / 12 / 16", " / ".join(map(str, a["blocks"])), " / ".join(map(str, b["blocks"]))))
    print("%-42s %20d %20d" % ("most chunks on one tile", a["most"], b["most"]))
    print("%-42s %20d %20d" % ("surviving pairs (the point-loop work)", pairs[0], pairs[1]))


if __name__ == "__main__":
    main()
