#!/usr/bin/env python3
"""CPU prototype (numpy, the kernel's culling rules without their slack) behind DESIGN.md section 3, "aligned shape": what do
the score launch's candidate lists cost when the super-tiles -- runs of 1024 consecutive points of the internal order, 16 groups
of 64 -- are nodes of the position k-d tree instead of straddling two or three of them?

Tree shapes (the left child of a node of cnt points; csrc/rh_internal.h, kd_left_count):
  today    ((cnt / 64 + 1) / 2) * 64 all the way down: at cfg3 the tree passes 1024 points in 512 nodes of 576 .. 640
  aligned  ((ceil(cnt / 1024) + 1) / 2) * 1024 above 1024 points, today's rule below: 305 nodes of exactly 1024 points and one
           of 180 at cfg3; super-tile k is tree node k
Under both, the leaf order is the tree down to 64 points, and the plane order (csrc/kdorder.hip) cuts every node of at most
1024 points by a k-d tree on the NORMALS (widest axis, median split, left child a multiple of 64) down to 64 points.

What is counted, per kind (planes over the plane order, spheres and cylinders over the leaf order):
  listed      (candidate, super-tile) pairs the list launch keeps: the kind's box test on the super-tile's box, for planes also
              the super-tile's normal-cell mask
  box-tested  candidates taken through the group tests by the score launch's blocks: a block is one 256-point tile, it walks
              its super-tile's list, so every listed candidate is tested once per tile of the super-tile
  visits      chunk visits: a block takes a kind's list in chunks of 64 candidates
  pairs       (candidate, group) pairs that survive: listed, and the group's own box (planes: and cells; cylinders: and the
              support clause) lets the candidate through
Every STRIDE-th of the 4096 bench candidates is taken and the counts are scaled by STRIDE (a list is STRIDE times as long), so
the figures stand next to the counters of tools/s4_stats.py; sphere and cylinder figures are off by up to a quarter in absolute
terms (no binary32 slack here, a coarser cylinder clause): read the ratios.  Cone candidates (cfg5) are not modelled.
Tests as in plane_order_proto.py.  eps = 0.3, alpha = 5 degrees.
    python tools/proto/kd_align_proto.py [cfg3|cfg5|cfg2] [points] [stride]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ransac_jl_amd import synth

np.seterr(all="ignore")
cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
prim, n, seed, outl, scanner = ["plane"] * 16 + ["sphere"] * 12 + ["cylinder"] * 12, 10_000_000, 3, 0.30, None
if cfg == "cfg2":
    prim, n, seed, outl = ["plane", "plane", "sphere", "sphere", "cylinder", "cylinder"], 1_000_000, 2, 0.0
if cfg == "cfg5":
    prim, n, seed, scanner = prim + ["cone"] * 8, 50_000_000, 5, [synth.BOX / 2] * 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else n
STRIDE = int(sys.argv[3]) if len(sys.argv) > 3 else 4
EPS, ALPHA, RCELL = 0.3, np.radians(5.0), np.radians(19.47)
NODE, TG, STG = 1024, 4, 16          # points per node / super-tile, groups per tile, groups per super-tile
t0 = time.time()
xyz, nrm, truth = synth.make_cloud(n, prim, outl, seed=seed, scanner=scanner)
idx = synth.make_subsets(n, 32, seed=seed)[0] - 1
P, N = xyz[idx], nrm[idx]
del xyz, nrm
S = len(idx)
G = (S + 63) // 64
NST = (G + STG - 1) // STG
cands = [c for c in synth.jittered_candidates(truth, 4096, seed=0)[::STRIDE] if c[0] != "cone"]
print("scene %.1f s: %d subset points, %d groups, %d super-tiles, %d candidates" % (time.time() - t0, S, G, NST, len(cands)), flush=True)


def kd_left(cnt, aligned):
    if aligned and cnt > NODE:
        return (((cnt + NODE - 1) // NODE + 1) // 2) * NODE
    return ((cnt // 64 + 1) // 2) * 64


def kd_split(keys, order, lo, hi, leaf, aligned, out_nodes=None):
    """balanced k-d on keys over order[lo:hi] in place: widest axis, the left child by kd_left, nodes of <= leaf points stay"""
    stack = [(lo, hi)]
    while stack:
        a, b = stack.pop()
        cnt = b - a
        if cnt <= leaf:
            if out_nodes is not None:
                out_nodes.append((a, b))
            continue
        sub = keys[order[a:b]]
        ax = int(np.argmax(sub.max(0) - sub.min(0)))
        nl = kd_left(cnt, aligned)
        part = np.argsort(sub[:, ax], kind="stable")
        order[a:b] = order[a:b][part]
        stack.append((a + nl, b))
        stack.append((a, a + nl))


def orders(aligned):
    """(leaf order, plane order, the nodes of at most 1024 points)"""
    o, nodes = np.arange(S), []
    kd_split(P, o, 0, S, NODE, aligned, nodes)
    leaf, plane = o.copy(), o
    for a, b in nodes:
        kd_split(P, leaf, a, b, 64, aligned)
        kd_split(N, plane, a, b, 64, aligned)
    return leaf, plane, nodes


def cells_of(v):
    """nsig_cell (csrc/score4_device.h) on rows of v"""
    a3 = np.abs(v)
    axis = np.where((a3[:, 0] >= a3[:, 1]) & (a3[:, 0] >= a3[:, 2]), 0, np.where(a3[:, 1] >= a3[:, 2], 1, 2))
    r = np.arange(len(v))
    m, a, b = v[r, axis], v[r, (axis + 1) % 3], v[r, (axis + 2) % 3]
    h = 0.5 * np.abs(m)
    i = (a >= -h).astype(int) + (a >= 0) + (a >= h)
    j = (b >= -h).astype(int) + (b >= 0) + (b >= h)
    return (axis * 2 + (m < 0)) * 16 + i * 4 + j


def cell_centres():
    c = np.zeros((96, 3))
    q = (-0.75, -0.25, 0.25, 0.75)
    for axis in range(3):
        for neg in range(2):
            for i in range(4):
                for j in range(4):
                    v = np.zeros(3)
                    v[axis], v[(axis + 1) % 3], v[(axis + 2) % 3] = (-1.0 if neg else 1.0), q[i], q[j]
                    c[(axis * 2 + neg) * 16 + i * 4 + j] = v / np.linalg.norm(v)
    return c


CENTRES = cell_centres()
assert np.array_equal(cells_of(CENTRES), np.arange(96))


def boxes_of(order):
    """groups and super-tiles of an order: (centre, half extents, cell mask) each"""
    o = np.concatenate([order, np.repeat(order[-1], G * 64 - S)])
    Pg = P[o].reshape(G, 64, 3)
    lo, hi = Pg.min(1), Pg.max(1)
    mask = np.zeros((G, 96), dtype=bool)
    mask[np.repeat(np.arange(G), 64), cells_of(N[o])] = True
    pad = NST * STG - G
    lo_s = np.concatenate([lo, np.repeat(lo[-1:], pad, 0)]).reshape(NST, STG, 3).min(1)
    hi_s = np.concatenate([hi, np.repeat(hi[-1:], pad, 0)]).reshape(NST, STG, 3).max(1)
    mask_s = np.concatenate([mask, np.zeros((pad, 96), dtype=bool)]).reshape(NST, STG, 96).any(1)
    return ((lo + hi) / 2, (hi - lo) / 2, mask), ((lo_s + hi_s) / 2, (hi_s - lo_s) / 2, mask_s), o


def passes(kind, v, pc, ph, mask):
    """the kind's box test on boxes (centre pc, half extents ph; planes: and the boxes' cell masks): True = not ruled out"""
    if kind == "plane":
        p0, oz = v[:3], v[3:6] / np.linalg.norm(v[3:6])
        cm = CENTRES @ oz >= np.cos(ALPHA + RCELL)
        return (np.abs((pc - p0) @ oz) <= EPS + ph @ np.abs(oz)) & mask[:, cm].any(1)
    if kind == "sphere":
        c0, Rr = v[:3], v[3]
        a = np.abs(pc - c0)
        return (np.linalg.norm(np.maximum(a - ph, 0), axis=1) <= Rr + EPS) & (np.linalg.norm(a + ph, axis=1) >= Rr - EPS)
    ax, c0, Rr = v[:3], v[3:6], v[6]
    tt = pc - c0
    q = tt - np.outer(tt @ ax, ax)
    rho = np.linalg.norm(q, axis=1)
    lip = max(1.0, abs(1 - ax @ ax)) * np.linalg.norm(ph, axis=1)
    ball = (rho <= Rr + EPS + lip) & (rho >= Rr - EPS - lip)
    g = q - np.outer(q @ ax, ax)
    w = rho * rho - (np.abs(g) * ph).sum(1)
    return ball & ~((w > 0) & (w * w > (Rr + EPS) ** 2 * rho * rho))


def census(aligned, label):
    t1 = time.time()
    leaf, plane, nodes = orders(aligned)
    sizes = [b - a for a, b in nodes]
    print("%-8s nodes of <= 1024 points: %d, %d .. %d points  (orders %.1f s)" % (label, len(nodes), min(sizes), max(sizes), time.time() - t1), flush=True)
    sets = {"plane": boxes_of(plane), "sphere": boxes_of(leaf)}
    sets["cylinder"] = sets["sphere"]
    st_of_g = np.arange(G) // STG
    tiles_of_st = np.bincount(np.arange((G + TG - 1) // TG) // (STG // TG), minlength=NST)
    listed = {k: np.zeros(NST, dtype=np.int64) for k in sets}
    pairs = {k: 0 for k in sets}
    cosa = np.cos(ALPHA)
    for kind, outw, v in cands:
        v = np.asarray(v, dtype=float)
        (gc, gh, gm), (sc, sh, sm), o = sets[kind]
        in_list = passes(kind, v, sc, sh, sm)
        ok = passes(kind, v, gc, gh, gm) & in_list[st_of_g]
        listed[kind] += in_list
        pairs[kind] += int(ok.sum())
        if kind == "plane":          # sound: no group with an inlier is ruled out at either level
            p0, oz = v[:3], v[3:6] / np.linalg.norm(v[3:6])
            inl = ((np.abs((P[o] - p0) @ oz) < EPS) & (N[o] @ oz > cosa)).reshape(G, 64).any(1)
            assert not (inl & ~ok).any()
    out = {}
    for kind in ("plane", "sphere", "cylinder"):
        ln = listed[kind] * STRIDE
        out[kind] = (int((ln * tiles_of_st).sum()), int((-(-ln // 64) * tiles_of_st).sum()), pairs[kind] * STRIDE)
        print("%-8s %-8s listed %9d  box-tested %9d  visits %7d  pairs %9d" % (label, kind, int(ln.sum()), *out[kind]), flush=True)
    return out


a, b = census(False, "today"), census(True, "aligned")
for kind in a:
    print("%-8s aligned / today: box-tested x %.3f  visits x %.3f  pairs x %.3f" % ((kind,) + tuple(y / x for x, y in zip(a[kind], b[kind]))))
