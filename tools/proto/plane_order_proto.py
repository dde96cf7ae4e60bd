#!/usr/bin/env python3
"""CPU prototype (numpy, the kernel's culling rules without their slack) behind DESIGN.md section 11, "plane order": how many
(candidate, group) pairs survive stage 1 when the 64-point groups of subset 1 are cut by the points' NORMALS inside a block of
1024 points of the position order, instead of by position all the way down?

Orders (every figure is the share of all (candidate, group) pairs):
  today    the 3-D k-d leaf order (balanced, widest axis, left child a multiple of 64)
  node     the position tree stopped at its nodes of <= 1024 points, then a k-d on the normals (widest axis, median split, left
           child a multiple of 64) down to groups of 64: the blocks are compact tree nodes of 9-10 groups at cfg3 (what
           csrc/kdorder.hip builds)
  st       the same normal tree inside every run of 1024 CONSECUTIVE points of the leaf order: the super-tiles of the score
           launch's candidate lists (built first, measured, replaced: profiles/r13/experiments.txt).  4883 groups do not halve
           down to 16: such a run straddles the position tree's nodes, so its points lie further apart than a node's
cfg3: today 0.0846 of all plane pairs survive, node 0.0605 (x 0.715; the kernel's counters: x 0.696), st 0.0728 (x 0.860; x 0.819).

Tests: the plane's support-function box test |d(centre)| <= eps + sum |n_k| h_k; the 96-cell cube map of the normals (nsig_cell,
6 faces x 4 x 4), a group's mask = the cells of its points, a candidate's mask = the cells whose centre lies within alpha + r_cell
of its normal (r_cell = 19.47 degrees); sphere: nearest / farthest point of the box against the band; cylinder: the two ball
clauses and the support clause of cyl_box_skip32.  eps = 0.3, alpha = 5 degrees, every STRIDE-th of the 4096 bench candidates.
    python tools/proto/plane_order_proto.py [cfg3|cfg2] [points] [stride]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ransac_jl_amd import synth

np.seterr(all="ignore")
cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
prim, n, seed, outl = ["plane"] * 16 + ["sphere"] * 12 + ["cylinder"] * 12, 10_000_000, 3, 0.30
if cfg == "cfg2":
    prim, n, seed, outl = ["plane", "plane", "sphere", "sphere", "cylinder", "cylinder"], 1_000_000, 2, 0.0
n = int(sys.argv[2]) if len(sys.argv) > 2 else n
STRIDE = int(sys.argv[3]) if len(sys.argv) > 3 else 4
EPS, ALPHA, RCELL = 0.3, np.radians(5.0), np.radians(19.47)
t0 = time.time()
xyz, nrm, truth = synth.make_cloud(n, prim, outl, seed=seed)
idx = synth.make_subsets(n, 32, seed=seed)[0] - 1
P, N = xyz[idx], nrm[idx]
S = len(idx)
G = (S + 63) // 64
cands = synth.jittered_candidates(truth, 4096, seed=0)[::STRIDE]
print("scene %.1f s: %d subset points, %d groups, %d candidates" % (time.time() - t0, S, G, len(cands)))


def kd_split(keys, order, lo, hi, leaf, out_nodes=None):
    """balanced k-d on keys over order[lo:hi] in place: widest axis, left child a multiple of 64, nodes of <= leaf points stay"""
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
        nl = ((cnt // 64 + 1) // 2) * 64
        part = np.argsort(sub[:, ax], kind="stable")          # (a total order, like the library's)
        order[a:b] = order[a:b][part]
        stack.append((a + nl, b))
        stack.append((a, a + nl))


def order_today():
    o = np.arange(S)
    kd_split(P, o, 0, S, 64)
    return o


def order_node():
    o = np.arange(S)
    nodes = []
    kd_split(P, o, 0, S, 1024, nodes)
    for a, b in nodes:
        kd_split(N, o, a, b, 64)
    return o, nodes


def order_st(base):
    o = base.copy()
    for a in range(0, S, 1024):
        kd_split(N, o, a, min(S, a + 1024), 64)
    return o


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
                    m = -1.0 if neg else 1.0
                    v = np.zeros(3)
                    v[axis], v[(axis + 1) % 3], v[(axis + 2) % 3] = m, q[i], q[j]   # (thresholds at a = +-|m| / 2: quotients of |m|)
                    c[(axis * 2 + neg) * 16 + i * 4 + j] = v / np.linalg.norm(v)
    return c


CENTRES = cell_centres()
assert np.array_equal(cells_of(CENTRES), np.arange(96))


def groups_of(order):
    pad = G * 64 - S
    o = np.concatenate([order, np.repeat(order[-1], pad)])
    Pg = P[o].reshape(G, 64, 3)
    pc, ph = (Pg.max(1) + Pg.min(1)) / 2, (Pg.max(1) - Pg.min(1)) / 2
    mask = np.zeros((G, 96), dtype=bool)
    mask[np.repeat(np.arange(G), 64), cells_of(N[o])] = True
    return o, pc, ph, mask


def census(order, label):
    o, pc, ph, mask = groups_of(order)
    hr = np.linalg.norm(ph, axis=1)
    tot = {"plane": [0, 0, 0, 0], "sphere": [0, 0], "cylinder": [0, 0]}
    cosa = np.cos(ALPHA)
    Po, No = P[o], N[o]
    for kind, outw, v in cands:
        v = np.asarray(v, dtype=float)
        sg = 1.0 if outw else -1.0
        if kind == "plane":
            p0, oz = v[:3], v[3:6] / np.linalg.norm(v[3:6])
            box = np.abs((pc - p0) @ oz) <= EPS + ph @ np.abs(oz)
            cm = CENTRES @ oz >= np.cos(ALPHA + RCELL)
            both = box & (mask[:, cm].any(1))
            inl = (np.abs((Po - p0) @ oz) < EPS) & (No @ oz > cosa)          # (compatiblesPlane, plane.jl:114-130)
            t = tot["plane"]
            t[0] += int(box.sum()); t[1] += int(both.sum()); t[2] += int(inl.reshape(G, 64).any(1).sum()); t[3] += G
            assert not (inl.reshape(G, 64).any(1) & ~both).any()          # sound: no group with an inlier is ruled out
        elif kind == "sphere":
            c0, Rr = v[:3], v[3]
            a = np.abs(pc - c0)
            dmin, dmax = np.linalg.norm(np.maximum(a - ph, 0), axis=1), np.linalg.norm(a + ph, axis=1)
            t = tot["sphere"]
            t[0] += int(((dmin <= Rr + EPS) & (dmax >= Rr - EPS)).sum()); t[1] += G
        elif kind == "cylinder":
            ax, c0, Rr = v[:3], v[3:6], v[6]
            tt = pc - c0
            q = tt - np.outer(tt @ ax, ax)
            rho = np.linalg.norm(q, axis=1)
            lip = max(1.0, abs(1 - ax @ ax)) * hr
            ball = (rho <= Rr + EPS + lip) & (rho >= Rr - EPS - lip)
            g = q - np.outer(q @ ax, ax)
            w = rho * rho - (np.abs(g) * ph).sum(1)
            support_skip = (w > 0) & (w * w > (Rr + EPS) ** 2 * rho * rho)
            t = tot["cylinder"]
            t[0] += int((ball & ~support_skip).sum()); t[1] += G
    pl = tot["plane"]
    print("%-6s plane: box %.4f  box + cells %.4f  groups with an inlier %.4f  cells per group %.1f | cylinder: box %.4f | sphere: box %.4f"
          % (label, pl[0] / pl[3], pl[1] / pl[3], pl[2] / pl[3], mask.sum(1).mean(), tot["cylinder"][0] / tot["cylinder"][1],
             tot["sphere"][0] / tot["sphere"][1]), flush=True)
    return pl[1] / pl[3]


t0 = time.time()
today = order_today()
print("position k-d %.1f s" % (time.time() - t0))
a = census(today, "today")
node, nodes = order_node()
print("nodes of the position tree with <= 1024 points: %d, %d .. %d points" % (len(nodes), min(b - a_ for a_, b in nodes), max(b - a_ for a_, b in nodes)))
b = census(node, "node")
c = census(order_st(today), "st")
print("plane pairs against today's: node %.3f, st %.3f" % (b / a, c / a))
