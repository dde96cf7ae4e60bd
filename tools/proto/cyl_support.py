"""CPU prototype: the cylinder's box test of the culled score kernel (score4_device.h, cyl_box_skip32) with the box bounded by
its SUPPORT along the radial direction at its centre instead of by its half diagonal.  numpy only, no GPU: the cfg3 cloud of
bench.py (synth, 10M points, subset 1 of 32 = 312 500 points), the k-d leaf order of cull_proto.py, the 1224 cylinder candidates
of the bench, both tests in binary64 without the binary32 slack.

For a box with centre c and half extents h, t = c - c0, q = t - a (a . t), rho_c = |q|, g = q - a (a . q):
    today's outer clause      rho_c - |h|                 > R + eps   =>  no point of the box in the band
    the support clause        rho_c - sum |g_k| h_k / rho_c > R + eps   =>  the same   (the tangent plane of the convex rho at c)
Per level of boxes the table counts the (candidate, box) pairs that today's test (outer and inner clause) lets through, and
what is left with the support clause ORed in; it also asserts, over every pair, that no pair with a point inside the distance
band |rho - R| < eps is skipped.  What it prints (profiles/r8/experiments.txt has the GPU's counters next to it):

    boxes                       today's test    + support clause    ratio
    groups (4883)                    567 862             511 631    0.901
    tiles (1221)                     299 740             258 302    0.862
    super-tiles (306)                129 654             109 271    0.843

(402 277 of the 5 976 792 pairs hold a band point.  The estimate the round started from read 507 459 / 257 449 / 109 271: it also
tightened the INNER clause -- the radius of the box's projection across the axis instead of |h| --, 0.8 % of the group pairs,
which was judged not worth its instructions and is not built.)

Not part of the product or the tests: a design aid (DESIGN.md sections 4 and 11).

    python tools/proto/cyl_support.py [points [candidates]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ransac_jl_amd import synth
from cull_proto import kd_order
from tile_lists import union_boxes

EPS = 0.3


def keeps(V, lo, hi):
    """[candidates, boxes] x 2: the box is let through by today's two clauses / by them and the support clause"""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ax, c0, R = V[:, 0:3], V[:, 3:6], V[:, 6][:, None]
    t = c[None, :, :] - c0[:, None, :]
    q = t - np.einsum("cbk,ck->cb", t, ax)[:, :, None] * ax[:, None, :]
    rho2 = (q * q).sum(2)
    rho = np.sqrt(rho2)
    hr = np.linalg.norm(h, axis=1)[None, :]
    ball = (rho <= R + EPS + hr) & ~((R - EPS - hr > 0) & (rho < R - EPS - hr))
    g = q - np.einsum("cbk,ck->cb", q, ax)[:, :, None] * ax[:, None, :]
    w = rho2 - (np.abs(g) * h[None]).sum(2)
    A = R + EPS
    return ball, ball & ~((w > 0) & (w * w > A * A * rho2))


def band_pairs(V, pad):
    """[candidates, groups]: some point of the group lies in the distance band"""
    ax, c0, R = V[:, 0:3], V[:, 3:6], V[:, 6]
    out = np.zeros((V.shape[0], pad.shape[0]), dtype=bool)
    P = pad.reshape(-1, 3)
    for i in range(V.shape[0]):
        t = P - c0[i]
        q = t - (t @ ax[i])[:, None] * ax[i]
        out[i] = (np.abs(np.sqrt((q * q).sum(1)) - R[i]) < EPS).reshape(pad.shape[0], 64).any(1)
    return out


def main():
    npts = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    ncand = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    prim = ["plane"] * 16 + ["sphere"] * 12 + ["cylinder"] * 12
    xyz, _nrm, truth = synth.make_cloud(npts, prim, 0.30, seed=3)
    subs = synth.make_subsets(npts, 32, seed=3)
    P = xyz[subs[0] - 1]
    P = P[kd_order(P)]
    s = P.shape[0]
    ng = (s + 63) // 64
    pad = np.vstack([P, np.repeat(P[-1:], ng * 64 - s, axis=0)]).reshape(ng, 64, 3)
    glo, ghi = pad.min(1), pad.max(1)
    V = np.array([np.asarray(v, dtype=float) for (kk, _o, v) in synth.jittered_candidates(truth, ncand, seed=0) if kk == "cylinder"])
    band = band_pairs(V, pad)
    print("%d subset points, %d groups, %d cylinder candidates, %d pairs, %d with a band point" % (s, ng, V.shape[0], band.size, band.sum()))
    print("%-28s %14s %18s %8s" % ("boxes", "today's test", "+ support clause", "ratio"))
    for name, k in (("groups", 1), ("tiles", 4), ("super-tiles", 16)):
        lo, hi = (glo, ghi) if k == 1 else union_boxes(glo, ghi, k)
        old = new = 0
        for i in range(0, V.shape[0], 64):
            b, n = keeps(V[i:i + 64], lo, hi)
            of = np.arange(ng) // k
            assert not (band[i:i + 64] & ~n[:, of]).any(), "a pair with a band point was skipped"
            old += int(b.sum()); new += int(n.sum())
        print("%-28s %14d %18d %8.3f" % ("%s (%d)" % (name, lo.shape[0]), old, new, new / max(1, old)))


if __name__ == "__main__":
    main()
