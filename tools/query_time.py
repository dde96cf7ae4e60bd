#!/usr/bin/env python3
"""rh_knn_query and rh_cloud_distance at full size, next to rh_knn in the same process: on the cfg2 / cfg3 clouds (1M / 10M
points), one warm-up call each, then the median wall time of five calls with their minimum and maximum, device arrays in
and out (no copies over the host link: the search and the passes around it).
 (a) reference = the cloud, queries = the cloud displaced by Gaussian noise of nn_median / 2 per axis (nn_median: the point
     spacing rh_remove_outliers reports), m = n, k = 1 and k = 16, idx + d2 + count written; rh_knn at the same n and k is
     the yardstick: per query the cross call does rh_knn's search minus the self entry, plus one key sort over m;
 (b) reference = the cloud thinned by voxeldownsample at beta = 2 x nn_median, queries = the full cloud: rh_cloud_distance
     (point metric, distances + indices + stats) and the transfer_labels path (rh_knn_query, k = 1, idx only; the gather
     that follows is numpy's), then R.transfer_labels itself with host arrays.
   python tools/query_time.py [cfg2 cfg3] [--k=16] [--no-b]
--k=K times case (a) at that k only and --no-b leaves case (b) out: a run under rocprofv3 --kernel-trace --stats then
holds the kernels of one comparison."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.init()                       # the HIP context exists before the library is asked for anything (like in bench.py)
torch.zeros(1, device="cuda")
import ransac_jl_amd as R
from ransac_jl_amd import _lib as L


def timed(fn):
    """(median, min, max) in ms of five calls after a warm-up"""
    fn()
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        runs.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(runs)), min(runs), max(runs)


def show(t):
    return "%.1f ms (%.1f - %.1f)" % t


def dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
KS = [int(a[4:]) for a in FLAGS if a.startswith("--k=")] or [1, 16]

for cfg in [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2", "cfg3"]:
    xyz = np.ascontiguousarray(R.synth.config(cfg)["xyz"])
    n = len(xyz)
    lib = R.lib()
    _, st = R.removeoutliers(xyz, k=1, return_stats=True)
    spacing = st["nn_median"]
    qry = xyz + np.random.default_rng(1).normal(0.0, 0.5 * spacing, size=xyz.shape)
    d_ref, d_qry = torch.from_numpy(xyz).cuda(), torch.from_numpy(qry).cuda()
    pr, pq = dptr(d_ref, C.c_double), dptr(d_qry, C.c_double)

    # (a) the lists, next to rh_knn
    for k in KS:
        d_idx = torch.zeros((n, k), dtype=torch.int32, device="cuda")
        d_d2 = torch.zeros((n, k), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        out = (dptr(d_idx, C.c_int32), dptr(d_d2, C.c_double), dptr(d_cnt, C.c_int32))
        t_query = timed(lambda: L.check(lib.rh_knn_query(pr, n, pq, n, k, 0.0, 0, *out)))
        full = int((d_cnt == k).sum().item())
        t_knn = timed(lambda: L.check(lib.rh_knn(pr, n, k, 0.0, 0, *out)))
        t_query2 = timed(lambda: L.check(lib.rh_knn_query(pr, n, pq, n, k, 0.0, 0, *out)))      # once more, behind the yardstick
        print("%s (a) n = m = %d, spacing %.4g, k = %d: rh_knn_query %s, again %s; rh_knn %s; %d of %d lists full"
              % (cfg, n, spacing, k, show(t_query), show(t_query2), show(t_knn), full, n), flush=True)
        del d_idx, d_d2, d_cnt

    if "--no-b" in FLAGS:
        continue
    # (b) thinned reference, the full cloud as queries
    thin = np.ascontiguousarray(R.voxeldownsample(xyz, 2.0 * spacing))
    nt = len(thin)
    d_thin = torch.from_numpy(thin).cuda()
    pt = dptr(d_thin, C.c_double)
    d_dist = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_nn = torch.zeros(n, dtype=torch.int32, device="cuda")
    prm, dst = L.DistanceParams(radius=0.0, threshold=spacing, metric=L.DIST_POINT), L.DistanceStats()
    t_dist = timed(lambda: L.check(lib.rh_cloud_distance(pt, None, nt, pr, n, C.byref(prm), 0, dptr(d_dist, C.c_double),
                                                         dptr(d_nn, C.c_int32), C.byref(dst))))
    t_label = timed(lambda: L.check(lib.rh_knn_query(pt, nt, pr, n, 1, 0.0, 0, dptr(d_nn, C.c_int32), None, None)))
    labels = (np.arange(nt) % 7).astype(np.int32)
    t_host = timed(lambda: R.transfer_labels(thin, labels, xyz))
    print("%s (b) reference %d points (beta = 2 x spacing), m = %d: rh_cloud_distance %s (mean %.4g rms %.4g max %.4g median "
          "%.4g, %d within a spacing); rh_knn_query k = 1, idx only %s; transfer_labels with host arrays %s"
          % (cfg, nt, n, show(t_dist), dst.mean, dst.rms, dst.max, dst.median, dst.n_within, show(t_label), show(t_host)),
          flush=True)
    del xyz, qry, thin, d_ref, d_qry, d_thin, d_dist, d_nn
