#!/usr/bin/env python3
"""rh_cluster at full size, next to the radius mode of rh_remove_outliers in the same run: on the cfg2 / cfg3 clouds (1M /
10M points), eps = 2 x nn_median (the point spacing that rh_remove_outliers reports), min_pts = 8, one warm-up call each,
then the median wall time of five calls of
   rh_cluster          with device arrays in and out -- coordinates, labels, kinds, counts, offsets, idx;
   rh_cluster          with host arrays (what R.cluster does);
   rh_remove_outliers  in radius mode, k = min_pts - 1, radius = eps, device arrays: it decides the same core flags (a
                       point with k others within eps) one wave per point with a sorted list, and is the only
                       yardstick there is.
The device-array calls leave out the copies over the host link.
   python tools/cluster_time.py [cfg2 cfg3]"""
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

MIN_PTS = 8


def median_ms(fn):
    fn()
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        runs.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(runs))


def dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


for cfg in sys.argv[1:] or ["cfg2", "cfg3"]:
    xyz = np.ascontiguousarray(R.synth.config(cfg)["xyz"])
    n = len(xyz)
    lib = R.lib()
    d_xyz = torch.from_numpy(xyz).cuda()
    d_keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ost, nk = L.OutlierStats(), C.c_int64()
    # the point spacing
    oprm = L.OutlierParams(k=1, mode=L.OUT_STATISTICAL, std_mul=2.0)
    L.check(lib.rh_remove_outliers(dptr(d_xyz, C.c_double), n, C.byref(oprm), 0, dptr(d_keep, C.c_uint8), None, 0, C.byref(nk), None,
                                   C.byref(ost)))
    eps = 2.0 * ost.nn_median
    oprm = L.OutlierParams(k=MIN_PTS - 1, mode=L.OUT_RADIUS, radius=eps)

    def radius_dev():
        L.check(lib.rh_remove_outliers(dptr(d_xyz, C.c_double), n, C.byref(oprm), 0, dptr(d_keep, C.c_uint8), None, 0, C.byref(nk),
                                       None, C.byref(ost)))

    ms_radius = median_ms(radius_dev)
    n_core_radius = int(ost.n_kept)
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    d_idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    prm, st, m = L.ClusterParams(eps=eps, min_pts=MIN_PTS, min_size=1, order=L.CLUSTER_BY_SIZE), L.ClusterStats(), C.c_int64()

    def cluster_dev():
        L.check(lib.rh_cluster(dptr(d_xyz, C.c_double), n, C.byref(prm), 0, dptr(d_labels, C.c_int32), dptr(d_kind, C.c_uint8), n,
                               dptr(d_counts, C.c_int64), dptr(d_offsets, C.c_int64), dptr(d_idx, C.c_int64), C.byref(m), C.byref(st)))

    def labels_dev():
        L.check(lib.rh_cluster(dptr(d_xyz, C.c_double), n, C.byref(prm), 0, dptr(d_labels, C.c_int32), None, 0, None, None, None,
                               C.byref(m), C.byref(st)))

    ms_dev = median_ms(cluster_dev)
    ms_labels = median_ms(labels_dev)
    ms_host = median_ms(lambda: R.cluster(xyz, eps, min_pts=MIN_PTS, order="size", return_kind=True, return_counts=True,
                                          return_lists=True))
    assert st.n_core == n_core_radius, (st.n_core, n_core_radius)          # the same core flags, two ways
    print("%s n=%d eps=%.4g (2 x nn_median) min_pts=%d: cluster %.1f ms (device arrays, labels + kinds + lists), %.1f ms (device "
          "arrays, labels only), %.1f ms (host arrays); M=%d core=%d border=%d noise=%d largest=%d; remove_outliers radius mode "
          "k=%d %.1f ms (device arrays, the same %d core points)"
          % (cfg, n, eps, MIN_PTS, ms_dev, ms_labels, ms_host, st.n_clusters, st.n_core, st.n_border, st.n_noise, st.largest,
             MIN_PTS - 1, ms_radius, n_core_radius), flush=True)
    del xyz, d_xyz, d_keep, d_labels, d_kind, d_counts, d_offsets, d_idx
