#!/usr/bin/env python3
"""rh_segment_smooth at full size, next to rh_knn at the same (n, k) in the same process: on the cfg2 / cfg3 clouds (1M /
10M points with their normals), k = 16, angle 25 degrees, no curvature (every point with a normal is a seed: the most
unions there can be), one warm-up call each, then the median wall time of five calls of
   rh_segment_smooth   with device arrays in and out -- coordinates, normals, labels, kinds, counts, offsets, idx;
   rh_segment_smooth   with device arrays, labels only;
   rh_segment_smooth   with host arrays (what R.segment_smooth does);
   rh_knn              k = 16, device arrays, index and d2 lists kept on the device: the one search the call is built on.
The device-array calls leave out the copies over the host link.  The last figure is the ratio of the first to rh_knn
(rh_orient_normals, which sorts the pairs and runs Boruvka rounds on the same search, costs 2.3 x rh_knn).
   python tools/segment_time.py [cfg2 cfg3]"""
import ctypes as C
import math
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

K = 16
ANGLE = math.radians(25.0)


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
    c = R.synth.config(cfg)
    xyz, nrm = np.ascontiguousarray(c["xyz"], dtype=np.float64), np.ascontiguousarray(c["nrm"], dtype=np.float64)
    n = len(xyz)
    lib = R.lib()
    d_xyz, d_nrm = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    d_nidx = torch.zeros(n * K, dtype=torch.int32, device="cuda")
    d_nd2 = torch.zeros(n * K, dtype=torch.float64, device="cuda")
    d_ncnt = torch.zeros(n, dtype=torch.int32, device="cuda")

    def knn_dev():
        L.check(lib.rh_knn(dptr(d_xyz, C.c_double), n, K, 0.0, 0, dptr(d_nidx, C.c_int32), dptr(d_nd2, C.c_double), dptr(d_ncnt, C.c_int32)))

    ms_knn = median_ms(knn_dev)
    del d_nidx, d_nd2, d_ncnt
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    d_idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    prm = L.SegmentParams(k=K, flags=0, radius=0.0, cos_angle=math.cos(ANGLE), curv_max=0.0, dist_max=0.0, min_size=1,
                          order=L.CLUSTER_BY_SIZE)
    st, m = L.SegmentStats(), C.c_int64()

    def segment_dev():
        L.check(lib.rh_segment_smooth(dptr(d_xyz, C.c_double), dptr(d_nrm, C.c_double), None, n, C.byref(prm), 0, dptr(d_labels, C.c_int32),
                                      dptr(d_kind, C.c_uint8), n, dptr(d_counts, C.c_int64), dptr(d_offsets, C.c_int64),
                                      dptr(d_idx, C.c_int64), C.byref(m), C.byref(st)))

    def labels_dev():
        L.check(lib.rh_segment_smooth(dptr(d_xyz, C.c_double), dptr(d_nrm, C.c_double), None, n, C.byref(prm), 0, dptr(d_labels, C.c_int32),
                                      None, 0, None, None, None, C.byref(m), C.byref(st)))

    ms_dev = median_ms(segment_dev)
    ms_labels = median_ms(labels_dev)
    ms_host = median_ms(lambda: R.segment_smooth(xyz, nrm, k=K, angle=ANGLE, order="size", return_kind=True, return_counts=True,
                                                 return_lists=True))
    print("%s n=%d k=%d angle=25deg: segment_smooth %.1f ms (device arrays, labels + kinds + lists), %.1f ms (device arrays, "
          "labels only), %.1f ms (host arrays); M=%d seed=%d border=%d unassigned=%d invalid=%d largest=%d; knn k=%d %.1f ms "
          "(device arrays, idx + d2 + count); segment_smooth / knn = %.2f"
          % (cfg, n, K, ms_dev, ms_labels, ms_host, st.n_regions, st.n_seed, st.n_border, st.n_unassigned, st.n_invalid, st.largest,
             K, ms_knn, ms_dev / ms_knn), flush=True)
    del xyz, nrm, d_xyz, d_nrm, d_labels, d_kind, d_counts, d_offsets, d_idx
