#!/usr/bin/env python3
"""rh_remove_outliers and rh_knn at full size, next to rh_estimate_normals in the same run: on the cfg2 / cfg3 clouds (1M /
10M points), k = 16, one warm-up call each, then the median wall time of five calls of
   rh_remove_outliers  (statistical, std_mul 2) with device arrays in and out -- coordinates, keep flags, kept list;
   rh_knn              with device arrays in and out, idx + d2 + count (the n x k lists: 12 k bytes per point);
   the two above       with host arrays (what R.removeoutliers / R.knn do);
   rh_estimate_normals with host arrays in and out (the only form that entry takes).
The device-array calls leave out the copies over the host link, so they time the search and the passes behind it.
   python tools/outliers_time.py [cfg2 cfg3]"""
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

K = 16


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
    d_kept = torch.zeros(n, dtype=torch.int32, device="cuda")
    prm, st, nk = L.OutlierParams(k=K, mode=L.OUT_STATISTICAL, std_mul=2.0), L.OutlierStats(), C.c_int64()

    def outliers_dev():
        L.check(lib.rh_remove_outliers(dptr(d_xyz, C.c_double), n, C.byref(prm), 0, dptr(d_keep, C.c_uint8),
                                       dptr(d_kept, C.c_int32), n, C.byref(nk), None, C.byref(st)))

    ms_out = median_ms(outliers_dev)
    ms_out_host = median_ms(lambda: R.removeoutliers(xyz, k=K, return_index=True))
    d_idx = torch.zeros((n, K), dtype=torch.int32, device="cuda")
    d_d2 = torch.zeros((n, K), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")

    def knn_dev():
        L.check(lib.rh_knn(dptr(d_xyz, C.c_double), n, K, 0.0, 0, dptr(d_idx, C.c_int32), dptr(d_d2, C.c_double),
                           dptr(d_cnt, C.c_int32)))

    ms_knn = median_ms(knn_dev)
    del d_idx, d_d2, d_cnt
    ms_knn_host = median_ms(lambda: R.knn(xyz, K, return_count=True))
    ms_nrm = median_ms(lambda: R.estimatenormals(xyz, k=K))
    print("%s n=%d k=%d: remove_outliers %.1f ms (device arrays; kept %d of %d, mu %.4g sigma %.4g nn_median %.4g), %.1f ms "
          "(host arrays); knn with lists %.1f ms (device arrays, %.0f MB of lists), %.1f ms (host arrays); estimate_normals "
          "%.1f ms (host arrays)"
          % (cfg, n, K, ms_out, st.n_kept, n, st.mu, st.sigma, st.nn_median, ms_out_host, ms_knn, 12e-6 * K * n, ms_knn_host,
             ms_nrm), flush=True)
    del xyz, d_xyz, d_keep, d_kept
