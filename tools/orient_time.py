#!/usr/bin/env python3
"""rh_orient_normals at full size, next to the list-writing rh_knn and rh_estimate_normals in the same run: on the cfg2 /
cfg3 clouds (1M / 10M points), k = 16, the normals those of rh_estimate_normals with the canonical sign (orient = 0), device
arrays in and out, one warm-up call each, then the median wall time of five calls of
   rh_knn               idx, d2 and count written: the same search, the floor of the orientation call;
   rh_estimate_normals  the call whose output is oriented;
   rh_orient_normals    normals, flips and components written, anchor = top, up = +z.
Prints the times, the ratio to rh_knn and the call's stats.
   python tools/orient_time.py [cfg2 cfg3]
   python tools/orient_time.py --single cfg3      one orientation call and nothing else timed: the run to put under
                                                  `rocprofv3 --kernel-trace --stats` for the per-kernel split (alone, no counters
                                                  in the same run); the rounds of that call = the launches of ori_select_kernel
                                                  minus the last one, which finds no edge between two trees."""
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
    return float(np.median(runs)), min(runs), max(runs)


def dptr(t, ct):
    return C.cast(t.data_ptr(), C.POINTER(ct))


args = sys.argv[1:]
single = "--single" in args
for cfg in [a for a in args if not a.startswith("--")] or ["cfg2", "cfg3"]:
    xyz = np.ascontiguousarray(R.synth.config(cfg)["xyz"])
    n = len(xyz)
    lib = R.lib()
    d_xyz = torch.from_numpy(xyz).cuda()
    d_nrm = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_flip = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_comp = torch.zeros(n, dtype=torch.int32, device="cuda")
    nprm = L.NormalsParams(k=K, orient=0, radius=0.0)
    oprm, st = L.OrientParams(k=K, anchor=L.ORI_ANCHOR_TOP, radius=0.0), L.OrientStats()
    oprm.up[:] = [0.0, 0.0, 1.0]

    def normals_dev():
        L.check(lib.rh_estimate_normals(dptr(d_xyz, C.c_double), n, C.byref(nprm), None, 0, dptr(d_nrm, C.c_double), None, None))

    def orient_dev():
        L.check(lib.rh_orient_normals(dptr(d_xyz, C.c_double), dptr(d_nrm, C.c_double), n, C.byref(oprm), 0, dptr(d_out, C.c_double),
                                      dptr(d_flip, C.c_int32), dptr(d_comp, C.c_int32), C.byref(st)))

    normals_dev()
    torch.cuda.synchronize()
    if single:
        t0 = time.perf_counter()
        orient_dev()
        print("%s n=%d k=%d: one rh_orient_normals call %.1f ms (first call of the process)" % (cfg, n, K, 1e3 * (time.perf_counter() - t0)),
              flush=True)
        continue
    d_idx = torch.zeros((n, K), dtype=torch.int32, device="cuda")
    d_d2 = torch.zeros((n, K), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")

    def knn_dev():
        L.check(lib.rh_knn(dptr(d_xyz, C.c_double), n, K, 0.0, 0, dptr(d_idx, C.c_int32), dptr(d_d2, C.c_double), dptr(d_cnt, C.c_int32)))

    ms_knn = median_ms(knn_dev)
    ms_nrm = median_ms(normals_dev)
    ms_ori = median_ms(orient_dev)
    print("%s n=%d k=%d: orient %.1f ms (%.1f .. %.1f), knn %.1f ms (%.1f .. %.1f), estimate_normals %.1f ms (%.1f .. %.1f); "
          "orient / knn = %.2f; vertices=%d edges=%d components=%d largest=%d flipped=%d inconsistent=%d min_tree_absdot=%.4g"
          % ((cfg, n, K) + ms_ori + ms_knn + ms_nrm + (ms_ori[0] / ms_knn[0], st.n_vertices, st.n_edges, st.n_components,
             st.largest_component, st.n_flipped, st.n_inconsistent, st.min_tree_absdot)), flush=True)
    del xyz, d_xyz, d_nrm, d_out, d_flip, d_comp, d_idx, d_d2, d_cnt
