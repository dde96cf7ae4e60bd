#!/usr/bin/env python3
"""What labelling every point costs: on the cfg2- and cfg3-sized synth scenes (1M / 10M points) run ransac(), then label
the whole cloud with all the shapes it found --
   device  rh_cloud_assign_dev on resident buffers, labels only and again with dist, counts and lists, by the cloud's
           timer (HIP events): median of five after a warm-up; against the time the 48 B per point take at the rate
           DESIGN.md records for the streaming refit scan (6.2 TB/s at 10M points);
   today   what a user does for the same answer on this commit: b calls of rh_refit (wall time, each one waits and reads
           its list back) and the merge of the b overlapping lists on the host (first shape wins: rh_refit returns no
           distances to do better with);
   raw     rh_assign_points on the host arrays, labels only: wall time -- the upload of 48 B per point dominates it.
   python tools/assign_time.py [cfg2 cfg3]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.cuda.init()                       # the HIP context exists before the library is asked for anything (like in bench.py)
torch.zeros(1, device="cuda")
import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth

HBM_RATE = 6.2e12                       # B/s: the streaming refit scan at 10M points
lib = R.lib()
for cfg in [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2", "cfg3"]:
    c = synth.config(cfg)
    xyz, nrm = c["xyz"], c["nrm"]
    n = len(xyz)
    pc = R.RANSACCloud(xyz, nrm, synth.make_subsets(n, c["r"], c["seed"]))
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    rp = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 200, "τ": 900, "prob_det": 0.9})
    cp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    R.ransac(pc, cp, setenabled=True, seed=99)                         # warm-up: the cloud's one-time allocations
    pc.enable_all()
    got, _ = R.ransac(pc, cp, seed=1234)
    pc.enable_all()
    b = len(got)
    print("%s n=%d: ransac() found %d shapes" % (cfg, n, b), flush=True)
    if b == 0:
        continue
    arr = (L.Shape * b)(*[e.c_shape for e in got])

    # the device entry on resident buffers
    sizes = [C.sizeof(arr), 4 * n, 8 * n, 8 * (b + 1), 8 * (b + 2), 8 * n]
    bufs = []
    for nbytes in sizes:
        d = C.c_void_p()
        L.check(lib.rh_dev_alloc(pc._h, nbytes, C.byref(d)))
        bufs.append(d)
    L.check(lib.rh_dev_upload(pc._h, bufs[0], C.cast(arr, C.c_void_p), sizes[0]))
    t_dev = {}
    for name, outs in (("labels", (bufs[1], None, None, None, None)), ("lists", tuple(bufs[1:]))):
        ms_all = []
        for k in range(6):
            ms = C.c_float()
            L.check(lib.rh_timer_start(pc._h))
            L.check(lib.rh_cloud_assign_dev(pc._h, bufs[0], b, C.byref(cp), 0, *outs))
            L.check(lib.rh_timer_stop(pc._h, C.byref(ms)))
            ms_all.append(ms.value)
        t_dev[name] = float(np.median(ms_all[1:]))
    labels = np.zeros(n, dtype=np.int32)
    counts = np.zeros(b + 1, dtype=np.int64)
    L.check(lib.rh_dev_download(pc._h, labels.ctypes.data_as(C.c_void_p), bufs[1], labels.nbytes))
    L.check(lib.rh_dev_download(pc._h, counts.ctypes.data_as(C.c_void_p), bufs[3], counts.nbytes))
    for d in bufs:
        L.check(lib.rh_dev_free(pc._h, d))
    assert np.array_equal(counts, np.bincount(labels, minlength=b + 1))
    t_hbm = 1e3 * 48.0 * n / HBM_RATE
    print("  rh_cloud_assign_dev, %d shapes: labels only %.3f ms, with dist + counts + lists %.3f ms; 48 B per point at %.1f TB/s: %.3f ms"
          "   (%d of %d points labelled)" % (b, t_dev["labels"], t_dev["lists"], HBM_RATE / 1e12, t_hbm, n - counts[0], n), flush=True)

    # today: b refits and the merge on the host
    today = []
    for k in range(3):
        t0 = time.perf_counter()
        lists = [R.refit(e.c_shape, pc, cp).inpoints for e in got]
        t_refit = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        merged = np.zeros(n, dtype=np.int32)
        for j in reversed(range(b)):
            merged[lists[j] - 1] = j + 1
        today.append((t_refit, 1e3 * (time.perf_counter() - t0)))
    t_refit, t_merge = np.median(np.array(today[1:]), axis=0)
    assert np.array_equal(merged > 0, labels > 0), "the union of the refit sets is not the labelled points"
    print("  today: %d x rh_refit %.2f ms wall + merge on the host %.2f ms (first shape wins; %d points labelled differently)"
          % (b, t_refit, t_merge, int((merged != labels).sum())), flush=True)

    # the raw-array entry: wall time, the upload included
    raw = []
    for k in range(3):
        t0 = time.perf_counter()
        lab = R.assign_points(xyz, nrm, arr, cp)
        raw.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(lab, labels)
    print("  rh_assign_points on host arrays (labels only, %d MB uploaded): %.1f ms wall" % (48 * n // 1000000, float(np.median(raw[1:]))),
          flush=True)
    del pc, xyz, nrm
