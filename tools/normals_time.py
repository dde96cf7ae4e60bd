#!/usr/bin/env python3
"""rh_estimate_normals at full size: HIP-event time of the call (host buffers in and out, synchronous) on the cfg2 / cfg3 /
cfg5 clouds (1M / 10M / 50M points), k = 16 and 32; one warm-up call per cloud, then the median of three.
   python tools/normals_time.py [cfg2 cfg3 cfg5]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.init()                       # the HIP context exists before the library is asked for anything (like in bench.py)
torch.zeros(1, device="cuda")
import ransac_jl_amd as R
from ransac_jl_amd import synth


def timed(xyz, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    nrm, flags = R.estimatenormals(xyz, k=k, return_flags=True)
    wall = time.perf_counter() - t0
    b.record()
    b.synchronize()
    return a.elapsed_time(b), 1e3 * wall, flags


for cfg in sys.argv[1:] or ["cfg2", "cfg3", "cfg5"]:
    xyz = synth.config(cfg)["xyz"]
    for k in (16, 32):
        timed(xyz, k)
        runs = [timed(xyz, k) for _ in range(3)]
        ev = float(np.median([r[0] for r in runs]))
        wall = float(np.median([r[1] for r in runs]))
        print("%s n=%d k=%d: %.1f ms (HIP events), %.1f ms wall, %.4f %% flagged"
              % (cfg, len(xyz), k, ev, wall, 100.0 * runs[-1][2].mean()), flush=True)
    del xyz
