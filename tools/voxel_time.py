#!/usr/bin/env python3
"""rh_voxel_downsample at full size: wall time of the call (host arrays in and out, synchronous) on the cfg2 / cfg3 / cfg5
clouds (1M / 10M / 50M points) at beta = 2 and 8 times the cloud's median nearest-neighbour distance, and with every
point in one cell (beta = the bounding box); one warm-up call, then the median of five.  Next to it the numpy twin of
tests/test_voxel_host.py on the same input (once), M / n, and the bytes the passes must move over the time, as a
fraction of the HBM peak.
   python tools/voxel_time.py [cfg2 cfg3 cfg5] [--mode centroid|first] [--no-normals] [--no-twin]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
torch.cuda.init()                       # the HIP context exists before the library is asked for anything (like in bench.py)
torch.zeros(1, device="cuda")
import ransac_jl_amd as R
from ransac_jl_amd import synth
from test_voxel_host import ref_voxel

HBM_PEAK = 8.0e12                       # bytes / s, MI355X


def bytes_moved(n, m, normals, centroid):
    """What the device passes must read and write (the host copies are not in it): 24 B of coordinates per point in the
    minimum, insert and (centroid) accumulate passes, 24 B of normals in the minimum and (centroid) accumulate passes, the
    4-byte words per point of the map, slots, flags and ranks, and the rows."""
    per_point = 24 * (3 if centroid else 2) + (24 * (2 if centroid else 1) if normals else 0)
    per_point += 4 * (1 + 2 + 2 + 2 + 3 + 3)     # valid w; valid r, slot w; valid + slot r, flag w; scan r + w; rows r; accumulate r, r, w
    per_row = 20 + (48 if centroid else 0) + 24 * (2 if normals else 1)
    return n * per_point + m * per_row


def timed(xyz, nrm, beta, mode):
    t0 = time.perf_counter()
    out = R.voxeldownsample(xyz, beta, normals=nrm, mode=mode, return_map=True)
    return 1e3 * (time.perf_counter() - t0), len(out[0])


args = [a for a in sys.argv[1:] if not a.startswith("--")]
mode = sys.argv[sys.argv.index("--mode") + 1] if "--mode" in sys.argv else "centroid"
args = [a for a in args if a != mode]
for cfg in args or ["cfg2", "cfg3", "cfg5"]:
    c = synth.config(cfg)
    xyz, nrm = c["xyz"], (None if "--no-normals" in sys.argv else c["nrm"])
    n = len(xyz)
    nn = synth.median_nn_distance(xyz)
    box = float((xyz.max(axis=0) - xyz.min(axis=0)).max()) * 1.001
    for name, beta in (("2 nn", 2 * nn), ("8 nn", 8 * nn), ("one cell", box)):
        timed(xyz, nrm, beta, mode)
        runs = [timed(xyz, nrm, beta, mode) for _ in range(5)]
        ms, m = float(np.median([r[0] for r in runs])), runs[-1][1]
        twin = float("nan")
        if "--no-twin" not in sys.argv:
            t0 = time.perf_counter()
            ref_voxel(xyz, nrm, beta, mode)
            twin = 1e3 * (time.perf_counter() - t0)
        moved = bytes_moved(n, m, nrm is not None, mode == "centroid")
        print("%s n=%d beta=%s (%.4g) %s%s: M/n = %.4f, %.1f ms wall (%.2f ns / point), numpy twin %.0f ms, %.0f MB through the "
              "passes = %.1f %% of HBM peak over the wall time"
              % (cfg, n, name, beta, mode, "" if nrm is None else " + normals", m / n, ms, 1e6 * ms / n, twin, moved / 1e6,
                 100.0 * moved / (ms * 1e-3) / HBM_PEAK), flush=True)
    del xyz, nrm, c
