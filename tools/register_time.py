#!/usr/bin/env python3
"""rh_register at full size: the cost of one iteration and where it goes, next to one rh_cloud_distance call (distances and
indices, no stats) on the same clouds -- that call pays the upload and the grid build every time, an iteration does not.
Reference = the cfg cloud with its normals (cfg2: 1M points, cfg3: 10M); queries = m of its points displaced by Gaussian
noise of half a point spacing per axis, then turned by one degree and shifted by two spacings.  Device arrays in, plane
metric unless --point, tolerances 0 so that every call runs exactly max_iter iterations.
   python tools/register_time.py [cfg2 cfg3] [--m=1000000] [--iters=8] [--point] [--split]
Wall times (one warm-up, then the median of five with minimum and maximum): a call of 1 iteration and a call of 1 + iters;
an iteration = the difference / iters, the set-up (upload, grid) = the rest of the first.
--split runs the case once more in a child process under rocprofv3 --kernel-trace --stats and sorts the kernels of the
iterations into transform + box + keys + sort / search / accumulate + fold; the host's share (the two round trips, the
6 x 6 solve) is what the wall time of an iteration has beyond them."""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
CFGS = [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2", "cfg3"]


def flag(name, default):
    for a in FLAGS:
        if a.startswith("--%s=" % name):
            return int(a.split("=", 1)[1])
    return default


M, ITERS = flag("m", 1000000), flag("iters", 8)
METRIC = "point" if "--point" in FLAGS else "plane"
GROUPS = (("transform + box + keys + sort", ("reg_transform_kernel", "nrm_minmax_kernel", "grid_minmax_fold_kernel", "xq_key_kernel",
                                              "rocprim", "radix", "onesweep", "histogram", "scan")),
          ("search", ("xq_kernel",)),
          ("accumulate + fold", ("reg_accumulate_kernel", "reg_fold_kernel")))


def split_of(trace_csv, iters):
    """per-iteration ms of each group from the kernel trace of ONE call of `iters` iterations: the set-up comes before the
    loop, so every dispatch from the first reg_transform_kernel on belongs to an iteration"""
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace_csv))))
    first = next(i for i, r in enumerate(rows) if "reg_transform_kernel" in r[2])
    tot = {g: 0.0 for g, _ in GROUPS}
    tot["other"] = 0.0
    for s, e, name in rows[first:]:
        for g, keys in GROUPS:
            if any(k in name for k in keys):
                tot[g] += (e - s) / 1e6
                break
        else:
            tot["other"] += (e - s) / 1e6
    return {g: v / iters for g, v in tot.items()}


def main():
    import torch
    torch.cuda.init()                   # the HIP context exists before the library is asked for anything (like in bench.py)
    torch.zeros(1, device="cuda")
    import ransac_jl_amd as R
    from ransac_jl_amd import _lib as L

    def dptr(t, ct):
        return C.cast(t.data_ptr(), C.POINTER(ct))

    def timed(fn, reps=5):
        fn()
        runs = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            runs.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(runs)), min(runs), max(runs)

    child = "--child" in FLAGS
    lib = R.lib()
    for cfg in CFGS:
        c = R.synth.config(cfg)
        xyz, nrm = np.ascontiguousarray(c["xyz"]), np.ascontiguousarray(c["nrm"])
        n, m = len(xyz), min(M, len(xyz))
        spacing = R.synth.median_nn_distance(xyz)
        rng = np.random.default_rng(1)
        pick = rng.choice(n, m, replace=False)
        q = xyz[pick] + rng.normal(0.0, 0.5 * spacing, size=(m, 3))
        th, ctr = np.radians(1.0), xyz.mean(axis=0)
        rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        q = np.ascontiguousarray((q - ctr) @ rot.T + ctr + np.array([2.0 * spacing, 0.0, 0.0]))
        d_ref, d_nrm, d_qry = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda(), torch.from_numpy(q).cuda()
        pr, pn, pq = dptr(d_ref, C.c_double), dptr(d_nrm, C.c_double), dptr(d_qry, C.c_double)
        out, res = np.zeros((3, 4)), L.RegisterResult()
        po = out.ctypes.data_as(C.POINTER(C.c_double))

        def reg(iters):
            prm = L.RegisterParams(radius=0.0, rot_tol=0.0, trans_tol=0.0, max_iter=iters,
                                   metric=L.DIST_PLANE if METRIC == "plane" else L.DIST_POINT)
            L.check(lib.rh_register(pr, pn if METRIC == "plane" else None, n, pq, m, C.byref(prm), None, 0, po, C.byref(res), None, None))
            assert res.iterations == iters, (res.iterations, res.status)

        if child:                       # under the profiler: one call
            reg(ITERS)
            torch.cuda.synchronize()
            continue
        t1, tk = timed(lambda: reg(1)), timed(lambda: reg(1 + ITERS))
        per = (tk[0] - t1[0]) / ITERS
        d_dist = torch.zeros(m, dtype=torch.float64, device="cuda")
        d_nn = torch.zeros(m, dtype=torch.int32, device="cuda")
        dprm = L.DistanceParams(radius=0.0, threshold=spacing, metric=L.DIST_PLANE if METRIC == "plane" else L.DIST_POINT)
        td = timed(lambda: L.check(lib.rh_cloud_distance(pr, pn if METRIC == "plane" else None, n, pq, m, C.byref(dprm), 0,
                                                         dptr(d_dist, C.c_double), dptr(d_nn, C.c_int32), None)))
        print("%s n = %d, m = %d, %s metric, spacing %.4g: 1 iteration %.1f ms (%.1f - %.1f), %d iterations %.1f ms (%.1f - %.1f): "
              "%.2f ms per iteration, set-up %.1f ms; rh_cloud_distance without stats %.1f ms (%.1f - %.1f); iteration / that "
              "call = %.2f; last rms %.4g, n_valid %d" % ((cfg, n, m, METRIC, spacing) + t1 + (1 + ITERS,) + tk
                                                        + (per, t1[0] - per) + td + (per / td[0], res.rms, res.n_valid)), flush=True)
        if "--split" in FLAGS:
            with tempfile.TemporaryDirectory() as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                       os.path.abspath(__file__), cfg, "--child", "--m=%d" % M, "--iters=%d" % ITERS] + (["--point"] if METRIC == "point" else [])
                run = subprocess.run(cmd, capture_output=True, text=True)
                found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
                if run.returncode != 0 or not found:
                    print("%s split: the profiled run failed (exit %d): %s" % (cfg, run.returncode, run.stderr[-400:]), flush=True)
                    continue
                parts = split_of(found[0], ITERS)
            dev = sum(parts.values())
            print("%s split per iteration: %s; kernels %.2f ms, host and round trips %.2f ms of %.2f ms"
                  % (cfg, ", ".join("%s %.2f ms" % kv for kv in parts.items()), dev, per - dev, per), flush=True)
        del d_ref, d_nrm, d_qry, xyz, nrm, q


if __name__ == "__main__":
    main()
