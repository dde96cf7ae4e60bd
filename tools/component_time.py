#!/usr/bin/env python3
"""What the connected-component filter costs: rh_refit against rh_refit_component on the largest plane and the largest
cylinder of the cfg2- and cfg3-sized synth scenes (1M / 10M points), beta = twice the scene's median nearest-neighbour
distance (from 256 sample points, exact), median of five calls after a warm-up (wall time of the synchronous call, index
list read back included); then ransac() end to end on the same cloud with the filter off and on.
   python tools/component_time.py [cfg2 cfg3] [--no-e2e]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.init()                       # the HIP context exists before the library is asked for anything (like in bench.py)
torch.zeros(1, device="cuda")
import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth


def median_nn(xyz, m=256, chunk=1 << 20):
    rng = np.random.default_rng(0)
    pick = rng.choice(len(xyz), size=m, replace=False)
    q = torch.from_numpy(xyz[pick]).cuda()
    best = torch.full((m,), float("inf"), dtype=torch.float64, device="cuda")
    for lo in range(0, len(xyz), chunk):
        d = torch.cdist(q, torch.from_numpy(xyz[lo:lo + chunk]).cuda())
        d[d == 0] = float("inf")        # the point itself (and exact duplicates, which synth does not make)
        best = torch.minimum(best, d.min(dim=1).values)
    return float(best.median().item())


def med5(f):
    f()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def shape_of(t):
    if t["kind"] == "plane":
        return R.FittedPlane(t["point"], t["normal"])
    return R.FittedCylinder(t["axis"], t["center"], t["radius"], True)


args = [a for a in sys.argv[1:] if not a.startswith("--")]
for cfg in args or ["cfg2", "cfg3"]:
    c = synth.config(cfg)
    xyz, nrm, truth = c["xyz"], c["nrm"], c["truth"]
    subs = synth.make_subsets(len(xyz), c["r"], c["seed"])
    pc = R.RANSACCloud(xyz, nrm, subs)
    beta = 2.0 * median_nn(xyz)
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    cp = R.params_to_c(R.ransacparameters(types), score_mode=L.SCORE_F64)
    print("%s n=%d beta=%.4f" % (cfg, len(xyz), beta), flush=True)
    for kind in ("plane", "cylinder"):
        t = max((t for t in truth if t["kind"] == kind), key=lambda t: t["n_points"])
        s = shape_of(t)
        t_refit, es = med5(lambda: R.refit(s, pc, cp))
        t_comp, (ec, st) = med5(lambda: R.refit_component(s, pc, cp, beta, True, return_stats=True))
        print("  largest %-8s rh_refit %.3f ms (%d points)   rh_refit_component %.3f ms (%d points kept, %d components)   + %.3f ms"
              % (kind, t_refit, es.inpoints.size, t_comp, ec.inpoints.size, st["n_components"], t_comp - t_refit), flush=True)
    if "--no-e2e" in sys.argv:
        continue
    rp = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 200, "τ": 900, "prob_det": 0.9})
    rcp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    for label, b in (("off", None), ("on", beta)):
        R.ransac(pc, rcp, setenabled=True, seed=99, component_beta=b)      # warm-up: the cloud's one-time allocations
        runs = []
        for _ in range(3):
            pc.enable_all()
            t0 = time.perf_counter()
            got, _, st = R.ransac(pc, rcp, seed=1234, return_stats=True, component_beta=b)
            runs.append(time.perf_counter() - t0)
        print("  ransac() filter %-3s %.1f ms, %d shapes, %d points extracted, extract share %.1f ms"
              % (label, 1e3 * float(np.median(runs)), len(got), sum(e.inpoints.size for e in got), 1e3 * st["seconds_extract"]), flush=True)
    del pc, xyz, nrm
