"""The bench's root-cell end-to-end leg alone: rh_ransac on the cfg3 cloud with the parameters of bench.py's end_to_end leg
(itermax 16384, minsubsetN 4096, seed 1234), a warm-up and five timed runs, their median.   python tools/e2e_leg.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, synth
c = synth.config("cfg3")
subs = synth.make_subsets(len(c["xyz"]), c["r"], c["seed"])
pc = R.RANSACCloud(c["xyz"], c["nrm"], subs)
types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
rp = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 16384, "τ": 900, "prob_det": 0.9})
rcp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
ts, ns = [], []
for r in range(6):
    pc.enable_all()
    got, secs, st = R.ransac(pc, rcp, seed=1234, return_stats=True)
    if r:
        ts.append(st["seconds"]); ns.append(len(got))
print("e2e cfg3 itermax 16384: %d shapes, rh_ransac median of 5: %.4f s (%s)" % (ns[0], float(np.median(ts)), " ".join("%.4f" % t for t in ts)))
