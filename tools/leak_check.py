#!/usr/bin/env python3
"""Repeated cloud creation / scoring (host batches, and device batches with four in flight) / rh_ransac: device and
host memory must stay flat."""
import ctypes as C
import os, sys, resource
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, dist as rdist, synth

xyz, nrm, truth = synth.make_cloud(60_000, ["plane", "sphere", "cylinder", "cone"], 0.2, seed=3)
subs = synth.make_subsets(60_000, 2, seed=3)
params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone],
                            iteration={"minsubsetN": 64, "itermax": 64, "τ": 300, "prob_det": 0.7})
shapes = [R.FittedPlane(truth[0]["point"], truth[0]["normal"])] * 50
cparams = R.params_to_c(params)
shapes_c = (L.Shape * len(shapes))(*[s.to_c() for s in shapes])
words = (subs[0].size + 63) // 64
ring_counts = [torch.zeros(len(shapes), dtype=torch.int32, device="cuda") for _ in range(4)]
ring_masks = [torch.zeros(len(shapes) * words, dtype=torch.int64, device="cuda") for _ in range(4)]


def batches_in_flight(pc):
    """every batch slot of the cloud gets its stream and its workspaces (counts only, then with masks -- a slot whose rows
    span several segments also holds a segment-mask table of its own): the cloud's destruction has to free them all"""
    lib = R.lib()
    bt = rdist.DeviceBatch(pc, shapes_c, len(shapes))
    R.set_option("batches_in_flight", 4, cloud=pc)
    R.set_option("st_cull", 1, cloud=pc)      # (super-tile lists whenever possible: the slots' list buffers as well)
    for with_masks in (False, True):
        for k in range(8):
            masks = C.c_void_p(ring_masks[k % 4].data_ptr()) if with_masks else None
            L.check(lib.rh_score_batch_dev(pc._h, bt.slice_ptr(0), len(shapes), C.byref(cparams), C.c_void_p(ring_counts[k % 4].data_ptr()), masks))
    L.check(lib.rh_cloud_sync(pc._h))
    R.set_option("batches_in_flight", None, cloud=pc)
    R.set_option("st_cull", None, cloud=pc)
    bt.free()


def snapshot():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2**20, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024

for rnd in range(6):
    for i in range(50):
        pc = R.RANSACCloud(xyz, nrm, subs)
        R.score_batch(pc, shapes, params, want_masks=(i % 2 == 0))
        batches_in_flight(pc)
        for mode in (0, 1):
            got, _ = R.ransac(pc, params, seed=i, sampling_streams=mode, octree_sampling=bool(mode and i % 3 == 0))
        if i % 10 == 0:   # a Float32 cloud's loop, the reference octree and its device gather as well
            pc32 = R.RANSACCloud(xyz, nrm, subs, force_eltype=np.float32)
            p32 = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder], iteration={"minsubsetN": 64, "itermax": 32, "τ": 300, "prob_det": 0.7})
            R.ransac(pc32, p32, seed=i, sampling_streams=1)
            R.cell_enabled_points(pc, pc.octree.children[0])
            del pc32
        del pc, got
    dev, host = snapshot()
    print("after %3d clouds / %3d ransac calls: device %.0f MiB in use, host max RSS %.0f MiB" % ((rnd + 1) * 50, (rnd + 1) * 100, dev, host), flush=True)
