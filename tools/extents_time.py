#!/usr/bin/env python3
"""What the extents of all extracted shapes cost: on the cfg2- and cfg3-sized synth scenes (1M / 10M points) run
ransac(), then time rh_result_extents for all shapes in one call --
   host    wall time of the synchronous call (lists uploaded from the result's pinned block, records read back): median
           of five calls after a warm-up;
   device  the four launches of rh_shape_extents_dev on resident lists, by the cloud's timer (HIP events): median of five;
           against the bytes the two passes move (8 B of index + 24 B of coordinates per listed point and pass);
   numpy   the twin of tests/test_extents_host.py on the same lists on the host, once.
   python tools/extents_time.py [cfg2 cfg3]"""
import ctypes as C
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
from ransac_jl_amd import _lib as L, synth
from test_extents_host import ref_extents

lib = R.lib()
for cfg in [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2", "cfg3"]:
    c = synth.config(cfg)
    xyz = c["xyz"]
    pc = R.RANSACCloud(xyz, c["nrm"], synth.make_subsets(len(xyz), c["r"], c["seed"]))
    types = [R.FittedPlane, R.FittedSphere, R.FittedCylinder]
    rp = R.ransacparameters(types, iteration={"minsubsetN": 4096, "itermax": 200, "τ": 900, "prob_det": 0.9})
    cp = R.params_to_c(rp, score_mode=L.SCORE_F64, sphere_uses_enabled=True, sampling_streams=1)
    R.ransac(pc, cp, setenabled=True, seed=99)                         # warm-up: the cloud's one-time allocations
    pc.enable_all()
    t0 = time.perf_counter()
    got, _ = R.ransac(pc, cp, seed=1234)
    t_ransac = 1e3 * (time.perf_counter() - t0)
    b, total = len(got), sum(e.inpoints.size for e in got)
    print("%s n=%d: ransac() %.1f ms, %d shapes, %d listed points" % (cfg, len(xyz), t_ransac, b, total), flush=True)

    # the host entry on the result's own lists: rebuild an rh_result over the views ransac() returned (they keep the pinned block alive)
    ex = (L.Extracted * b)()
    for j, e in enumerate(got):
        ex[j].shape = e.c_shape
        ex[j].n_inpoints = e.inpoints.size
        ex[j].inpoints = e.inpoints.ctypes.data_as(C.POINTER(C.c_int64))
    res = L.Result(shapes=ex, n_shapes=b)
    out = (L.Extent * b)()
    host = []
    for k in range(6):
        t0 = time.perf_counter()
        L.check(lib.rh_result_extents(pc._h, C.byref(res), out))
        host.append(1e3 * (time.perf_counter() - t0))
    t_host = float(np.median(host[1:]))

    # the device entry on resident lists
    arr = (L.Shape * b)(*[e.c_shape for e in got])
    off = np.zeros(b + 1, dtype=np.int64)
    np.cumsum([e.inpoints.size for e in got], out=off[1:])
    idx = np.concatenate([e.inpoints for e in got])
    bufs = []
    for src, nbytes in ((C.cast(arr, C.c_void_p), C.sizeof(arr)), (off.ctypes.data_as(C.c_void_p), off.nbytes),
                        (idx.ctypes.data_as(C.c_void_p), idx.nbytes), (None, C.sizeof(out))):
        d = C.c_void_p()
        L.check(lib.rh_dev_alloc(pc._h, nbytes, C.byref(d)))
        if src is not None:
            L.check(lib.rh_dev_upload(pc._h, d, src, nbytes))
        bufs.append(d)
    dev = []
    for k in range(6):
        ms = C.c_float()
        L.check(lib.rh_timer_start(pc._h))
        L.check(lib.rh_shape_extents_dev(pc._h, bufs[0], b, bufs[1], bufs[2], total, bufs[3]))
        L.check(lib.rh_timer_stop(pc._h, C.byref(ms)))
        dev.append(ms.value)
    t_dev = float(np.median(dev[1:]))
    out2 = (L.Extent * b)()
    L.check(lib.rh_dev_download(pc._h, C.cast(out2, C.c_void_p), bufs[3], C.sizeof(out2)))
    assert bytes(out2) == bytes(out), "the two entries disagree"
    for d in bufs:
        L.check(lib.rh_dev_free(pc._h, d))
    moved = 2 * 32 * total
    print("  rh_result_extents host wall %.3f ms   four launches on the device %.3f ms = %.0f GB/s of %d MB gathered"
          % (t_host, t_dev, moved / t_dev / 1e6, moved // 1000000), flush=True)

    t0 = time.perf_counter()
    refs = [ref_extents(xyz, e.c_shape, e.inpoints) for e in got]
    t_np = 1e3 * (time.perf_counter() - t0)
    worst = max(float(np.abs(np.array(o.lo) - r["lo"]).max()) for o, r in zip(out, refs))
    print("  numpy twin on the host %.1f ms (largest |lo - twin's lo| %.2e)" % (t_np, worst), flush=True)
    del pc, xyz
