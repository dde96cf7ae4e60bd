#!/usr/bin/env python3
"""Global registration at working size, stage by stage: rh_describe on both clouds, rh_match_features (plain and mutual),
rh_register_global, and the rh_register refinement that follows.  The clouds: the even and the odd points of the cfg
cloud (cfg2: 1M points with normals) -- two disjoint samples of one scene -- each thinned with voxeldownsample (mode
"first": points and normals stay as they are) at a voxel width of --voxel point spacings, the second one turned by 137
degrees and shifted.  Device arrays in and out.
   python tools/global_time.py [cfg2] [--voxel=4] [--k=32] [--trials=20000] [--out=profiles/global/global_time.txt]
Wall times of whole calls (one warm-up, then the median of five with minimum and maximum); the result is printed and
written to --out."""
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
CFGS = [a for a in sys.argv[1:] if not a.startswith("--")] or ["cfg2"]


def flag(name, default, conv=float):
    for a in FLAGS:
        if a.startswith("--%s=" % name):
            return conv(a.split("=", 1)[1])
    return default


VOXEL, K, TRIALS = flag("voxel", 4.0), flag("k", 32, int), flag("trials", 20000, int)
OUT = flag("out", os.path.join(ROOT, "profiles", "global", "global_time.txt"), str)


def rigid(deg, shift, about):
    ax = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    th = math.radians(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    return np.hstack([Rm, (about - Rm @ about + shift)[:, None]])


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
            torch.cuda.synchronize()
            runs.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(runs)), min(runs), max(runs)

    lib = R.lib()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for cfg in CFGS:
        c = R.synth.config(cfg)
        xyz, nrm = np.ascontiguousarray(c["xyz"]), np.ascontiguousarray(c["nrm"])
        spacing = R.synth.median_nn_distance(xyz)
        beta = VOXEL * spacing
        ref, rn = R.voxeldownsample(np.ascontiguousarray(xyz[0::2]), beta, normals=np.ascontiguousarray(nrm[0::2]), mode="first")
        qry, qn = R.voxeldownsample(np.ascontiguousarray(xyz[1::2]), beta, normals=np.ascontiguousarray(nrm[1::2]), mode="first")
        motion = rigid(137.0, np.array([300.0, -200.0, 100.0]), xyz.mean(axis=0))
        truth = qry
        qry = np.ascontiguousarray(R.transform_points(motion, qry))
        qn = np.ascontiguousarray(R.transform_normals(motion, qn))
        n, m = len(ref), len(qry)
        thin = R.synth.median_nn_distance(ref)
        tau = 1.5 * thin
        d_ref, d_rn, d_qry, d_qn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ref, rn, qry, qn))
        d_dr = torch.zeros((n, L.DESC_DIM), dtype=torch.int16, device="cuda")
        d_dq = torch.zeros((m, L.DESC_DIM), dtype=torch.int16, device="cuda")
        d_idx = torch.zeros(m, dtype=torch.int32, device="cuda")
        dp, u16, i32 = C.c_double, C.c_uint16, C.c_int32

        def describe(x, nr, cnt, out):
            L.check(lib.rh_describe(dptr(x, dp), dptr(nr, dp), cnt, K, 0.0, 0, dptr(out, u16), None))

        def match(flags):
            L.check(lib.rh_match_features(dptr(d_dr, u16), n, dptr(d_dq, u16), m, flags, 0, dptr(d_idx, i32), None))

        say("%s: %d points, spacing %.4g, voxel %.4g -> reference %d, queries %d points, spacing %.4g, tau %.4g, k %d, %d trials"
            % (cfg, len(xyz), spacing, beta, n, m, thin, tau, K, TRIALS))
        t = timed(lambda: describe(d_ref, d_rn, n, d_dr))
        say("  rh_describe reference       %9.2f ms (%.2f - %.2f)" % t)
        t = timed(lambda: describe(d_qry, d_qn, m, d_dq))
        say("  rh_describe queries         %9.2f ms (%.2f - %.2f)" % t)
        t = timed(lambda: match(L.MATCH_MUTUAL))
        say("  rh_match_features mutual    %9.2f ms (%.2f - %.2f)" % t)
        t = timed(lambda: match(0))
        pairs = float(n) * float(m)
        say("  rh_match_features           %9.2f ms (%.2f - %.2f): %.3g pairs, %.1f G pairs/s, %.2f T multiply-adds/s"
            % (t + (pairs, pairs / t[0] / 1e6, pairs * 33 / t[0] / 1e9)))
        idx = d_idx.cpu().numpy()
        good = np.linalg.norm(truth - ref[idx - 1], axis=1) <= tau
        cq = torch.arange(1, m + 1, dtype=torch.int32, device="cuda")
        out, res = np.zeros((3, 4)), L.GlobalResult()
        prm = L.GlobalParams(trials=TRIALS, seed=1, tau=tau, edge_ratio=0.9, min_edge=0.0)

        def ransac():
            L.check(lib.rh_register_global(dptr(d_ref, dp), n, dptr(d_qry, dp), m, dptr(cq, i32), dptr(d_idx, i32), m, C.byref(prm),
                                           None, 0, out.ctypes.data_as(C.POINTER(dp)), C.byref(res), None))

        t = timed(ransac)
        say("  rh_register_global          %9.2f ms (%.2f - %.2f): %d correspondences (%.1f %% within tau of the truth), %d valid "
            "trials, best count %d" % (t + (m, 100.0 * good.mean(), res.n_valid_trials, res.best_count)))
        inv = np.hstack([motion[:, :3].T, -(motion[:, :3].T @ motion[:, 3])[:, None]])
        Mr = out[:, :3] @ inv[:, :3].T
        rot = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Mr) - 1.0) / 2.0))))
        say("  coarse result: %.2f degrees from the true rotation, largest point error %.4g (%.2f thinned spacings)"
            % (rot, np.linalg.norm(R.transform_points(out, qry) - truth, axis=1).max(),
               np.linalg.norm(R.transform_points(out, qry) - truth, axis=1).max() / thin))
        rp = L.RegisterParams(radius=3.0 * tau, rot_tol=1e-9, trans_tol=1e-9, metric=L.DIST_PLANE, max_iter=50)
        fin, rres = np.zeros((3, 4)), L.RegisterResult()

        def refine():
            L.check(lib.rh_register(dptr(d_ref, dp), dptr(d_rn, dp), n, dptr(d_qry, dp), m, C.byref(rp), out.ctypes.data_as(C.POINTER(dp)),
                                    0, fin.ctypes.data_as(C.POINTER(dp)), C.byref(rres), None, None))

        t = timed(refine)
        say("  rh_register from it         %9.2f ms (%.2f - %.2f): %s after %d iterations, largest point error %.4g"
            % (t + (L.REG_STATUS_NAMES[rres.status], rres.iterations, np.linalg.norm(R.transform_points(fin, qry) - truth, axis=1).max())))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
