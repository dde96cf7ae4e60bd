"""CPU prototype: the classifier of the round kinds (score4_device.h, cls_round_ab with the records of cls_make) in the squared
quantities n2 = |q|^2 and s |s|, s = sgn (q . np), against the form with the reciprocal root (nr = n2 rsq(n2), s / nr) it
replaced.  numpy only, no GPU: a cfg3-style cloud (synth, 2M points, subset 1 of 32 = 62 500 points), the first 400 sphere and
400 cylinder candidates of the bench's jittered_candidates, three threshold settings.  Both forms are evaluated in binary32 --
every fused multiply-add as one binary64 operation rounded to binary32 -- with the margins of their cls_make, and held against
the exact binary64 test in the reference's operation order:

    violations   points a form calls surely-in that the exact test rejects, or surely-out that it accepts (must be 0)
    undecided    points a form sends to the exact test (0 <= u <= 1)
    worst        max |x32 - x64| / width of the two scaled quantities where ua64 < 2 (the audit's limit is 0.3)
    crude        undecided points of the squared form when the margin of the normal half covers every |s| <= sqrt(3) Nm nrmax
                 instead of |s| <= cos(alpha) nrmax + ds (why that is enough: score4_device.h)

Not part of the product or the tests: a design aid (DESIGN.md sections 4 and 11; the GPU's counters are in profiles/r10).

    python tools/proto/root_free.py [points [candidates per kind]]"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ransac_jl_amd import synth

U = 2.0 ** -24
S = 2.0
S3 = math.sqrt(3.0)
f32 = np.float32


def fma(a, b, c):
    """binary32 operands (the product is exact in binary64), one rounding to binary64, one to binary32"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def margins(kind, v, eps, cosa, M, Nm):
    """e, mD as cls_make has them; the old form's (mN, wD, wN) and the new form's (m2, mv, mv_crude); usable flags"""
    if kind == "sphere":
        c0, R = v[0:3], v[3]
        e = 2.01 * U * (M + np.abs(c0).max())
    else:
        a, c0, R = v[0:3], v[3:6], v[6]
        e = U * (M + np.abs(c0).max()) * (3.01 + 8.04 * np.abs(a).max() * np.abs(a).sum())
    mD = S * (S3 * e + 7.0 * U * (abs(R) + abs(eps))) + 1e-30
    nrmax, nrmin = R + eps + 3.0 * mD, R - eps - 3.0 * mD
    old = None
    if nrmin > 0:
        mN = S * ((3.0 * Nm + S3 * (abs(cosa) + 0.25)) * e / nrmin + (8.7 * Nm + 6.0 * (abs(cosa) + 0.25)) * U) + 1e-30
        if mN <= 0.25 and cosa - (mN + 8.0 * U * Nm) > 0:
            old = (2.0 * mD, 2.0 * (mN + 8.0 * U * Nm))
    nq = nrmax + S3 * e
    K, c2 = R * R + eps * eps, cosa * cosa
    dn2 = 2.0 * nrmax * S3 * e + 3.0 * e * e + 4.0 * U * nq * nq + 6.0 * U * K
    m2 = S * dn2 + 1e-30
    ds = 3.0 * Nm * e + 5.0 * U * Nm * S3 * nq
    rest = ds * ds + c2 * dn2 + 8.0 * U * c2 * nq * nq
    mv = S * (2.0 * (cosa * nrmax + ds) * ds + rest) + 1e-30
    mvc = S * (2.0 * (S3 * Nm * nrmax) * ds + rest) + 1e-30
    n2min = (R - eps) ** 2 - 2.0 * m2
    ok = lambda m: eps >= 0 and cosa > 0 and nrmin > 0 and n2min > 0 and c2 * n2min > 1.001 * m
    return old, ((m2, mv) if ok(mv) else None), ((m2, mvc) if ok(mvc) else None)


def evaluate(kind, v, sgn, P, Nn, eps, cosa, M, Nm):
    """per form: (violations, undecided, worst a, worst b), or None where the candidate is exact-only"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    nx, ny, nz = Nn[:, 0], Nn[:, 1], Nn[:, 2]
    X, Y, Z, NX, NY, NZ = (a.astype(f32) for a in (x, y, z, nx, ny, nz))
    if kind == "sphere":
        qx, qy, qz, R = x - v[0], y - v[1], z - v[2], v[3]
        QX, QY, QZ = X - f32(v[0]), Y - f32(v[1]), Z - f32(v[2])
    else:
        ax, ay, az, cx, cy, cz, R = v[:7]
        tx, ty, tz = x - cx, y - cy, z - cz
        sd = (ax * tx + ay * ty) + az * tz
        qx, qy, qz = (x - ax * sd) - cx, (y - ay * sd) - cy, (z - az * sd) - cz
        TX, TY, TZ = X - f32(cx), Y - f32(cy), Z - f32(cz)
        SD = fma(TZ, f32(az), fma(TY, f32(ay), TX * f32(ax)))
        QX, QY, QZ = fma(SD, -f32(ax), TX), fma(SD, -f32(ay), TY), fma(SD, -f32(az), TZ)
    n2 = (qx * qx + qy * qy) + qz * qz
    nr = np.sqrt(n2)
    inv = 1.0 / nr
    dt = ((inv * qx) * nx + (inv * qy) * ny) + (inv * qz) * nz
    acc = (np.abs(nr - R) < eps) & (sgn * dt > cosa)
    qn = (qx * nx + qy * ny) + qz * nz
    N2 = fma(QZ, QZ, fma(QY, QY, QX * QX))
    QN = fma(QZ, NZ, fma(QY, NY, QX * NX))
    old, new, crude = margins(kind, v, eps, cosa, M, Nm)
    out = []
    if old is None:
        out.append(None)
    else:
        wD, wN = old
        eDlo, cNhi = eps - 0.5 * wD, cosa + 0.5 * wN
        INR = (1.0 / np.sqrt((N2 + f32(1e-37)).astype(np.float64))).astype(f32)
        NR, DT = N2 * INR, QN * INR
        ua = fma(np.abs(NR - f32(R)), f32(1.0 / wD), f32(-eDlo / wD))
        ub = fma(DT, f32(-sgn / wN), f32(cNhi / wN))
        a64, b64 = (np.abs(nr - R) - eDlo) / wD, (cNhi - sgn * dt) / wN
        out.append((ua, ub, a64, b64))
    for m in (new, crude):
        if m is None:
            out.append(None)
            continue
        m2, mv = m
        W2, Wv = 2.0 * m2, 2.0 * mv
        K, H = R * R + eps * eps, 2.0 * R * eps
        ua = fma(np.abs(N2 - f32(K)), f32(1.0 / W2), f32(-(H - m2) / W2))
        ub = fma(QN * np.abs(QN), f32(-sgn / Wv), fma(N2, f32(cosa * cosa / Wv), f32(0.5)))
        a64 = (np.abs(n2 - K) - (H - m2)) / W2
        b64 = (mv + (cosa * cosa * n2 - sgn * qn * np.abs(qn))) / Wv
        out.append((ua, ub, a64, b64))
    res = []
    for o in out:
        if o is None:
            res.append(None)
            continue
        ua, ub, a64, b64 = o
        u = np.maximum(ua, ub)
        near = a64 < 2.0
        res.append((int(((u < 0) & ~acc).sum() + ((u > 1) & acc).sum()), int(((u >= 0) & (u <= 1)).sum()),
                    float(np.abs(ua[near] - a64[near]).max(initial=0.0)), float(np.abs(ub[near] - b64[near]).max(initial=0.0))))
    return res, len(P)


def main():
    npts = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    ncand = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    prim = ["plane"] * 16 + ["sphere"] * 12 + ["cylinder"] * 12
    xyz, nrm, truth = synth.make_cloud(npts, prim, 0.30, seed=3)
    subs = synth.make_subsets(npts, 32, seed=3)
    P, Nn = xyz[subs[0] - 1], nrm[subs[0] - 1]
    M, Nm = np.abs(xyz).max(), np.abs(nrm).max()
    cands = synth.jittered_candidates(truth, 4096, seed=0)
    picks = [c for c in cands if c[0] == "sphere"][:ncand] + [c for c in cands if c[0] == "cylinder"][:ncand]
    print("%d subset points, %d candidates" % (len(P), len(picks)))
    print("%-14s %-8s %10s %12s %12s %10s %10s %8s" % ("(eps, alpha)", "form", "violations", "undecided", "exact-only", "worst a", "worst b", "vs old"))
    for eps, adeg in ((0.3, 5.0), (0.01, 1.0), (5.0, 60.0)):
        cosa = math.cos(math.radians(adeg))
        tot = {k: [0, 0, 0, 0.0, 0.0] for k in ("old", "new", "crude")}
        for kind, outw, v in picks:
            res, n = evaluate(kind, np.asarray(v, dtype=float), 1.0 if outw else -1.0, P, Nn, eps, cosa, M, Nm)
            for k, r in zip(("old", "new", "crude"), res):
                t = tot[k]
                if r is None:
                    t[1] += n; t[2] += 1          # exact-only: every point undecided
                else:
                    t[0] += r[0]; t[1] += r[1]; t[3] = max(t[3], r[2]); t[4] = max(t[4], r[3])
        for k in ("old", "new", "crude"):
            t = tot[k]
            print("%-14s %-8s %10d %12d %12d %10.3f %10.3f %+7.1f%%" % ("(%g, %g)" % (eps, adeg), k, t[0], t[1], t[2], t[3], t[4],
                                                                       100.0 * (t[1] / max(1, tot["old"][1]) - 1.0)))


if __name__ == "__main__":
    main()
