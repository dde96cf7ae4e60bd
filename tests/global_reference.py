"""The numpy twins of rh_describe, rh_match_features and rh_register_global (include/ransac_hip.h), written from the
header: brute-force neighbours in rh_knn's order, every pair feature in the stated operation order (numpy's elementwise
operations are single IEEE binary64 operations, nothing is contracted), hypotheses in Python floats.
tests/test_global_gpu.py holds the library to them for equality of bytes; tests/test_global_host.py pins the twins."""
import ctypes as C
import math

import numpy as np

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from register_reference import apply, ref_register
from test_knn_host import ref_knn

DIM, DESC_MAX = 33, 7938
OK, NO_TRIAL = 0, 1


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def ref_pair(pi, ni, pj, nj):
    """Step 2 for arrays of pairs (.., 3): (f1, f2, psi, degenerate)."""
    pi, ni, pj, nj = (np.asarray(a, dtype=np.float64) for a in (pi, ni, pj, nj))
    with np.errstate(all="ignore"):
        d = pj - pi
        d2 = dot(d, d)
        u, s = ni, nj
        v = cross(u, d)
        v2 = dot(v, v)
        w = cross(u, v)
        ln, vl = np.sqrt(d2), np.sqrt(v2)
        f1 = dot(u, d) / ln
        f2 = dot(v, s) / vl
        a = dot(w, s) / vl
        b = dot(u, s)
        g = np.abs(a) + np.abs(b)
        r = b / g
        psi = np.where(a >= 0.0, 1.0 - r, 3.0 + r)
        deg = (d2 == 0.0) | (v2 == 0.0) | (g == 0.0) | np.isnan(f1) | np.isnan(f2) | np.isnan(psi)
    return f1, f2, psi, deg


def ref_bin(x):
    """Step 3: clamp(floor(x), 0, 10), decided in binary64."""
    with np.errstate(all="ignore"):
        t = np.floor(np.asarray(x, dtype=np.float64))
        return np.where(t < 0.0, 0, np.where(t > 10.0, 10, np.nan_to_num(t, nan=0.0, posinf=10.0, neginf=0.0))).astype(np.int64)


def ref_bins(f1, f2, psi):
    return ref_bin((f1 + 1.0) * 5.5), ref_bin((f2 + 1.0) * 5.5), ref_bin(psi * 2.75)


def ref_describe(xyz, nrm, k, radius=0.0, nb=None):
    """rh_describe: (desc [n, 33] uint16, count [n] int32, S [n, 33])."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    idx, _, count = ref_knn(xyz, k, radius, nb)
    use = idx > 0
    j = np.where(use, idx - 1, 0).astype(np.int64)
    f1, f2, psi, deg = ref_pair(xyz[:, None, :], nrm[:, None, :], xyz[j], nrm[j])
    b1, b2, b3 = ref_bins(f1, f2, psi)
    add = use & ~deg
    S = np.zeros((n, DIM), dtype=np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], idx.shape)
    for off, b in ((0, b1), (11, b2), (22, b3)):
        np.add.at(S, (rows[add], off + b[add]), 1)
    D = count[:, None].astype(np.int64) * S + (S[j] * use[:, :, None]).sum(axis=1)
    assert D.max(initial=0) <= DESC_MAX
    return D.astype(np.uint16), count, S


def ref_sqdist(ref, qry):
    """sum_c (q_c - r_c)^2 for all pairs, [m, n] int64.  Formed as |q|^2 + |r|^2 - 2 q.r in binary64, where it is exact:
    every partial sum is an integer below 2^53 (tests/test_global_host.py holds it to the literal int64 form)."""
    r, q = np.asarray(ref, dtype=np.float64), np.asarray(qry, dtype=np.float64)
    d = (q * q).sum(axis=1)[:, None] + (r * r).sum(axis=1)[None, :] - 2.0 * (q @ r.T)
    return d.astype(np.int64)


def ref_match(ref, qry, mutual=False):
    """rh_match_features: (idx [m] int32 1-based, dist [m] uint32)."""
    m = len(qry)
    idx, dist = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    back_d = np.full(len(ref), np.iinfo(np.int64).max)
    back_i = np.zeros(len(ref), dtype=np.int64)
    for lo in range(0, m, 1024):
        d = ref_sqdist(ref, qry[lo:lo + 1024])
        at = np.argmin(d, axis=1)                                  # the first minimum: ties to the smaller index
        idx[lo:lo + len(at)] = at + 1
        dist[lo:lo + len(at)] = d[np.arange(len(at)), at]
        col = np.argmin(d, axis=0)                                 # from the reference side, chunk by chunk in query order
        cd = d[col, np.arange(len(ref))]
        better = cd < back_d                                       # strict: an earlier chunk's query keeps a tie
        back_d[better], back_i[better] = cd[better], lo + col[better] + 1
    if mutual:
        idx[back_i[idx - 1] != np.arange(1, m + 1)] = 0
    return idx.astype(np.int32), dist.astype(np.uint32)


# ------------------------------------------------------------------------ hypotheses ----
def fdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def ref_frame(x0, x1, x2):
    """Step 3: F as nested lists F[k][0 .. 2] = e1_k, e2_k, e3_k, or None when the frame does not exist."""
    h = [x1[k] - x0[k] for k in range(3)]
    hh = fdot(h, h)
    if not hh > 0.0:
        return None
    hl = math.sqrt(hh)
    e1 = [h[k] / hl for k in range(3)]
    gv = fcross(e1, [x2[k] - x0[k] for k in range(3)])
    g2 = fdot(gv, gv)
    if not g2 > 0.0:
        return None
    gl = math.sqrt(g2)
    e3 = [gv[k] / gl for k in range(3)]
    e2 = fcross(e3, e1)
    return [[e1[k], e2[k], e3[k]] for k in range(3)]


def ref_hypothesis(q, r, edge_ratio=0.9, min_edge=0.0):
    """Steps 2 to 4 for the triple q[0 .. 2] -> r[0 .. 2] (lists of 3 floats): (R nested lists, t list), or a string naming
    the clause that makes the trial not valid ("edge", "frame"; the caller tests the indices)."""
    ee, mm = edge_ratio * edge_ratio, min_edge * min_edge
    for x, y in ((0, 1), (0, 2), (1, 2)):
        dq = [q[x][k] - q[y][k] for k in range(3)]
        dr = [r[x][k] - r[y][k] for k in range(3)]
        lq, lr = fdot(dq, dq), fdot(dr, dr)
        if not lq >= ee * lr or not lr >= ee * lq or not lq >= mm:
            return "edge"
    Fq, Fr = ref_frame(*q), ref_frame(*r)
    if Fq is None or Fr is None:
        return "frame"
    cq = [((q[0][k] + q[1][k]) + q[2][k]) / 3.0 for k in range(3)]
    cr = [((r[0][k] + r[1][k]) + r[2][k]) / 3.0 for k in range(3)]
    Rm = [[(Fr[k][0] * Fq[l][0] + Fr[k][1] * Fq[l][1]) + Fr[k][2] * Fq[l][2] for l in range(3)] for k in range(3)]
    t = [cr[k] - ((Rm[k][0] * cq[0] + Rm[k][1] * cq[1]) + Rm[k][2] * cq[2]) for k in range(3)]
    return Rm, t


def ref_draw_triples(seed, trials, c):
    """Step 1: three draws rh_rng_range(c) - 1 per trial, in order (the library's host generator, which tests/test_abi.py
    holds to the oracle's)."""
    rng = L.Rng()
    lib = R.lib()
    lib.rh_rng_seed(C.byref(rng), seed)
    return np.array([lib.rh_rng_range(C.byref(rng), c) - 1 for _ in range(3 * trials)], dtype=np.int32).reshape(trials, 3)


def ref_count(T, q, r, tau):
    """Step 5 for one transform (3x4) over all pairs."""
    z = apply(T, q) - r
    return int((dot(z, z) <= tau * tau).sum())


def ref_global(ref, qry, corr_qry, corr_ref, tau, trials=None, seed=0, edge_ratio=0.9, min_edge=0.0, triples=None):
    """rh_register_global: dict transform (3x4), status, best_trial, best_count, n_valid_trials, counts (int32), triples."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float64).reshape(-1, 3)
    q, r = qry[np.asarray(corr_qry, dtype=np.int64) - 1], ref[np.asarray(corr_ref, dtype=np.int64) - 1]
    c = len(q)
    tri = ref_draw_triples(seed, trials, c) if triples is None else np.asarray(triples, dtype=np.int32).reshape(-1, 3)
    ql, rl = q.tolist(), r.tolist()
    counts = np.full(len(tri), -1, dtype=np.int32)
    hyp = {}
    for t, (a, b, d) in enumerate(tri.tolist()):
        if a == b or a == d or b == d:
            continue
        h = ref_hypothesis([ql[a], ql[b], ql[d]], [rl[a], rl[b], rl[d]], edge_ratio, min_edge)
        if isinstance(h, str):
            continue
        T = np.hstack([np.array(h[0]), np.array(h[1])[:, None]])
        hyp[t] = T
        counts[t] = ref_count(T, q, r, tau)
    best = int(np.argmax(counts)) if hyp else -1                   # the first maximum: ties to the smaller trial
    T = hyp[best] if hyp else np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    return dict(transform=T, status=OK if hyp else NO_TRIAL, best_trial=best, best_count=int(counts[best]) if hyp else -1,
                n_valid_trials=len(hyp), counts=counts, triples=tri)


def ref_register_global(ref, qry, ref_nrm, qry_nrm, tau, k=32, feature_radius=0.0, trials=20000, edge_ratio=0.9, min_edge=0.0,
                        mutual=False, seed=0, refine=True, radius=None):
    """R.register_global, stage by stage; dict with the coarse result of ref_global plus corr_qry, corr_ref and, with
    refine, "register" (ref_register's dict, plane metric) and "T" (3x4)."""
    dref, _, _ = ref_describe(ref, ref_nrm, k, feature_radius)
    dqry, _, _ = ref_describe(qry, qry_nrm, k, feature_radius)
    idx, _ = ref_match(dref, dqry, mutual)
    corr_qry = (np.flatnonzero(idx > 0) + 1).astype(np.int32)
    corr_ref = idx[idx > 0].astype(np.int32)
    out = ref_global(ref, qry, corr_qry, corr_ref, tau, trials, seed, edge_ratio, min_edge)
    out.update(corr_qry=corr_qry, corr_ref=corr_ref, T=out["transform"])
    if refine:
        out["register"] = ref_register(ref, qry, normals=ref_nrm, metric="plane", radius=3.0 * tau if radius is None else radius,
                                       init=out["transform"])
        out["T"] = out["register"]["transform"]
    return out
