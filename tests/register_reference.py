"""The numpy twin of rh_register (include/ransac_hip.h), written from the header: brute-force nearest neighbours in the
order rh_knn_query fixes, every sum through ref_tree, Cholesky and the Cayley step in Python floats in the stated order.
tests/test_register_gpu.py holds the library to it for equality; tests/test_register_host.py pins the twin itself."""
import math

import numpy as np

from test_knn_host import ref_tree

CONVERGED, MAX_ITER, DEGENERATE, TOO_FEW = 0, 1, 2, 3
STATUS = {CONVERGED: "converged", MAX_ITER: "max_iter", DEGENERATE: "degenerate", TOO_FEW: "too_few"}


def ref_nearest(ref, pts, radius=0.0):
    """nn (0-based, -1: not valid) of every point: the first entry of rh_knn_query's order -- smallest
    d^2 = (dx*dx + dy*dy) + dz*dz with dx = r.x - p.x, ties to the smaller reference index (argmin takes the first)."""
    m = pts.shape[0]
    nn = np.empty(m, dtype=np.int64)
    d2 = np.empty(m)
    for lo in range(0, m, 512):
        p = pts[lo:lo + 512]
        dx = ref[None, :, 0] - p[:, None, 0]
        dy = ref[None, :, 1] - p[:, None, 1]
        dz = ref[None, :, 2] - p[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        at = np.argmin(d, axis=1)
        nn[lo:lo + len(p)] = at
        d2[lo:lo + len(p)] = d[np.arange(len(p)), at]
    if radius > 0:
        nn[~(d2 <= radius * radius)] = -1
    return nn


def S(leaf):
    """S() of the header: T() + 0.0"""
    return float(ref_tree(leaf)) + 0.0


def ref_cholesky_solve(H, g):
    """Step 6: x of H x = g, or None when a pivot is refused.  H: 6x6 nested lists (symmetric), g: 6 floats."""
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            v = H[j][i]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            if j < i:
                L[i][j] = v / L[j][j]
            else:
                if not v > 1e-10 * H[i][i]:
                    return None
                L[i][i] = math.sqrt(v)
    z, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = g[i]
        for k in range(i):
            v = v - L[i][k] * z[k]
        z[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = z[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x


def ref_cayley_update(x, R, t):
    """Step 7: the new (R, t) as nested lists / list of Python floats."""
    a0, a1, a2 = 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    d, f = 1.0 + aa, 1.0 - aa
    Cm = [[(f + 2.0 * (a0 * a0)) / d, (2.0 * (a0 * a1) - 2.0 * a2) / d, (2.0 * (a0 * a2) + 2.0 * a1) / d],
          [(2.0 * (a0 * a1) + 2.0 * a2) / d, (f + 2.0 * (a1 * a1)) / d, (2.0 * (a1 * a2) - 2.0 * a0) / d],
          [(2.0 * (a0 * a2) - 2.0 * a1) / d, (2.0 * (a1 * a2) + 2.0 * a0) / d, (f + 2.0 * (a2 * a2)) / d]]
    Rn = [[(Cm[k][0] * R[0][l] + Cm[k][1] * R[1][l]) + Cm[k][2] * R[2][l] for l in range(3)] for k in range(3)]
    tn = [((Cm[k][0] * t[0] + Cm[k][1] * t[1]) + Cm[k][2] * t[2]) + x[3 + k] for k in range(3)]
    return Rn, tn


def ref_register(ref, qry, normals=None, metric=None, radius=0.0, max_iter=50, rot_tol=1e-9, trans_tol=1e-9, init=None):
    """rh_register, step by step.  Returns a dict: transform (3x4), status, iterations, n_valid, rms, n_valid_it (int32
    [max_iter]) and rms_it ([max_iter])."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float64).reshape(-1, 3)
    if metric is None:
        metric = "point" if normals is None else "plane"
    nrm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    c = 0.5 * (ref.min(axis=0) + ref.max(axis=0))
    A = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]) if init is None else np.asarray(init, dtype=np.float64)[:3]
    cf = [float(v) for v in c]
    R = [[float(A[k, l]) for l in range(3)] for k in range(3)]
    t = [(((R[k][0] * cf[0] + R[k][1] * cf[1]) + R[k][2] * cf[2]) + float(A[k, 3])) - cf[k] for k in range(3)]
    y = qry - c
    n_valid_it, rms_it = np.zeros(max_iter, dtype=np.int32), np.zeros(max_iter)
    status, iters, nv, rms = MAX_ITER, 0, 0, 0.0
    for it in range(max_iter):
        yp = np.stack([((R[k][0] * y[:, 0] + R[k][1] * y[:, 1]) + R[k][2] * y[:, 2]) + t[k] for k in range(3)], axis=1)
        nn = ref_nearest(ref, yp + c, radius)
        valid = nn >= 0
        at = np.where(valid, nn, 0)
        nv = int(valid.sum())
        e = (ref[at] - c) - yp
        y0, y1, y2 = yp[:, 0], yp[:, 1], yp[:, 2]

        def Sv(leaf):
            return S(np.where(valid, leaf, 0.0))

        H = [[0.0] * 6 for _ in range(6)]
        if metric == "plane":
            n0, n1, n2 = nrm[at, 0], nrm[at, 1], nrm[at, 2]
            a = [y1 * n2 - y2 * n1, y2 * n0 - y0 * n2, y0 * n1 - y1 * n0, n0, n1, n2]
            b = (e[:, 0] * n0 + e[:, 1] * n1) + e[:, 2] * n2
            for u in range(6):
                for v in range(u, 6):
                    H[u][v] = H[v][u] = Sv(a[u] * a[v])
            g = [Sv(a[u] * b) for u in range(6)]
            E = Sv(b * b)
        else:
            P00, P11, P22 = Sv(y0 * y0), Sv(y1 * y1), Sv(y2 * y2)
            P01, P02, P12 = Sv(y0 * y1), Sv(y0 * y2), Sv(y1 * y2)
            Y0, Y1, Y2 = Sv(y0), Sv(y1), Sv(y2)
            H[0][0], H[1][1], H[2][2] = P11 + P22, P00 + P22, P00 + P11
            H[0][1] = H[1][0] = -P01
            H[0][2] = H[2][0] = -P02
            H[1][2] = H[2][1] = -P12
            H[0][4] = H[4][0] = -Y2
            H[0][5] = H[5][0] = Y1
            H[1][3] = H[3][1] = Y2
            H[1][5] = H[5][1] = -Y0
            H[2][3] = H[3][2] = -Y1
            H[2][4] = H[4][2] = Y0
            H[3][3] = H[4][4] = H[5][5] = float(nv)
            g = [Sv(y1 * e[:, 2] - y2 * e[:, 1]), Sv(y2 * e[:, 0] - y0 * e[:, 2]), Sv(y0 * e[:, 1] - y1 * e[:, 0]),
                 Sv(e[:, 0]), Sv(e[:, 1]), Sv(e[:, 2])]
            E = Sv((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        rms = math.sqrt(E / float(nv)) if nv else 0.0
        n_valid_it[it], rms_it[it] = nv, rms
        iters = it + 1
        if nv < 6:
            status = TOO_FEW
            break
        x = ref_cholesky_solve(H, g)
        if x is None:
            status = DEGENERATE
            break
        R, t = ref_cayley_update(x, R, t)
        if (math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) <= rot_tol
                and math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) <= trans_tol):
            status = CONVERGED
            break
    T = np.zeros((3, 4))
    for k in range(3):
        T[k, :3] = R[k]
        T[k, 3] = (t[k] + cf[k]) - ((R[k][0] * cf[0] + R[k][1] * cf[1]) + R[k][2] * cf[2])
    return dict(transform=T, status=status, iterations=iters, n_valid=nv, rms=rms, n_valid_it=n_valid_it, rms_it=rms_it)


def apply(T, pts):
    """the transform on points, in the state's operation order"""
    pts = np.asarray(pts, dtype=np.float64)
    return np.stack([((T[k, 0] * pts[:, 0] + T[k, 1] * pts[:, 1]) + T[k, 2] * pts[:, 2]) + T[k, 3] for k in range(3)], axis=1)


def rigid(deg, shift, seed, about):
    """a 3x4 motion: a turn by deg about a random axis through `about`, then a shift of length `shift` in a random direction"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = math.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    d = rng.normal(size=3)
    d *= shift / np.linalg.norm(d)
    return np.hstack([Rm, (about - Rm @ about + d)[:, None]])
