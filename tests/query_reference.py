"""The numpy twin of rh_knn_query and rh_cloud_distance (include/ransac_hip.h): brute force in the operation order the
header fixes, so that tests/test_query_gpu.py can hold the library to it for equality.  tests/test_query_host.py pins the
twin itself by hand-derived cases."""
import numpy as np

from test_knn_host import ref_tree


def ref_query_order(ref, qry, kmax):
    """The first kmax reference points of every query's order, nothing left out: (idx [m, kmax] 0-based, d2 [m, kmax]);
    -1 / inf past the end when n < kmax.  Equal d^2 keep the reference's index order (a stable sort)."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float64).reshape(-1, 3)
    n, m = ref.shape[0], qry.shape[0]
    kk = min(kmax, n)
    idx = np.full((m, kmax), -1, dtype=np.int64)
    d2 = np.full((m, kmax), np.inf)
    for lo in range(0, m, 512):
        q = qry[lo:lo + 512]
        dx = ref[None, :, 0] - q[:, None, 0]
        dy = ref[None, :, 1] - q[:, None, 1]
        dz = ref[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        order = np.argsort(d, axis=1, kind="stable")[:, :kk]               # stable: equal d^2 keep index order
        idx[lo:lo + q.shape[0], :kk] = order
        d2[lo:lo + q.shape[0], :kk] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def ref_knn_query(ref, qry, k, radius=0.0, nb=None):
    """rh_knn_query: (idx [m, k] int32 1-based, 0 past count; d2 [m, k], +inf past count; count [m] int32).
    nb: ref_query_order(ref, qry, >= k), to share one search between calls."""
    idx, d2 = nb if nb is not None else ref_query_order(ref, qry, k)
    idx, d2 = idx[:, :k], d2[:, :k]
    use = idx >= 0
    if radius > 0:
        use &= d2 <= radius * radius
    return (np.where(use, idx + 1, 0).astype(np.int32), np.where(use, d2, np.inf), use.sum(axis=1).astype(np.int32))


def ref_cloud_distance(ref, qry, normals=None, radius=0.0, threshold=np.inf, metric=None):
    """rh_cloud_distance, step by step.  Returns a dict: dist [m], nn_idx [m] int32 (1-based, 0: not valid), n_valid,
    n_within, argmax (1-based, 0: none), mean, rms, max, median."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float64).reshape(-1, 3)
    if metric is None:
        metric = "point" if normals is None else "plane"
    idx, d2, count = ref_knn_query(ref, qry, 1, radius)
    nn, valid = idx[:, 0], count >= 1
    at = np.where(valid, nn - 1, 0)
    if metric == "plane":
        nrm = np.asarray(normals, dtype=np.float64).reshape(-1, 3)[at]
        e = qry - ref[at]
        d = np.abs((e[:, 0] * nrm[:, 0] + e[:, 1] * nrm[:, 1]) + e[:, 2] * nrm[:, 2])
    else:
        d = np.sqrt(np.where(valid, d2[:, 0], 0.0))
    dist = np.where(valid, d, np.inf)
    nv = int(valid.sum())
    dv = np.where(valid, d, 0.0)
    out = dict(dist=dist, nn_idx=np.where(valid, nn, 0).astype(np.int32), n_valid=nv,
               n_within=int((valid & (dist <= threshold)).sum()), argmax=0, mean=0.0, rms=0.0, max=0.0, median=0.0)
    if nv:
        out["mean"] = float(ref_tree(dv) / nv)
        out["rms"] = float(np.sqrt(ref_tree(dv * dv) / nv))
        out["max"] = float(d[valid].max())
        out["argmax"] = int(np.flatnonzero(valid & (d == out["max"]))[0]) + 1
        out["median"] = float(np.sort(d[valid])[(nv - 1) // 2])
    return out
