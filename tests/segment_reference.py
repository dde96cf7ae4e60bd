"""The numpy twin of rh_segment_smooth (include/ransac_hip.h states the definition in full): region growing by smoothness
by brute force, every decision the binary64 comparison or the integer arithmetic the header names, step by step.  No
grid and no order of processing: rh_knn's lists from the n x n matrix of d^2 in row chunks (a stable argsort, the point
itself left out by its index), the pairs either way round, the regions by union-find over the smooth seed pairs, the
border points by the (d2, index) minimum over their smooth seed partners.
tests/test_segment_host.py pins the twin by hand-derived cases, tests/test_segment_gpu.py holds the library to it."""
import numpy as np

NOISE, BORDER, CORE = 0, 1, 2
UNSIGNED = 1
ROWS = 512          # rows of the d^2 matrix held at a time
STATS = ("n_regions", "n_seed", "n_border", "n_unassigned", "n_invalid", "n_small", "largest")


def knn_lists(X, k, radius=0.0):
    """step 2, directed: (i, j, d2) for every j in N(i), in the order of rh_knn's lists.  Also returns tie: a list was cut
    between two equal d^2 (the index decided who is a neighbour)."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    src, dst, dd, tie = [], [], [], False
    for lo in range(0, n, ROWS):
        q = X[lo:lo + ROWS]
        dx = X[None, :, 0] - q[:, None, 0]
        dy = X[None, :, 1] - q[:, None, 1]
        dz = X[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        d[np.arange(len(q)), lo + np.arange(len(q))] = -1.0                  # the point itself sorts first and is cut off
        full = np.argsort(d, axis=1, kind="stable")                          # stable: equal d^2 keep index order
        order = full[:, 1:k + 1]
        d2 = np.take_along_axis(d, order, axis=1)
        if order.shape[1] == k and n > k + 1:
            tie = tie or bool((np.take_along_axis(d, full[:, k + 1:k + 2], axis=1)[:, 0] == d2[:, -1]).any())
        use = np.ones(order.shape, dtype=bool) if radius <= 0 else d2 <= np.float64(radius) * np.float64(radius)
        rows = np.broadcast_to(lo + np.arange(len(q))[:, None], order.shape)
        src.append(rows[use]); dst.append(order[use]); dd.append(d2[use])
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, dtype=t)
    return cat(src, np.int64), cat(dst, np.int64), cat(dd, np.float64), tie


def in_v(N):
    """step 1: the points whose normal is not (0, 0, 0)"""
    return ~((N[:, 0] == 0.0) & (N[:, 1] == 0.0) & (N[:, 2] == 0.0))


def smooth_pairs(X, N, i, j, cos_angle, dist_max=0.0, flags=0):
    """step 3 for the pairs (i[t], j[t]), both ends in V: each operation rounded on its own"""
    ni, nj = N[i], N[j]
    dot = (ni[:, 0] * nj[:, 0] + ni[:, 1] * nj[:, 1]) + ni[:, 2] * nj[:, 2]
    a = np.abs(dot) if flags & UNSIGNED else dot
    ok = a >= np.float64(cos_angle)
    if dist_max > 0:
        dx, dy, dz = X[j, 0] - X[i, 0], X[j, 1] - X[i, 1], X[j, 2] - X[i, 2]
        ei = (ni[:, 0] * dx + ni[:, 1] * dy) + ni[:, 2] * dz
        ej = (nj[:, 0] * (-dx) + nj[:, 1] * (-dy)) + nj[:, 2] * (-dz)
        ok &= (np.abs(ei) <= np.float64(dist_max)) & (np.abs(ej) <= np.float64(dist_max))
    return ok


def components_uf(n, seed, ei, ej):
    """comp[i] = the smallest seed of the connected component of seed i under the edges (ei, ej), -1 for no seed:
    union-find, the smaller root stays"""
    parent = np.arange(n, dtype=np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(ei.tolist(), ej.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([find(a) for a in range(n)], dtype=np.int64)
    comp[~seed] = -1
    return comp


def components_propagate(n, seed, ei, ej):
    """the same components a second, independent way: every seed starts with its own index as its mark and takes the
    smallest mark among its neighbours, round after round, until nothing changes"""
    mark = np.where(seed, np.arange(n, dtype=np.int64), -1)
    while True:
        new = mark.copy()
        np.minimum.at(new, ei, mark[ej])
        np.minimum.at(new, ej, mark[ei])
        if np.array_equal(new, mark):
            return mark
        mark = new


def ref_segment(X, N, curv=None, k=16, radius=0.0, cos_angle=0.9, curv_max=0.05, dist_max=0.0, flags=0, min_size=1,
                order="size", return_graph=False):
    """rh_segment_smooth.  Returns a dict: labels (int32), kind (uint8), counts (int64 [M + 1], label 0 first), offsets
    (int64 [M + 2]), idx (int64 [n], 1-based, grouped by label, ascending within a label), lists, the fields of STATS, and
    the diagnostic counts
      contested     border points whose smooth seed partners lie in more than one region,
      reverse_only  border points whose winning seed is not in their own N(i),
      knn_tie       a neighbour list was cut between equal d^2,
      border_tie    a border point's smallest d2 is reached by more than one smooth seed partner.
    With return_graph also comp (the region root per seed, -1 otherwise) and edges (the smooth seed-seed pairs)."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    v = in_v(N)
    if curv is None:
        seed = v.copy()
    else:
        with np.errstate(invalid="ignore"):
            seed = v & (np.asarray(curv, dtype=np.float64).reshape(-1) <= np.float64(curv_max))   # a NaN makes no seed
    di, dj, dd, knn_tie = knn_lists(X, k, radius)
    # i ~ j: the directed pairs either way round; own[t]: j is in N(i) for the pair as seen from i
    pi, pj, pd = np.concatenate([di, dj]), np.concatenate([dj, di]), np.concatenate([dd, dd])
    own = np.concatenate([np.ones(len(di), dtype=bool), np.zeros(len(di), dtype=bool)])
    keep = v[pi] & v[pj]
    pi, pj, pd, own = pi[keep], pj[keep], pd[keep], own[keep]
    sm = smooth_pairs(X, N, pi, pj, cos_angle, dist_max, flags)
    pi, pj, pd, own = pi[sm], pj[sm], pd[sm], own[sm]
    # step 5
    ss = seed[pi] & seed[pj] & (pi < pj)
    comp = components_uf(n, seed, pi[ss], pj[ss])
    # step 6: from the non-seed end i to the seed end j, the smallest (d2, j)
    bo = ~seed[pi] & seed[pj]
    bi, bj, bd, bown = pi[bo], pj[bo], pd[bo], own[bo]
    srt = np.lexsort((bj, bd, bi))
    bi, bj, bd, bown = bi[srt], bj[srt], bd[srt], bown[srt]
    first = np.ones(len(bi), dtype=bool)
    first[1:] = bi[1:] != bi[:-1]
    near = np.full(n, -1, dtype=np.int64)
    near[bi[first]] = bj[first]
    is_border = near >= 0
    contested = reverse_only = border_tie = 0
    for i in np.flatnonzero(is_border):
        m = bi == i
        contested += len(np.unique(comp[bj[m]])) > 1
        reverse_only += not bown[m & (bj == near[i])].any()
        border_tie += len(np.unique(bj[m & (bd == bd[m][0])])) > 1
    root = np.where(seed, comp, np.where(is_border, comp[np.maximum(near, 0)], -1))
    kind = np.where(seed, CORE, np.where(is_border, BORDER, NOISE)).astype(np.uint8)
    # steps 8, 9: rh_cluster's
    size = np.bincount(root[root >= 0], minlength=n)
    roots = np.flatnonzero((comp == np.arange(n)) & (size >= min_size))
    if order in ("size", 1):
        roots = roots[np.lexsort((roots, -size[roots]))]
    elif order not in ("index", 0):
        raise ValueError("order %r" % (order,))
    m = len(roots)
    label_of_root = np.zeros(n + 1, dtype=np.int32)          # (slot n: root -1)
    label_of_root[roots] = np.arange(1, m + 1, dtype=np.int32)
    labels = label_of_root[root]
    counts = np.bincount(labels, minlength=m + 1).astype(np.int64)
    offsets = np.zeros(m + 2, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    idx = (np.argsort(labels, kind="stable") + 1).astype(np.int64)
    out = dict(labels=labels, kind=kind, counts=counts, offsets=offsets, idx=idx,
               lists=[idx[offsets[q]:offsets[q + 1]] for q in range(m + 1)], n_regions=m, n_seed=int(seed.sum()),
               n_border=int(is_border.sum()), n_unassigned=int((v & ~seed & ~is_border).sum()), n_invalid=int((~v).sum()),
               n_small=int(((kind != NOISE) & (labels == 0)).sum()), largest=int(counts[1:].max()) if m else 0,
               contested=int(contested), reverse_only=int(reverse_only), knn_tie=bool(knn_tie), border_tie=int(border_tie))
    if return_graph:
        out["comp"] = comp
        out["seed"] = seed
        out["edges"] = (pi[ss], pj[ss])
    return out
