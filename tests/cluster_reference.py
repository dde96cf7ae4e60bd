"""The numpy twin of rh_cluster (include/ransac_hip.h states the definition in full): density-based clustering by brute
force, every decision the binary64 comparison or the integer arithmetic the header names.  No grid, no cell, no order of
processing: the n x n matrix of d^2 in row chunks, the core flags from its row sums, the clusters by a breadth-first
search over the core-core edges, the border points by the row minimum over the core columns.
tests/test_cluster_host.py pins the twin by hand-derived cases, tests/test_cluster_gpu.py holds the library to it."""
import numpy as np

NOISE, BORDER, CORE = 0, 1, 2
ROWS = 512          # rows of the d^2 matrix held at a time


def d2_rows(xyz, a, b):
    """d^2 of the points a .. b - 1 to every point: (dx*dx + dy*dy) + dz*dz, each operation rounded on its own"""
    dx = xyz[a:b, None, 0] - xyz[None, :, 0]
    dy = xyz[a:b, None, 1] - xyz[None, :, 1]
    dz = xyz[a:b, None, 2] - xyz[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _neighbour_rows(xyz, eps2):
    """per row chunk: (a, b, d2, nb) with nb[r, j] = j is a neighbour of a + r"""
    n = len(xyz)
    for a in range(0, n, ROWS):
        b = min(n, a + ROWS)
        d2 = d2_rows(xyz, a, b)
        nb = d2 <= eps2
        nb[np.arange(b - a), np.arange(a, b)] = False      # left out by its index: a duplicate stays a neighbour
        yield a, b, d2, nb


def components(n, core, ei, ej):
    """comp[i] = the smallest core index of the connected component of core point i in the graph of the edges (ei, ej),
    -1 for a point that is no core point.  Breadth-first, a whole frontier at a time."""
    both_i, both_j = np.concatenate([ei, ej]), np.concatenate([ej, ei])
    order = np.argsort(both_i, kind="stable")
    adj = both_j[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(both_i, minlength=n), out=ptr[1:])
    comp = np.full(n, -1, dtype=np.int64)
    for s in np.flatnonzero(core):
        if comp[s] >= 0:
            continue
        comp[s] = s
        front = np.array([s], dtype=np.int64)
        while front.size:
            lens = ptr[front + 1] - ptr[front]
            tot = int(lens.sum())
            if tot == 0:
                break
            first = np.repeat(ptr[front] - (np.cumsum(lens) - lens), lens)
            nxt = adj[first + np.arange(tot)]
            nxt = np.unique(nxt[comp[nxt] < 0])
            comp[nxt] = s
            front = nxt
    return comp


def ref_cluster(xyz, eps, min_pts=8, min_size=1, order="index", return_graph=False):
    """rh_cluster.  Returns a dict: labels (int32), kind (uint8), counts (int64 [M + 1], noise first), offsets (int64
    [M + 2]), idx (int64 [n], 1-based, grouped by label, ascending within a label), lists (the M + 1 index arrays),
    n_clusters, n_core, n_border, n_noise, n_small, largest.  With return_graph also n_core_components (the clusters
    before the min_size filter) and edges (the core-core pairs i < j)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    eps2 = np.float64(eps) * np.float64(eps)
    deg = np.zeros(n, dtype=np.int64)
    for a, b, _, nb in _neighbour_rows(xyz, eps2):
        deg[a:b] = nb.sum(axis=1)
    core = 1 + deg >= min_pts
    ei, ej = [], []
    near = np.full(n, -1, dtype=np.int64)                   # the nearest core neighbour of a point that is no core point
    for a, b, d2, nb in _neighbour_rows(xyz, eps2):
        nb &= core[None, :]
        r, j = np.nonzero(nb & core[a:b, None])
        up = a + r < j                                      # every pair once
        ei.append(a + r[up])
        ej.append(j[up])
        masked = np.where(nb, d2, np.inf)
        first_min = np.argmin(masked, axis=1)               # the first minimum: ties to the smaller index
        has = np.isfinite(masked[np.arange(b - a), first_min]) & ~core[a:b]
        near[a:b][has] = first_min[has]
    ei, ej = np.concatenate(ei).astype(np.int64), np.concatenate(ej).astype(np.int64)
    comp = components(n, core, ei, ej)
    root = np.where(core, comp, np.where(near >= 0, comp[np.maximum(near, 0)], -1))
    kind = np.where(core, CORE, np.where(near >= 0, BORDER, NOISE)).astype(np.uint8)
    size = np.bincount(root[root >= 0], minlength=n)
    roots = np.flatnonzero((comp == np.arange(n)) & (size >= min_size))     # ascending: the numbering by index
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
               lists=[idx[offsets[k]:offsets[k + 1]] for k in range(m + 1)], n_clusters=m, n_core=int(core.sum()),
               n_border=int((kind == BORDER).sum()), n_noise=int((kind == NOISE).sum()),
               n_small=int(((kind != NOISE) & (labels == 0)).sum()), largest=int(counts[1:].max()) if m else 0)
    if return_graph:
        out["n_core_components"] = int((comp == np.arange(n)).sum())
        out["edges"] = (ei, ej)
    return out
