"""The numpy twin of rh_orient_normals (include/ransac_hip.h): the definition step by step, by other means than the
library's -- brute-force neighbour lists, Kruskal with a plain union-find over the edges in the total order, parities by a
walk of the forest -- so that tests/test_orient_gpu.py can hold the library to it for equality.  tests/test_orient_host.py
pins the twin itself by hand-derived cases."""
import numpy as np

ANCHOR_FIRST, ANCHOR_TOP = 0, 1
STATS = ("n_vertices", "n_edges", "n_components", "n_tree_edges", "n_flipped", "n_inconsistent", "largest_component")


def in_v(N):
    """step 1: the points whose normal is not (0, 0, 0)"""
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    return ~((N[:, 0] == 0.0) & (N[:, 1] == 0.0) & (N[:, 2] == 0.0))


def _unique_pairs(i, j, N):
    """directed (i, j) pairs, 0-based -> the undirected edges with both ends in V, as a sorted (E, 2) int64 array"""
    v = in_v(N)
    keep = v[i] & v[j] & (i != j)
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    key = np.unique(lo.astype(np.int64) << 32 | hi.astype(np.int64))
    return np.stack([key >> 32, key & 0xFFFFFFFF], axis=1).astype(np.int64).reshape(-1, 2)


def edges_brute(X, N, k, radius=0.0):
    """step 2 by brute force: rh_knn's neighbours of every point (a stable argsort of d^2 with the point itself left out
    by its index, the first k, those beyond the radius dropped), either way round."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    src, dst = [], []
    for lo in range(0, n, 512):
        q = X[lo:lo + 512]
        dx = X[None, :, 0] - q[:, None, 0]
        dy = X[None, :, 1] - q[:, None, 1]
        dz = X[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        d[np.arange(q.shape[0]), lo + np.arange(q.shape[0])] = -1.0          # the point itself sorts first and is cut off
        order = np.argsort(d, axis=1, kind="stable")[:, 1:k + 1]             # stable: equal d^2 keep index order
        dd = np.take_along_axis(d, order, axis=1)
        use = np.ones(order.shape, dtype=bool) if radius <= 0 else dd <= radius * radius
        rows = np.broadcast_to(lo + np.arange(q.shape[0])[:, None], order.shape)
        src.append(rows[use])
        dst.append(order[use])
    i = np.concatenate(src) if src else np.zeros(0, dtype=np.int64)
    j = np.concatenate(dst) if dst else np.zeros(0, dtype=np.int64)
    return _unique_pairs(i.astype(np.int64), j.astype(np.int64), N)


def edges_from_lists(idx, N):
    """step 2 from rh_knn's index lists (n x k, 1-based, 0 past count): a mid-size case starts here"""
    idx = np.asarray(idx).astype(np.int64)
    rows = np.broadcast_to(np.arange(idx.shape[0], dtype=np.int64)[:, None], idx.shape)
    use = idx > 0
    return _unique_pairs(rows[use], idx[use] - 1, N)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def orient_from_edges(X, N, edges, anchor=ANCHOR_TOP, up=(0.0, 0.0, 1.0)):
    """steps 3 .. 9.  Returns a dict: normals (the dtype of N), flip, component (int32), the integer stats, min_tree_absdot,
    and tree (the forest's edges, (T, 2), in the order Kruskal took them)."""
    Nin = np.asarray(N)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    N64 = np.asarray(Nin, dtype=np.float64).reshape(-1, 3)
    up = np.asarray(up, dtype=np.float64).reshape(3)
    n = X.shape[0]
    v = in_v(N64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    ei, ej = edges[:, 0], edges[:, 1]
    dot = _dot3(N64[ei], N64[ej])                                            # step 3
    a, s = np.abs(dot), (dot < 0).astype(np.int64)
    order = np.lexsort((ej, ei, -a))                                         # step 4: descending a, ascending i, ascending j

    parent = list(range(n))                                                  # step 5: Kruskal

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    tree = []
    li, lj = ei.tolist(), ej.tolist()
    for e in order.tolist():
        ri, rj = find(li[e]), find(lj[e])
        if ri != rj:
            parent[ri] = rj
            tree.append(e)
    tree = np.array(tree, dtype=np.int64)

    adj = [[] for _ in range(n)]                                             # step 6: a walk of the forest
    for e in tree.tolist():
        adj[li[e]].append((lj[e], int(s[e])))
        adj[lj[e]].append((li[e], int(s[e])))
    par = np.zeros(n, dtype=np.int64)
    comp = np.zeros(n, dtype=np.int32)
    m = 0
    for start in range(n):                                                   # ascending: components numbered by smallest index
        if not v[start] or comp[start]:
            continue
        m += 1
        comp[start] = m
        stack = [start]
        while stack:
            x = stack.pop()
            for y, sy in adj[x]:
                if not comp[y]:
                    comp[y] = m
                    par[y] = par[x] ^ sy
                    stack.append(y)

    flip = np.full(n, -1, dtype=np.int32)                                    # steps 7 and 8
    t = _dot3(X, up[None, :]) + 0.0
    t = np.where(np.isnan(t), -np.inf, t)
    largest = 0
    for c in range(1, m + 1):
        members = np.flatnonzero(comp == c)
        largest = max(largest, len(members))
        if anchor == ANCHOR_TOP:
            anc = members[np.flatnonzero(t[members] == t[members].max())[0]]
            want = int(_dot3(N64[anc], up) < 0)
        else:
            anc, want = members[0], 0
        flip[members] = par[members] ^ par[anc] ^ want
    out = np.array(Nin).reshape(-1, 3)
    out[flip == 1] = -out[flip == 1]
    fl = np.where(flip == 1, 1, 0)
    return dict(normals=out, flip=flip, component=comp, tree=edges[tree],
                n_vertices=int(v.sum()), n_edges=len(edges), n_components=m, n_tree_edges=len(tree),
                n_flipped=int((flip == 1).sum()), n_inconsistent=int((s ^ fl[ei] ^ fl[ej]).sum()), largest_component=largest,
                min_tree_absdot=float(a[tree].min()) if len(tree) else float("inf"))


def ref_orient(X, N, k, radius=0.0, anchor=ANCHOR_TOP, up=(0.0, 0.0, 1.0)):
    """rh_orient_normals on brute-force neighbour lists"""
    return orient_from_edges(X, N, edges_brute(X, N, k, radius), anchor, up)


def boruvka_parity(n, edges, N):
    """The forest again, the way the library finds it: rounds in which every tree picks its smallest outgoing edge in the
    total order, hooks with parity par(u) ^ s ^ par(v), the smaller root staying on a mutual pick, then flattening.
    Returns (root, parity to the root, rounds); used to check that this reproduces Kruskal's parities."""
    N64 = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    dot = _dot3(N64[edges[:, 0]], N64[edges[:, 1]])
    order = np.lexsort((edges[:, 1], edges[:, 0], -np.abs(dot)))
    eu, ev, es = edges[order, 0], edges[order, 1], (dot[order] < 0).astype(np.int64)
    root, par = np.arange(n), np.zeros(n, dtype=np.int64)
    rounds = 0
    while True:
        ru, rv = root[eu], root[ev]
        live = np.flatnonzero(ru != rv)
        if not len(live):
            return root, par, rounds
        rounds += 1
        best = np.full(n, len(eu), dtype=np.int64)
        np.minimum.at(best, ru[live], live)
        np.minimum.at(best, rv[live], live)
        new_root, new_par = root.copy(), par.copy()
        link, lpar = np.arange(n), np.zeros(n, dtype=np.int64)
        for c in np.flatnonzero(best < len(eu)).tolist():
            b = best[c]
            u, w = eu[b], ev[b]
            d = root[w] if root[u] == c else root[u]
            if best[d] == b and c < d:
                continue
            link[c], lpar[c] = d, par[u] ^ es[b] ^ par[w]
        for x in range(n):
            r, p = root[x], par[x]
            while link[r] != r:
                r, p = link[r], p ^ lpar[r]
            new_root[x], new_par[x] = r, p
        root, par = new_root, new_par
