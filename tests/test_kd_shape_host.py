"""The shape of the position k-d tree of subset 1 (csrc/rh_internal.h: kd_left_count, the one statement that the device order,
the host order and the plane order's blocks share), through rh_dbg_kd_shape (diag build, no GPU).

  - Not aligned: the nodes of at most 1024 points and the leaves are those of a restatement of the rule in Python / numpy.
  - Aligned: every split is at a multiple of 64; every node of more than 1024 points splits at a multiple of 1024 into two
    non-empty parts; node k of at most 1024 points is exactly [1024 k, min(s, 1024 k + 1024)); the tree is no higher than the
    unaligned one.
  - By size ("kd_align" = 0, the default) a subset below 1000 tiles of 256 points takes today's shape.

Sizes: every s in 1 .. 20 000 (leaves included: every node size up to 1024 occurs there, and below 1024 points a node's subtree
depends on its size alone), 2000 random s up to 2^31 - 1 (log-uniform, so that every magnitude is met: 1960 between 2^10 and
2^26, 40 above, whose lists run to millions of nodes each, 2^31 - 1 itself among them; nodes and splits only: 2^31 points have
33 M leaves), and the subsets of cfg3, cfg5 and of the parity test's host / device
comparison: 312 500, 1 562 500 and 66 667 points."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

pytestmark = pytest.mark.diag

NAMED = [312_500, 1_562_500, 66_667]
MIN_TILES = 1000          # the by-size rule (include/ransac_hip.h, "kd_align")


def shape(s, aligned, leaves=False):
    """rh_dbg_kd_shape -> dict(nodes [k, 2], splits [m, 3], leaves [l, 2] or None, depth, aligned)"""
    lib = L.lib("diag")
    i64p = C.POINTER(C.c_int64)
    info = np.zeros(5, dtype=np.int64)
    ncap = s // 512 + 2           # (a node of at most 1024 points whose parent had more holds at least 512)
    nodes = np.empty((ncap, 2), dtype=np.int64)
    splits = np.empty((ncap, 3), dtype=np.int64)
    lcap = s // 32 + 2 if leaves else 0
    lv = np.empty((lcap, 2), dtype=np.int64) if leaves else None
    L.check(lib.rh_dbg_kd_shape(s, aligned, info.ctypes.data_as(i64p), nodes.ctypes.data_as(i64p), ncap, splits.ctypes.data_as(i64p), ncap,
                                lv.ctypes.data_as(i64p) if leaves else None, lcap))
    nn, ns, nl, depth, al = (int(v) for v in info)
    assert nn <= ncap and ns <= ncap and nl <= lcap
    return dict(nodes=nodes[:nn], splits=splits[:ns], leaves=lv[:nl] if leaves else None, depth=depth, aligned=al)


def restated(s, most):
    """today's rule, level by level in numpy: (the nodes of at most `most` points in position order, the tree's height over them)"""
    lo, hi = np.array([0], dtype=np.int64), np.array([s], dtype=np.int64)
    depth = 0
    while True:
        cnt = hi - lo
        big = cnt > most
        if not big.any():
            return np.stack([lo, hi], axis=1), depth
        depth += 1
        mid = lo + ((cnt // 64 + 1) // 2) * 64
        # a node that splits is replaced by its two children, in place
        rep = np.where(big, 2, 1)
        at = np.cumsum(rep) - rep
        nlo, nhi = np.empty(rep.sum(), dtype=np.int64), np.empty(rep.sum(), dtype=np.int64)
        nlo[at], nhi[at] = lo, np.where(big, mid, hi)
        nlo[at[big] + 1], nhi[at[big] + 1] = mid[big], hi[big]
        lo, hi = nlo, nhi


_STARTS = {}


def starts(cnt, most, memo=_STARTS):
    """today's rule by recursion on the node's size (a node's subtree depends on its size alone): the starts of its nodes of at
    most `most` points, relative to its own; kept per size, so that a run over consecutive sizes only ever adds a level (large
    sizes bring a memo of their own and drop it)"""
    key = (cnt, most)
    if key not in memo:
        if cnt <= most:
            memo[key] = np.zeros(1, dtype=np.int64)
        else:
            nl = ((cnt // 64 + 1) // 2) * 64
            memo[key] = np.concatenate([starts(nl, most, memo), nl + starts(cnt - nl, most, memo)])
    return memo[key]


def height(s):
    """today's rule: levels until every node holds at most 64 points, by the distinct node sizes of each level"""
    sizes, depth = {s}, 0
    while any(c > 64 for c in sizes):
        sizes = {h for c in sizes for h in ((((c // 64 + 1) // 2) * 64, c - ((c // 64 + 1) // 2) * 64) if c > 64 else ())}
        depth += 1
    return depth


def _ranges(st, s):
    return np.stack([st, np.append(st[1:], s)], axis=1)


def check_unaligned(s, leaves):
    got = shape(s, 0, leaves)
    want = _ranges(starts(s, 1024, _STARTS if s <= 20_000 else {}), s)
    assert np.array_equal(got["nodes"], want), s
    assert got["aligned"] == 0 and got["depth"] == height(s), s
    if leaves:
        assert np.array_equal(got["leaves"], _ranges(starts(s, 64), s)), s
    return got


def check_aligned(s, leaves, unaligned_depth):
    got = shape(s, 1, leaves)
    nodes, splits = got["nodes"], got["splits"]
    k = np.arange(len(nodes), dtype=np.int64)
    assert len(nodes) == (s + 1023) // 1024, s
    assert np.array_equal(nodes[:, 0], 1024 * k) and np.array_equal(nodes[:, 1], np.minimum(s, 1024 * k + 1024)), s
    if len(splits):
        lo, mid, hi = splits.T
        assert (hi - lo > 1024).all() and (mid % 1024 == 0).all() and (lo < mid).all() and (mid < hi).all(), s
        assert (lo % 1024 == 0).all()
        assert lo[0] == 0 and hi[0] == s
    else:
        assert s <= 1024
    assert len(splits) == len(nodes) - 1          # a binary tree over the nodes
    assert got["depth"] <= unaligned_depth, (s, got["depth"], unaligned_depth)
    if leaves:
        lv = got["leaves"]
        assert lv[0, 0] == 0 and lv[-1, 1] == s and np.array_equal(lv[1:, 0], lv[:-1, 1])
        assert (lv[:, 0] % 64 == 0).all() and (lv[:, 1] > lv[:, 0]).all() and (lv[:, 1] - lv[:, 0] <= 64).all(), s
        assert (lv[:-1, 1] - lv[:-1, 0] == 64).all()          # only the last group is partial
        # inside a node of at most 1024 points: today's rule
        for nlo, nhi in nodes[[0, -1]]:
            sel = (lv[:, 0] >= nlo) & (lv[:, 1] <= nhi)
            assert np.array_equal(lv[sel] - nlo, _ranges(starts(int(nhi - nlo), 64), int(nhi - nlo))), (s, nlo)
    return got


def test_the_two_restatements_agree():
    for s in (1, 64, 65, 1024, 1025, 9421, 66_667, 312_500):
        for most in (64, 1024):
            assert np.array_equal(restated(s, most)[0], _ranges(starts(s, most), s)), (s, most)
        assert restated(s, 64)[1] == height(s)


def test_every_size_up_to_20000():
    for s in range(1, 20_001):
        un = check_unaligned(s, True)
        al = check_aligned(s, True, un["depth"])
        if s <= 1024:
            assert np.array_equal(al["leaves"], un["leaves"]) and al["depth"] == un["depth"]


def test_random_sizes_up_to_2_to_the_31():
    rng = np.random.default_rng(1414)
    sizes = np.concatenate([np.floor(2.0 ** rng.uniform(10.0, 26.0, 1960)), np.floor(2.0 ** rng.uniform(26.0, 31.0, 38)),
                            [2 ** 31 - 1, 2 ** 31 - 1024]]).astype(np.int64)
    assert len(sizes) == 2000 and sizes.max() == 2 ** 31 - 1 and sizes.min() >= 1024
    for s in sizes:
        s = int(s)
        un = check_unaligned(s, False)
        check_aligned(s, False, un["depth"])


@pytest.mark.parametrize("s", NAMED)
def test_the_benchmark_s_and_the_parity_test_s_subsets(s):
    un = check_unaligned(s, True)
    al = check_aligned(s, True, un["depth"])
    if s == 312_500:          # cfg3: 305 nodes of exactly 1024 points and one of 180; today 512 nodes of 576 .. 640
        sizes = al["nodes"][:, 1] - al["nodes"][:, 0]
        assert len(sizes) == 306 and (sizes[:-1] == 1024).all() and sizes[-1] == 180
        us = un["nodes"][:, 1] - un["nodes"][:, 0]
        assert len(us) == 512 and us.min() >= 576 - 64 and us.max() <= 640


def test_by_size_takes_today_s_shape_below_the_threshold():
    first = MIN_TILES * 256 - 255          # the smallest subset of 1000 tiles
    for s in (1, 1024, 1025, 8300, 9421, 66_667, first - 1):
        got = shape(s, -1, s < 70_000)
        un = shape(s, 0, s < 70_000)
        assert got["aligned"] == 0 and np.array_equal(got["nodes"], un["nodes"]) and got["depth"] == un["depth"], s
        if got["leaves"] is not None:
            assert np.array_equal(got["leaves"], un["leaves"])
    for s in (first, 312_500, 1_562_500):
        assert shape(s, -1)["aligned"] == 1, s
    # the option (of the library asked: the diag build's own): 1 = always, 2 = never
    lib = L.lib("diag")
    try:
        L.check(lib.rh_set_option(None, b"kd_align", 1))
        assert shape(9421, -1)["aligned"] == 1
        L.check(lib.rh_set_option(None, b"kd_align", 2))
        assert shape(312_500, -1)["aligned"] == 0
        assert lib.rh_set_option(None, b"kd_align", 3) != 0
    finally:
        L.check(lib.rh_set_option(None, b"kd_align", L.OPTION_UNSET))
    assert shape(312_500, -1)["aligned"] == 1
