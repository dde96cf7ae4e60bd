"""The undecided word of the counts-only score launches, read off the two-bit books in place (csrc/score4_device.h, "Books in
place") as the HOST runs it -- diag build, no GPU -- through the very functions of the kernel (rh_dbg_books2_inplace).

The packed word keeps the books' bit order: bit L stands for point pi(L).  For every input the point set {pi(L) : bit L of the
packed word} must be the point set of rh_dbg_books2's point-ordered undecided word, and pi must be a permutation of 0 .. 63.
Inputs: the special values of test_books2_host.py at the word borders (0, 15, 16, 31, 32, 47, 48, 63) and 1000 seeded random
sequences.  The deposit of a point-ordered word into the books' order (what the pairs that ignore their books queue: their
group's enabled word) is the inverse map."""
import ctypes as C

import numpy as np

from ransac_jl_amd import _lib as L

import test_books2_host as B2

_fp, _u64p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)


def inplace(u2, point_words=None):
    u2 = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1, 64)
    n = len(u2)
    packed, pi = np.zeros(n, dtype=np.uint64), np.full(64, -1, dtype=np.int32)
    dep = None
    if point_words is not None:
        point_words = np.ascontiguousarray(point_words, dtype=np.uint64)
        assert len(point_words) == n
        dep = np.zeros(n, dtype=np.uint64)
    L.check(L.lib("diag").rh_dbg_books2_inplace(u2.ctypes.data_as(_fp), n, packed.ctypes.data_as(_u64p), pi.ctypes.data_as(_i32p),
                                                None if dep is None else point_words.ctypes.data_as(_u64p),
                                                None if dep is None else dep.ctypes.data_as(_u64p)))
    return packed, pi, dep


def to_point_order(words, pi):
    """bit L of every word -> bit pi[L]"""
    bits = (words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return (bits << pi.astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def _check(u2):
    _cnt, _sure, und, _any = B2.books(u2)
    packed, pi, _ = inplace(u2)
    assert sorted(pi.tolist()) == list(range(64))
    got = to_point_order(packed, pi)
    bad = np.flatnonzero(got != und)
    assert bad.size == 0, (bad[:4], got[bad[:4]], und[bad[:4]])
    assert [bin(int(x)).count("1") for x in packed] == [bin(int(x)).count("1") for x in und]
    return packed, und


def test_the_map_is_the_one_the_packing_defines():
    _p, pi, _ = inplace(np.zeros((0, 64), dtype=np.float32))
    assert sorted(pi.tolist()) == list(range(64))
    # word q's point j sits at bit 31 - 2 j of its half (q even) or, shifted right by one, at bit 30 - 2 j (q odd)
    for q in range(4):
        for j in range(16):
            assert pi[32 * (q // 2) + (31 - 2 * j if q % 2 == 0 else 30 - 2 * j)] == 16 * q + j
    # one undecided point at a time
    rows = np.full((64, 64), 5.0, dtype=np.float32)
    rows[np.arange(64), np.arange(64)] = 0.25
    packed, _und = _check(rows)
    for p in range(64):
        assert int(packed[p]) == 1 << int(np.flatnonzero(pi == p)[0])


def test_special_values_at_the_word_borders():
    rows = []
    for fill in (np.float32(5.0), np.float32(-3.0), np.float32(0.25)):     # among points that are out / in / undecided
        for v in B2.SPECIAL:
            for p in B2.BORDERS:
                r = np.full(64, fill, dtype=np.float32); r[p] = v
                rows.append(r)
    for v in B2.SPECIAL:                                                   # ... and at all eight borders at once, and everywhere
        r = np.full(64, 7.0, dtype=np.float32); r[list(B2.BORDERS)] = v
        rows.append(r)
        rows.append(np.full(64, v, dtype=np.float32))
    packed, und = _check(np.array(rows))
    assert (und != 0).any() and (und == 0).any()


def test_random_sequences():
    rng = np.random.default_rng(2024)
    a = (rng.normal(size=(334, 64)) * 2.0).astype(np.float32)
    b = rng.integers(0, 2 ** 32, size=(333, 64), dtype=np.uint64).astype(np.uint32).view(np.float32)
    c = np.array(B2.SPECIAL, dtype=np.float32)[rng.integers(0, len(B2.SPECIAL), size=(333, 64))]
    seqs = np.vstack([a, b, c])
    assert seqs.shape == (1000, 64)
    packed, und = _check(seqs)
    assert (und != 0).any()


def test_deposit_brings_a_point_ordered_word_into_the_books_order():
    rng = np.random.default_rng(7)
    words = rng.integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    words[:6] = [0, 0xFFFFFFFFFFFFFFFF, 1, 1 << 63, 0x3F, 0x8000000180008001]     # none, all, the ends, a short last group, the borders
    _packed, pi, dep = inplace(np.zeros((1000, 64), dtype=np.float32), words)
    assert np.array_equal(to_point_order(dep, pi), words)
