"""The protocol of the enabled bits (csrc/enabled_state.h) against an independent model, on the CPU.  rh_dbg_enabled_events
(diag build, host code only) runs event sequences on fresh states and returns the queries' answers after every event.  The
model knows nothing of the flags: it keeps an epoch that every change of the bits advances, the epoch at which each derived
structure was made, who wrote the shared total last, and what a refit scan in flight has left behind.

Soundness, on every sequence: a query says "exists" only where the model says the structure was made from the bits as they
are (for the directory also: the total is its own).  Non-vacuity, on the sequences that carry the speed of the product:
there the query must say "exists"."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ransac_jl_amd import _lib as L

# events of rh_dbg_enabled_events (include/ransac_hip_diag.h)
REPLACED, REPLACED_COPY, CLEARED, CLEARED_BOTH = 0, 1, 2, 3
SCAN_STREAM, SCAN_STREAM_APPLY, SCAN_CULLED, SCAN_CULLED_APPLY = 4, 5, 6, 7
FOLD, FOLD_EMPTY, SCRATCH, DIRECTORY, LIST, RECORDS, MIRROR, LONG, VERY_LONG, NOTHING = 8, 9, 10, 11, 12, 13, 14, 15, 16, 17
N_EVENTS = 18
# answer bits
DIR, LST, REC, MIR, SUMS, SCAN_SUMS, WANT = 1, 2, 4, 8, 16, 32, 64
LENGTH = 5


def run_events(seqs):
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    out = np.zeros(seqs.shape, dtype=np.uint16)
    L.check(L.lib("diag").rh_dbg_enabled_events(seqs.ctypes.data_as(C.POINTER(C.c_uint8)), seqs.shape[0], seqs.shape[1],
                                                out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def all_sequences(length):
    grids = np.indices((N_EVENTS,) * length, dtype=np.uint8)
    return grids.reshape(length, -1).T.copy()


class Model:
    """All sequences at once: every field is an array over the sequences."""

    def __init__(self, n):
        self.epoch = np.zeros(n, np.int32)
        neg = lambda: np.full(n, -1, np.int32)
        self.dir_ep, self.list_ep, self.rec_ep, self.mir_ep, self.sums_ep = neg(), neg(), neg(), neg(), neg()
        self.total_is_dirs = np.zeros(n, bool)       # who wrote the shared total last: the directory (else somebody else)
        self.scan_ep = neg()                         # a refit scan in flight: the epoch of the bits it read
        self.ahead = np.zeros(n, bool)               # ... it has cleared its inliers in the mirror (made at mir_ep) already
        self.scan_sums = np.zeros(n, bool)           # ... and its mask's block popcounts are in the scan scratch
        self.very_long = np.zeros(n, np.int32)       # very long windows since the directory was made

    # what exists
    def directory(self): return (self.dir_ep == self.epoch) & self.total_is_dirs
    def list(self): return self.list_ep == self.epoch
    def records(self): return self.rec_ep == self.epoch
    def block_sums(self): return self.sums_ep == self.epoch
    # the mirror matches the bits, or is ahead of them by exactly the inliers of the scan in flight on these bits
    def mirror(self): return (self.mir_ep == self.epoch) & (~self.ahead | (self.scan_ep == self.epoch))

    def drop_ahead(self, m):
        """the mirror of the sequences m is ahead by a scan that will not be folded: it matches no bits at all"""
        bad = m & self.ahead
        self.mir_ep[bad] = -1
        self.ahead[bad] = False

    def step(self, ev):
        old = self.epoch.copy()
        for e in (REPLACED, REPLACED_COPY):
            m = ev == e
            self.drop_ahead(m)
            self.epoch[m] += 1
            if e == REPLACED_COPY:
                self.mir_ep[m] = self.epoch[m]
        for e in (CLEARED, CLEARED_BOTH):
            m = ev == e
            self.drop_ahead(m)
            self.epoch[m] += 1
            if e == CLEARED_BOTH:
                k = m & (self.mir_ep == old)
                self.mir_ep[k] = self.epoch[k]
        for e in (SCAN_STREAM, SCAN_STREAM_APPLY, SCAN_CULLED, SCAN_CULLED_APPLY):
            m = ev == e
            self.drop_ahead(m)
            self.scan_ep[m] = self.epoch[m]
            self.scan_sums[m] = e == SCAN_CULLED_APPLY
            if e == SCAN_CULLED_APPLY:
                self.ahead[m & (self.mir_ep == self.epoch)] = True
        for e in (FOLD, FOLD_EMPTY):
            m = ev == e
            keep = m & self.ahead & (self.scan_ep == old) & (self.mir_ep == old)
            self.epoch[m] += 1
            self.drop_ahead(m & ~keep)
            self.mir_ep[keep] = self.epoch[keep]
            self.ahead[keep] = False
            self.total_is_dirs[m] = False          # the list's length
            self.sums_ep[m] = self.epoch[m]
            self.scan_sums[m] = False              # scanned in place
            self.scan_ep[m] = -1
        m = ev == SCRATCH
        self.total_is_dirs[m] = False
        self.scan_sums[m] = False
        m = ev == DIRECTORY
        self.dir_ep[m] = self.epoch[m]
        self.total_is_dirs[m] = True
        self.sums_ep[m] = -1                       # scanned in place
        self.very_long[m] = 0
        m = ev == LIST                             # made from the directory: worth what the directory is
        self.list_ep[m] = np.where(self.directory()[m], self.epoch[m], -1)
        m = ev == RECORDS                          # made from the list
        self.rec_ep[m] = np.where(self.list()[m], self.epoch[m], -1)
        m = ev == MIRROR
        self.mir_ep[m] = self.epoch[m]
        self.ahead[m] = False
        m = ev == VERY_LONG
        self.very_long[m] += 1


@pytest.fixture(scope="module")
def enumeration():
    seqs = all_sequences(LENGTH)
    return seqs, run_events(seqs)


def test_sound_on_every_sequence(enumeration):
    seqs, ans = enumeration
    assert seqs.shape == (N_EVENTS ** LENGTH, LENGTH)
    M = Model(seqs.shape[0])
    for t in range(LENGTH):
        M.step(seqs[:, t])
        check_sound(M, ans[:, t], seqs[:, :t + 1])


def check_sound(M, a, seqs):
    for bit, exists, name in ((DIR, M.directory(), "directory"), (LST, M.list(), "list"), (REC, M.records(), "records"),
                              (MIR, M.mirror(), "mirror"), (SUMS, M.block_sums(), "block sums"),
                              (SCAN_SUMS, M.scan_sums, "the scan's sums")):
        bad = ((a & bit) != 0) & ~exists
        assert not bad.any(), "%s said to exist after %s" % (name, seqs[np.flatnonzero(bad)[0]].tolist())


def test_sound_on_every_reachable_state():
    """Beyond LENGTH: breadth first over the states themselves, until no sequence reaches a new one.  A state is what can be
    told apart from outside -- the answers now, the answers after a fold (which shows whether a scan is ahead in the mirror)
    and the model's own state relative to its epoch -- and every state found is extended by every event."""
    frontier, seen, depth = [()], set(), 0
    while frontier:
        depth += 1
        assert depth <= 16, "the reachable states keep growing"
        seqs = np.array([s + (e,) for s in frontier for e in range(N_EVENTS)], dtype=np.uint8)
        ans = run_events(np.c_[seqs, np.full(len(seqs), FOLD, dtype=np.uint8)])
        M = Model(len(seqs))
        for t in range(depth):
            M.step(seqs[:, t])
        check_sound(M, ans[:, depth - 1], seqs)
        e = M.epoch
        state = np.c_[ans[:, depth - 1] & ~np.uint16(WANT), ans[:, depth], M.dir_ep == e, M.total_is_dirs, M.list_ep == e, M.rec_ep == e,
                      M.mir_ep == e, M.ahead, M.scan_ep == e, M.sums_ep == e, M.scan_sums, np.minimum(M.very_long, 2)]
        frontier = []
        for s, key in zip(seqs.tolist(), map(tuple, state.tolist())):
            if key not in seen:
                seen.add(key)
                frontier.append(tuple(s))
    assert depth > LENGTH and len(seen) > 100      # (the exhaustive enumeration alone does not reach every state)


def test_records_from_the_second_very_long_window_on(enumeration):
    seqs, ans = enumeration
    M = Model(seqs.shape[0])
    for t in range(LENGTH):
        ev = seqs[:, t]
        M.step(ev)
        a = ans[:, t]
        has_rec = (a & REC) != 0
        asked = (ev == LONG) | (ev == VERY_LONG)
        want = has_rec | ((ev == VERY_LONG) & (M.very_long >= 2))
        assert np.array_equal(((a & WANT) != 0)[asked], want[asked])
        assert not (a[~asked] & WANT).any()


def answers(*events):
    return run_events(np.array([events], dtype=np.uint8))[0].tolist()


def test_culled_scan_with_apply_keeps_the_mirror_and_skips_both_popcount_passes():
    a = answers(MIRROR, SCAN_CULLED_APPLY, FOLD)
    assert a[1] & SCAN_SUMS                        # the fold does not count the mask's blocks
    assert a[2] & MIR and a[2] & SUMS              # the mirror is valid, the next directory does not count the bits' blocks
    assert not a[2] & DIR


def test_streaming_scan_leaves_the_mirror_stale_and_the_block_sums():
    a = answers(MIRROR, SCAN_STREAM_APPLY, FOLD)
    assert not a[1] & SCAN_SUMS
    assert not a[2] & MIR and a[2] & SUMS


@pytest.mark.parametrize("scan", [SCAN_STREAM, SCAN_CULLED])
def test_scan_without_apply_leaves_the_mirror_stale(scan):
    a = answers(MIRROR, scan, FOLD)
    assert a[1] & MIR and not a[1] & SCAN_SUMS
    assert not a[2] & MIR and a[2] & SUMS


def test_directory_list_and_records_outlive_scoring_and_reads():
    for tail in itertools.product((NOTHING, LONG, VERY_LONG, MIRROR, LIST, RECORDS), repeat=3):
        a = answers(DIRECTORY, LIST, RECORDS, *tail)
        assert all(x & (DIR | LST | REC) == DIR | LST | REC for x in a[2:]), tail


def test_scratch_taken_drops_the_directory_and_nothing_else():
    a = answers(MIRROR, DIRECTORY, LIST, SCRATCH, DIRECTORY)
    assert a[2] & DIR and a[2] & LST and a[2] & MIR
    assert not a[3] & DIR and a[3] & MIR
    assert a[4] & DIR and not a[4] & LST           # today a rebuilt directory starts without its list


def test_header_stands_alone_under_sanitizers(tmp_path):
    """enabled_state.h needs nothing but a C++ compiler: tests/native/enabled_state_check.cpp, a stand-alone program, built
    with the address and undefined-behaviour sanitizers"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "enabled_state_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-I", os.path.join(root, "ransac.jl_amd", "csrc"),
                           os.path.join(root, "tests", "native", "enabled_state_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0 bad", (out.stdout[-2000:], out.stderr[-2000:])


def test_rejects_an_unknown_event():
    with pytest.raises(L.RansacHipError):
        answers(NOTHING, 18)
