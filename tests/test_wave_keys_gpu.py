"""wave_each_key (csrc/wave_keys.h) on its own: "one action per distinct key of a wave", the step under the atomics of
rh_cluster, rh_orient_normals, rh_assign_points, the component filter and the sampler's draw counts.  rh_dbg_wave_keys (diag
build) runs it in one block of 256 threads = 4 waves; the three tallies it returns -- per key the sum of popcount(same), per
key the smallest leader, the number of calls -- are compared with numpy, exactly.  The sizes are the smallest that reach every
branch: a single lane, a wave short of one lane, a full wave, one lane into the second wave, the full block."""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

SIZES = (1, 63, 64, 65, 256)
NO_LEADER = 0x7F7F7F7F
# (name, uint32 instantiation, the key value that has to appear, a step to further keys that stays inside the type)
FLAVOURS = [("i32_zero", 0, 0, 1), ("i32_max", 0, 2**31 - 1, -1), ("u32_top", 1, 0xFFFFFFFE, -1)]


def _pattern(name, n, v, step, rng):
    i = np.arange(n, dtype=np.int64)
    act = np.ones(n, dtype=np.uint8)
    if name == "one_key":
        keys = np.full(n, v)
    elif name == "all_distinct":
        keys = v + step * i
    elif name == "two_alternating":
        keys = v + step * 7 * (i & 1)
    elif name == "runs_across_waves":      # runs of 48: 48 .. 95 and 144 .. 191 straddle the boundaries at 64 and at 192
        keys = v + step * (i // 48)
    elif name == "inactive_30_percent":    # few keys, so that inactive lanes hold the keys of active ones
        keys = v + step * rng.integers(0, 5, n)
        keys[0] = v
        act = (rng.random(n) >= 0.3).astype(np.uint8)
    elif name == "all_inactive":
        keys = v + step * (i % 3)
        act = np.zeros(n, dtype=np.uint8)
    else:
        raise AssertionError(name)
    return keys.astype(np.int64), act


def _expected(keys, act, slot, nslots):
    total = np.zeros(nslots, dtype=np.int64)
    minlead = np.full(nslots, NO_LEADER, dtype=np.int64)
    calls = 0
    for w in range(0, len(keys), 64):
        k, a, s = keys[w:w + 64], act[w:w + 64] != 0, slot[w:w + 64]
        for key in np.unique(k[a]):
            lanes = np.flatnonzero(a & (k == key))
            calls += 1                                  # one call per distinct (wave, key) among the active lanes
            total[s[lanes[0]]] += len(lanes)            # popcount(same)
            minlead[s[lanes[0]]] = min(minlead[s[lanes[0]]], w + lanes[0])
    return total, minlead, calls


@pytest.mark.parametrize("pattern", ["one_key", "all_distinct", "two_alternating", "runs_across_waves", "inactive_30_percent",
                                     "all_inactive"])
@pytest.mark.parametrize("flavour", FLAVOURS, ids=[f[0] for f in FLAVOURS])
def test_wave_each_key_against_numpy(flavour, pattern):
    _, u32, v, step = flavour
    rng = np.random.default_rng(20260901)
    lib = R.lib()
    for n in SIZES:
        keys, act = _pattern(pattern, n, v, step, rng)
        assert keys.min() >= 0 and keys.max() <= (0xFFFFFFFF if u32 else 2**31 - 1) and (keys == v).any()
        distinct, slot = np.unique(keys, return_inverse=True)
        slot = slot.astype(np.int32)
        nslots = len(distinct)
        k32 = keys.astype(np.uint32)
        total = np.zeros(nslots, dtype=np.int32)
        minlead = np.zeros(nslots, dtype=np.int32)
        scal = np.zeros(2, dtype=np.int32)
        L.check(lib.rh_dbg_wave_keys(k32.ctypes.data_as(C.POINTER(C.c_uint32)), act.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     slot.ctypes.data_as(C.POINTER(C.c_int32)), n, nslots, u32, 0,
                                     total.ctypes.data_as(C.POINTER(C.c_int32)), minlead.ctypes.data_as(C.POINTER(C.c_int32)),
                                     scal.ctypes.data_as(C.POINTER(C.c_int32))))
        e_total, e_minlead, e_calls = _expected(keys, act, slot, nslots)
        assert scal[1] == 0, (n, "a lane outside the converged wave, or a wrong ballot")
        assert int(scal[0]) == e_calls, (n, int(scal[0]), e_calls)
        assert np.array_equal(total, e_total), (n, total, e_total)
        assert np.array_equal(minlead, e_minlead), (n, minlead, e_minlead)
