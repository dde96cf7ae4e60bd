"""The device sampler and its minimal-set fits, held to the oracle set by set.  rh_dbg_sample_fit (diag build) runs one
window of rhk_sample_fit -- the call rh_ransac's windows make -- and returns every candidate it fitted; the oracle's
orc_sample_fit_iteration (the loop body of orc_ransac) states the same window on the CPU.  Every comparison is exact: the
list of (slot, level, shape bytes), the draws per iteration, and no set that gave up.  Every test asserts through info_out that
the kernels it is about ran.  The scenes, the runs and the conditions under which a case occurs are those of
tests/test_sampler_host.py, which asserts the conditions from the oracle alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from test_sampler_host import (CAPACITY, CONES, DEGENERATE, GRAZING, HOSTILE, LONG, LONG_OTHER_BITS, OCT, OCT_CONES, PREFILTER, RANKS_MIXED, RANKS_TINY,
                               SHARDS, TAB_MAX, enabled_mask, params_of, reference, rid, scene)

pytestmark = [pytest.mark.gpu, pytest.mark.diag]

RANKS_FUSED, OCT_FUSED, TWO_KERNELS = 1, 2, 3      # info_out[2]


class Win:
    """what rh_dbg_sample_fit returned"""

    def __init__(self, entries, n_out, draws, gave_up, info):
        self.entries, self.n_out, self.draws, self.gave_up = entries, n_out, draws, gave_up
        self.depth, self.tab_level, self.kernels, self.dn, self.cone, self.sel_list, self.crec, self.tab = info


def new_cloud(name, f32):
    xyz, nrm = scene(name)
    return R.RANSACCloud(xyz, nrm, [np.arange(1, 9, dtype=np.int64)], force_eltype=np.float32 if f32 else None)


@functools.lru_cache(maxsize=None)
def cloud(name, f32):
    return new_cloud(name, f32)


def window(pc, r, P=None, rank=0, world=1, cap=None):
    cp = params_of(r)
    if cap is None:
        cap = r.m * r.iters * len(r.types)
    out = (L.DbgCand * max(1, cap))()
    n_out, gave = C.c_int32(), C.c_int32()
    draws = (C.c_uint64 * r.iters)()
    info = (C.c_int32 * 8)()
    Pp = None
    if P is not None:
        Pbuf = np.zeros(r.iters * 32)              # (room for the deepest octree: a depth that differs from the oracle's fails the comparison, nothing else)
        Pbuf[: P.size] = np.asarray(P, dtype=np.float64).reshape(-1)
        Pp = Pbuf.ctypes.data_as(C.POINTER(C.c_double))
    L.check(R.lib().rh_dbg_sample_fit(pc._h, C.byref(cp), r.seed, r.k0, r.iters, Pp, rank, world, out, cap, C.byref(n_out), draws,
                                      C.byref(gave), info))
    got = [(out[i].slot, out[i].level, bytes(out[i].shape)) for i in range(min(cap, n_out.value))]
    return Win(got, n_out.value, [int(d) for d in draws], gave.value, list(info))


def prepared(r, pc=None):
    """the cloud of the run with its enabled bits set, and the oracle's window"""
    pc = pc if pc is not None else cloud(r.scene, r.f32)
    pc.set_enabled(enabled_mask(pc.size, r.en, r.seed))
    return pc, reference(r)


def check_equal(w, ref, r):
    assert w.gave_up == 0
    assert w.n_out == len(ref.entries), (rid(r), w.n_out, len(ref.entries))
    assert w.draws == ref.draws, (rid(r), w.draws, ref.draws)
    if w.entries != ref.entries:
        got, exp = set(w.entries), set(ref.entries)
        raise AssertionError("%s: %d device candidates the oracle does not have, %d oracle candidates the device does not have; "
                             "first: %r / %r" % (rid(r), len(got - exp), len(exp - got), sorted(got - exp)[:1], sorted(exp - got)[:1]))
    assert w.dn == (3 if r.drawN == 3 else 0)      # drawN = 3: the unrolled instantiation, else the generic one


# 1. fused rank-space kernel, short windows
@pytest.mark.parametrize("r", RANKS_MIXED + RANKS_TINY, ids=rid)
def test_fused_rank_space_kernel(r):
    pc, ref = prepared(r)
    w = window(pc, r)
    assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 0, 0)
    check_equal(w, ref, r)


# 2. its pre-filter: the same batch through the two-kernel form, which has none
@pytest.mark.parametrize("r", PREFILTER + GRAZING, ids=rid)
def test_prefilter_drops_no_set_that_fits(r):
    pc, ref = prepared(r)
    w = window(pc, r)
    assert (w.kernels, w.crec) == (RANKS_FUSED, 0)
    check_equal(w, ref, r)
    with R.option("no_fused_sampler", 1, pc):
        w2 = window(pc, r)
    assert (w2.kernels, w2.cone) == (TWO_KERNELS, 0)
    check_equal(w2, ref, r)
    assert w2.entries == w.entries and w2.draws == w.draws


# 3. long windows: the flat select list, then the compact records
@pytest.mark.parametrize("r", LONG, ids=rid)
def test_long_windows_select_list_and_compact_records(r):
    pc = new_cloud(r.scene, r.f32)                 # (the records appear with the second long window on the same bits: a cloud of its own)
    pc, ref = prepared(r, pc)
    with R.option("long_window_sets", 512, pc):
        w = window(pc, r)
        assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 1, 0)
        check_equal(w, ref, r)
        w = window(pc, r)
        assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 1, 1)
        check_equal(w, ref, r)
        with R.option("no_crec", 1, pc):
            w = window(pc, r)
            assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 1, 0)
            check_equal(w, ref, r)
        with R.option("no_fused_sampler", 1, pc):  # the sampler kernel of the two-kernel form reads the records too
            w = window(pc, r)
            assert (w.kernels, w.sel_list, w.crec) == (TWO_KERNELS, 1, 1)
            check_equal(w, ref, r)
        # other bits: the records of the old ones are stale
        r2 = r._replace(en=LONG_OTHER_BITS)
        pc, ref2 = prepared(r2, pc)
        assert ref2.entries != ref.entries
        w = window(pc, r2)
        assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 1, 0)
        check_equal(w, ref2, r2)
        w = window(pc, r2)
        assert (w.kernels, w.sel_list, w.crec) == (RANKS_FUSED, 1, 1)
        check_equal(w, ref2, r2)


# 4. two-kernel form with cones
@pytest.mark.parametrize("r", CONES, ids=rid)
def test_two_kernel_form_with_cones(r):
    pc, ref = prepared(r)
    w = window(pc, r)
    assert (w.kernels, w.cone, w.crec) == (TWO_KERNELS, 1, 0)
    check_equal(w, ref, r)


# 5. fused octree kernel, with and without the cell directory, and the two-kernel form on the same window
@pytest.mark.parametrize("r", OCT, ids=rid)
def test_fused_octree_kernel(r):
    pc, ref = prepared(r)
    w = window(pc, r, ref.P)
    assert (w.kernels, w.tab) == (OCT_FUSED, 1)
    assert w.depth == ref.depth and w.tab_level == min(ref.depth, TAB_MAX)
    check_equal(w, ref, r)
    with R.option("no_oct_tab", 1, pc):
        w2 = window(pc, r, ref.P)
    assert (w2.kernels, w2.tab) == (OCT_FUSED, 0)
    check_equal(w2, ref, r)
    with R.option("no_fused_sampler", 1, pc):
        w3 = window(pc, r, ref.P)
    assert (w3.kernels, w3.cone, w3.tab) == (TWO_KERNELS, 0, 1)
    check_equal(w3, ref, r)


# 6. octree sampling with cones
@pytest.mark.parametrize("r", OCT_CONES, ids=rid)
def test_octree_sampling_with_cones(r):
    pc, ref = prepared(r)
    w = window(pc, r, ref.P)
    assert (w.kernels, w.cone, w.tab) == (TWO_KERNELS, 1, 1) and w.depth == ref.depth
    check_equal(w, ref, r)


# 7. shards: the ranks' windows together are the one-process window
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("r", SHARDS, ids=rid)
def test_shards_add_up_to_the_one_process_window(r, world):
    pc, ref = prepared(r)
    parts = [window(pc, r, ref.P, rank, world) for rank in range(world)]
    nt = len(r.types)
    for rank, w in enumerate(parts):
        assert w.gave_up == 0 and w.n_out == len(w.entries) > 0
        assert all((slot // nt) % r.m % world == rank for slot, _lev, _b in w.entries)   # set j belongs to rank j % world
    assert sorted(e for w in parts for e in w.entries) == ref.entries
    assert [sum(w.draws[it] for w in parts) for it in range(r.iters)] == ref.draws
    check_equal(window(pc, r, ref.P), ref, r)      # ... and the cloud draws all the sets again afterwards


# 8. capacity
@pytest.mark.parametrize("r", CAPACITY, ids=rid)
def test_capacity_smaller_than_the_count(r):
    pc, ref = prepared(r)
    cap = len(ref.entries) // 3
    assert cap >= 3
    w = window(pc, r, ref.P, cap=cap)
    assert w.n_out == len(ref.entries) and len(w.entries) == cap and w.draws == ref.draws and w.gave_up == 0
    assert set(w.entries) <= set(ref.entries) and len(set(w.entries)) == cap
    assert [e[0] for e in w.entries] == sorted(e[0] for e in w.entries)
    check_equal(window(pc, r, ref.P), ref, r)


# 9. degenerate cloud, all four types, root cell and octree
@pytest.mark.parametrize("r", DEGENERATE + HOSTILE, ids=rid)
def test_degenerate_cloud(r):
    pc, ref = prepared(r)
    w = window(pc, r, ref.P)
    assert (w.kernels, w.cone) == (TWO_KERNELS, 1) and w.depth == ref.depth
    check_equal(w, ref, r)
    nt = len(r.types)
    ok = {(it, int(j)) for it in range(r.iters) for j in np.flatnonzero(ref.sets[it]["ok"])}
    assert all(((slot // nt) // r.m, (slot // nt) % r.m) in ok for slot, _lev, _b in w.entries)   # no shape from a set the reference rejects
    with R.option("no_fused_sampler", 1, pc):
        check_equal(window(pc, r, ref.P), ref, r)


def test_refuses_a_cloud_without_an_enabled_point_and_bad_arguments():
    r = RANKS_TINY[0]
    pc = cloud(r.scene, r.f32)
    pc.set_enabled(np.zeros(pc.size, dtype=bool))
    cp = params_of(r)
    out = (L.DbgCand * 4)()
    n_out = C.c_int32(-1)
    lib = R.lib()
    args = (None, 0, 1, out, 4, C.byref(n_out), None, None, None)
    assert lib.rh_dbg_sample_fit(pc._h, C.byref(cp), 1, 1, 1, *args) == L.RH_E_INVALID
    assert b"no enabled point" in lib.rh_last_error()
    pc.enable_all()
    assert lib.rh_dbg_sample_fit(pc._h, C.byref(cp), 1, 1, 1, *args) == L.RH_OK and n_out.value >= 0      # (the optional outputs may be NULL)
    assert lib.rh_dbg_sample_fit(pc._h, C.byref(cp), 1, 1, 0, *args) == L.RH_E_INVALID                    # no iteration
    assert lib.rh_dbg_sample_fit(pc._h, C.byref(cp), 1, 1, 1, None, 2, 2, out, 4, C.byref(n_out), None, None, None) == L.RH_E_INVALID   # rank outside the world
