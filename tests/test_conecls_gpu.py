"""The score kernel's cone code (csrc/score4_device.h: the cone record of cls_make, cls_cone_ab with its reciprocal root and its
axis guard, cone_box_skip32) on the scene of tests/cone_scene.py, product library: points on the edges of the band and of the
angle test, on both sides of the axis guard, on the axis, on the apex and within a binary32 step of it; candidates with non-unit
axes, opening angles from 0.004 to beyond pi, an apex in the cloud, an apex 2^19 away, and apex coordinates no binary32 record
can hold.  The shortcuts change which pairs are decided in binary32 or skipped, never what a candidate counts: counts and dense
masks must equal the oracle's bit for bit on the Float64 and on the Float32 cloud -- culled kernel (score_path = groups) with
the super-tile lists on and off and rows of the default height and of 4, the counts-only call, the device-batch call the
benchmark times (with rh_score_launch_info naming the culled kernel), the brute kernel -- and rh_refit of the exact copies,
culled and streaming, must return the oracle's lists.  (That the scene is not vacuous is checked without a GPU, against the
oracle alone: test_conecls_host.py.)"""
import ctypes as C

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L
from ransac_jl_amd import dist as rdist
from oracle import oracle as orc

import cone_scene as S

pytestmark = pytest.mark.gpu

_OPTS = ("score_path", "s4_rows", "refit_path", "st_cull")


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    for k in _OPTS:
        R.set_option(k, None)


def params():
    p = R.ransacparameters([R.FittedCone])
    p["cone"]["ϵ"] = S.EPS
    p["cone"]["α"] = S.ALPHA
    return R.params_to_c(p)


def as_orc(arr, b):
    out = (orc.Shape * max(1, b))()
    C.memmove(out, arr, C.sizeof(L.Shape) * b)
    return out


class Case:
    """one element type: the clouds of both sides (the library's by score path), the batch, the oracle's answer -- made once"""

    def __init__(self, f32):
        self.f32, self.sc = f32, S.scene()
        self.xyz, self.nrm = self.sc.arrays(f32)
        self.subs = [np.arange(1, S.N + 1, dtype=np.int64)]
        self.oc = (orc.Cloud32 if f32 else orc.Cloud)(self.xyz, self.nrm, self.subs[0])
        self.oc.set_enabled(self.sc.enabled_chunks())
        self.arr = S.shapes(R.lib(), L.Shape, f32)
        self.oarr = as_orc(self.arr, S.B)
        self.cp = params()
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        self.ref_c, self.ref_m = self.oc.score_batch(self.oarr, self.op, want_masks=True)
        self.ref_c.setflags(write=False); self.ref_m.setflags(write=False)
        self.pcs = {}

    def pc(self, path="groups"):
        if path not in self.pcs:
            with R.option("score_path", path):          # (read when a cloud is created)
                kw = dict(force_eltype=np.float32) if self.f32 else {}
                self.pcs[path] = R.RANSACCloud(self.xyz, self.nrm, self.subs, **kw)
            self.pcs[path].set_enabled(self.sc.en)
        return self.pcs[path]


_CASES = {}


def case(f32):
    if f32 not in _CASES:
        _CASES[f32] = Case(f32)
    return _CASES[f32]


def _check(cs, pc, tag):
    got_c, got_m = R.score_batch(pc, cs.arr, cs.cp, want_masks=True)
    bad = np.flatnonzero(got_c != cs.ref_c)
    assert len(bad) == 0, (tag, bad[:8], [cs.sc.tags[i] for i in bad[:8]], got_c[bad][:8], cs.ref_c[bad][:8])
    assert np.array_equal(got_m, cs.ref_m), tag
    assert np.array_equal(R.score_batch(pc, cs.arr, cs.cp), cs.ref_c), (tag, "counts only")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counts_and_masks_equal_the_oracle_culled_and_brute(f32):
    cs = case(f32)
    assert cs.ref_c[0] > 300 and cs.ref_c[2] > 300 and cs.ref_c[1] > 50 and cs.ref_c[3] > 50, cs.ref_c[:4]
    pc = cs.pc("groups")
    for lists in (1, 2):
        for rows in (None, 4):
            with R.option("st_cull", lists, cloud=pc), R.option("s4_rows", rows, cloud=pc):
                _check(cs, pc, (f32, "groups", lists, rows))
    _check(cs, cs.pc("brute"), (f32, "brute"))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_device_batch_runs_the_culled_kernel_and_counts_the_same(f32):
    cs = case(f32)
    pc, lib = cs.pc("groups"), R.lib()
    batch = rdist.DeviceBatch(pc, cs.arr, S.B)
    d_cn = C.c_void_p()
    L.check(lib.rh_dev_alloc(pc._h, 4 * S.B, C.byref(d_cn)))
    try:
        for lists in (1, 2):
            with R.option("st_cull", lists, cloud=pc):
                L.check(lib.rh_score_batch_dev(pc._h, batch.slice_ptr(0), S.B, C.byref(cs.cp), d_cn, None))
                L.check(lib.rh_cloud_sync(pc._h))
                info = (C.c_int32 * 4)()
                L.check(lib.rh_score_launch_info(pc._h, info))
                assert info[0] > 0 and info[1] == (1 if lists == 1 else 0) and info[3] == (S.N + 255) // 256, list(info)
                got = np.zeros(S.B, dtype=np.int32)
                L.check(lib.rh_dev_download(pc._h, got.ctypes.data_as(C.c_void_p), d_cn, 4 * S.B))
                assert np.array_equal(got, cs.ref_c), (f32, lists, np.flatnonzero(got != cs.ref_c)[:8])
    finally:
        lib.rh_dev_free(pc._h, d_cn)
        batch.free()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_refit_of_the_exact_copies_culled_and_streaming(f32):
    cs = case(f32)
    pc = cs.pc("groups")
    which = [i for i, t in enumerate(cs.sc.tags) if t in ("exact", "exact-in", "axislen")]
    assert len(which) == 10
    exp = {i: cs.oc.refit(cs.oarr[i], cs.op) for i in which}
    assert len(exp[0]) > 300 and len(exp[2]) > 300 and len(exp[1]) > 50 and len(exp[3]) > 50
    for path in ("culled", "scan"):
        with R.option("refit_path", path, cloud=pc):
            for i in which:
                got = R.refit(cs.arr[i], pc, cs.cp).inpoints
                assert np.array_equal(got, exp[i]), (f32, path, i, len(got), len(exp[i]))
