"""Interleaved calls on one cloud: everything that changes the enabled bits or lives off a structure derived from them, in
seeded random order, against a numpy model of the bits.  After every step isenabled equals the model, and the step's own
result equals what the model says: the popcount, the r-th set bit, the oracle's refit list on the model's bits, the counts
of a fresh cloud given the model's bits, the minimal sets of a second cloud that only ever gets them through set_enabled.
Only isenabled is read after EVERY step: the other checks take the scan scratch or build the directory themselves, and run
after every step they would put the cloud into the same state each time -- the interleavings are the point.  Every 8 steps
and at the end a short ransac() -- rank sampling, then octree sampling -- equals the same calls on a fresh cloud given the
model's bits.

Sizes: an empty cloud, a last word short of one bit, one full word, and 64 * 1024 + 37 points: a partial last word and two
scan blocks (RH_WORDS_PER_BLOCK = 1024 words), the smallest size at which the scan of the block sums and the fold's own
summing of the blocks before it both have something to add."""
import ctypes as C
import functools

import numpy as np
import pytest

import ransac_jl_amd as R
from oracle import oracle as orc
from ransac_jl_amd import _lib as L
from ransac_jl_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (0, 63, 64, 64 * 1024 + 37)
STEPS = 150
RANSAC_EVERY = 8


@functools.lru_cache(maxsize=None)
def scene(n):
    """plane + sphere + a fifth outliers; the shapes asked about are the scene's own two and two that miss"""
    xyz, nrm, truth = synth.make_cloud(max(n, 64), ["plane", "sphere"], 0.2, seed=11)
    plane, sphere = truth
    shapes = [R.FittedPlane(plane["point"], plane["normal"]), R.FittedSphere(sphere["center"], sphere["radius"], True),
              R.FittedPlane(plane["point"] + 3.0 * np.asarray(plane["normal"]), plane["normal"]),
              R.FittedSphere(sphere["center"], 0.5 * sphere["radius"], False)]
    subs = synth.make_subsets(n, 16 if n > 4096 else 1, seed=11) if n > 0 else [np.zeros(0, dtype=np.int64)]
    return xyz[:n].copy(), nrm[:n].copy(), subs, shapes


def chunks_of(mask):
    bits = np.zeros((mask.size + 63) // 64 * 64, dtype=np.uint8)
    bits[: mask.size] = mask
    return np.packbits(bits, bitorder="little").view(np.uint64)


class Run:
    def __init__(self, n, path, f32):
        self.n, self.path, self.f32 = n, path, f32
        self.xyz, self.nrm, self.subs, self.shapes = scene(n)
        self.pc = self.cloud()
        self.ref = self.cloud()                                   # only ever: set_enabled(model), then one read-only call
        self.oc = orc.Cloud(self.xyz, self.nrm, self.subs[0], f32=f32)
        self.params = R.ransacparameters([R.FittedPlane, R.FittedSphere], iteration={"itermax": 48, "minsubsetN": 64})
        self.cp = R.params_to_c(self.params)
        self.op = orc.Params.from_buffer_copy(bytes(self.cp))
        wide = R.params_to_c(self.params)                         # the least-squares refit selects within 3 eps
        for k in range(4):
            wide.eps[k] = 3.0 * wide.eps[k]
        self.op3 = orc.Params.from_buffer_copy(bytes(wide))
        self.model = np.ones(n, dtype=bool)
        self.rs = np.random.default_rng([n, len(path), int(f32)])

    def cloud(self):
        pc = R.RANSACCloud(self.xyz, self.nrm, self.subs, force_eltype=np.float32 if self.f32 else None)
        R.set_option("refit_path", self.path, cloud=pc)
        return pc

    def c_shape(self, s):
        return R.shape_f32(s) if self.f32 else s.to_c()

    def oracle_refit(self, s, op):
        self.oc.set_enabled(chunks_of(self.model))
        return self.oc.refit(orc.Shape.from_buffer_copy(bytes(self.c_shape(s))), op)

    def ref_cloud(self):
        self.ref.set_enabled(self.model)
        return self.ref

    # ---- the steps ----
    def set_enabled(self):
        self.model = self.rs.random(self.n) < self.rs.choice([0.0, 0.3, 0.9, 1.0])
        self.pc.set_enabled(self.model)

    def enable_all(self):
        self.model = np.ones(self.n, dtype=bool)
        self.pc.enable_all()

    def invalidate(self):
        k = 0 if self.n == 0 else int(self.rs.choice([1, 7, self.n // 3 + 1, self.n + 5]))   # (the last: longer than the cloud)
        idx = self.rs.integers(1, self.n + 1, size=k) if k else np.zeros(0, dtype=np.int64)   # duplicates included
        self.model[idx - 1] = False
        R.invalidate_indexes(self.pc, idx)

    def refit(self):
        s = self.shapes[self.rs.integers(len(self.shapes))]
        assert np.array_equal(R.refit(s, self.pc, self.cp).inpoints, self.oracle_refit(s, self.op))

    def refit_component(self):
        if self.n == 0:
            return
        s = self.shapes[self.rs.integers(2)]
        beta, conn26 = float(self.rs.choice([0.5, 2.0])), bool(self.rs.integers(2))
        got, st = R.refit_component(s, self.pc, self.cp, beta, conn26, return_stats=True)
        exp, est = R.refit_component(s, self.ref_cloud(), self.cp, beta, conn26, return_stats=True)
        whole = self.oracle_refit(s, self.op)
        assert st == est and st["n_refit"] == whole.size
        assert np.array_equal(got.inpoints, exp.inpoints) and np.isin(got.inpoints, whole).all()

    def refit_lsq(self):
        if self.n == 0 or self.f32:                               # (Float64 clouds only)
            return
        s = self.shapes[self.rs.integers(2)]
        near = self.oracle_refit(s, self.op3).size
        if near < 8:
            with pytest.raises(R.RansacHipError):
                R.refit_lsq(s, self.pc, self.cp, max_iter=2)
        else:
            assert R.refit_lsq(s, self.pc, self.cp, max_iter=2)[1] == near

    def count_enabled(self):
        assert self.pc.count_enabled() == int(self.model.sum())

    def select_enabled(self):
        on = np.flatnonzero(self.model) + 1
        k = int(self.rs.choice([3, 1500]))                        # (1024 ranks and fewer go through pinned memory)
        ranks = self.rs.integers(0, on.size + 2, size=k)          # 0 and count + 1: no such point
        exp = np.where((ranks >= 1) & (ranks <= on.size), np.append(on, 0)[np.clip(ranks - 1, 0, on.size)], 0)
        assert np.array_equal(R.select_enabled(self.pc, ranks), exp)

    def sample_sets(self):
        if self.model.sum() < 3:
            return
        seed = int(self.rs.integers(1 << 30))
        out = []
        for pc in (self.pc, self.ref_cloud()):
            rng = L.Rng()
            R.lib().rh_rng_seed(C.byref(rng), seed)
            idx, ok, _ = R.sample_sets(pc, 3, rng, 5)
            out.append((idx.copy(), ok.copy(), rng.draws))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
        assert self.model[out[0][0][out[0][0] > 0] - 1].all()

    def score(self):
        arr = (L.Shape * len(self.shapes))(*[self.c_shape(s) for s in self.shapes])
        fresh = self.cloud()
        fresh.set_enabled(self.model)
        assert np.array_equal(R.score_batch(self.pc, arr, self.cp), R.score_batch(fresh, arr, self.cp))

    def ransac(self):
        if self.model.sum() < 16:
            return
        fresh = self.cloud()
        fresh.set_enabled(self.model)
        for octree in (False, True):
            cp = R.params_to_c(self.params, sampling_streams=1, octree_sampling=octree)
            got, _ = R.ransac(self.pc, cp, seed=5)
            exp, _ = R.ransac(fresh, cp, seed=5)
            assert len(got) == len(exp)
            for g, e in zip(got, exp):
                assert bytes(g.c_shape) == bytes(e.c_shape) and np.array_equal(g.inpoints, e.inpoints)
                self.model[g.inpoints - 1] = False
            assert np.array_equal(self.pc.isenabled, self.model) and np.array_equal(fresh.isenabled, self.model)

    KINDS = (set_enabled, enable_all, invalidate, refit, refit_component, refit_lsq, count_enabled, select_enabled,
             sample_sets, score)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("path", ["scan", "culled"])
@pytest.mark.parametrize("n", SIZES)
def test_interleaved_calls_follow_the_model(n, path, f32):
    run = Run(n, path, f32)
    for k in range(1, STEPS + 1):
        step = Run.KINDS[run.rs.integers(len(Run.KINDS))]
        step(run)
        assert np.array_equal(run.pc.isenabled, run.model), (k, step.__name__)
        if k % RANSAC_EVERY == 0 or k == STEPS:
            run.ransac()
