"""Everything bound to a cloud -- its own buffers, the batch workspaces and their slots, the workspaces grown on demand,
the buffers rh_ransac parks on it between runs, the device scratch of the reference octree -- is held by the owners of
csrc/dev_buf.h and goes with the cloud: creating a cloud, using it and destroying it leaves the device's free memory
where it was.

Protocol and reasoning are those of tests/test_call_scope_gpu.py: the figure is the whole device's free memory
(torch.cuda.mem_get_info), in steps of 2 MiB; it moves in a use's FIRST round only (the runtime's start, the code
objects) and by exactly 0 bytes from the second round on, so 0 is what is allowed.  Other processes may share the device
and a step of theirs can fall into a window; a leak grows with the rounds and shows in every window, a step from outside
does not: one warm-up round, then up to three windows of 20 rounds, and one of them must show 0.  The cloud has 200 000
points, so the smallest per-point buffer (one byte per point) lost once a round comes to 4 MB a window, two steps of the
figure; a lost scalar buffer, event or stream is below what this figure can show (tests/native/dev_buf_check.cpp counts
those on a runtime of its own).

include/ransac_hip.h defines no input that rh_cloud_create refuses after its first device buffers exist (the arguments
are checked before the first allocation; from there on only a failing HIP call or host allocation ends it early), so
that way out has no case here."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L, dist as rdist, synth

pytestmark = pytest.mark.gpu

N = 200_000
KINDS4 = [R.FittedPlane, R.FittedSphere, R.FittedCylinder, R.FittedCone]
KMAP = {"plane": L.PLANE, "sphere": L.SPHERE, "cylinder": L.CYLINDER, "cone": L.CONE}


def _shapes_c(cands):
    arr = (L.Shape * len(cands))()
    for i, (name, outw, v) in enumerate(cands):
        arr[i].kind, arr[i].outwards = KMAP[name], int(outw)
        for j, x in enumerate(v):
            arr[i].v[j] = float(x)
        R.lib().rh_shape_finalize(C.byref(arr[i]))
    return arr


@pytest.fixture(scope="module")
def scene():
    """computed once and left unchanged: the points, two subsets, the candidate batches, the parameters"""
    xyz, nrm, truth = synth.make_cloud(N, ["plane", "sphere", "cylinder", "cone"], 0.2, seed=3)
    s = {"xyz": xyz, "nrm": nrm, "subs": synth.make_subsets(N, 2, seed=3)}
    s["small"] = _shapes_c(synth.jittered_candidates(truth, 64, seed=1))
    s["large"] = _shapes_c(synth.jittered_candidates(truth, 1500, seed=2))
    s["params"] = R.ransacparameters(KINDS4)
    s["plane"] = R.FittedPlane(truth[0]["point"], truth[0]["normal"])
    s["shapes4"] = [R.shape_from_c(s["small"][i]) for i in range(4)]
    words = (s["subs"][0].size + 63) // 64
    s["ring_counts"] = [torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(4)]
    s["ring_masks"] = [torch.zeros(64 * words, dtype=torch.int64, device="cuda") for _ in range(4)]
    return s


def _cloud(s, f32=False):
    return R.RANSACCloud(s["xyz"], s["nrm"], s["subs"], force_eltype=np.float32 if f32 else None)


def _score_batch(s):
    """64 and then 1 500 candidates, without and with masks: the second batch makes the batch workspace and the mask
    buffers grow after their first use"""
    pc = _cloud(s)
    for want_masks in (False, True):
        for batch in (s["small"], s["large"]):
            R.score_batch(pc, batch, s["params"], want_masks=want_masks)


def _batches_in_flight(s):
    """every batch slot gets its stream, its events and its workspaces -- counts, then masks -- and, with st_cull = 1, its
    super-tile lists"""
    pc = _cloud(s)
    lib, cp, b = R.lib(), R.params_to_c(s["params"]), 64
    bt = rdist.DeviceBatch(pc, s["small"], b)
    R.set_option("batches_in_flight", 4, cloud=pc)
    R.set_option("st_cull", 1, cloud=pc)
    for with_masks in (False, True):
        for k in range(8):
            masks = C.c_void_p(s["ring_masks"][k % 4].data_ptr()) if with_masks else None
            L.check(lib.rh_score_batch_dev(pc._h, bt.slice_ptr(0), b, C.byref(cp), C.c_void_p(s["ring_counts"][k % 4].data_ptr()), masks))
    L.check(lib.rh_cloud_sync(pc._h))
    bt.free()


def _refits(s):
    pc = _cloud(s)
    ex = R.refit(s["plane"], pc, s["params"])
    R.refit_component(s["plane"], pc, s["params"], 0.5)
    R.refit_lsq(s["plane"], pc, s["params"])
    R.shape_extents(pc, [ex])
    R.assign_cloud(pc, s["shapes4"], s["params"])


def _ransac(s, f32, sampling_streams, octree):
    """twice in a row on one cloud: the second run takes back what the first one parked on the cloud, and parks it again"""
    pc = _cloud(s, f32)
    prm = R.ransacparameters(KINDS4, iteration={"minsubsetN": 64, "itermax": 32, "τ": 300, "prob_det": 0.7})
    for seed in (1, 2):
        R.ransac(pc, prm, seed=seed, sampling_streams=sampling_streams, octree_sampling=octree)


def _octree_cell(s):
    """the reference octree's device scratch (rh_octree) belongs to the tree.  An OctreeCell and its `.data` refer to each
    other, so Python lets go of a tree only when its cyclic collector runs -- measured round by round, parent commit and
    this one alike: 2 MiB less free memory per round, back to the start every 13 or 14 rounds.  The round therefore ends
    with a collection of the young generations: what is under test is the library's ownership, not the collector's timing."""
    pc = _cloud(s)
    R.cell_enabled_points(pc, pc.octree.children[0])
    del pc
    gc.collect(1)


USES = {"score_batch": _score_batch, "batches_in_flight": _batches_in_flight, "refits": _refits, "octree_cell": _octree_cell}
for _f32 in (False, True):
    USES["ransac_%s_host" % ("f32" if _f32 else "f64")] = lambda s, f=_f32: _ransac(s, f, 0, False)
    USES["ransac_%s_device" % ("f32" if _f32 else "f64")] = lambda s, f=_f32: _ransac(s, f, 1, False)
    USES["ransac_%s_octree" % ("f32" if _f32 else "f64")] = lambda s, f=_f32: _ransac(s, f, 1, True)


@pytest.mark.parametrize("name", sorted(USES))
def test_a_cloud_takes_its_buffers_with_it(scene, name):
    one_round = USES[name]   # creates a cloud, uses it; the cloud goes with the round's last reference to it

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    one_round(scene)
    seen = []
    for _ in range(3):
        warm = free_bytes()
        for _ in range(20):
            one_round(scene)
        seen.append(warm - free_bytes())
        print("%s: free before the window %d, after its 20 rounds %d bytes less" % (name, warm, seen[-1]))
        if seen[-1] == 0:
            break
    assert 0 in seen, seen
