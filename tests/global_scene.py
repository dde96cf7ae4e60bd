"""The scene of the global-registration tests: a floor, a wall, a half-sphere and a half-cylinder, a quarter of the points
on each, exact normals, noise sigma = 0.003 on the points; two DISJOINT samples of it of 2048 points each, the second one
moved by an arbitrary rotation and a shift of about 5 units.  Shared by tests/test_global_host.py (the condition of the
twin chain) and tests/test_global_gpu.py (the library against that chain)."""
import math

import numpy as np

from register_reference import apply, rigid

SIGMA = 0.003
N = 2048                      # points per sample
TAU, K, TRIALS, EDGE_RATIO = 0.1, 32, 20000, 0.9
SEEDS = (1, 2, 3)


def surfaces(per, rng):
    """per points on each of the four surfaces: (xyz, normals), before noise"""
    u, v = rng.uniform(0.0, 1.0, size=(2, 4, per))
    z0, o1 = np.zeros(per), np.ones(per)
    floor = np.stack([2.0 * u[0], 1.5 * v[0], z0], axis=1), np.stack([z0, z0, o1], axis=1)
    wall = np.stack([z0, 1.5 * u[1], 1.0 * v[1]], axis=1), np.stack([o1, z0, z0], axis=1)
    ph, ct = 2.0 * math.pi * u[2], v[2]                            # uniform on the upper half-sphere: cos(theta) uniform
    st = np.sqrt(1.0 - ct * ct)
    sn = np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=1)
    sphere = np.array([1.3, 0.8, 0.0]) + 0.45 * sn, sn
    an = math.pi * u[3]
    cn = np.stack([np.cos(an), z0, np.sin(an)], axis=1)
    cyl = np.stack([0.6 + 0.25 * cn[:, 0], 0.1 + 1.2 * v[3], 0.25 * cn[:, 2]], axis=1), cn
    return (np.concatenate([s[0] for s in (floor, wall, sphere, cyl)]), np.concatenate([s[1] for s in (floor, wall, sphere, cyl)]))


def make(seed=0, n=N):
    """dict: ref, ref_nrm (sample A, as it lies), qry, qry_nrm (sample B, moved), motion (3x4, scene -> query frame),
    inverse (3x4, the motion the registration should find), truth (sample B where it lies in the reference's frame)."""
    rng = np.random.default_rng(1000 + seed)
    xyz, nrm = surfaces(2 * n // 4, rng)
    xyz = xyz + rng.normal(0.0, SIGMA, size=xyz.shape)
    order = rng.permutation(len(xyz))
    a, b = order[:n], order[n:2 * n]                               # disjoint: no point is in both samples
    motion = rigid(137.0, 5.0, 11 + seed, np.array([1.0, 0.75, 0.3]))
    Rm = motion[:, :3]
    inverse = np.hstack([Rm.T, -(Rm.T @ motion[:, 3])[:, None]])
    return dict(ref=np.ascontiguousarray(xyz[a]), ref_nrm=np.ascontiguousarray(nrm[a]),
                qry=np.ascontiguousarray(apply(motion, xyz[b])), qry_nrm=np.ascontiguousarray(nrm[b] @ Rm.T),
                motion=motion, inverse=inverse, truth=np.ascontiguousarray(xyz[b]))


def rotation_error_deg(T, inverse):
    """the angle of T's rotation against the true one"""
    M = np.asarray(T)[:3, :3] @ np.asarray(inverse)[:3, :3].T
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(M) - 1.0) / 2.0))))


def point_error(T, scene):
    """the largest distance of a moved query from where it lies in the reference's frame"""
    return float(np.linalg.norm(apply(np.asarray(T)[:3], scene["qry"]) - scene["truth"], axis=1).max())
