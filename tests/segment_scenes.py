"""The clouds of tests/test_segment_host.py and tests/test_segment_gpu.py: each scene is (xyz, normals, curvature or None,
the keyword arguments of segment_reference.ref_segment).  Everything is synthetic -- no other tool of the library is
involved -- and small enough for the brute-force twin.  twin(name) computes a scene's reference once and shares it."""
import numpy as np

from segment_reference import UNSIGNED, ref_segment

COS25, COS20, COS10 = float(np.cos(np.radians(25.0))), float(np.cos(np.radians(20.0))), float(np.cos(np.radians(10.0)))


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _jittered(nu, nv, rng, jitter=0.25):
    """(nu * nv, 2): a grid over the unit square, every point moved by up to `jitter` of a cell"""
    u, v = np.meshgrid((np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv, indexing="ij")
    g = np.stack([u.ravel(), v.ravel()], axis=1)
    return g + rng.uniform(-jitter, jitter, size=g.shape) / [nu, nv]


def corner():
    """three orthogonal patches of 22 x 22 points meeting in the axes; the normals bend towards the nearer crease and
    carry a little noise, the curvature is 0.2 exp(-d / 0.04) of the distance d to the nearer crease"""
    rng = np.random.default_rng(31)
    pts, nrm, curv = [], [], []
    for axis in range(3):                                   # the patch in the plane x_axis = 0
        a, b = (axis + 1) % 3, (axis + 2) % 3
        g = _jittered(22, 22, rng)
        p = np.zeros((len(g), 3))
        p[:, a], p[:, b] = g[:, 0], g[:, 1]
        own = np.zeros(3); own[axis] = 1.0
        # the crease at x_a = 0 is shared with the patch whose normal is e_a, the one at x_b = 0 with e_b
        d = np.minimum(g[:, 0], g[:, 1])
        other = np.where((g[:, 0] < g[:, 1])[:, None], np.eye(3)[a], np.eye(3)[b])
        w = 0.5 * np.exp(-d / 0.04)
        pts.append(p)
        nrm.append(_unit(own + w[:, None] * other + rng.normal(0, 0.01, size=p.shape)))
        curv.append(0.2 * np.exp(-d / 0.04))
    order = rng.permutation(3 * 484)
    return (np.concatenate(pts)[order], np.concatenate(nrm)[order], np.concatenate(curv)[order],
            dict(k=12, cos_angle=COS25, curv_max=0.05))


def fold():
    """2400 points on two half-planes 30 degrees apart; the band |s| < 0.05 around the crease carries the bisector normal
    and a high curvature"""
    rng = np.random.default_rng(32)
    s, t = rng.uniform(-1, 1, 2400), rng.uniform(0, 1.2, 2400)
    c30, s30 = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    p = np.where((s < 0)[:, None], np.stack([s, t, 0 * s], axis=1), np.stack([s * c30, t, s * s30], axis=1))
    na, nb = np.array([0.0, 0.0, 1.0]), np.array([-s30, 0.0, c30])
    band = np.abs(s) < 0.05
    n = np.where(band[:, None], _unit((na + nb)[None, :]), np.where((s < 0)[:, None], na, nb))
    return p, n, np.where(band, 0.2, 0.0), dict(k=12, cos_angle=COS20, curv_max=0.05)


def _sheet(rng):
    g = _jittered(50, 50, rng) * 2.0 - 1.0
    return np.stack([g[:, 0], g[:, 1], 0 * g[:, 0]], axis=1)


STEP_EXTRA = 4     # the last points of `steps`: a pair at exactly dist_max, a pair one ulp beyond it


def steps(dist_max):
    """2500 points, z = 0 for x < 0 and z = 0.03 for x > 0, all normals +z; far away a pair whose tangent-plane distance is
    exactly 0.015 and a pair whose distance is the next double.  The radius keeps the pairs to themselves."""
    p = _sheet(np.random.default_rng(33))
    p[p[:, 0] > 0, 2] = 0.03
    extra = np.array([[3.0, 0.0, 0.0], [3.05, 0.0, 0.015], [-3.0, 0.0, 0.0], [-3.05, 0.0, np.nextafter(0.015, 1.0)]])
    p = np.concatenate([p, extra])
    return p, np.tile([0.0, 0.0, 1.0], (len(p), 1)), None, dict(k=12, radius=0.12, cos_angle=0.9, dist_max=dist_max)


def flipped(flags):
    """the flat sheet with random normal signs"""
    rng = np.random.default_rng(34)
    p = _sheet(rng)
    n = np.tile([0.0, 0.0, 1.0], (len(p), 1)) * rng.choice([-1.0, 1.0], size=(len(p), 1))
    return p, n, None, dict(k=12, cos_angle=0.9, flags=flags)


def ribbon(permuted):
    """a strip of 5000 points along a helix, two points across, the normals turning slowly with the helix: one region, so
    one union chain crosses every block"""
    i = np.arange(5000)
    t = 0.04 * (i // 2)
    p = np.stack([3 * np.cos(t), 3 * np.sin(t), 0.08 * t + 0.04 * (i % 2)], axis=1)
    n = np.stack([np.cos(t), np.sin(t), 0 * t], axis=1)
    if permuted:
        o = np.random.default_rng(35).permutation(5000)
        p, n = p[o], n[o]
    return p, n, None, dict(k=8, cos_angle=COS10)


def lattice(k):
    """integer coordinates, equal normals, a checkerboard of seeds, in a random order: d2 ties everywhere -- in the search,
    and in the border choice, which goes to the smaller index"""
    x, y = np.meshgrid(np.arange(30), np.arange(30), indexing="ij")
    o = np.random.default_rng(36).permutation(900)
    p = np.stack([x.ravel(), y.ravel(), 0 * x.ravel()], axis=1).astype(np.float64)[o]
    curv = ((x.ravel() + y.ravel()) % 2).astype(np.float64)[o]
    return p, np.tile([0.0, 0.0, 1.0], (900, 1)), curv, dict(k=k, cos_angle=0.9, curv_max=0.5, order="index")


def holes():
    """the corner scene with every seventh normal (0, 0, 0) and a NaN curvature here and there"""
    p, n, c, kw = corner()
    n, c = n.copy(), c.copy()
    n[::7] = 0.0
    c[3::50] = np.nan
    return p, n, c, kw


def sparse():
    """a radius that leaves some points without a neighbour: the sheet thinned at random"""
    rng = np.random.default_rng(37)
    p = _sheet(rng)[rng.permutation(2500)[:1001]]
    return p, np.tile([0.0, 0.0, 1.0], (len(p), 1)), None, dict(k=6, radius=0.06, cos_angle=0.9)


MAKERS = {"corner": corner, "fold": fold, "steps_off": lambda: steps(0.0), "steps_on": lambda: steps(0.015),
          "flipped_unsigned": lambda: flipped(UNSIGNED), "flipped_signed": lambda: flipped(0),
          "ribbon": lambda: ribbon(False), "ribbon_permuted": lambda: ribbon(True),
          "lattice4": lambda: lattice(4), "lattice8": lambda: lattice(8), "holes": holes, "sparse": sparse,
          "identical": lambda: (np.tile([[1.5, -2.0, 0.25]], (500, 1)), np.tile([[0.0, 1.0, 0.0]], (500, 1)), None,
                                dict(k=16, cos_angle=0.9)),
          "one": lambda: (np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 1.0]]), None, dict(k=16, cos_angle=0.9)),
          "five": lambda: (np.arange(15, dtype=np.float64).reshape(5, 3) * 0.1, np.tile([[0.0, 0.0, 1.0]], (5, 1)),
                           np.array([0.0, 0.0, 1.0, 0.0, 0.0]), dict(k=16, cos_angle=0.9, curv_max=0.5))}
_DATA, _REF = {}, {}


def scene(name):
    """(xyz, normals, curvature or None, keyword arguments), made once and read-only"""
    if name not in _DATA:
        p, n, c, kw = MAKERS[name]()
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (p, n)] + [None if c is None else np.ascontiguousarray(c, dtype=np.float64)]
        for a in arrs:
            if a is not None:
                a.setflags(write=False)
        _DATA[name] = (arrs[0], arrs[1], arrs[2], kw)
    return _DATA[name]


def twin(name, **over):
    """the twin's result for a scene, with keyword arguments replaced by `over`; computed once per case and shared"""
    key = (name, tuple(sorted(over.items())))
    if key not in _REF:
        p, n, c, kw = scene(name)
        _REF[key] = ref_segment(p, n, c, **dict(kw, **over))
    return _REF[key]
