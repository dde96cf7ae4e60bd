"""Oriented extents of extracted shapes (rh_shape_extents, include/ransac_hip.h): `ref_extents`, the numpy twin of the
header's six steps that tests/test_extents_gpu.py holds the device against, checked here against shapes whose extents are
known in closed form; the header / binding / JSON side of the feature.  No GPU."""
import io as _io
import json
import os
import re

import numpy as np

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_EMPTY, EXT_NO_DIRECTION = 1, 2


def _origin_axis(shape):
    v = np.array(list(shape.v), dtype=np.float64)
    if shape.kind == L.PLANE:
        return v[0:3].copy(), v[3:6].copy()
    if shape.kind == L.SPHERE:
        return v[0:3].copy(), None
    if shape.kind == L.CYLINDER:
        return v[3:6].copy(), v[0:3].copy()
    return v[0:3].copy(), v[3:6].copy()


def _signed_unit(u):
    u = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return -u if u[int(np.argmax(np.abs(u)))] < 0 else u      # argmax: the first one on ties


def fallback_u(w):
    k = int(np.argmin(np.abs(w)))                              # the first one on ties
    e = np.zeros(3)
    e[k] = 1.0
    u = e - w * w[k]
    return u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])


def box_and_distance(xyz, shape, idx, origin, frame):
    """steps 4 and 5, in the header's operation order: plain float64 ufuncs, which numpy never fuses
    -> lo[3], hi[3], e[n]"""
    p = np.asarray(xyz, dtype=np.float64)[np.asarray(idx, dtype=np.int64) - 1]
    dx, dy, dz = p[:, 0] - origin[0], p[:, 1] - origin[1], p[:, 2] - origin[2]
    t = [(dx * f[0] + dy * f[1]) + dz * f[2] for f in np.asarray(frame).reshape(3, 3)]
    v = list(shape.v)
    if shape.kind == L.PLANE:
        e = t[2]
    elif shape.kind == L.SPHERE:
        e = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) - v[3]
    elif shape.kind == L.CYLINDER:
        e = np.sqrt(t[0] * t[0] + t[1] * t[1]) - v[6]
    else:
        e = np.sqrt(t[0] * t[0] + t[1] * t[1]) * v[7] + t[2] * v[8]
    return np.array([x.min() for x in t]), np.array([x.max() for x in t]), e


def ref_extents(xyz, shape, idx, frame=None):
    """The six steps of include/ransac_hip.h for one shape (an _lib.Shape) and its 1-based index list -> dict with the
    fields of rh_extent.  frame: steps 4 to 6 from this frame instead of the twin's own (they are exact given the frame)."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n = idx.size
    origin, axis = _origin_axis(shape)
    out = dict(n=n, kind=int(shape.kind), flags=0, origin=origin, frame=np.zeros((3, 3)), lo=np.zeros(3), hi=np.zeros(3),
               centroid=np.zeros(3), lam=np.zeros(3), dist_rms=0.0, dist_maxabs=0.0)
    if n == 0:
        out["flags"] = EXT_EMPTY
        return out
    p = np.asarray(xyz, dtype=np.float64)[idx - 1]
    q = p - p[0]
    m = q.sum(axis=0) / n
    S = (q[:, :, None] * q[:, None, :]).sum(axis=0) / n - np.outer(m, m)
    out["centroid"] = p[0] + m
    if axis is None:
        lam, vec = np.linalg.eigh(S)
        order = np.argsort(-lam, kind="stable")
        out["lam"] = lam[order]
        if out["lam"][0] > 0:
            u, v = _signed_unit(vec[:, order[0]]), _signed_unit(vec[:, order[1]])
            fr = np.stack([u, v, np.cross(u, v)])
        else:
            out["flags"] |= EXT_NO_DIRECTION
            fr = np.eye(3)
    else:
        w = axis / np.sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])
        P = np.eye(3) - np.outer(w, w)
        M = P @ S @ P
        lam, vec = np.linalg.eigh((M + M.T) / 2)
        order = np.argsort(-lam, kind="stable")
        out["lam"] = np.array([lam[order[0]], lam[order[1]], 0.0])
        if out["lam"][0] > 0:
            u = vec[:, order[0]]
            u = _signed_unit(u - w * (w @ u))
        else:
            out["flags"] |= EXT_NO_DIRECTION
            u = fallback_u(w)
        fr = np.stack([u, np.cross(w, u), w])
    out["frame"] = fr if frame is None else np.asarray(frame, dtype=np.float64).reshape(3, 3)
    out["lo"], out["hi"], e = box_and_distance(xyz, shape, idx, origin, out["frame"])
    out["dist_maxabs"] = float(np.abs(e).max())
    out["dist_rms"] = float(np.sqrt((e * e).sum() / n))
    return out


# ------------------------------------------------------------------ inputs with a known answer ----
def _basis(z):
    z = np.asarray(z, dtype=np.float64)
    z = z / np.linalg.norm(z)
    a = np.array([1.0, 0, 0]) if abs(z[0]) < 0.9 else np.array([0, 1.0, 0])
    x = np.cross(z, a)
    x /= np.linalg.norm(x)
    return x, np.cross(z, x), z


def rectangle(n, rng, sides=(20.0, 10.0), normal=(0.3, -0.5, 0.8), centre=(40.0, 50.0, 60.0), noise=0.0):
    x, y, z = _basis(normal)
    uv = rng.uniform(-0.5, 0.5, size=(n, 2)) * np.asarray(sides)
    p = np.asarray(centre) + uv[:, :1] * x + uv[:, 1:] * y + rng.normal(0, noise, size=(n, 1)) * z if noise else \
        np.asarray(centre) + uv[:, :1] * x + uv[:, 1:] * y
    return p, R.FittedPlane(centre, z).to_c(), x


def cylinder_part(n, rng, r=4.0, heights=(3.0, 17.0), arc=(0.0, 2 * np.pi), axis=(0.5, 0.7, -0.4), centre=(30.0, 20.0, 70.0)):
    x, y, z = _basis(axis)
    th, h = rng.uniform(arc[0], arc[1], n), rng.uniform(heights[0], heights[1], n)
    p = np.asarray(centre) + h[:, None] * z + r * (np.cos(th)[:, None] * x + np.sin(th)[:, None] * y)
    return p, R.FittedCylinder(z, centre, r, True).to_c(), (x, y, z)


def cone_frustum(n, rng, half=np.radians(25.0), slant=(6.0, 30.0), arc=(0.0, 2 * np.pi), axis=(-0.2, 0.6, 0.75), apex=(55.0, 45.0, 35.0)):
    x, y, z = _basis(axis)
    th, s = rng.uniform(arc[0], arc[1], n), rng.uniform(slant[0], slant[1], n)
    radial = np.cos(th)[:, None] * x + np.sin(th)[:, None] * y
    p = np.asarray(apex) + s[:, None] * (np.cos(half) * z + np.sin(half) * radial)
    return p, R.FittedCone(apex, z, 2 * half, True).to_c(), (x, y, z)


def sphere_patch(n, rng, r=8.0, lon=(-np.pi, np.pi), lat=(np.radians(30.0), np.pi / 2), pole=(0.4, 0.5, 0.77), centre=(60.0, 30.0, 40.0)):
    """points with latitude (above the equator of `pole`) and longitude in the given ranges; the default is the cap
    within 60 degrees of the pole"""
    x, y, z = _basis(pole)
    lo, la = rng.uniform(lon[0], lon[1], n), np.arcsin(rng.uniform(np.sin(lat[0]), np.sin(lat[1]), n))
    d = np.cos(la)[:, None] * (np.cos(lo)[:, None] * x + np.sin(lo)[:, None] * y) + np.sin(la)[:, None] * z
    return np.asarray(centre) + r * d, R.FittedSphere(centre, r, True).to_c(), (x, y, z)


def _all(n):
    return np.arange(1, n + 1, dtype=np.int64)


# ------------------------------------------------------------------------------------- the twin ----
def test_rectangle_on_a_tilted_plane():
    rng = np.random.default_rng(1)
    p, shape, long_side = rectangle(20000, rng)
    e = ref_extents(p, shape, _all(len(p)))
    assert e["n"] == 20000 and e["flags"] == 0 and e["kind"] == L.PLANE
    assert abs(e["frame"][0] @ long_side) >= np.cos(np.radians(1.0))
    size = e["hi"] - e["lo"]
    assert abs(size[0] - 20.0) <= 0.2 and abs(size[1] - 10.0) <= 0.1 and size[2] <= 1e-12
    assert e["dist_maxabs"] <= 1e-12 and e["dist_rms"] <= e["dist_maxabs"]
    assert np.allclose(e["lam"][:2], [400.0 / 12, 100.0 / 12], rtol=0.03) and e["lam"][2] == 0.0
    assert np.allclose(e["centroid"], p.mean(axis=0), rtol=0, atol=1e-10)
    fr = e["frame"]
    assert np.abs(fr @ fr.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(fr) - 1.0) <= 1e-12
    assert np.array_equal(fr[2], np.array(list(shape.v)[3:6]) / np.sqrt((shape.v[3] ** 2 + shape.v[4] ** 2) + shape.v[5] ** 2))
    # duplicates count as given, the order does not matter beyond rounding
    idx = np.concatenate([_all(len(p)), _all(100)])[rng.permutation(20100)]
    d = ref_extents(p, shape, idx)
    assert d["n"] == 20100 and np.array_equal(d["lo"], box_and_distance(p, shape, idx, d["origin"], d["frame"])[0])


def test_cylinder_heights_and_half_cylinder():
    rng = np.random.default_rng(2)
    p, shape, (x, y, z) = cylinder_part(20000, rng)
    e = ref_extents(p, shape, _all(len(p)))
    assert np.array_equal(e["origin"], [30.0, 20.0, 70.0])
    assert abs(e["lo"][2] - 3.0) <= 0.01 and abs(e["hi"][2] - 17.0) <= 0.01          # heights in [3, 17] along the axis
    assert e["dist_maxabs"] <= 1e-12
    assert np.allclose(e["lam"][:2], [8.0, 8.0], rtol=0.05)                              # r^2 / 2 both: no direction, lambda tells
    # half a cylinder: the (u, v) box is 2r x r, u along the chord
    p, shape, (x, y, z) = cylinder_part(20000, rng, arc=(0.0, np.pi))
    e = ref_extents(p, shape, _all(len(p)))
    assert (e["lam"][0] - e["lam"][1]) / e["lam"][0] >= 0.5
    assert abs(e["frame"][0] @ x) >= np.cos(np.radians(1.0))
    size = e["hi"] - e["lo"]
    assert abs(size[0] - 8.0) <= 0.08 and abs(size[1] - 4.0) <= 0.04 and abs(size[2] - 14.0) <= 0.02


def test_cone_frustum_and_spherical_cap():
    rng = np.random.default_rng(3)
    half = np.radians(25.0)
    p, shape, (x, y, z) = cone_frustum(20000, rng)
    e = ref_extents(p, shape, _all(len(p)))
    assert abs(e["lo"][2] - 6.0 * np.cos(half)) <= 0.01 and abs(e["hi"][2] - 30.0 * np.cos(half)) <= 0.01
    assert e["dist_maxabs"] <= 1e-12
    # the widest ring has radius 30 sin(half): the (u, v) box is that circle's, whatever the in-plane rotation
    assert np.allclose((e["hi"] - e["lo"])[:2], 2 * 30.0 * np.sin(half), rtol=0.01)
    # the cap within 60 degrees of a pole: two equal tangential eigenvalues, the smallest along the pole
    p, shape, (x, y, z) = sphere_patch(20000, rng)
    e = ref_extents(p, shape, _all(len(p)))
    assert e["lam"][0] >= e["lam"][1] >= e["lam"][2] > 0
    assert np.allclose(e["lam"], [64 * (1 - 7 / 12) / 2, 64 * (1 - 7 / 12) / 2, 64 * 0.25 / 12], rtol=0.05)
    assert abs(e["frame"][2] @ z) >= np.cos(np.radians(2.0))
    size = e["hi"] - e["lo"]
    assert abs(size[2] - 4.0) <= 0.04 and np.allclose(size[:2], 2 * 8.0 * np.sin(np.radians(60.0)), rtol=0.01)
    assert e["dist_maxabs"] <= 1e-12


def test_degenerate_lists():
    rng = np.random.default_rng(4)
    p, shape, _ = rectangle(50, rng)
    e = ref_extents(p, shape, [])
    assert e["flags"] == EXT_EMPTY and e["n"] == 0 and not e["frame"].any() and np.array_equal(e["origin"], [40.0, 50.0, 60.0])
    for idx in ([7], [7] * 500):
        e = ref_extents(p, shape, idx)
        assert e["flags"] == EXT_NO_DIRECTION and np.array_equal(e["lo"], e["hi"]) and not e["lam"].any()
        assert np.array_equal(e["frame"][0], fallback_u(e["frame"][2])) and np.array_equal(e["centroid"], p[6])
    _, sph, _ = sphere_patch(5, rng)
    e = ref_extents(p, sph, [3, 3])
    assert e["flags"] == EXT_NO_DIRECTION and np.array_equal(e["frame"], np.eye(3))


# --------------------------------------------------------------- header, binding, JSON ----
def test_header_declares_the_entry_points_and_the_binding_has_them():
    hdr = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_shape_extents", "rh_shape_extents_dev", "rh_result_extents"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(R.lib(), name)
    assert "rh_extent;" in hdr and "RH_EXT_EMPTY = 1" in hdr and "RH_EXT_NO_DIRECTION = 2" in hdr
    import ctypes as C
    assert C.sizeof(L.Extent) == 8 + 4 + 4 + 8 * (3 + 9 + 3 + 3 + 3 + 3 + 2) == 224
    assert L.Extent.origin.offset == 16 and L.Extent.frame.offset == 40 and L.Extent.dist_rms.offset == 208


def test_todict_carries_the_extent_only_when_asked():
    rng = np.random.default_rng(5)
    p, shape, _ = rectangle(300, rng)
    es = R.ExtractedShape(R.shape_from_c(shape), _all(300))
    before = json.dumps(R.toDict([es]))
    ref = ref_extents(p, shape, es.inpoints)
    c = L.Extent(n=ref["n"], kind=ref["kind"], flags=ref["flags"], dist_rms=ref["dist_rms"], dist_maxabs=ref["dist_maxabs"])
    for f, key in (("origin", "origin"), ("lo", "lo"), ("hi", "hi"), ("centroid", "centroid"), ("lam", "lam")):
        getattr(c, f)[:] = list(ref[key])
    c.frame[:] = list(ref["frame"].reshape(-1))
    es.extent = R.Extent(c)
    assert np.array_equal(es.extent.frame, ref["frame"]) and np.array_equal(es.extent.size, ref["hi"] - ref["lo"])
    assert json.dumps(R.toDict([es])) == before and "extent" not in R.toDict(es)
    d = R.toDict([es, R.ExtractedShape(es.shape, es.inpoints)], extents=True)["primitives"]
    assert sorted(d[0]["extent"]) == ["centroid", "frame", "hi", "lo", "maxabs", "origin", "rms"]
    assert d[0]["extent"]["hi"] == list(ref["hi"]) and d[0]["extent"]["frame"][2] == list(ref["frame"][2])
    assert "extent" not in d[1] and {k: v for k, v in d[0].items() if k != "extent"} == d[1]
    a, b = _io.StringIO(), _io.StringIO()
    R.exportJSON(a, [es])
    R.exportJSON(b, [es], extents=True)
    assert a.getvalue() == json.dumps(json.loads(before), separators=(",", ":"))
    assert json.loads(b.getvalue())["primitives"][0]["extent"]["rms"] == ref["dist_rms"]
