"""The two-bit books of the score kernel's point loops (csrc/score4_device.h, "Two-bit books") as the HOST runs them -- diag
build, no GPU -- through the very functions of the kernel.

rh_dbg_books2: 64 values u' in, pushed in point order (books2_push: the host form of v_alignbit_b32(w, bits(u'), 30)), then the
kernel's read-outs: the count of surely-in points, the point-ordered surely-in word, the point-ordered undecided word and "any
undecided".  Expected: surely in <=> the sign bit of u' is set (-0 and a NaN with the sign set included); undecided <=> the sign is
clear and u' < 2; everything else -- u' >= 2, +inf, a NaN with a clear sign -- is out.  (No NaN arrives in the kernel: a pair
whose record or tile is not finite ignores its books.  The verdict on one is pinned here all the same.)  The thresholds' special
values at the word borders (positions 0, 15, 16, 31, 32, 47, 48, 63) and 1000 seeded random sequences.

rh_dbg_cls_u2: u by the functions the audits and rh_dbg_cls_round use on cls_make's record, u' by the point loops' path -- that
record doubled in registers (cls_double), the inline 1/2 of the round kinds as 1.  bits(u') == bits(2 u) for every point of the
threshold constructions of test_rootfree_host.py (spheres, cylinders) and of their plane counterpart, with a Float64 and a
Float32 cloud's margins: the decisions are those of u, except that u = 1 exactly is out."""
import ctypes as C
import math

import numpy as np
import pytest

import ransac_jl_amd as R
from ransac_jl_amd import _lib as L

import test_rootfree_host as RH

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
BORDERS = (0, 15, 16, 31, 32, 47, 48, 63)


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


# u = u' / 2 of the issue's list (+-0, +-2^-149, +-2^-126, 0.5, 1 - 2^-24, 1, 1 + 2^-23, 2, +-1e30, +-inf) as u', and the NaNs
SPECIAL_U = [0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126), 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 2.0,
             1e30, -1e30, math.inf, -math.inf]
SPECIAL = [np.float32(2.0) * np.float32(u) for u in SPECIAL_U] + [np.float32(u) for u in SPECIAL_U] + \
          [_f32(0x7fc00000), _f32(0xffc00000), _f32(0x7f800001), _f32(0x3fffffff), _f32(0x40000000), _f32(0x80000001)]


def books(u2):
    u2 = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1, 64)
    n = len(u2)
    cnt, sure, und, anyu = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    L.check(L.lib("diag").rh_dbg_books2(u2.ctypes.data_as(_fp), n, cnt.ctypes.data_as(C.POINTER(C.c_int32)), sure.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        und.ctypes.data_as(C.POINTER(C.c_uint64)), anyu.ctypes.data_as(C.POINTER(C.c_uint8))))
    return cnt, sure, und, anyu


def expected(u2):
    """(count, sure word, undecided word, any) from the bit patterns: the sign bit; sign clear and below bits(2.0f)"""
    b = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1, 64).view(np.uint32)
    s = (b >> 31) != 0
    u = b < 0x40000000
    w = (np.uint64(1) << np.arange(64, dtype=np.uint64))[None, :]
    return s.sum(axis=1).astype(np.int32), (s * w).sum(axis=1, dtype=np.uint64), (u * w).sum(axis=1, dtype=np.uint64), u.any(axis=1).astype(np.uint8)


def _check(u2):
    got, want = books(u2), expected(u2)
    for g, w_, name in zip(got, want, ("sure count", "sure word", "undecided word", "any undecided")):
        bad = np.flatnonzero(g != w_)
        assert bad.size == 0, (name, bad[:4], g[bad[:4]], w_[bad[:4]])


def test_expected_words_say_what_the_docstring_says():
    """the bit-pattern rule of `expected` is the value rule: sure <=> sign set, undecided <=> sign clear and u' < 2"""
    v = np.array([x for x in SPECIAL if not np.isnan(x)], dtype=np.float32)
    b = v.view(np.uint32)
    assert np.array_equal((b >> 31) != 0, np.signbit(v))
    assert np.array_equal(b < 0x40000000, ~np.signbit(v) & (v < 2.0))
    nan_clear, nan_set = _f32(0x7fc00000).view(np.uint32), _f32(0xffc00000).view(np.uint32)
    assert not (nan_clear >> 31) and not nan_clear < 0x40000000          # a NaN with a clear sign: out
    assert nan_set >> 31                                                   # ... with the sign set: "surely in" (none arrives)


def test_special_values_at_the_word_borders():
    rows = []
    for fill in (np.float32(5.0), np.float32(-3.0), np.float32(0.25)):     # among points that are out / in / undecided
        for v in SPECIAL:
            for p in BORDERS:
                r = np.full(64, fill, dtype=np.float32); r[p] = v
                rows.append(r)
    for v in SPECIAL:                                                      # ... and at all eight borders at once, and everywhere
        r = np.full(64, 7.0, dtype=np.float32); r[list(BORDERS)] = v
        rows.append(r)
        rows.append(np.full(64, v, dtype=np.float32))
    rows = np.array(rows)
    _check(rows)
    cnt, sure, und, anyu = books(rows)
    # spelled out for one row of each verdict: u' = 2 (u = 1 exactly) at point 16 among surely-in points is out, not undecided
    r = np.full(64, -1.0, dtype=np.float32); r[16] = 2.0
    c1, s1, u1, a1 = books(r)
    assert c1[0] == 63 and s1[0] == np.uint64(0xFFFFFFFFFFFFFFFF ^ (1 << 16)) and u1[0] == 0 and a1[0] == 0
    r[16] = np.float32(2.0) * np.float32(1.0 - 2.0 ** -24); r[63] = 0.0; r[0] = -0.0
    c1, s1, u1, a1 = books(r)
    assert c1[0] == 62 and u1[0] == np.uint64((1 << 16) | (1 << 63)) and a1[0] == 1 and (int(s1[0]) & 1) == 1


def test_random_sequences():
    rng = np.random.default_rng(2024)
    # a third each: values about the thresholds, random bit patterns (NaNs, infinities and subnormals among them), picks of the special values
    a = (rng.normal(size=(334, 64)) * 2.0).astype(np.float32)
    b = rng.integers(0, 2 ** 32, size=(333, 64), dtype=np.uint64).astype(np.uint32).view(np.float32)
    c = np.array(SPECIAL, dtype=np.float32)[rng.integers(0, len(SPECIAL), size=(333, 64))]
    seqs = np.vstack([a, b, c])
    assert seqs.shape == (1000, 64)
    _check(seqs)
    cnt, sure, und, anyu = books(seqs)
    assert (cnt > 0).any() and (und != 0).any() and (sure & und == 0).all()


def _u_and_u2(shape, cp, M, Nm, xyz, nrm, f32):
    n = len(xyz)
    xyz, nrm = np.ascontiguousarray(xyz, dtype=np.float64), np.ascontiguousarray(nrm, dtype=np.float64)
    u, u2, rec = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(16, dtype=np.float32)
    L.check(L.lib("diag").rh_dbg_cls_u2(C.byref(shape), C.byref(cp), float(M), float(Nm), int(f32), n, xyz.ctypes.data_as(_dp), nrm.ctypes.data_as(_dp),
                                        u.ctypes.data_as(_fp), u2.ctypes.data_as(_fp), rec.ctypes.data_as(_fp)))
    return u, u2, rec


def _plane_points(v, eps, alpha, n_random, rng):
    """the plane's counterpart of test_rootfree_host._points: d = +-eps (1 +- k 2^-24) with the plane's normal, on the plane with the
    normal at alpha (1 +- k 2^-23) from it, the zero point, random points"""
    p0, n = np.array(v[:3]), np.array(v[3:6])
    n = n / np.linalg.norm(n)
    t = RH._perp(n)
    k = np.arange(65)
    P, Nn = [], []
    for _ in range(3):
        base = p0 + rng.uniform(-30, 30) * t + rng.uniform(-30, 30) * np.cross(n, t)
        for edge in (-eps, eps):
            for sg in (-1.0, 1.0):
                d = edge * (1.0 + sg * k * 2.0 ** -24)
                P.append(base + d[:, None] * n); Nn.append(np.tile(n, (65, 1)))
        for sg in (-1.0, 1.0):
            th = alpha * (1.0 + sg * k * 2.0 ** -23)
            P.append(np.tile(base, (65, 1))); Nn.append(np.cos(th)[:, None] * n + np.sin(th)[:, None] * t)
    P.append(np.zeros((1, 3))); Nn.append(np.zeros((1, 3)))
    P.append(p0 + rng.uniform(-50, 50, (n_random, 3)))
    nn = rng.normal(size=(n_random, 3))
    Nn.append(nn / np.linalg.norm(nn, axis=1)[:, None])
    return np.vstack(P), np.vstack(Nn)


def _plane_candidates():
    for off in RH.OFFSETS:
        for d in ((0.0, 0.0, 1.0), (0.36, 0.48, 0.8), (-0.6, 0.0, 0.8)):
            yield 1, [off, off * 0.75, -off * 0.5] + list(d), True


def _params(eps, alpha_deg):
    params = R.ransacparameters([R.FittedPlane, R.FittedSphere, R.FittedCylinder])
    for k in ("plane", "sphere", "cylinder"):
        params[k]["ϵ"] = float(eps)
        params[k]["α"] = math.radians(alpha_deg)
    return R.params_to_c(params)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("eps,alpha_deg", RH.SETTINGS)
@pytest.mark.parametrize("kind", [L.PLANE, L.SPHERE, L.CYLINDER], ids=["plane", "sphere", "cylinder"])
def test_doubled_record_gives_exactly_twice_u(kind, eps, alpha_deg, f32):
    cp = _params(eps, alpha_deg)
    eps_c = cp.eps[kind]
    rng = np.random.default_rng(77 + kind)
    usable = points = undecided = 0
    for outwards, v, _plain in (_plane_candidates() if kind == L.PLANE else RH._candidates(kind)):
        sgn = 1.0 if outwards else -1.0
        if kind == L.PLANE:
            xyz, nrm = _plane_points(v, eps_c, math.radians(alpha_deg), 2000, rng)
        else:
            xyz, nrm, _iz, _nb = RH._points(kind, v, sgn, eps_c, math.radians(alpha_deg), 2000, rng)
        if f32:                               # a Float32 cloud holds binary32 points (and takes the tripled margins)
            xyz, nrm = xyz.astype(np.float32).astype(np.float64), nrm.astype(np.float32).astype(np.float64)
        M, Nm = np.abs(xyz).max(), np.abs(nrm).max()
        shape = RH._shape(kind, outwards, v)
        if kind == L.PLANE:
            L.lib("diag").rh_shape_finalize(C.byref(shape))
        u, u2, rec = _u_and_u2(shape, cp, M, Nm, xyz, nrm, f32)
        if np.isnan(rec[15]):
            continue
        usable += 1
        assert not np.isnan(u).any() and not np.isnan(u2).any()
        twice = np.float32(2.0) * u
        bad = np.flatnonzero(twice.view(np.uint32) != u2.view(np.uint32))
        assert bad.size == 0, (kind, v, f32, bad[:5], u[bad[:5]], u2[bad[:5]])
        # the decisions are those of u; u = 1 exactly, undecided by u <= 1, is out
        b2 = u2.view(np.uint32)
        assert np.array_equal((b2 >> 31) != 0, np.signbit(u))
        assert np.array_equal(b2 < 0x40000000, ~np.signbit(u) & (u < 1.0))
        points += len(u)
        undecided += int((b2 < 0x40000000).sum())
    assert usable >= 3 and points > 5000 and undecided > 0, (usable, points, undecided)
