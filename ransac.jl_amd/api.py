"""Host-side mirror of the reference's API for the hot path -- same names, argument meaning
and error behaviour as cserteGT3/RANSAC.jl v0.6.0 (paths in comments are under
/root/reference/src), with every data-parallel step routed through the C ABI of
libransac_hip.so.  Nothing here computes a score or an inlier set on the CPU."""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import CONE, CYLINDER, PLANE, SPHERE, check, lib


# ----------------------------------------------------------------- options ----
def _opt_value(key, value):
    if value is None:
        return L.OPTION_UNSET
    if isinstance(value, str):
        table = {"score_path": L.SCORE_PATH, "refit_path": L.REFIT_PATH}.get(key)
        if table is None or value not in table:
            raise ValueError("option %r has no value %r" % (key, value))
        return table[value]
    return int(value)


def set_option(key, value, cloud=None):
    """rh_set_option (include/ransac_hip.h): a tuning option for one cloud or, with cloud=None, process-wide.  value: an
    int, one of the names of score_path ("auto" / "brute" / "groups") and refit_path ("auto" / "scan" / "culled"), or None
    to clear the setting.  The library itself reads no environment variable."""
    check(lib().rh_set_option(None if cloud is None else cloud._h, key.encode(), _opt_value(key, value)))


def get_option(key, cloud=None):
    """the option's value as the library sees it for this cloud, or None when nobody has set it"""
    v, st = C.c_int64(), C.c_int32()
    check(lib().rh_get_option(None if cloud is None else cloud._h, key.encode(), C.byref(v), C.byref(st)))
    return v.value if st.value else None


class option:
    """with option("refit_path", "scan"): ...   -- set, then put back what was there"""

    def __init__(self, key, value, cloud=None):
        self.key, self.value, self.cloud = key, value, cloud

    def __enter__(self):
        # what the cloud / the process itself holds (not what a cloud inherits): cleared again on exit when it held nothing
        self.old = get_option(self.key, self.cloud) if self.cloud is None else None
        set_option(self.key, self.value, self.cloud)
        return self

    def __exit__(self, *exc):
        set_option(self.key, self.old, self.cloud)
        return False


# ------------------------------------------------------------------ shapes ----
class FittedShape:
    """abstract supertype of all fitted shapes (fitting.jl:6)"""
    kind = None

    def to_c(self):
        raise NotImplementedError


def _vec(a):
    a = np.asarray(a, dtype=np.float64).reshape(3)
    return a


class FittedPlane(FittedShape):  # shapes/plane.jl:8-11
    kind = PLANE

    def __init__(self, point, normal):
        self.point, self.normal = _vec(point), _vec(normal)

    def to_c(self):
        return _mk(PLANE, False, list(self.point) + list(self.normal))

    def __repr__(self):
        return "FittedPlane(normal: %s, point: %s)" % (self.normal, self.point)


class FittedSphere(FittedShape):  # shapes/sphere.jl:9-13
    kind = SPHERE

    def __init__(self, center, radius, outwards):
        self.center, self.radius, self.outwards = _vec(center), float(radius), bool(outwards)

    def to_c(self):
        return _mk(SPHERE, self.outwards, list(self.center) + [self.radius])

    def __repr__(self):
        return "FittedSphere(center: %s, R: %s, %s)" % (self.center, self.radius, "outwards" if self.outwards else "inwards")


class FittedCylinder(FittedShape):  # shapes/cylinder.jl:11-16
    kind = CYLINDER

    def __init__(self, axis, center, radius, outwards):
        self.axis, self.center, self.radius, self.outwards = _vec(axis), _vec(center), float(radius), bool(outwards)

    def to_c(self):
        return _mk(CYLINDER, self.outwards, list(self.axis) + list(self.center) + [self.radius])

    def __repr__(self):
        return "FittedCylinder(center: %s, axis: %s, R: %s, %s)" % (
            self.center, self.axis, self.radius, "outwards" if self.outwards else "inwards")


class FittedCone(FittedShape):  # shapes/cone.jl:11-19
    kind = CONE

    def __init__(self, apex, axis, opang, outwards):
        self.apex, self.axis, self.opang, self.outwards = _vec(apex), _vec(axis), float(opang), bool(outwards)

    def to_c(self):
        return _mk(CONE, self.outwards, list(self.apex) + list(self.axis) + [self.opang])

    def __repr__(self):
        return "FittedCone(apex: %s, axis: %s, w: %s, %s)" % (
            self.apex, self.axis, self.opang, "outwards" if self.outwards else "inwards")


def _mk(kind, outwards, v):
    s = L.Shape()
    s.kind = kind
    s.outwards = int(bool(outwards))
    for i, x in enumerate(v):
        s.v[i] = float(x)
    lib().rh_shape_finalize(C.byref(s))
    return s


def shape_from_c(s):
    v = list(s.v)
    if s.kind == PLANE:
        return FittedPlane(v[0:3], v[3:6])
    if s.kind == SPHERE:
        return FittedSphere(v[0:3], v[3], bool(s.outwards))
    if s.kind == CYLINDER:
        return FittedCylinder(v[0:3], v[3:6], v[6], bool(s.outwards))
    if s.kind == CONE:
        return FittedCone(v[0:3], v[3:6], v[6], bool(s.outwards))
    raise ValueError("unknown kind %d" % s.kind)


def strt(x):  # fitting.jl:66; shapes/*.jl `strt`
    return L.KIND_NAMES[x.kind]


DEFAULT_SHAPE_DICT = {"plane": FittedPlane, "cone": FittedCone, "cylinder": FittedCylinder, "sphere": FittedSphere}
_KIND_OF = {FittedPlane: PLANE, FittedSphere: SPHERE, FittedCylinder: CYLINDER, FittedCone: CONE}


class ExtractedShape:  # fitting.jl:81-84
    def __init__(self, shape, inpoints):
        self.shape = shape
        self.inpoints = np.asarray(inpoints, dtype=np.int64)

    def __repr__(self):
        return "Cand: (%s), %d ps" % (strt(self.shape), len(self.inpoints))


class ConfidenceInterval:  # confidenceintervals.jl:1-6
    def __init__(self, x, y):
        if x > y:
            raise ValueError("out of order")
        self.min, self.max, self.E = float(x), float(y), (float(x) + float(y)) / 2

    def __repr__(self):
        return "CI: [%s, %s]" % (self.min, self.max)


def E(x):  # confidenceintervals.jl:43
    return x.E


def notsoconfident(x, y):  # confidenceintervals.jl:20-22
    return ConfidenceInterval(min(x, y), max(x, y))


def estimatescore(S1length, Plength, sigma, score_mode=L.SCORE_INT64_WRAP):  # confidenceintervals.jl:71-74
    lo, hi, e = C.c_double(), C.c_double(), C.c_double()
    check(lib().rh_estimatescore(int(S1length), int(Plength), int(sigma), score_mode,
                                 C.byref(lo), C.byref(hi), C.byref(e)))
    ci = ConfidenceInterval.__new__(ConfidenceInterval)
    ci.min, ci.max, ci.E = lo.value, hi.value, e.value
    return ci


def prob(n, s, N, k):  # utilities.jl:262
    return lib().rh_prob(float(n), int(s), int(N), int(k))


# -------------------------------------------------------------- parameters ----
def defaultshapeparameters(T):  # shapes/*.jl defaultshapeparameters
    a = math.radians(5)
    if T is FittedPlane:
        return {"plane": {"ϵ": 0.3, "α": a}}
    if T is FittedSphere:
        return {"sphere": {"ϵ": 0.3, "α": a, "sphere_par": 0.02}}
    if T is FittedCylinder:
        return {"cylinder": {"ϵ": 0.3, "α": a}}
    if T is FittedCone:
        return {"cone": {"ϵ": 0.3, "α": a, "minconeopang": math.radians(2)}}
    raise TypeError(T)


def defaultiterationparameters(shape_types):  # utilities.jl:332-347
    return {"iteration": {"drawN": 3, "minsubsetN": 15, "prob_det": 0.9, "shape_types": list(shape_types),
                          "τ": 900, "itermax": 1000, "extract_s": "nofminset", "terminate_s": "nofminset"}}


def defaultcommonparameters():  # utilities.jl:368-373
    return {"common": {"collin_threshold": 0.2, "parallelthrdeg": 1.0}}


def defaultparameters(shape_types):  # utilities.jl:391-399
    p = defaultiterationparameters(shape_types)
    p.update(defaultcommonparameters())
    for T in shape_types:
        p.update(defaultshapeparameters(T))
    return p


DEFAULT_PARAMETERS = defaultparameters([FittedPlane, FittedCone, FittedCylinder, FittedSphere])  # RANSAC.jl:94

_ALIASES = {"eps": "ϵ", "epsilon": "ϵ", "alpha": "α", "tau": "τ"}


def _norm_keys(d):
    return {_ALIASES.get(k, k): v for k, v in d.items()}


def ransacparameters(p=None, **kwargs):  # utilities.jl:425-464
    """ransacparameters(; kw...), ransacparameters(p; kw...) or ransacparameters([types]; kw...).
    Nested dicts stand in for NamedTuples; `eps`/`alpha`/`tau` are accepted for ϵ/α/τ."""
    if p is None:
        base = DEFAULT_PARAMETERS
    elif isinstance(p, (list, tuple)):
        base = defaultparameters(list(p))
    else:
        base = p
    newp = {k: dict(v) for k, v in base.items()}
    for a, val in kwargs.items():
        old = newp.get(a, {})
        merged = dict(old)
        merged.update(_norm_keys(val))
        newp[a] = merged
    return newp


_S = {"lengthC": L.S_LENGTHC, "allcand": L.S_ALLCAND, "nofminset": L.S_NOFMINSET}


def params_to_c(params, score_mode=L.SCORE_INT64_WRAP, sphere_uses_enabled=False, sampling_streams=0,
                octree_sampling=False, octree_max_depth=10):
    """Flatten the nested parameter dict into rh_params.  Shapes absent from the dict keep the
    library defaults (they are never used: `shape_types` selects what is fitted)."""
    c = L.Params()
    lib().rh_default_params(C.byref(c))
    for name, kind in (("plane", PLANE), ("sphere", SPHERE), ("cylinder", CYLINDER), ("cone", CONE)):
        if name in params:
            sp = _norm_keys(params[name])
            c.eps[kind] = sp.get("ϵ", c.eps[kind])
            c.alpha[kind] = sp.get("α", c.alpha[kind])
    if "sphere" in params:
        c.sphere_par = _norm_keys(params["sphere"]).get("sphere_par", c.sphere_par)
    if "cone" in params:
        c.minconeopang = _norm_keys(params["cone"]).get("minconeopang", c.minconeopang)
    if "common" in params:
        c.collin_threshold = params["common"].get("collin_threshold", c.collin_threshold)
        c.parallelthrdeg = params["common"].get("parallelthrdeg", c.parallelthrdeg)
    if "iteration" in params:
        it = _norm_keys(params["iteration"])
        c.drawN = it.get("drawN", c.drawN)
        c.minsubsetN = it.get("minsubsetN", c.minsubsetN)
        c.prob_det = it.get("prob_det", c.prob_det)
        c.tau = int(it.get("τ", c.tau))
        c.itermax = int(it.get("itermax", c.itermax))
        c.extract_s = _S[str(it.get("extract_s", "nofminset")).lstrip(":")]
        c.terminate_s = _S[str(it.get("terminate_s", "nofminset")).lstrip(":")]
        if "shape_types" in it:
            st = it["shape_types"]
            c.n_shape_types = len(st)
            for i, T in enumerate(st):
                c.shape_types[i] = _KIND_OF[T] if T in _KIND_OF else int(T)
    c.score_mode = score_mode
    c.sphere_uses_enabled = int(bool(sphere_uses_enabled))
    c.sampling_streams = int(sampling_streams)
    c.octree_sampling = int(bool(octree_sampling))
    c.octree_max_depth = int(octree_max_depth)
    lib().rh_params_finalize(C.byref(c))
    return c


def _cparams(params):
    return params if isinstance(params, L.Params) else params_to_c(params)


# ------------------------------------------------------------------ octree ----
class OctreeCell:
    """A cell of the reference's octree (RegionTrees.Cell with OctreeNode data: octree.jl:147-150): `.data.incellpoints`
    (1-based indices, a numpy array), `.data.depth` (root = 1), `.boundary` = (origin, widths), `.children`, `.parent`."""

    class _Data:
        def __init__(self, cell):
            self._c = cell

        @property
        def depth(self):
            return self._c._info()[2]

        @property
        def incellpoints(self):
            n = self._c._info()[5]
            out = np.zeros(max(1, n), dtype=np.int64)
            check(lib().rh_octree_node_points(self._c._t._h, self._c.index, _p(out, C.c_int64), n))
            return out[:n]

    def __init__(self, tree, index):
        self._t, self.index = tree, int(index)
        self.data = OctreeCell._Data(self)

    def _info(self):
        o, w = np.zeros(3), np.zeros(3)
        d, par, npts = C.c_int32(), C.c_int32(), C.c_int64()
        ch = (C.c_int32 * 8)()
        check(lib().rh_octree_node_info(self._t._h, self.index, _p(o, C.c_double), _p(w, C.c_double), C.byref(d), C.byref(par), ch, C.byref(npts)))
        return o, w, d.value, par.value, list(ch), npts.value

    @property
    def boundary(self):
        o, w = self._info()[:2]
        return o, w

    @property
    def parent(self):
        par = self._info()[3]
        return None if par < 0 else OctreeCell(self._t, par)

    @property
    def children(self):
        ch = self._info()[4]
        return None if ch[0] < 0 else [OctreeCell(self._t, k) for k in ch]

    def isleaf(self):
        return self._info()[4][0] < 0

    def __eq__(self, other):
        return isinstance(other, OctreeCell) and other._t is self._t and other.index == self.index

    def __hash__(self):
        return hash((id(self._t), self.index))

    def __repr__(self):
        i = self._info()
        return "OctreeNode: %d ps, %d d" % (i[5], i[2])


class _Octree:
    def __init__(self, vertices):
        self._h = C.c_void_p()
        v = np.asarray(vertices)
        if v.dtype == np.float32:   # a Float32 cloud's tree: the geometry in binary32, as the reference computes it there
            self.vertices = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
            check(lib().rh_octree_build_f32(_p(self.vertices, C.c_float), self.vertices.shape[0], C.byref(self._h)))
            return
        self.vertices = _f64(vertices).reshape(-1, 3)
        check(lib().rh_octree_build(_p(self.vertices, C.c_double), self.vertices.shape[0], C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().rh_octree_destroy(h)
            except (AttributeError, TypeError):
                pass
            self._h = None


def buildoctree(vertices):
    """buildoctree(vertices) -> the root Cell (octree.jl:237-244).  float32 vertices: the binary32 tree (rh_octree_build_f32)."""
    return OctreeCell(_Octree(vertices), 0)


def octreedepth(pc_or_cell):
    """octreedepth(pc) / octreedepth(cell) (octree.jl:212-230): the depth of the deepest leaf."""
    cell = pc_or_cell.octree if hasattr(pc_or_cell, "octree") else pc_or_cell
    d = C.c_int32()
    check(lib().rh_octree_info(cell._t._h, None, C.byref(d), None))
    return d.value


def findleaf(cell, p):
    """findleaf(pc.octree, p) (RegionTrees; fitting.jl:397)."""
    q = _f64(p).reshape(3)
    out = C.c_int32()
    check(lib().rh_octree_findleaf(cell._t._h, _p(q, C.c_double), C.byref(out)))
    return OctreeCell(cell._t, out.value)


def getnthcell(c, n):
    """getnthcell(c, n) (octree.jl:11-22): the ancestor of c (or c) at depth n, None if there is none."""
    out = C.c_int32()
    check(lib().rh_octree_getnthcell(c._t._h, c.index, int(n), C.byref(out)))
    return None if out.value < 0 else OctreeCell(c._t, out.value)


def iswithinrectangle(rect, p):
    """iswithinrectangle(rect, p) (octree.jl:187-196); rect = (origin, widths): vmin < p <= vmax on every axis."""
    o, w = (np.asarray(rect[0], dtype=np.float64), np.asarray(rect[1], dtype=np.float64))
    q = np.asarray(p, dtype=np.float64)
    return bool(np.all(o < q) and np.all(o + w >= q))


def cell_enabled_points(pc, cell):
    """cell.data.incellpoints[pc.isenabled[cell.data.incellpoints]] (fitting.jl:405-407), gathered on the device."""
    cap = cell._info()[5]
    out = np.zeros(max(1, cap), dtype=np.int64)
    n = C.c_int64()
    check(lib().rh_octree_cell_enabled(pc._h, cell._t._h, cell.index, _p(out, C.c_int64), cap, C.byref(n)))
    return out[: n.value]


# ------------------------------------------------------------------- cloud ----
def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class RANSACCloud:
    """RANSACCloud(vertices, normals, numofsubsets | subsets) (octree.jl:37-138).  The points,
    normals, subset 1 and the enabled bits live in HBM on `device`; the host keeps the arrays
    it was given (for the O(1) minimal-set fits) and the subset index lists."""

    def __init__(self, vertices, normals, subsets, device=0, seed=None, force_eltype=None):
        """force_eltype = numpy.float32: a Float32 cloud (octree.jl:102-109) -- scoring and refit then compute in
        binary32 like the reference does on such a cloud, and so does ransac() (fits included, all four kinds); refit_lsq stays Float64-only."""
        self.is_f32 = force_eltype is not None and np.dtype(force_eltype) == np.float32
        if force_eltype is not None and not self.is_f32 and np.dtype(force_eltype) != np.float64:
            raise ValueError("force_eltype must be float32 or float64")
        if self.is_f32:
            self.vertices32 = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
            self.normals32 = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            vertices, normals = self.vertices32.astype(np.float64), self.normals32.astype(np.float64)
        self.vertices = _f64(vertices).reshape(-1, 3)
        self.normals = _f64(normals).reshape(-1, 3)
        assert self.vertices.shape == self.normals.shape, "Every point must have a normal."
        self.size = self.vertices.shape[0]
        if isinstance(subsets, (int, np.integer)):
            assert subsets > 0, "At least 1 subset please!"
            rng = np.random.default_rng(seed)
            alls = rng.permutation(self.size).astype(np.int64) + 1   # randperm(l): octree.jl:131
            ssl = self.size // int(subsets)
            subs = [alls[i * ssl:(i + 1) * ssl] for i in range(int(subsets) - 1)]
            subs.append(alls[(int(subsets) - 1) * ssl:])
            subsets = subs
        self.subsets = [np.ascontiguousarray(s, dtype=np.int64) for s in subsets]
        self.device = device
        h = C.c_void_p()
        s1 = self.subsets[0]
        if self.is_f32:
            check(lib().rh_cloud_create_f32(_p(self.vertices32, C.c_float), _p(self.normals32, C.c_float), self.size,
                                            _p(s1, C.c_int64), s1.size, device, C.byref(h)))
        else:
            check(lib().rh_cloud_create(_p(self.vertices, C.c_double), _p(self.normals, C.c_double), self.size,
                                        _p(s1, C.c_int64), s1.size, device, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().rh_cloud_destroy(h)
            except (AttributeError, TypeError):
                pass   # interpreter shutdown: the module globals are gone, the process frees the device memory
            self._h = None

    @property
    def nchunks(self):
        return (self.size + 63) // 64

    @property
    def octree(self):
        """pc.octree (octree.jl:47, built by the constructor there; here on first use: rh_ransac never reads it)"""
        if getattr(self, "_octree", None) is None:
            self._octree = buildoctree(self.vertices32 if self.is_f32 else self.vertices)   # (a Float32 cloud: the binary32 tree)
        return self._octree

    @property
    def isenabled(self):
        """pc.isenabled as a bool array (a copy; write it back with set_enabled)."""
        ch = np.zeros(max(1, self.nchunks), dtype=np.uint64)
        check(lib().rh_cloud_get_enabled(self._h, _p(ch, C.c_uint64), self.nchunks))
        bits = np.unpackbits(ch[: self.nchunks].view(np.uint8), bitorder="little")
        return bits[: self.size].astype(bool)

    def enabled_chunks(self):
        ch = np.zeros(max(1, self.nchunks), dtype=np.uint64)
        check(lib().rh_cloud_get_enabled(self._h, _p(ch, C.c_uint64), self.nchunks))
        return ch[: self.nchunks]

    def set_enabled(self, mask_or_chunks):
        a = np.asarray(mask_or_chunks)
        if a.dtype == np.uint64:
            ch = np.ascontiguousarray(a).reshape(-1)
            if ch.size != self.nchunks:
                raise ValueError("set_enabled: %d chunks given, the cloud has %d (ceil(size / 64))" % (ch.size, self.nchunks))
        else:
            if a.size != self.size:
                raise ValueError("set_enabled: mask of length %d for a cloud of %d points" % (a.size, self.size))
            bits = np.zeros(self.nchunks * 64, dtype=np.uint8)
            bits[: self.size] = a.reshape(-1).astype(np.uint8)
            ch = np.packbits(bits, bitorder="little").view(np.uint64)
        n_given = ch.size   # the library checks this against its own word count
        ch = np.ascontiguousarray(ch if ch.size else np.zeros(1, dtype=np.uint64))
        check(lib().rh_cloud_set_enabled(self._h, _p(ch, C.c_uint64), n_given))

    def enable_all(self):
        check(lib().rh_cloud_enable_all(self._h))

    def set_stream(self, hip_stream):
        """Enqueue this cloud's work on the caller's HIP stream (an int handle, e.g.
        torch.cuda.current_stream().cuda_stream; None = back to the cloud's own stream)."""
        check(lib().rh_cloud_set_stream(self._h, C.c_void_p(hip_stream or 0), 0 if hip_stream is None else 1))

    def count_enabled(self):
        out = C.c_int64()
        check(lib().rh_cloud_count_enabled(self._h, C.byref(out)))
        return out.value

    def set_component_filter(self, beta, conn26=True):
        """With beta > 0 every extraction of ransac() on this cloud takes only the largest connected component of the best
        candidate's refit set (voxel grid of size beta; refit_component); beta <= 0 or None: off, the default."""
        check(lib().rh_cloud_set_component_filter(self._h, float(beta or 0.0), 1 if conn26 else 0))

    @property
    def component_filter(self):
        """(beta, conn26) of set_component_filter; beta = 0.0: off"""
        beta, conn = C.c_double(), C.c_int32()
        check(lib().rh_cloud_get_component_filter(self._h, C.byref(beta), C.byref(conn)))
        return beta.value, bool(conn.value)

    def __repr__(self):
        return "RANSACCloud of size %d & %d subsets" % (self.size, len(self.subsets))


# ---------------------------------------------------------------- hot path ----
def fit(T, p, n, pc, params):
    """fit(::Type{T}, p, n, pc, params) -> T or None (shapes/*.jl `fit`).  Float32 points (a Float32 cloud's, or numpy
    float32 arrays) are fitted in Float32 like Julia fits SVector{3,Float32}s (rh_fit_f32)."""
    f32 = bool(getattr(pc, "is_f32", False)) or (getattr(p, "dtype", None) == np.float32 and getattr(n, "dtype", None) == np.float32)
    if f32:
        p, n = np.asarray(p, dtype=np.float32), np.asarray(n, dtype=np.float32)
    p, n = _f64(p).reshape(-1, 3), _f64(n).reshape(-1, 3)
    assert p.shape[0] > 2, "At least 3 point is needed."
    assert p.shape == n.shape, "Size must be the same."
    out, ok = L.Shape(), C.c_int32()
    kind = _KIND_OF[T] if T in _KIND_OF else int(T)
    check((lib().rh_fit_f32 if f32 else lib().rh_fit)(kind, _p(p, C.c_double), _p(n, C.c_double), p.shape[0], C.byref(_cparams(params)),
                                                     C.byref(out), C.byref(ok)))
    return shape_from_c(out) if ok.value else None


def _shape_array(cands, f32=False):
    arr = (L.Shape * max(1, len(cands)))()
    for i, s in enumerate(cands):
        arr[i] = s if isinstance(s, L.Shape) else s.to_c()
        if f32:
            lib().rh_shape_finalize_f32(C.byref(arr[i]))
    return arr


def shape_f32(s):
    """The Float32 form of a shape (what `fit` returns on a Float32 cloud): fields rounded to binary32, a cone's
    cos / sin of -opang/2 as binary32 (rh_shape_finalize_f32).  Returns the C record."""
    cs = L.Shape.from_buffer_copy(bytes(s if isinstance(s, L.Shape) else s.to_c()))
    lib().rh_shape_finalize_f32(C.byref(cs))
    return cs


def score_batch(pc, candidates, params, want_masks=False):
    """One launch for the whole batch, all shape kinds (replaces the loop of scorecandidates!,
    fitting.jl:181-190).  Returns counts[b] (and masks[b, ceil(S/64)] over subset positions)."""
    b = len(candidates)
    arr = candidates if isinstance(candidates, C.Array) else _shape_array(candidates, getattr(pc, "is_f32", False))
    counts = np.zeros(max(1, b), dtype=np.int32)
    w = (pc.subsets[0].size + 63) // 64
    masks = np.zeros((max(1, b), max(1, w)), dtype=np.uint64) if want_masks else None
    check(lib().rh_score_batch(pc._h, arr, b, C.byref(_cparams(params)), _p(counts, C.c_int32),
                               _p(masks, C.c_uint64) if want_masks else None))
    if want_masks:
        if w == 0:
            return counts[:b], masks[:b, :0]
        flat = masks.reshape(-1)[: b * w].reshape(b, w) if masks.shape[1] != w else masks[:b]
        return counts[:b], flat
    return counts[:b]


def scorecandidate(pc, candidate, subsetID, params):
    """scorecandidate(pc, candidate, subsetID, params) -> (ConfidenceInterval, inpoints)
    (shapes/plane.jl:61-71 ...).  Only subset 1 lives on the device, as only subset 1 is ever
    scored by the reference (iterations.jl:95)."""
    if subsetID != 1:
        raise ValueError("only subsetID == 1 is resident on the device (iterations.jl:95)")
    cp = _cparams(params)
    counts, masks = score_batch(pc, [candidate], cp, want_masks=True)
    s1 = pc.subsets[0]
    bits = np.unpackbits(masks[0].view(np.uint8), bitorder="little")[: s1.size].astype(bool)
    inpoints = s1[bits]
    assert inpoints.size == counts[0]
    return estimatescore(s1.size, pc.size, int(counts[0]), cp.score_mode), inpoints


def push2candidatesandlevels(candidates, candidate, levels, current_level):  # utilities.jl:473-481
    """Push `candidate` (one shape or a list of shapes) and its octree level."""
    if isinstance(candidate, (list, tuple)):
        candidates.extend(candidate)
        levels.extend([current_level] * len(candidate))
    else:
        candidates.append(candidate)
        levels.append(current_level)


def forcefitshapes(points, normals, parameters, candidates, level_array, octree_lev, pc):  # forcefitshapes!: fitting.jl:165-173
    """Call `fit` for every type of iteration.shape_types, in that order, and append what fits."""
    for T in parameters["iteration"]["shape_types"]:
        fitted = fit(T, points, normals, pc, parameters)
        if fitted is not None:
            push2candidatesandlevels(candidates, fitted, level_array, octree_lev)


def findAABB(points):  # utilities.jl:125-136
    """(min, max) corners of the axis-aligned box of the points (host helper; the device builds its own boxes)."""
    a = _f64(points)
    return a.min(axis=0), a.max(axis=0)


def smallestdistance(points):  # utilities.jl:187-199 (exported, unused by ransac(): iterations.jl:57 is a comment)
    a = _f64(points)
    assert a.shape[0] > 1, "At least two point is needed for that."
    d = np.linalg.norm(a[:, None, :] - a[None, :, :], axis=2)
    return float(d[~np.eye(a.shape[0], dtype=bool)].min())


def setfloattype(nt, T):  # utilities.jl:488-504
    """Convert every real-but-not-integer value of a nested parameter dict to numpy type T."""
    out = {}
    for k, v in nt.items():
        if isinstance(v, dict):
            out[k] = setfloattype(v, T)
        elif isinstance(v, (float, np.floating)) and not isinstance(v, bool):
            out[k] = T(v)
        else:
            out[k] = v
    return out


class IterationCandidates:  # fitting.jl:94-131
    """Struct of arrays of the scored candidates: shapes, scores (ConfidenceInterval), inpoints."""

    def __init__(self):
        self.shapes, self.scores, self.inpoints = [], [], []

    def __len__(self):
        return len(self.shapes)

    def __repr__(self):
        return "IterationCandidates: %d candidates" % len(self)


def recordscore(ic, shape, score, inpoints):  # recordscore!: fitting.jl:114-119
    ic.shapes.append(shape)
    ic.scores.append(score)
    ic.inpoints.append(inpoints)
    return ic


def deleteat(ic, arg):  # deleteat!(ic, arg): fitting.jl:126-131 (1-based index or ascending list of them)
    idx = [arg] if isinstance(arg, (int, np.integer)) else list(arg)
    for i in sorted(idx, reverse=True):
        for a in (ic.shapes, ic.scores, ic.inpoints):
            del a[i - 1]
    return ic


def findhighestscore(A):  # fitting.jl:140-158: first maximum of E (strict >), overlap flag
    if len(A) == 0:
        return {"index": 0, "overlap": False}
    ind, highest = 1, E(A.scores[0])
    for i, sc in enumerate(A.scores, start=1):
        if E(sc) > highest:
            highest, ind = E(sc), i
    best = A.scores[ind - 1]
    for i, sc in enumerate(A.scores, start=1):
        if i != ind and (sc.min <= best.max and best.min <= sc.max):   # isoverlap: confidenceintervals.jl:29-36
            return {"index": ind, "overlap": True}
    return {"index": ind, "overlap": False}


def scorecandidates(pc, iterationcandidates, candidates, subsetID, params, octree_levels=None):
    """scorecandidates! (fitting.jl:181-190) with the sequential loop replaced by ONE batched launch; the
    results are recorded in candidate order and the two input lists are emptied like the reference does.
    (`levelscore` is not kept: it never influences a result)"""
    if subsetID != 1:
        raise ValueError("only subsetID == 1 is resident on the device (iterations.jl:95)")
    if candidates:
        cp = _cparams(params)
        counts, masks = score_batch(pc, candidates, cp, want_masks=True)
        s1 = pc.subsets[0]
        for cand, cnt, m in zip(candidates, counts, masks):
            bits = np.unpackbits(m.view(np.uint8), bitorder="little")[: s1.size].astype(bool)
            recordscore(iterationcandidates, cand, estimatescore(s1.size, pc.size, int(cnt), cp.score_mode), s1[bits])
    del candidates[:]
    if octree_levels is not None:
        del octree_levels[:]


def removeinvalidshapes(pc, candidates):  # removeinvalidshapes!: fitting.jl:209-221
    en = pc.isenabled
    toremove = [i for i, ip in enumerate(candidates.inpoints, start=1) if ip.size and not en[ip - 1].all()]
    deleteat(candidates, toremove)


def refit(s, pc, params):
    """refit(s, pc, params) -> ExtractedShape (shapes/plane.jl:137-143 ...)."""
    out = np.zeros(max(1, pc.size), dtype=np.int64)
    n = C.c_int64()
    cs = s if isinstance(s, L.Shape) else (shape_f32(s) if getattr(pc, "is_f32", False) else s.to_c())
    check(lib().rh_refit(pc._h, C.byref(cs), C.byref(_cparams(params)), _p(out, C.c_int64), pc.size, C.byref(n)))
    return ExtractedShape(s if not isinstance(s, L.Shape) else shape_from_c(s), out[: n.value].copy())


def refit_component(s, pc, params, beta, conn26=True, return_stats=False):
    """The largest connected patch of refit(s, pc, params): connectivity on a voxel grid of size beta over the inliers,
    26-neighbourhood (conn26) or faces only, size counted in points, ties to the component with the smallest point index
    (include/ransac_hip.h has the definition in full).  -> ExtractedShape; with return_stats also
    {"n_refit": the whole refit set's size, "n_components": ...}."""
    out = np.zeros(max(1, pc.size), dtype=np.int64)
    n, n_refit, n_comp = C.c_int64(), C.c_int64(), C.c_int32()
    cs = s if isinstance(s, L.Shape) else (shape_f32(s) if getattr(pc, "is_f32", False) else s.to_c())
    check(lib().rh_refit_component(pc._h, C.byref(cs), C.byref(_cparams(params)), float(beta), 1 if conn26 else 0,
                                   _p(out, C.c_int64), pc.size, C.byref(n), C.byref(n_refit), C.byref(n_comp)))
    es = ExtractedShape(s if not isinstance(s, L.Shape) else shape_from_c(s), out[: n.value].copy())
    return (es, {"n_refit": n_refit.value, "n_components": n_comp.value}) if return_stats else es


def refit_lsq(s, pc, params, max_iter=10):
    """Least-squares refit of `s` to its compatible points within 3*eps (the step the reference omits,
    docs/src/ransac.md:163-168).  Returns (shape, n_used, rms, iterations)."""
    out, n, rms, it = L.Shape(), C.c_int64(), C.c_double(), C.c_int32()
    cs = s if isinstance(s, L.Shape) else s.to_c()
    check(lib().rh_refit_lsq(pc._h, C.byref(cs), C.byref(_cparams(params)), max_iter, C.byref(out), C.byref(n),
                             C.byref(rms), C.byref(it)))
    return shape_from_c(out), n.value, rms.value, it.value


def estimatenormals(vertices, k=16, radius=0.0, viewpoint=None, hints=None, device=0, return_curvature=False,
                    return_flags=False, consistent=False):
    """Oriented normals for a cloud without them (rh_estimate_normals: PCA of the k nearest neighbours, the step
    docs/src/ransac.md:13 leaves to the user).  vertices: (n, 3) float64 or float32; the result has that dtype and
    feeds RANSACCloud(vertices, normals, subsets) as is.  radius > 0 drops neighbours farther than it; viewpoint
    (3-vector) turns every normal towards it, hints ((n, 3), e.g. scanner directions or rough normals) along them;
    neither: the largest component positive.  Degenerate points get (0, 0, 0) and flag 1.
    consistent=True (a cloud with neither viewpoint nor hints): the normals of the canonical sign are then turned by
    orientnormals with the same k (63 at most) and radius (anchor "top", up = +z), so that neighbouring normals agree.
    Returns normals, then curvature and / or flags when asked for."""
    if viewpoint is not None and hints is not None:
        raise ValueError("estimatenormals: give a viewpoint or hints, not both")
    if consistent:
        if viewpoint is not None or hints is not None:
            raise ValueError("estimatenormals: consistent=True is for clouds with neither a viewpoint nor hints")
        out = estimatenormals(vertices, k=k, radius=radius, device=device, return_curvature=return_curvature,
                              return_flags=return_flags)
        out = out if isinstance(out, tuple) else (out,)
        out = (orientnormals(vertices, out[0], k=k, radius=radius, device=device),) + out[1:]
        return out[0] if len(out) == 1 else out
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    prm = L.NormalsParams(k=int(k), orient=0, radius=float(radius))
    h = None
    if viewpoint is not None:
        prm.orient = 1
        prm.viewpoint[:] = [float(x) for x in np.asarray(viewpoint, dtype=np.float64).reshape(3)]
    if hints is not None:
        prm.orient = 2
        h = np.ascontiguousarray(hints, dtype=t).reshape(-1, 3)
        if h.shape[0] != n:
            raise ValueError("estimatenormals: %d hints for %d points" % (h.shape[0], n))
    nrm = np.zeros((n, 3), dtype=t)
    curv = np.zeros(n, dtype=t) if return_curvature else None
    flags = np.zeros(n, dtype=np.int32) if return_flags else None
    fn = lib().rh_estimate_normals_f32 if f32 else lib().rh_estimate_normals
    check(fn(_p(xyz, ct), n, C.byref(prm), None if h is None else _p(h, ct), device, _p(nrm, ct),
             None if curv is None else _p(curv, ct), None if flags is None else _p(flags, C.c_int32)))
    out = (nrm,) + ((curv,) if return_curvature else ()) + ((flags,) if return_flags else ())
    return out[0] if len(out) == 1 else out


def orientnormals(vertices, normals, k=16, radius=0.0, anchor="top", up=(0, 0, 1), device=0, return_info=False):
    """Turn the normals of a cloud so that neighbouring normals agree, without a viewpoint (rh_orient_normals;
    include/ransac_hip.h has the definition in full): the sign is carried along the minimum spanning forest of the
    k-nearest-neighbour graph (knn's neighbours for k and radius, either way round), whose edges are ordered by descending
    |ni . nj|, then by their indices (Hoppe et al. 1992).  Every connected part of the graph is turned as a whole:
    anchor "top" makes the normal of its topmost point along `up` point up (outward normals on a closed surface),
    "first" keeps the normal of its smallest index as given.  Points with a zero normal (the degenerate points of
    estimatenormals) take no part.  vertices, normals: (n, 3), both float32 take the float32 entry, otherwise float64.
    Returns the normals (a normal is either kept bit for bit or negated), with return_info also a dict: flip (int32 per
    point: 1 flipped, 0 kept, -1 zero normal), component (int32, 1 .. M by smallest index, 0 for a zero normal) and the
    stats n_vertices, n_edges, n_components, n_tree_edges, n_flipped, n_inconsistent (edges whose ends still disagree),
    largest_component and min_tree_absdot (the weakest link the sign was carried over)."""
    anchors = {"first": L.ORI_ANCHOR_FIRST, "top": L.ORI_ANCHOR_TOP}
    if isinstance(anchor, str) and anchor not in anchors:
        raise ValueError("orientnormals: anchor %r is neither 'first' nor 'top'" % (anchor,))
    f32 = np.asarray(vertices).dtype == np.float32 and np.asarray(normals).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    if nrm.shape[0] != n:
        raise ValueError("orientnormals: %d normals for %d points" % (nrm.shape[0], n))
    prm = L.OrientParams(k=int(k), anchor=int(anchors.get(anchor, anchor)), radius=float(radius))
    prm.up[:] = [float(x) for x in np.asarray(up, dtype=np.float64).reshape(3)]
    out = np.array(nrm)
    flip = np.full(max(n, 1), -1, dtype=np.int32) if return_info else None
    comp = np.zeros(max(n, 1), dtype=np.int32) if return_info else None
    st = L.OrientStats()
    fn = lib().rh_orient_normals_f32 if f32 else lib().rh_orient_normals
    check(fn(_p(xyz, ct), _p(nrm, ct), n, C.byref(prm), device, _p(out, ct), None if flip is None else _p(flip, C.c_int32),
             None if comp is None else _p(comp, C.c_int32), C.byref(st)))
    if not return_info:
        return out
    info = {f: getattr(st, f) for f, _ in L.OrientStats._fields_}
    info.update(flip=flip[:n], component=comp[:n])
    return out, info


def knn(vertices, k, radius=0.0, return_dist=True, return_count=False, device=0):
    """The k nearest neighbours of every point among the other points (rh_knn: exact, d^2 = (dx*dx + dy*dy) + dz*dz in
    binary64, ties to the smaller index; a duplicate of the point is a neighbour at distance 0).  vertices: (n, 3) float64
    or float32 (widened exactly).  k: 1 .. 63; radius > 0 drops neighbours farther than it.
    Returns idx (n, k) int32, 1-based, 0 where a point has fewer neighbours; then with return_dist the squared distances
    (n, k) float64, +inf there; then with return_count the neighbours per point (n,) int32."""
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n, k = xyz.shape[0], int(k)
    kk = k if 1 <= k <= L.KNN_MAX_K else 1            # (the library refuses the call; nothing is written)
    idx = np.zeros((n, kk), dtype=np.int32)
    d2 = np.full((n, kk), np.inf) if return_dist else None
    cnt = np.zeros(n, dtype=np.int32) if return_count else None
    fn = lib().rh_knn_f32 if f32 else lib().rh_knn
    check(fn(_p(xyz, ct), n, k, float(radius), device, _p(idx, C.c_int32), None if d2 is None else _p(d2, C.c_double),
             None if cnt is None else _p(cnt, C.c_int32)))
    out = (idx,) + ((d2,) if return_dist else ()) + ((cnt,) if return_count else ())
    return out[0] if len(out) == 1 else out


def _cloud_pair(who, reference, queries, extra=None):
    """The two clouds (and the reference's `extra` rows) as (n, 3) / (m, 3) arrays of one dtype: float32 when all are,
    float64 otherwise (a mixed pair is widened, exactly)."""
    arrs = [np.asarray(a) for a in (reference, queries) + ((extra,) if extra is not None else ())]
    f32 = all(a.dtype == np.float32 for a in arrs)
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    arrs = [np.ascontiguousarray(a, dtype=t).reshape(-1, 3) for a in arrs]
    if extra is not None and arrs[2].shape[0] != arrs[0].shape[0]:
        raise ValueError("%s: %d normals for %d reference points" % (who, arrs[2].shape[0], arrs[0].shape[0]))
    return f32, ct, arrs


def knn_query(reference, queries, k, radius=0.0, return_dist=True, return_count=False, device=0):
    """The k nearest points of `reference` for every point of `queries` (rh_knn_query: exact, d^2 = (dx*dx + dy*dy) + dz*dz
    in binary64, ties to the smaller reference index; no point is left out, so a reference point equal to the query is its
    first neighbour at 0 -- knn() is the call for a cloud's own points).  reference (n, 3), queries (m, 3): both float32
    take the float32 entry (widened exactly on the device), a mixed pair is widened to float64 here.  k: 1 .. 63;
    radius > 0 drops neighbours farther than it.
    Returns idx (m, k) int32, 1-based rows of `reference` in the order of `queries`, 0 where a query has fewer neighbours;
    then with return_dist the squared distances (m, k) float64, +inf there; then with return_count the neighbours per
    query (m,) int32."""
    f32, ct, (ref, qry) = _cloud_pair("knn_query", reference, queries)
    n, m, k = ref.shape[0], qry.shape[0], int(k)
    kk = k if 1 <= k <= L.KNN_MAX_K else 1            # (the library refuses the call; nothing is written)
    idx = np.zeros((m, kk), dtype=np.int32)
    d2 = np.full((m, kk), np.inf) if return_dist else None
    cnt = np.zeros(m, dtype=np.int32) if return_count else None
    fn = lib().rh_knn_query_f32 if f32 else lib().rh_knn_query
    check(fn(_p(ref, ct), n, _p(qry, ct), m, k, float(radius), device, _p(idx, C.c_int32),
             None if d2 is None else _p(d2, C.c_double), None if cnt is None else _p(cnt, C.c_int32)))
    out = (idx,) + ((d2,) if return_dist else ()) + ((cnt,) if return_count else ())
    return out[0] if len(out) == 1 else out


def cloud_distance(reference, queries, normals=None, radius=0.0, threshold=math.inf, metric=None, return_index=False,
                   return_stats=False, device=0):
    """How far every point of `queries` lies from the cloud `reference` (rh_cloud_distance; include/ransac_hip.h has the
    definition in full).  metric "point": the distance to the nearest reference point; "plane": |(q - r) . n| with r that
    point and n its row of `normals` (the reference's, used as given); the default is "plane" when normals are given and
    "point" otherwise.  radius > 0: a query without a reference point within it is not valid and gets +inf.
    Returns dist (m,) float64, then on request: return_index the nearest reference point of every query (1-based int32, 0:
    none), return_stats a dict n_valid, n_within (valid queries with dist <= threshold), argmax (1-based, 0: none), mean,
    rms, max, median over the valid queries.  The measures are one-sided, queries -> reference: the symmetric Hausdorff
    distance is the larger `max` of the two calls with the clouds exchanged, the Chamfer distance the sum of their `mean`."""
    metrics = {"point": L.DIST_POINT, "plane": L.DIST_PLANE}
    if metric is None:
        metric = "point" if normals is None else "plane"
    if isinstance(metric, str) and metric not in metrics:
        raise ValueError("cloud_distance: metric %r is neither 'point' nor 'plane'" % (metric,))
    f32, ct, arrs = _cloud_pair("cloud_distance", reference, queries, normals)
    ref, qry, nrm = arrs[0], arrs[1], (arrs[2] if normals is not None else None)
    n, m = ref.shape[0], qry.shape[0]
    prm = L.DistanceParams(radius=float(radius), threshold=float(threshold), metric=int(metrics.get(metric, metric)))
    dist = np.full(m, np.inf)
    nn = np.zeros(m, dtype=np.int32) if return_index else None
    st = L.DistanceStats()
    fn = lib().rh_cloud_distance_f32 if f32 else lib().rh_cloud_distance
    check(fn(_p(ref, ct), None if nrm is None else _p(nrm, ct), n, _p(qry, ct), m, C.byref(prm), device, _p(dist, C.c_double),
             None if nn is None else _p(nn, C.c_int32), C.byref(st) if return_stats else None))
    out = (dist,) + ((nn,) if return_index else ())
    out += (({f: getattr(st, f) for f, _ in L.DistanceStats._fields_},) if return_stats else ())
    return out[0] if len(out) == 1 else out


def transfer_labels(reference, labels, queries, radius=0.0, fill=0, device=0):
    """Carry a per-point attribute from one cloud to another: row j of the result is labels[i] for the point i of
    `reference` nearest to queries[j] (knn_query with k = 1), or `fill` when radius > 0 and no reference point lies within
    it.  labels: (n,) or (n, ...), any dtype -- labels of assign_points or cluster found on a thinned or cleaned cloud,
    normals, colours.  Returns an array of shape (m, ...) and the dtype of labels."""
    lab = np.asarray(labels)
    n = np.asarray(reference).reshape(-1, 3).shape[0]
    if lab.shape[:1] != (n,):
        raise ValueError("transfer_labels: %d labels for %d reference points" % (lab.shape[0] if lab.ndim else 0, n))
    idx = knn_query(reference, queries, 1, radius=radius, return_dist=False, device=device)[:, 0]
    out = np.full((idx.shape[0],) + lab.shape[1:], fill, dtype=lab.dtype)
    hit = idx > 0
    out[hit] = lab[idx[hit] - 1]
    return out


def register(reference, queries, normals=None, metric=None, radius=0.0, max_iter=50, rot_tol=1e-9, trans_tol=1e-9, init=None,
             device=0, return_info=False):
    """The rigid motion that brings the cloud `queries` onto the cloud `reference` by iterative closest point
    (rh_register; include/ransac_hip.h has the definition in full).  metric "point": the distance to the nearest
    reference point is minimised; "plane": the distance to its tangent plane, with `normals` the reference's (used as
    given); the default is "plane" when normals are given and "point" otherwise.  radius > 0: a query without a reference
    point within it takes no part in an iteration.  init: a 3x4 or 4x4 start (the identity by default); ICP finds the
    nearest minimum, so it has to be roughly right.  The iteration stops when a step turns by at most rot_tol and moves by
    at most trans_tol, or after max_iter iterations.
    Returns the 4x4 float64 matrix T with x' = T[:3, :3] @ x + T[:3, 3]; with return_info also a dict status ("converged",
    "max_iter", "degenerate", "too_few"), iterations, n_valid and rms of the last iteration, and history: n_valid and rms
    of every iteration run.  transform_points(T, queries) moves the cloud."""
    metrics = {"point": L.DIST_POINT, "plane": L.DIST_PLANE}
    if metric is None:
        metric = "point" if normals is None else "plane"
    if isinstance(metric, str) and metric not in metrics:
        raise ValueError("register: metric %r is neither 'point' nor 'plane'" % (metric,))
    f32, ct, arrs = _cloud_pair("register", reference, queries, normals)
    ref, qry, nrm = arrs[0], arrs[1], (arrs[2] if normals is not None else None)
    n, m = ref.shape[0], qry.shape[0]
    ini = None
    if init is not None:
        ini = np.asarray(init, dtype=np.float64)
        if ini.shape not in ((3, 4), (4, 4)):
            raise ValueError("register: init must be 3x4 or 4x4, not %r" % (ini.shape,))
        ini = np.ascontiguousarray(ini[:3])
    max_iter = int(max_iter)
    prm = L.RegisterParams(radius=float(radius), rot_tol=float(rot_tol), trans_tol=float(trans_tol),
                           metric=int(metrics.get(metric, metric)), max_iter=max_iter)
    hist = max_iter if 1 <= max_iter <= L.REG_MAX_ITERATIONS else 1      # (the library refuses the call; nothing is written)
    out = np.zeros((3, 4))
    res = L.RegisterResult()
    nv_it, rms_it = np.zeros(hist, dtype=np.int32), np.zeros(hist)
    fn = lib().rh_register_f32 if f32 else lib().rh_register
    check(fn(_p(ref, ct), None if nrm is None else _p(nrm, ct), n, _p(qry, ct), m, C.byref(prm),
             None if ini is None else _p(ini, C.c_double), device, _p(out, C.c_double), C.byref(res), _p(nv_it, C.c_int32),
             _p(rms_it, C.c_double)))
    T = np.vstack([out, [0.0, 0.0, 0.0, 1.0]])
    if not return_info:
        return T
    it = int(res.iterations)
    return T, dict(status=L.REG_STATUS_NAMES.get(res.status, res.status), iterations=it, n_valid=int(res.n_valid),
                   rms=float(res.rms), history=dict(n_valid=nv_it[:it].copy(), rms=rms_it[:it].copy()))


def describe(vertices, normals, k=32, radius=0.0, return_count=False, device=0):
    """An integer point-feature histogram per point (rh_describe; include/ransac_hip.h has the definition in full): for
    every point the angles between its normal, its neighbours' normals and the lines to them, binned 3 x 11 and summed
    with the neighbours' own histograms.  Invariant under a rigid motion of points and normals, up to values on a bin
    edge.  vertices, normals: (n, 3), both float32 (widened exactly) or float64; the normals are used as given.
    k: 1 .. 63 neighbours; radius > 0 drops neighbours farther than it.
    Returns desc (n, 33) uint16, values 0 .. 7938; then with return_count the neighbours per point (n,) int32."""
    arrs = [np.asarray(vertices), np.asarray(normals)]
    f32 = all(a.dtype == np.float32 for a in arrs)
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz, nrm = (np.ascontiguousarray(a, dtype=t).reshape(-1, 3) for a in arrs)
    if nrm.shape[0] != xyz.shape[0]:
        raise ValueError("describe: %d normals for %d points" % (nrm.shape[0], xyz.shape[0]))
    n = xyz.shape[0]
    desc = np.zeros((n, L.DESC_DIM), dtype=np.uint16)
    cnt = np.zeros(n, dtype=np.int32) if return_count else None
    fn = lib().rh_describe_f32 if f32 else lib().rh_describe
    check(fn(_p(xyz, ct), _p(nrm, ct), n, int(k), float(radius), device, _p(desc, C.c_uint16),
             None if cnt is None else _p(cnt, C.c_int32)))
    return (desc, cnt) if return_count else desc


def match_features(ref_desc, qry_desc, mutual=False, return_dist=False, device=0):
    """For every row of qry_desc the row of ref_desc with the smallest sum of squared differences (rh_match_features: an
    exact integer, ties to the smaller index).  Both: (rows, 33) uint16 as describe returns them.  mutual: an entry is 0
    unless the query is in turn the best query of its reference row.
    Returns idx (m,) int32, 1-based rows of ref_desc; then with return_dist the sums (m,) uint32."""
    ref = np.ascontiguousarray(ref_desc, dtype=np.uint16)
    qry = np.ascontiguousarray(qry_desc, dtype=np.uint16)
    for a in (ref, qry):
        if a.ndim != 2 or a.shape[1] != L.DESC_DIM:
            raise ValueError("match_features: descriptors are (rows, %d), not %r" % (L.DESC_DIM, a.shape))
    n, m = ref.shape[0], qry.shape[0]
    idx = np.zeros(m, dtype=np.int32)
    dist = np.zeros(m, dtype=np.uint32) if return_dist else None
    check(lib().rh_match_features(_p(ref, C.c_uint16), n, _p(qry, C.c_uint16), m, L.MATCH_MUTUAL if mutual else 0, device,
                                  _p(idx, C.c_int32), None if dist is None else _p(dist, C.c_uint32)))
    return (idx, dist) if return_dist else idx


def register_global(reference, queries, ref_normals, qry_normals, tau, k=32, feature_radius=0.0, trials=20000, edge_ratio=0.9,
                    min_edge=0.0, mutual=False, seed=0, triples=None, refine=True, metric=None, radius=None, device=0,
                    return_info=False):
    """The rigid motion that brings the cloud `queries` onto the cloud `reference` WITHOUT a start: describe() on both
    clouds (k, feature_radius), match_features() from the queries to the reference (mutual: entries of 0 are dropped), then
    rh_register_global -- `trials` hypotheses from three correspondences each, drawn from `seed` (or the given `triples`,
    (trials, 3) 0-based into the correspondences), kept when their edges agree within edge_ratio and the query edges are
    at least min_edge long, and scored by the correspondences they bring within tau.  include/ransac_hip.h has the
    definitions in full.
    tau: about 1.5 point spacings (the nn_median that removeoutliers reports): matches are only as exact as the sampling,
    and a hypothesis from three of them is off by about as much.
    refine: the result starts register(reference, queries, normals=ref_normals, metric=metric, radius=radius, init=T);
    radius defaults to 3 tau there.
    Returns the 4x4 float64 matrix; with return_info also a dict: coarse (the 4x4 of the best hypothesis), counts (trials,),
    status ("ok", "no_trial"), best_trial, best_count, n_valid_trials, corr_qry and corr_ref (1-based int32) and, with
    refine, register's info under "register"."""
    f32, ct, (ref, qry) = _cloud_pair("register_global", reference, queries)
    dref = describe(ref, np.asarray(ref_normals, dtype=ref.dtype), k=k, radius=feature_radius, device=device)
    dqry = describe(qry, np.asarray(qry_normals, dtype=qry.dtype), k=k, radius=feature_radius, device=device)
    idx = match_features(dref, dqry, mutual=mutual, device=device)
    corr_qry = np.ascontiguousarray((np.flatnonzero(idx > 0) + 1).astype(np.int32))
    corr_ref = np.ascontiguousarray(idx[idx > 0].astype(np.int32))
    c, trials = len(corr_qry), int(trials)
    tri = None
    if triples is not None:
        tri = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        trials = tri.shape[0]
    prm = L.GlobalParams(trials=trials, seed=int(seed), tau=float(tau), edge_ratio=float(edge_ratio), min_edge=float(min_edge))
    out, res = np.zeros((3, 4)), L.GlobalResult()
    counts = np.zeros(trials if 1 <= trials <= L.GLOBAL_MAX_TRIALS else 1, dtype=np.int32)
    fn = lib().rh_register_global_f32 if f32 else lib().rh_register_global
    check(fn(_p(ref, ct), ref.shape[0], _p(qry, ct), qry.shape[0], _p(corr_qry, C.c_int32), _p(corr_ref, C.c_int32), c, C.byref(prm),
             None if tri is None else _p(tri, C.c_int32), device, _p(out, C.c_double), C.byref(res), _p(counts, C.c_int32)))
    coarse = np.vstack([out, [0.0, 0.0, 0.0, 1.0]])
    T, reg = coarse, None
    if refine:
        T, reg = register(ref, qry, normals=np.asarray(ref_normals, dtype=ref.dtype), metric=metric,
                          radius=3.0 * float(tau) if radius is None else radius, init=coarse, device=device, return_info=True)
    if not return_info:
        return T
    info = dict(coarse=coarse, counts=counts, status=L.GLOB_STATUS_NAMES.get(res.status, res.status), best_trial=int(res.best_trial),
                best_count=int(res.best_count), n_valid_trials=int(res.n_valid_trials), corr_qry=corr_qry, corr_ref=corr_ref)
    if refine:
        info["register"] = reg
    return T, info


def _rigid(who, T):
    T = np.asarray(T, dtype=np.float64)
    if T.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: the transform must be 3x4 or 4x4, not %r" % (who, T.shape))
    return T


def transform_points(T, points):
    """x' = T[:3, :3] @ x + T[:3, 3] for every row of points (n, 3), in float64 and in register's operation order:
    ((R_k0*x + R_k1*y) + R_k2*z) + t_k.  T: 3x4 or 4x4, e.g. what register returns."""
    T = _rigid("transform_points", T)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def transform_normals(T, normals):
    """n' = T[:3, :3] @ n for every row of normals (n, 3): directions turn with a rigid motion and do not move."""
    T = _rigid("transform_normals", T)
    p = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z for k in range(3)], axis=1)


def removeoutliers(vertices, k=16, std_mul=2.0, mode="statistical", radius=0.0, threshold=None, normals=None, device=0,
                   return_index=False, return_stats=False, return_mean_dist=False):
    """Drop the stray points of a raw cloud (rh_remove_outliers; include/ransac_hip.h has the definition in full).  With
    m_i the mean distance of point i to its k nearest neighbours (within radius, when radius > 0):
    mode "statistical" keeps m_i <= mu + std_mul * sigma (mean and standard deviation of the m_i), "absolute" keeps
    m_i <= threshold, "radius" keeps the points with at least k other points within radius.  A point without a neighbour
    is dropped.  vertices: (n, 3) float64 or float32; normals (optional, same shape) are thinned along.
    Returns the kept vertices, then the kept normals when they were given, then on request: return_index the kept points'
    1-based indices (ascending, int32), return_stats a dict n_valid, n_kept, mu, sigma, tau, nn_median (the median
    nearest-neighbour distance: the cloud's point spacing), return_mean_dist the m_i of every point (+inf: no
    neighbour)."""
    modes = {"statistical": L.OUT_STATISTICAL, "absolute": L.OUT_ABSOLUTE, "radius": L.OUT_RADIUS}
    if isinstance(mode, str) and mode not in modes:
        raise ValueError("removeoutliers: mode %r is none of %s" % (mode, sorted(modes)))
    mode = int(modes.get(mode, mode))
    if mode == L.OUT_ABSOLUTE and threshold is None:
        raise ValueError("removeoutliers: mode 'absolute' needs a threshold")
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = None
    if normals is not None:
        nrm = np.asarray(normals).reshape(-1, 3)
        if nrm.shape[0] != n:
            raise ValueError("removeoutliers: %d normals for %d points" % (nrm.shape[0], n))
    prm = L.OutlierParams(k=int(k), mode=mode, std_mul=float(std_mul), radius=float(radius),
                          threshold=0.0 if threshold is None else float(threshold))
    keep = np.zeros(n, dtype=np.uint8)
    idx = np.zeros(max(n, 1), dtype=np.int32)
    mean = np.zeros(n) if return_mean_dist else None
    st, nk = L.OutlierStats(), C.c_int64(0)
    fn = lib().rh_remove_outliers_f32 if f32 else lib().rh_remove_outliers
    check(fn(_p(xyz, ct), n, C.byref(prm), device, _p(keep, C.c_uint8), _p(idx, C.c_int32), n, C.byref(nk),
             None if mean is None else _p(mean, C.c_double), C.byref(st)))
    idx = idx[:nk.value].copy()
    out = (xyz[idx - 1],) + ((nrm[idx - 1],) if nrm is not None else ())
    out += ((idx,) if return_index else ())
    out += (({f: getattr(st, f) for f, _ in L.OutlierStats._fields_},) if return_stats else ())
    out += ((mean,) if return_mean_dist else ())
    return out[0] if len(out) == 1 else out


def cluster(vertices, eps, min_pts=8, min_size=1, order="index", device=0, return_kind=False, return_counts=False,
            return_lists=False, return_stats=False):
    """Split a raw cloud into its spatially connected parts (rh_cluster: DBSCAN, include/ransac_hip.h has the definition in
    full).  Two points are neighbours when d^2 <= eps*eps (the boundary counts); a point with at least min_pts points
    within eps, itself included, is a core point; the clusters are the connected components of the core points, a point
    that is no core point joins the cluster of its nearest core neighbour (ties to the smaller index), the rest is noise,
    and so are clusters of fewer than min_size points.  min_pts = 1 is plain Euclidean cluster extraction.  order "index"
    numbers the clusters by their smallest core point's index, "size" by descending size.  eps is usually a small multiple
    of the point spacing (removeoutliers(..., return_stats=True)["nn_median"]).  vertices: (n, 3) float64 or float32
    (widened exactly).
    Returns labels (int32, 0 = noise, 1 .. M), then on request: return_kind uint8 per point (_lib.PT_NOISE / PT_BORDER /
    PT_CORE), return_counts int64[M + 1] (noise first), return_lists (offsets[M + 2], idx[n]): the 1-based indices grouped
    by label, noise first, ascending within a label (lists_from_assignment splits them), return_stats a dict n_clusters,
    n_core, n_border, n_noise, n_small, largest."""
    orders = {"index": L.CLUSTER_BY_INDEX, "size": L.CLUSTER_BY_SIZE}
    if isinstance(order, str) and order not in orders:
        raise ValueError("cluster: order %r is neither 'index' nor 'size'" % (order,))
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    prm = L.ClusterParams(eps=float(eps), min_pts=int(min_pts), min_size=int(min_size), order=int(orders.get(order, order)))
    labels = np.zeros(max(n, 1), dtype=np.int32)
    kind = np.zeros(max(n, 1), dtype=np.uint8) if return_kind else None
    counts = np.zeros(n + 1, dtype=np.int64) if return_counts else None
    offsets = np.zeros(n + 2, dtype=np.int64) if return_lists else None
    idx = np.zeros(max(n, 1), dtype=np.int64) if return_lists else None
    st, m = L.ClusterStats(), C.c_int64(0)
    fn = lib().rh_cluster_f32 if f32 else lib().rh_cluster
    check(fn(_p(xyz, ct), n, C.byref(prm), device, _p(labels, C.c_int32), None if kind is None else _p(kind, C.c_uint8), n,
             None if counts is None else _p(counts, C.c_int64), None if offsets is None else _p(offsets, C.c_int64),
             None if idx is None else _p(idx, C.c_int64), C.byref(m), C.byref(st)))
    m = int(m.value)
    out = (labels[:n],) + ((kind[:n],) if return_kind else ()) + ((counts[:m + 1].copy(),) if return_counts else ())
    out += ((offsets[:m + 2].copy(), idx[:n]) if return_lists else ())
    out += (({f: int(getattr(st, f)) for f, _ in L.ClusterStats._fields_},) if return_stats else ())
    return out[0] if len(out) == 1 else out


def cluster_inpoints(vertices, inpoints, eps, **kw):
    """The clusters of the points vertices[inpoints - 1] (inpoints: 1-based indices, e.g. an ExtractedShape's, or the
    unlabelled list of assign_points): a list of int64 arrays, one per cluster in the order of cluster(...), each holding
    that cluster's members as 1-based indices into `vertices` -- the caller's indexing -- in the order in which inpoints
    lists them.  Noise is left out.  kw: min_pts, min_size, order, device of cluster()."""
    bad = [k for k in kw if k not in ("min_pts", "min_size", "order", "device")]
    if bad:
        raise TypeError("cluster_inpoints: unexpected argument %s" % bad[0])
    v = np.asarray(vertices)
    v = v.reshape(-1, 3)
    sel = np.asarray(inpoints, dtype=np.int64).reshape(-1)
    if sel.size == 0:
        return []
    if sel.min() < 1 or sel.max() > v.shape[0]:
        raise ValueError("cluster_inpoints: an index outside 1 .. %d" % v.shape[0])
    _, offsets, idx = cluster(v[sel - 1], eps, return_lists=True, **kw)
    return [sel[part - 1] for part in lists_from_assignment(offsets, idx)[1:]]


def segment_smooth(vertices, normals, curvature=None, k=16, radius=0.0, angle=math.radians(25.0), curv_max=0.05, dist_max=0.0,
                   unsigned=False, min_size=1, order="size", device=0, return_kind=False, return_counts=False,
                   return_lists=False, return_stats=False, cos_angle=None):
    """Split a cloud with normals into its smooth sheets (rh_segment_smooth: region growing by smoothness, restated so
    that nothing depends on an order; include/ransac_hip.h has the definition in full).  Two points are linked when one is
    among the other's k nearest neighbours (within radius, when radius > 0), their normals differ by at most `angle`
    (radians; unsigned: up to sign) and, with dist_max > 0, each lies within dist_max of the other's tangent plane.  A
    point whose curvature is at most curv_max is a seed (every point with a normal, when no curvature is given); the
    regions are the connected components of the seeds, a point that is no seed joins the region of its nearest linked
    seed (ties to the smaller index), the rest has no label, and neither have regions of fewer than min_size points nor
    points whose normal is (0, 0, 0).  order "size" numbers the regions by descending size, "index" by their smallest
    seed's index.  The cosine of `angle` is taken here and handed on; cos_angle= gives it directly instead.
    vertices, normals: (n, 3) float64 or float32 (widened exactly; the normals and the curvature take the dtype of the
    vertices), curvature: (n,), e.g. estimatenormals(..., return_curvature=True).
    Returns labels (int32, 0 = none, 1 .. M), then on request: return_kind uint8 per point (_lib.PT_NOISE / PT_BORDER /
    PT_CORE = seed), return_counts int64[M + 1] (label 0 first), return_lists (offsets[M + 2], idx[n]): the 1-based indices
    grouped by label, ascending within a label (lists_from_assignment splits them), return_stats a dict n_regions, n_seed,
    n_border, n_unassigned, n_invalid, n_small, largest."""
    orders = {"index": L.CLUSTER_BY_INDEX, "size": L.CLUSTER_BY_SIZE}
    if isinstance(order, str) and order not in orders:
        raise ValueError("segment_smooth: order %r is neither 'index' nor 'size'" % (order,))
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    if nrm.shape[0] != n:
        raise ValueError("segment_smooth: %d normals for %d points" % (nrm.shape[0], n))
    curv = None
    if curvature is not None:
        curv = np.ascontiguousarray(curvature, dtype=t).reshape(-1)
        if curv.shape[0] != n:
            raise ValueError("segment_smooth: %d curvatures for %d points" % (curv.shape[0], n))
    prm = L.SegmentParams(k=int(k), flags=L.SEG_UNSIGNED if unsigned else 0, radius=float(radius),
                          cos_angle=math.cos(float(angle)) if cos_angle is None else float(cos_angle), curv_max=float(curv_max),
                          dist_max=float(dist_max), min_size=int(min_size), order=int(orders.get(order, order)))
    labels = np.zeros(max(n, 1), dtype=np.int32)
    kind = np.zeros(max(n, 1), dtype=np.uint8) if return_kind else None
    counts = np.zeros(n + 1, dtype=np.int64) if return_counts else None
    offsets = np.zeros(n + 2, dtype=np.int64) if return_lists else None
    idx = np.zeros(max(n, 1), dtype=np.int64) if return_lists else None
    st, m = L.SegmentStats(), C.c_int64(0)
    fn = lib().rh_segment_smooth_f32 if f32 else lib().rh_segment_smooth
    check(fn(_p(xyz, ct), _p(nrm, ct), None if curv is None else _p(curv, ct), n, C.byref(prm), device, _p(labels, C.c_int32),
             None if kind is None else _p(kind, C.c_uint8), n, None if counts is None else _p(counts, C.c_int64),
             None if offsets is None else _p(offsets, C.c_int64), None if idx is None else _p(idx, C.c_int64), C.byref(m), C.byref(st)))
    m = int(m.value)
    out = (labels[:n],) + ((kind[:n],) if return_kind else ()) + ((counts[:m + 1].copy(),) if return_counts else ())
    out += ((offsets[:m + 2].copy(), idx[:n]) if return_lists else ())
    out += (({f: int(getattr(st, f)) for f, _ in L.SegmentStats._fields_},) if return_stats else ())
    return out[0] if len(out) == 1 else out


def segment_inpoints(vertices, normals, inpoints, curvature=None, **kw):
    """The smooth regions of the points vertices[inpoints - 1] (inpoints: 1-based indices, e.g. the unlabelled list of
    assign_points): a list of int64 arrays, one per region in the order of segment_smooth(...), each holding that region's
    members as 1-based indices into `vertices` -- the caller's indexing -- in the order in which inpoints lists them.
    Points without a label are left out.  kw: k, radius, angle, cos_angle, curv_max, dist_max, unsigned, min_size, order,
    device of segment_smooth()."""
    bad = [k for k in kw if k not in ("k", "radius", "angle", "cos_angle", "curv_max", "dist_max", "unsigned", "min_size", "order", "device")]
    if bad:
        raise TypeError("segment_inpoints: unexpected argument %s" % bad[0])
    v = np.asarray(vertices).reshape(-1, 3)
    nrm = np.asarray(normals).reshape(-1, 3)
    sel = np.asarray(inpoints, dtype=np.int64).reshape(-1)
    if sel.size == 0:
        return []
    if sel.min() < 1 or sel.max() > v.shape[0]:
        raise ValueError("segment_inpoints: an index outside 1 .. %d" % v.shape[0])
    curv = None if curvature is None else np.asarray(curvature).reshape(-1)[sel - 1]
    _, offsets, idx = segment_smooth(v[sel - 1], nrm[sel - 1], curv, return_lists=True, **kw)
    return [sel[part - 1] for part in lists_from_assignment(offsets, idx)[1:]]


def voxeldownsample(vertices, beta, normals=None, mode="centroid", align_normals=False, device=0, return_index=False,
                    return_counts=False, return_map=False):
    """Thin a raw cloud on a voxel grid of width beta (rh_voxel_downsample, include/ransac_hip.h has the definition in
    full): one point per occupied cell, rows in the order in which the cells first appear.  vertices: (n, 3) float64 or
    float32, the result has that dtype; normals (optional, same shape) are thinned along.  mode "centroid": the mean of
    the cell's points (exact integer sums: the same bits whatever the order of the points) and the normalised sum of
    their normals, with align_normals each normal first turned to the side of the cell's first (for
    estimatenormals(...) output without a viewpoint or hints, whose sign flips inside a cell); mode "first": the cell's
    first point and its normal as they are.  Points with a non-finite coordinate (or a non-finite / larger-than-2 normal
    component) are dropped.
    Returns the thinned vertices, then the normals when they were given, then on request: return_index the 1-based index
    of every cell's first point, return_counts the points per cell, return_map row_of_point (n int32: the 1-based row of
    every point, 0 for a dropped one; expand_inpoints carries a shape's point list back through it)."""
    modes = {"first": L.VOX_FIRST, "centroid": L.VOX_CENTROID}
    if isinstance(mode, str) and mode not in modes:
        raise ValueError("voxeldownsample: mode %r is neither 'first' nor 'centroid'" % (mode,))
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=t).reshape(-1, 3)
        if nrm.shape[0] != n:
            raise ValueError("voxeldownsample: %d normals for %d points" % (nrm.shape[0], n))
    prm = L.VoxelParams(beta=float(beta), mode=int(modes.get(mode, mode)), flags=L.VOX_ALIGN_NORMALS if align_normals else 0)
    xo = np.empty((max(n, 1), 3), dtype=t)
    no = np.empty((max(n, 1), 3), dtype=t) if nrm is not None else None
    first = np.empty(max(n, 1), dtype=np.int64) if return_index else None
    count = np.empty(max(n, 1), dtype=np.int32) if return_counts else None
    rowof = np.zeros(n, dtype=np.int32) if return_map else None
    m = C.c_int64(0)
    fn = lib().rh_voxel_downsample_f32 if f32 else lib().rh_voxel_downsample
    check(fn(_p(xyz, ct), None if nrm is None else _p(nrm, ct), n, C.byref(prm), device, _p(xo, ct),
             None if no is None else _p(no, ct), None if first is None else _p(first, C.c_int64),
             None if count is None else _p(count, C.c_int32), n, None if rowof is None else _p(rowof, C.c_int32),
             C.byref(m), None))
    m = int(m.value)
    out = (xo[:m].copy(),) + ((no[:m].copy(),) if no is not None else ())
    out += ((first[:m].copy(),) if return_index else ()) + ((count[:m].copy(),) if return_counts else ())
    out += ((rowof,) if return_map else ())
    return out[0] if len(out) == 1 else out


def expand_inpoints(inpoints, row_of_point):
    """The full-cloud 1-based indices, ascending, of the points whose row (row_of_point of voxeldownsample) is in
    `inpoints`, a list of 1-based indices into the thinned cloud: what carries an ExtractedShape found on the thinned
    cloud back to the raw scan."""
    rows = np.asarray(row_of_point)
    want = np.zeros(int(rows.max(initial=0)) + 1, dtype=bool)
    idx = np.asarray(inpoints, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 1 or idx.max() >= want.size):
        raise ValueError("expand_inpoints: a row outside 1 .. %d" % (want.size - 1))
    want[idx] = True
    return np.flatnonzero(want[rows] & (rows > 0)).astype(np.int64) + 1


class Extent:
    """Where a shape's points lie and how well they sit on it (rh_extent, include/ransac_hip.h has the definition in full):
    n, kind, flags (EXT_EMPTY / EXT_NO_DIRECTION of _lib), origin[3], frame[3, 3] (rows u, v, w), lo[3] / hi[3] (the box
    of the points along u, v, w, measured from origin), centroid[3], lam[3] (the scatter along u, v -- and w for spheres),
    dist_rms, dist_maxabs.  `c` keeps the C record."""

    def __init__(self, c):
        self.c = L.Extent.from_buffer_copy(bytes(c))
        self.n, self.kind, self.flags = int(c.n), int(c.kind), int(c.flags)
        self.origin = np.array(c.origin, dtype=np.float64)
        self.frame = np.array(c.frame, dtype=np.float64).reshape(3, 3)
        self.lo, self.hi = np.array(c.lo, dtype=np.float64), np.array(c.hi, dtype=np.float64)
        self.centroid = np.array(c.centroid, dtype=np.float64)
        self.lam = np.array(c.lam, dtype=np.float64)
        self.dist_rms, self.dist_maxabs = float(c.dist_rms), float(c.dist_maxabs)

    @property
    def size(self):
        """hi - lo: the sides of the box along u, v, w"""
        return self.hi - self.lo

    def __repr__(self):
        return "Extent(%s, %d ps, %s, rms %.3g)" % (L.KIND_NAMES.get(self.kind, "?"), self.n, self.size, self.dist_rms)


def shape_extents(pc, extracted_shapes):
    """Oriented extents and fit residuals of shapes with their point lists, all in ONE call on the device
    (rh_shape_extents): for every ExtractedShape -- or (shape, 1-based index array) pair -- an Extent.  The lists may be
    in any order and hold duplicates; Float64 and Float32 clouds.  Nothing on the cloud changes."""
    pairs = [(x.shape, x.inpoints, getattr(x, "c_shape", None)) if isinstance(x, ExtractedShape) else (x[0], x[1], None)
             for x in extracted_shapes]
    b = len(pairs)
    if b == 0:
        return []
    arr = (L.Shape * b)()
    for j, (s, _, cs) in enumerate(pairs):
        arr[j] = cs if cs is not None else (s if isinstance(s, L.Shape) else s.to_c())
    lists = [np.ascontiguousarray(i, dtype=np.int64).reshape(-1) for _, i, _ in pairs]
    off = np.zeros(b + 1, dtype=np.int64)
    np.cumsum([a.size for a in lists], out=off[1:])
    idx = np.ascontiguousarray(np.concatenate(lists)) if off[-1] else np.zeros(1, dtype=np.int64)
    out = (L.Extent * b)()
    check(lib().rh_shape_extents(pc._h, arr, b, _p(off, C.c_int64), _p(idx, C.c_int64), out))
    return [Extent(e) for e in out]


def _assign_shapes(shapes, who):
    """FittedShapes, ExtractedShapes (their c_shape when they carry one) or L.Shapes -> the C array, as shape_extents unpacks them"""
    cs = []
    for x in shapes:
        if isinstance(x, ExtractedShape):
            c = getattr(x, "c_shape", None)
            x = c if c is not None else x.shape
        cs.append(x if isinstance(x, L.Shape) else x.to_c())
    if len(cs) > L.ASSIGN_MAX_SHAPES:
        raise ValueError("%s: %d shapes, at most %d in one call" % (who, len(cs), L.ASSIGN_MAX_SHAPES))
    arr = (L.Shape * max(1, len(cs)))()
    for j, c in enumerate(cs):
        arr[j] = c
    return arr, len(cs)


def _assign_outputs(n, b, return_dist, return_counts, return_lists):
    labels = np.zeros(max(1, n), dtype=np.int32)
    dist = np.empty(max(1, n), dtype=np.float64) if return_dist else None
    counts = np.zeros(b + 1, dtype=np.int64) if return_counts else None
    offsets = np.zeros(b + 2, dtype=np.int64) if return_lists else None
    idx = np.zeros(max(1, n), dtype=np.int64) if return_lists else None
    ptrs = (_p(labels, C.c_int32), None if dist is None else _p(dist, C.c_double), None if counts is None else _p(counts, C.c_int64),
            None if offsets is None else _p(offsets, C.c_int64), None if idx is None else _p(idx, C.c_int64))

    def result():
        out = (labels[:n],) + ((dist[:n],) if return_dist else ()) + ((counts,) if return_counts else ())
        out += ((offsets, idx[:n]) if return_lists else ())
        return out[0] if len(out) == 1 else out
    return ptrs, result


def assign_points(vertices, normals, shapes, params, use_normals=True, device=0, return_dist=False, return_counts=False,
                  return_lists=False):
    """Label every point of a raw scan with its nearest compatible shape (rh_assign_points, include/ransac_hip.h has the
    definition in full): label j + 1 for the shape j that claims the point -- rh_refit's test, distance < eps and angle
    within alpha -- at the smallest distance, ties to the earlier shape; 0 when none does.  vertices: (n, 3) float64 or
    float32 (promoted exactly; the tests run in binary64 either way); normals: the same shape, or None -- then, or with
    use_normals = False, the distance alone decides.  shapes: FittedShapes, ExtractedShapes or C shape records, at most 1024.
    No RANSACCloud is needed: this is the stage that carries shapes found on a thinned cloud back to the scan, point by
    point.  Returns labels (int32), then on request: return_dist the winner's distance (-1 for label 0), return_counts
    int64[b + 1] (unlabelled first), return_lists (offsets[b + 2], idx[n]): the 1-based indices grouped by label, label 0
    first, ascending within a group (lists_from_assignment splits them)."""
    f32 = np.asarray(vertices).dtype == np.float32
    t, ct = (np.float32, C.c_float) if f32 else (np.float64, C.c_double)
    xyz = np.ascontiguousarray(vertices, dtype=t).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=t).reshape(-1, 3)
        if nrm.shape[0] != n:
            raise ValueError("assign_points: %d normals for %d points" % (nrm.shape[0], n))
    arr, b = _assign_shapes(shapes, "assign_points")
    ptrs, result = _assign_outputs(n, b, return_dist, return_counts, return_lists)
    fn = lib().rh_assign_points_f32 if f32 else lib().rh_assign_points
    check(fn(_p(xyz, ct), None if nrm is None else _p(nrm, ct), n, arr, b, C.byref(_cparams(params)),
             0 if use_normals else L.ASSIGN_NO_NORMALS, device, *ptrs))
    return result()


def assign_cloud(pc, shapes, params, enabled_only=False, use_normals=True, return_dist=False, return_counts=False,
                 return_lists=False):
    """assign_points on a RANSACCloud's resident points (rh_cloud_assign; Float64 and Float32 clouds, both tested in
    binary64 with the shapes as given).  enabled_only: a disabled point gets label 0 whatever its geometry.  Nothing on the
    cloud changes."""
    arr, b = _assign_shapes(shapes, "assign_cloud")
    ptrs, result = _assign_outputs(pc.size, b, return_dist, return_counts, return_lists)
    flags = (0 if use_normals else L.ASSIGN_NO_NORMALS) | (L.ASSIGN_ENABLED_ONLY if enabled_only else 0)
    check(lib().rh_cloud_assign(pc._h, arr, b, C.byref(_cparams(params)), flags, *ptrs))
    return result()


def lists_from_assignment(offsets, idx):
    """The per-label index arrays of an assignment's lists: element 0 the unlabelled points, element j + 1 the points of
    shape j (1-based, ascending) -- what shape_extents takes as a shape's list."""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if offsets.size < 2 or offsets[0] != 0 or offsets[-1] != idx.size or (np.diff(offsets) < 0).any():
        raise ValueError("lists_from_assignment: offsets do not partition %d indices" % idx.size)
    return [idx[offsets[k]:offsets[k + 1]] for k in range(offsets.size - 1)]


def invalidate_indexes(pc, indexlist):  # invalidate_indexes!: fitting.jl:197-202
    idx = np.ascontiguousarray(indexlist, dtype=np.int64)
    check(lib().rh_invalidate(pc._h, _p(idx, C.c_int64), idx.size))


def select_enabled(pc, ranks):
    """k-th enabled point of the root cell: the `enabled_inds[nexti]` of fitting.jl:405-422."""
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.zeros(max(1, r.size), dtype=np.int64)
    check(lib().rh_select_enabled(pc._h, _p(r, C.c_int64), r.size, _p(out, C.c_int64)))
    return out[: r.size]


def sample_sets(pc, drawN, rng, k):
    """samplepointcloud4!(pc, ...) (fitting.jl:383-430) k times in a row on `rng` (an _lib.Rng: rh_rng_seed / an injected
    stream) -- one launch for the k minimal sets of an iteration, the generator advanced exactly as k sequential calls would
    advance it.  Returns (idx, ok, level): k x drawN point indices (1-based), the reference's two return values per set."""
    k = int(k)
    idx = np.zeros((max(1, k), int(drawN)), dtype=np.int64)
    ok = np.zeros(max(1, k), dtype=np.int32)
    lev = np.zeros(max(1, k), dtype=np.int32)
    check(lib().rh_sample_sets(pc._h, int(drawN), C.byref(rng), k, _p(idx, C.c_int64), _p(ok, C.c_int32), _p(lev, C.c_int32)))
    return idx[:k], ok[:k].astype(bool), lev[:k]


def fit_sets(pc, sets, ok, params):
    """forcefitshapes! (fitting.jl:165-173) over the minimal sets of an iteration in one call (rh_fit_sets): returns (list of
    rh_shape in candidate order, index of the set each came from)."""
    sets = np.ascontiguousarray(sets, dtype=np.int64)
    k, drawN = sets.shape
    okc = None if ok is None else np.ascontiguousarray(ok, dtype=np.int32)
    cp = _cparams(params)
    cap = max(1, k * max(1, cp.n_shape_types))
    arr = (L.Shape * cap)()
    so = np.zeros(cap, dtype=np.int32)
    n = C.c_int32()
    f32 = bool(getattr(pc, "is_f32", False))
    xyz = pc.vertices if not f32 else np.ascontiguousarray(pc.vertices32, dtype=np.float64)
    nrm = pc.normals if not f32 else np.ascontiguousarray(pc.normals32, dtype=np.float64)
    check(lib().rh_fit_sets(_p(xyz, C.c_double), _p(nrm, C.c_double), _p(sets, C.c_int64), None if okc is None else _p(okc, C.c_int32),
                            k, drawN, C.byref(cp), 1 if f32 else 0, arr, _p(so, C.c_int32), cap, C.byref(n)))
    return [arr[i] for i in range(n.value)], so[: n.value]


class _ResultOwner:
    """Keeps an rh_result (and with it the pinned block of index lists) alive; frees it on collection."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().rh_result_free(C.byref(self.res))
        except Exception:   # interpreter shutdown
            pass


class MpGroup:
    """The processes of one node that run ransac() on ONE scene together (rh_mp, include/ransac_hip.h): one process per
    GPU, each with a replica of the cloud.  Collective constructor: every rank passes the same name."""

    def __init__(self, name, rank, world, slot_bytes=0):
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        check(lib().rh_mp_open(name.encode(), self.rank, self.world, int(slot_bytes), C.byref(h)))
        self._h = h

    def allgather(self, payload):
        """bytes of equal length from every rank -> list of `world` bytes objects, in rank order"""
        payload = bytes(payload)
        out = C.create_string_buffer(len(payload) * self.world)
        check(lib().rh_mp_allgather(self._h, payload, len(payload), out))
        return [out.raw[i * len(payload):(i + 1) * len(payload)] for i in range(self.world)]

    def close(self):
        if getattr(self, "_h", None):
            lib().rh_mp_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ransac(pc, params, setenabled=False, reset_rand=False, seed=1234, stream=None,
           score_mode=L.SCORE_INT64_WRAP, sphere_uses_enabled=False, sampling_streams=0, octree_sampling=False,
           return_stats=False, mp=None, component_beta=None, component_conn26=True, extents=False):
    """ransac(pc, params[, setenabled]; reset_rand) -> (Vector{ExtractedShape}, seconds)
    (iterations.jl:14-21, 35-162).  `reset_rand` reseeds the generator with 1234 like
    Random.seed!(1234); `stream` injects raw 64-bit draws (rand(1:n) = 1 + floor(u*n/2^64)).
    mp: an MpGroup -- the loop is then run by all its ranks together on this one scene (rh_ransac_mp: the minimal
    sets of every iteration dealt round-robin to the ranks); every rank gets the same result as a single process.
    component_beta: this call runs with pc.set_component_filter(component_beta, component_conn26) -- every extraction
    keeps the largest connected patch of its refit set -- and the cloud's previous setting is restored afterwards
    (None: the cloud's own setting holds).
    extents: after the loop, one rh_result_extents call for all extracted shapes; every ExtractedShape then carries an
    Extent as `.extent` (shape_extents; off by default: the result objects are what they were)."""
    if component_beta is not None:
        previous = pc.component_filter
        pc.set_component_filter(component_beta, component_conn26)
        try:
            return ransac(pc, params, setenabled, reset_rand, seed, stream, score_mode, sphere_uses_enabled, sampling_streams,
                          octree_sampling, return_stats, mp, extents=extents)
        finally:
            pc.set_component_filter(*previous)
    if setenabled:
        pc.enable_all()
    cp = params if isinstance(params, L.Params) else params_to_c(params, score_mode, sphere_uses_enabled, sampling_streams, octree_sampling)
    rng = L.Rng()
    lib().rh_rng_seed(C.byref(rng), 1234 if reset_rand else seed)
    keep = None
    if stream is not None:
        keep = np.ascontiguousarray(stream, dtype=np.uint64)
        rng.stream = _p(keep, C.c_uint64)
        rng.stream_len = keep.size
    res = L.Result()
    if mp is not None:
        check(lib().rh_ransac_mp(pc._h, _p(pc.vertices, C.c_double), _p(pc.normals, C.c_double), C.byref(cp),
                                 C.byref(rng), mp._h, C.byref(res)))
    elif getattr(pc, "is_f32", False):   # a Float32 cloud: the loop in binary32, from the Float32 arrays as they are
        check(lib().rh_ransac_f32(pc._h, _p(pc.vertices32, C.c_float), _p(pc.normals32, C.c_float), C.byref(cp),
                                  C.byref(rng), C.byref(res)))
    else:
        check(lib().rh_ransac(pc._h, _p(pc.vertices, C.c_double), _p(pc.normals, C.c_double), C.byref(cp),
                              C.byref(rng), C.byref(res)))
    # the index lists stay where rh_ransac put them (one pinned block per run): every `inpoints` is a
    # zero-copy view whose base keeps the result alive; rh_result_free runs when the last view is gone
    owner = _ResultOwner(res)
    extracted = []
    for i in range(res.n_shapes):
        e = res.shapes[i]
        if e.n_inpoints > 0:
            raw = (C.c_int64 * e.n_inpoints).from_address(C.addressof(e.inpoints.contents))
            raw._owner = owner
            idx = np.frombuffer(raw, dtype=np.int64)
        else:
            idx = np.zeros(0, dtype=np.int64)
        es = ExtractedShape(shape_from_c(e.shape), idx)
        es.score_E, es.iteration, es.c_shape = e.score_E, e.iteration, L.Shape.from_buffer_copy(bytes(e.shape))
        extracted.append(es)
    if extents and res.n_shapes > 0:
        ext = (L.Extent * res.n_shapes)()
        check(lib().rh_result_extents(pc._h, C.byref(res), ext))
        for es, e in zip(extracted, ext):
            es.extent = Extent(e)
    stats = {"iterations": res.iterations, "candidates_scored": res.candidates_scored,
             "scored_left": res.scored_left, "seconds": res.seconds, "seconds_score": res.seconds_score,
             "seconds_extract": res.seconds_extract, "seconds_host": res.seconds_host,
             "seconds_to_last_extraction": res.seconds_to_last_extraction, "draws": rng.draws}
    del owner
    seconds = stats["seconds"]
    return (extracted, seconds, stats) if return_stats else (extracted, seconds)


# ------------------------------------------ parameter-space bitmap (dormant) ----
def largestconncomp(bimage, indmap=None, connectivity="default", device=0):
    """largestconncomp(bimage, indmap, conn) (parameterspacebitmap.jl:69-109).  bimage[x, y];
    connectivity "default" (4) or "eight".  Returns the indmap entries of the largest component
    (or 0-based column-major linear indices when indmap is None)."""
    conn8 = {"default": 0, "eight": 1, 4: 0, 8: 1, False: 0, True: 1}[connectivity]
    bm = np.asarray(bimage, dtype=np.uint8)
    xs, ys = bm.shape
    flat = np.ascontiguousarray(bm.reshape(-1, order="F"))
    out = np.zeros(max(1, flat.size), dtype=np.int64)
    n = C.c_int64()
    check(lib().rh_largestconncomp(_p(flat, C.c_uint8), xs, ys, conn8, device, _p(out, C.c_int64), out.size, C.byref(n)))
    lin = out[: n.value].copy()
    if indmap is None:
        return lin
    res = []
    for li in lin:
        v = indmap[int(li) % xs][int(li) // xs]
        res.extend(v if isinstance(v, (list, tuple, np.ndarray)) else [v])
    return res


def bitmapparameters(parameters, compatibility, beta, idsource=None):  # parameterspacebitmap.jl:12-60
    prm = _f64(parameters).reshape(-1, 2)
    comp = np.ascontiguousarray(compatibility, dtype=np.uint8)
    n = prm.shape[0]
    assert n == comp.size and (idsource is None or len(idsource) == n), "Everything must have the same length."
    ids = None if idsource is None else np.ascontiguousarray(idsource, dtype=np.int64)
    xs, ys, bx, by = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
    idp = None if ids is None else _p(ids, C.c_int64)
    check(lib().rh_bitmapparameters(_p(prm, C.c_double), _p(comp, C.c_uint8), idp, n, beta, C.byref(xs), C.byref(ys),
                                    C.byref(bx), C.byref(by), None, None))
    bitmap = np.zeros(xs.value * ys.value, dtype=np.uint8)
    idxmap = np.zeros(xs.value * ys.value, dtype=np.int64)
    check(lib().rh_bitmapparameters(_p(prm, C.c_double), _p(comp, C.c_uint8), idp, n, beta, C.byref(xs), C.byref(ys),
                                    C.byref(bx), C.byref(by), _p(bitmap, C.c_uint8), _p(idxmap, C.c_int64)))
    shp = (xs.value, ys.value)
    return bitmap.reshape(shp, order="F").astype(bool), idxmap.reshape(shp, order="F"), (bx.value, by.value)
