/*
 * ransac_hip.h -- C ABI of libransac_hip.so: the MI355X-native (gfx950, HIP)
 * replacement for the data-parallel hot path of cserteGT3/RANSAC.jl v0.6.0.
 *
 * The reference has no FFI; its boundary is Julia multiple dispatch on
 * FittedShape subtypes (src/fitting.jl:8-66).  Each entry point below names the
 * reference function it replaces (paths under /root/reference).  A Julia
 * `ccall` shim (julia/RANSACHIP.jl) or any FFI binds these.
 *
 * Conventions
 *  - every call returns int: 0 = ok, negative = error (RH_E_*); the message is
 *    available from rh_last_error() on the calling thread;
 *  - the caller allocates every output; the library never keeps a host pointer
 *    past the call and never calls back into the host runtime (GC-safe);
 *  - point indices cross the boundary 1-based int64, like `inpoints::Vector{Int}`
 *    (src/fitting.jl:81-84);
 *  - enabled bits use BitVector's layout: uint64 chunks, bit i%64 of chunk i/64,
 *    LSB first (src/octree.jl:42);
 *  - one host thread per rh_cloud at a time; calls are synchronous unless the
 *    name ends in _dev (those enqueue on the cloud's HIP stream);
 *  - all arithmetic is IEEE binary64 in the reference's operation order
 *    (no FMA contraction), so inlier sets are bit-identical to the CPU path.
 *  - there is NO CPU fallback: without a usable HIP device every cloud call
 *    fails with RH_E_NODEVICE.
 */
#ifndef RANSAC_HIP_H
#define RANSAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RH_VERSION 125

enum {
    RH_OK = 0,
    RH_E_INVALID = -1,   /* bad argument (the reference would hit an @assert) */
    RH_E_NODEVICE = -2,  /* no HIP device / HIP runtime error */
    RH_E_NOMEM = -3,     /* out of device, pinned or host memory: every entry says so (a failed allocation is never RH_E_NODEVICE) */
    RH_E_CAPACITY = -4,  /* caller-provided output too small; *n_out holds the needed size */
    RH_E_INTERNAL = -5,
};

/* shape kinds */
enum { RH_PLANE = 0, RH_SPHERE = 1, RH_CYLINDER = 2, RH_CONE = 3 };

/* POD candidate = the reference's FittedShape structs flattened:
 *   RH_PLANE    FittedPlane    (src/shapes/plane.jl:8-11)     v[0..2]=point  v[3..5]=normal
 *   RH_SPHERE   FittedSphere   (src/shapes/sphere.jl:9-13)    v[0..2]=center v[3]=radius
 *   RH_CYLINDER FittedCylinder (src/shapes/cylinder.jl:11-16) v[0..2]=axis   v[3..5]=center v[6]=radius
 *   RH_CONE     FittedCone     (src/shapes/cone.jl:11-19)     v[0..2]=apex   v[3..5]=axis   v[6]=opang
 *                              v[7]=cos(-opang/2), v[8]=sin(-opang/2): computed by the HOST
 *                              (the reference evaluates them in rodrigues, src/utilities.jl:21-22);
 *                              rh_shape_finalize fills them with fdlibm-algorithm kernels (det_math.h: the
 *                              same bits on host and device, <= 1 ulp from any libm).
 * `outwards` is the Bool field of sphere/cylinder/cone; ignored for planes. */
typedef struct {
    int32_t kind;
    int32_t outwards;
    double v[10];
} rh_shape;

enum { RH_SCORE_INT64_WRAP = 0, RH_SCORE_F64 = 1 };
enum { RH_S_LENGTHC = 1, RH_S_ALLCAND = 2, RH_S_NOFMINSET = 3 };

/* Parameters = the reference's nested NamedTuple (src/utilities.jl:332-399 and the
 * defaultshapeparameters of each shape file), flattened.  Per-kind arrays are
 * indexed by RH_* kind.  cos_alpha[] / cos_parallelthr are thresholds computed by
 * the host (rh_params_finalize uses the C libm). */
typedef struct {
    double eps[4];             /* <shape>.eps  */
    double alpha[4];           /* <shape>.alpha (rad) */
    double cos_alpha[4];       /* cos(alpha): isparallel, src/utilities.jl:115-117 */
    double collin_threshold;   /* common.collin_threshold */
    double parallelthrdeg;     /* common.parallelthrdeg */
    double cos_parallelthr;    /* cosd(parallelthrdeg) */
    double sphere_par;         /* sphere.sphere_par */
    double minconeopang;       /* cone.minconeopang */
    double prob_det;           /* iteration.prob_det */
    int64_t tau;               /* iteration.tau */
    int64_t itermax;           /* iteration.itermax */
    int32_t drawN;             /* iteration.drawN */
    int32_t minsubsetN;        /* iteration.minsubsetN */
    int32_t extract_s;         /* iteration.extract_s  (RH_S_*) */
    int32_t terminate_s;       /* iteration.terminate_s */
    int32_t n_shape_types;
    int32_t shape_types[8];    /* iteration.shape_types as RH_* kinds, in order */
    int32_t score_mode;        /* RH_SCORE_INT64_WRAP = the reference's wrapping Int64 product
                                  (src/confidenceintervals.jl:54,72); RH_SCORE_F64 = fixed */
    int32_t sphere_uses_enabled; /* 0 = reference behaviour (src/shapes/sphere.jl:121,131) */
    int32_t sampling_streams;  /* 0 = one sequential random stream (the reference's structure, host-side
                                  sampling); 1 = one stream per (iteration, minimal set), a pure function
                                  of (seed, k, j): sampling + plane/sphere/cylinder fits run on the device */
    int32_t octree_sampling;   /* 0 = every minimal set from the root cell: the reference's live behaviour
                                  (constructor bug); 1 = what docs/src/ransac.md:73-96 describes:
                                  a level is drawn from the level distribution and the other points come from
                                  the first point's cell at that level (linear Morton octree; needs
                                  sampling_streams = 1) */
    int32_t octree_max_depth;  /* depth cap of the linear octree (default 10) */
} rh_params;

typedef struct rh_cloud rh_cloud;

/* ---- library ---- */
int rh_version(void);
const char *rh_last_error(void);
int rh_device_count(int *n_out);

/* ---- parameters (src/utilities.jl:332-399; RANSAC.jl:94) ---- */
void rh_default_params(rh_params *p);
void rh_params_finalize(rh_params *p);
void rh_shape_finalize(rh_shape *s);

/* ---- cloud: replaces RANSACCloud (src/octree.jl:37-59, ctors :78-138) ----
 * xyz_aos / nrm_aos: n x 3 doubles, i.e. Julia's Vector{SVector{3,Float64}} memory
 * as is; subset1_idx_1based: pc.subsets[1] (the only subset the reference scores,
 * src/iterations.jl:95).  Transposes to SoA in HBM, stores subset 1 contiguously in
 * subset order; all points start enabled (src/octree.jl:84). */
int rh_cloud_create(const double *xyz_aos, const double *nrm_aos, int64_t n,
                    const int64_t *subset1_idx_1based, int64_t s, int device, rh_cloud **out);
/* RANSACCloud(...; force_eltype = Float32) (src/octree.jl:102-109): xyz_aos / nrm_aos are Julia's
 * Vector{SVector{3,Float32}} memory as is.  On such a cloud rh_score_batch(_dev), rh_refit, rh_invalidate,
 * rh_select_enabled and the enabled-bit calls work and every per-point operation is a binary32 operation (the shapes'
 * fields are rounded to binary32 on entry; rh_shape_finalize_f32 prepares a Float32 shape: fields rounded, the cone's
 * cos / sin as binary32); eps and cos_alpha stay doubles and are compared after exact promotion, like Julia compares a
 * Float32 with a Float64.  rh_ransac runs on such a cloud too (rh_ransac_f32), all four kinds; rh_refit_lsq is Float64-only. */
int rh_cloud_create_f32(const float *xyz_aos, const float *nrm_aos, int64_t n,
                        const int64_t *subset1_idx_1based, int64_t s, int device, rh_cloud **out);
void rh_shape_finalize_f32(rh_shape *s);
int rh_cloud_destroy(rh_cloud *c);
int rh_cloud_info(const rh_cloud *c, int64_t *n, int64_t *s, int *device);
/* pc.isenabled (BitVector.chunks) in / out; nchunks must be ceil(n/64) */
int rh_cloud_set_enabled(rh_cloud *c, const uint64_t *chunks, int64_t nchunks);
int rh_cloud_get_enabled(rh_cloud *c, uint64_t *chunks, int64_t nchunks);
int rh_cloud_enable_all(rh_cloud *c);                   /* ransac(pc, params, true): src/iterations.jl:14-21 */
int rh_cloud_count_enabled(rh_cloud *c, int64_t *out);  /* count(pc.isenabled): src/iterations.jl:75 */

/* ---- hot path ---- */

/* Replaces scorecandidates! (src/fitting.jl:181-190) = B x scorecandidate
 * (plane.jl:61-71, sphere.jl:118-134, cylinder.jl:172-183, cone.jl:155-167) with one
 * batched launch for all candidates of all kinds.  counts_out[b] = number of compatible (and, except
 * for spheres in reference mode, enabled) points of subset 1.  masks_out (optional):
 * b rows of ceil(s/64) words; bit j of row i = subset position j is an inpoint of
 * candidate i, so inpoints = subsets[1][mask] in subset order. */
int rh_score_batch(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p,
                   int32_t *counts_out, uint64_t *masks_out_or_null);

/* Same, all buffers resident in HBM on the cloud's device, enqueued on the cloud's
 * stream without synchronising (bench / multi-GPU plumbing). d_counts must hold b
 * int32 (overwritten). */
int rh_score_batch_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p,
                       int32_t *d_counts, uint64_t *d_masks_or_null);

/* Replaces refit (plane.jl:137-143, sphere.jl:179-190, cylinder.jl:228-234,
 * cone.jl:176-182): all enabled compatible points of the WHOLE cloud, ascending
 * 1-based.  If more than cap are found returns RH_E_CAPACITY with *n_out = needed. */
int rh_refit(rh_cloud *c, const rh_shape *shape, const rh_params *p,
             int64_t *idx_out_1based, int64_t cap, int64_t *n_out);

/* ---- the largest connected patch of a refit set (Schnabel et al. 2007, section 4.4; no live counterpart in the reference,
 *      whose parameterspacebitmap.jl is dead code) ----
 * rh_refit returns every enabled compatible point of the whole cloud: two coplanar table tops come out as one plane.
 * rh_refit_component keeps the largest connected component of that set, with connectivity on a 3-D voxel grid:
 *  1. I = the set rh_refit returns for (cloud, shape, params).  Its points are finite (a NaN or inf fails the distance test);
 *  2. o = the componentwise minimum of the coordinates over I (binary64; on a Float32 cloud the floats promoted exactly);
 *  3. the cell of point i is (floor((x_i - o_x) / beta), floor((y_i - o_y) / beta), floor((z_i - o_z) / beta)): IEEE
 *     binary64 subtraction and division, no contraction, floor, then integers.  beta must be finite and > 0, and no axis may
 *     have more than 2^20 cells: RH_E_INVALID otherwise;
 *  4. two occupied cells are adjacent when every coordinate differs by at most 1 (conn26 != 0), or, with conn26 = 0, when
 *     exactly one coordinate differs by exactly 1;
 *  5. a component is a maximal set of occupied cells joined by adjacency; its size is its number of POINTS, not of cells;
 *     the largest wins, and among equals the one that holds the smallest point index;
 *  6. the result is the points of I in the winning component, ascending and 1-based like rh_refit's.  An empty I gives
 *     an empty result and RH_OK.
 * The same list on every run and under either refit_path; the enabled bits are not changed.  *n_out = the size of the
 * winning component (RH_E_CAPACITY when it exceeds cap, like rh_refit); optional: *n_refit_out = |I|, *n_components_out =
 * the number of components.  Works on Float64 and Float32 clouds; RH_E_INVALID on clouds of 2^31 points or more. */
int rh_refit_component(rh_cloud *c, const rh_shape *shape, const rh_params *p, double beta, int32_t conn26,
                       int64_t *idx_out_1based, int64_t cap, int64_t *n_out,
                       int64_t *n_refit_out_or_null, int32_t *n_components_out_or_null);
/* The same filter as a step of rh_ransac / rh_ransac_f32: with beta > 0 every extraction takes only the winning component
 * of the best candidate's refit set -- only those points reach inpoints and are invalidated; the rest of the set stays
 * enabled, so the second table top can be found as a shape of its own.  beta <= 0: off (the default; an extraction's
 * launches are then exactly those of a cloud that never had a filter).  The setting lives on the cloud (rh_params mirrors
 * the reference's parameters).  rh_ransac_mp returns RH_E_INVALID while a filter is set.  A NaN or infinite beta:
 * RH_E_INVALID.  The getter reports beta = 0 for "off". */
int rh_cloud_set_component_filter(rh_cloud *c, double beta, int32_t conn26);   /* beta <= 0: off (the default) */
int rh_cloud_get_component_filter(const rh_cloud *c, double *beta_out, int32_t *conn26_out);

/* ---- oriented extents and fit residuals of extracted shapes (no live counterpart in the reference: its findOBB_,
 *      src/orientedbox_.jl, is unexported and unused, and toDict / exportJSON write the bare parameters) ----
 * rh_ransac returns unbounded primitives with index lists.  These calls add, for b shapes at once, the frame each
 * shape's points suggest, the box of the points in that frame, and how far the points sit from the shape.
 * Shape j's points are idx[offsets[j] .. offsets[j+1]): 1-based indices into the cloud, in any order, duplicates counted
 * as given.  The cloud's resident coordinates are read (a Float32 cloud's floats promoted exactly); every operation below
 * is an IEEE binary64 operation, none contracted.  Nothing on the cloud changes (enabled bits, refit state, ...).
 *  1. invalid input -- RH_E_INVALID: offsets[0] != 0, decreasing offsets, (the _dev entry: offsets[b] != total,) an index
 *     outside 1..N, a listed point with a non-finite coordinate, a kind outside 0..3, a plane / cylinder / cone whose
 *     axis has norm 0 or a non-finite norm.  Indices are checked on the device before anything is read through them; the
 *     kernels raise a flag word the host entries read back with the results, and every record of such a call carries
 *     RH_EXT_INVALID (what a caller of the _dev entry can test).  b == 0: RH_OK;
 *  2. moments: p0 = the first listed point, q_i = p_i - p0, m = sum q_i / n, S = sum q_i q_i^T / n - m m^T,
 *     centroid = p0 + m (sums in a fixed order that depends on the list's length alone);
 *  3. frame (rows u, v, w).  a = the plane's normal / the cylinder's axis / the cone's axis;
 *     w = a / sqrt((ax*ax + ay*ay) + az*az), component by component; u = the unit eigenvector of the largest eigenvalue
 *     of (I - w w^T) S (I - w w^T), made orthogonal to w again and normalised, its component of largest magnitude
 *     positive (the first one on a tie); v = w x u; lambda[0] >= lambda[1] the two in-plane eigenvalues, lambda[2] = 0.
 *     Spheres: u, v = the eigenvectors of the two largest eigenvalues of S, each with that sign rule, w = u x v, lambda =
 *     the three eigenvalues, descending.  When lambda[0] is not positive (one point, coincident points):
 *     RH_EXT_NO_DIRECTION, and with k the index of the smallest |w_k| (the first on a tie) u = e_k - w (w . e_k),
 *     normalised; for spheres the frame is the identity.  A nearly isotropic scatter (a full cylinder) gets whatever
 *     orthonormal frame the solver yields: lambda tells;
 *  4. extents: d = p_i - origin componentwise (origin: the plane's point, the sphere's or the cylinder's center, the
 *     cone's apex); the coordinate along a frame row f is t = (dx*fx + dy*fy) + dz*fz; lo / hi = the minima / maxima of
 *     (tu, tv, tw) over the listed points;
 *  5. distance: plane e = tw; sphere e = sqrt((tu*tu + tv*tv) + tw*tw) - r; cylinder e = sqrt(tu*tu + tv*tv) - r; cone
 *     e = sqrt(tu*tu + tv*tv)*v[7] + tw*v[8] (rh_shape_finalize's cos and sin of -opang/2);
 *     dist_maxabs = max |e_i|, dist_rms = sqrt(sum e_i^2 / n);
 *  6. an empty list: RH_EXT_EMPTY, kind and origin set, everything else zero.
 * Steps 4 to 6 are exact given the frame (lo, hi, dist_maxabs: the very bits; dist_rms: a sum in a fixed order).  The
 * same bits on every run, and for a shape whether it is passed alone or among others. */
enum { RH_EXT_EMPTY = 1, RH_EXT_NO_DIRECTION = 2, RH_EXT_INVALID = 4 };
typedef struct {
    int64_t n;               /* listed points */
    int32_t kind;            /* copy of the shape's kind */
    int32_t flags;           /* RH_EXT_* */
    double origin[3];        /* plane: point; sphere: center; cylinder: center; cone: apex */
    double frame[9];         /* rows u, v, w: orthonormal, right-handed (w = u x v) */
    double lo[3], hi[3];     /* min / max over the points of their coordinates along u, v, w, measured from origin */
    double centroid[3];
    double lambda[3];        /* scatter along u, v (and w for spheres; 0 otherwise) */
    double dist_rms, dist_maxabs;   /* signed distance to the shape: root mean square, largest magnitude */
} rh_extent;
/* host arrays in and out; one wait */
int rh_shape_extents(rh_cloud *c, const rh_shape *shapes, int32_t b,
                     const int64_t *offsets /* b + 1 */, const int64_t *idx_1based, rh_extent *out);
/* everything resident on the cloud's device, enqueued on the cloud's stream without synchronising: four launches.
 * total = offsets[b] = the number of entries of d_idx_1based (the host cannot read the offsets; the grid is sized by it) */
int rh_shape_extents_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const int64_t *d_offsets,
                         const int64_t *d_idx_1based, int64_t total, rh_extent *d_out);

/* ---- every point labelled with its nearest compatible shape (no counterpart in the reference, whose extraction is
 *      greedy: a point on two shapes stays with the one extracted first, src/iterations.jl:124-140) ----
 * n points with optional normals, b shapes in the caller's order (0 <= b <= RH_ASSIGN_MAX_SHAPES) and finalised
 * parameters, of which eps[kind] and cos_alpha[kind] are used.
 *  1. for point i and shape j, (d_ij, t_ij) are the two compared quantities of the reference's compatibles* test
 *     (plane.jl:114-130, sphere.jl:144-172, cylinder.jl:194-221, cone.jl:132-153): d the distance side --
 *     |dot(o_z, p - point)|, |norm(p - o) - R|, |norm(curr_norm) - R|, |dist| of project2cone --, t the angle side.
 *     IEEE binary64 operations in the reference's order, none contracted: the bits the score and refit kernels compare;
 *  2. shape j claims point i when d_ij < eps[kind_j] and t_ij > cos_alpha[kind_j] -- rh_refit's predicate.  Without
 *     normals (nrm_aos_or_null = NULL) or with RH_ASSIGN_NO_NORMALS the distance half alone decides.  A NaN fails every
 *     comparison: a point with a non-finite coordinate, or a shape with a zero axis, claims nothing, and no validation
 *     pass is needed for them;
 *  3. label[i] = j + 1 for the claiming shape of smallest d_ij, among equal d the smallest j in the caller's order;
 *     label[i] = 0 when no shape claims the point.  int32;
 *  4. dist[i] (optional) = d_ij of the winner, -1.0 for label 0;
 *  5. counts[0 .. b] (optional, int64): counts[0] = the unlabelled points, counts[j + 1] = the points of shape j;
 *  6. lists (optional; offsets[b + 2] and idx[n], both or neither): the 1-based indices of the points grouped by label,
 *     label 0 first, ascending within each group; offsets[k] .. offsets[k + 1] is label k's run and offsets[b + 1] = n:
 *     the stable partition of 1 .. n by label.  idx[offsets[j + 1] .. offsets[j + 2]) is shape j's list as
 *     rh_shape_extents takes it;
 *  7. Float32 input (the _f32 entry, a Float32 cloud) is promoted exactly and tested in binary64, the shapes taken as
 *     given.  On a Float32 cloud a point within rounding of a threshold can therefore be claimed differently than by
 *     rh_refit, whose tests run in binary32: one definition for both element types;
 *  8. the cloud entries with RH_ASSIGN_ENABLED_ONLY: a disabled point gets label 0 and dist -1 whatever its geometry.
 *     Nothing on the cloud changes;
 *  9. the same bits on every run; a point's label and dist do not depend on which other points are in the call.
 * RH_E_INVALID, checked on the host before the first device call: b outside 0 .. 1024, a kind outside 0 .. 3 (host
 * shapes; a device-resident shape of another kind claims nothing), n < 0 or n >= 2^31, a null required pointer, one of
 * offsets / idx without the other, unknown flag bits, RH_ASSIGN_ENABLED_ONLY on the raw-array entries.  b == 0: every
 * label 0, counts[0] = n, RH_OK.  n == 0: RH_OK.
 * The raw-array entries (the scan that was thinned before detection: no rh_cloud needed) upload the arrays whole --
 * 24 or 48 bytes per point in binary64, half that in binary32 -- and return RH_E_NOMEM when they do not fit. */
enum { RH_ASSIGN_NO_NORMALS = 1, RH_ASSIGN_ENABLED_ONLY = 2 };
#define RH_ASSIGN_MAX_SHAPES 1024
int rh_assign_points(const double *xyz_aos, const double *nrm_aos_or_null, int64_t n, const rh_shape *shapes, int32_t b,
                     const rh_params *p, int32_t flags, int device, int32_t *labels_out, double *dist_out_or_null,
                     int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null);
int rh_assign_points_f32(const float *xyz_aos, const float *nrm_aos_or_null, int64_t n, const rh_shape *shapes, int32_t b,
                         const rh_params *p, int32_t flags, int device, int32_t *labels_out, double *dist_out_or_null,
                         int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null);
/* the cloud's resident coordinates (Float64 or Float32 cloud), host arrays out, one wait */
int rh_cloud_assign(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, int32_t flags, int32_t *labels_out,
                    double *dist_out_or_null, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
                    int64_t *idx_out_or_null);
/* everything resident on the cloud's device, enqueued on the cloud's stream without synchronising and without a host
 * read-back: d_labels[n], d_dist[n], d_counts[b + 1], d_offsets[b + 2], d_idx[n] */
int rh_cloud_assign_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p, int32_t flags,
                        int32_t *d_labels, double *d_dist_or_null, int64_t *d_counts_or_null, int64_t *d_offsets_or_null,
                        int64_t *d_idx_or_null);

/* Least-squares refit -- the step of the paper the reference leaves out (docs/src/ransac.md:163-168;
 * its `refit` returns the shape unchanged).  NOT part of parity runs.  Selects the enabled points
 * compatible with `shape` at 3*eps, then fits: plane = total least squares; sphere / cylinder / cone
 * = Gauss-Newton on the geometric distance (normal equations accumulated on the device with f64
 * MFMA, solved on the host).  rms = root mean square distance of the selected points (for the
 * iterative kinds: before the last step). */
int rh_refit_lsq(rh_cloud *c, const rh_shape *shape, const rh_params *p, int32_t max_iter, rh_shape *out,
                 int64_t *n_used, double *rms, int32_t *iters_done);

/* Replaces invalidate_indexes! (src/fitting.jl:197-202). */
int rh_invalidate(rh_cloud *c, const int64_t *idx_1based, int64_t n);

/* Replaces the enabled-cell gather of samplepointcloud4! (src/fitting.jl:405-407,
 * 415-422) for the root cell: idx_out[i] = the ranks[i]-th enabled point (1-based
 * rank, ascending index order), 0 if the rank is out of range. */
int rh_select_enabled(rh_cloud *c, const int64_t *ranks_1based, int32_t k, int64_t *idx_out_1based);

/* ---- host-side pieces of the plugin API (O(1) per minimal set) ---- */

/* fit(::Type{T}, p, n, pc, params) (plane.jl:33-57, sphere.jl:87-114,
 * cylinder.jl:135-168, cone.jl:123-128).  p, n: lp x 3 AoS.  *fitted = 0 is the
 * reference's `nothing`. */
int rh_fit(int kind, const double *p, const double *n, int32_t lp, const rh_params *prm,
           rh_shape *out, int32_t *fitted);
/* The same on the points of a Float32 cloud (RANSACCloud(...; force_eltype = Float32), octree.jl:102-109: p[i], n[i] are
 * SVector{3,Float32}, so plane.jl:33-57 / sphere.jl:29-114 / cylinder.jl:34-168 run in Float32 and return Float32 shapes;
 * the parameters stay what the caller made them, utilities.jl:488-503).  p, n carry the Float32 values as doubles.
 * RH_CONE (round 5): cone.jl:39-61 + 87-128 in binary32 -- rank() and \ of a Matrix{Float32} (LAPACK's single-precision
 * SVD and LU upstream) are a one-sided Jacobi SVD and an LU with partial pivoting in float here, acos / cos / sin the
 * deterministic double kernels rounded once: like the Float64 cone fit a restatement the reference cannot pin (it holds no
 * cone fixture); held bit for bit against the oracle's own binary32 twin. */
int rh_fit_f32(int kind, const double *p, const double *n, int32_t lp, const rh_params *prm,
               rh_shape *out, int32_t *fitted);

/* forcefitshapes! (src/fitting.jl:165-173) for the k minimal sets of an iteration in one call (what rh_sample_sets drew):
 * fit(T, ...) for every type of p->shape_types, in that order, on every set with ok[j] != 0 (ok = NULL: every set); the shapes
 * that fit are appended to shapes_out in (set, type) order -- the reference's candidate order -- with set_out[i] = the set a
 * shape came from.  xyz_aos / nrm_aos: the cloud's host arrays (n x 3 doubles; for f32 != 0 they hold a Float32 cloud's values
 * and the fits run in binary32, rh_fit_f32).  drawN: 3 .. 16, else RH_E_INVALID: every type's fit is given all drawN points
 * and fit_plane reads three of them (rh_sample_sets also draws sets of two).  Host-side, O(1) per set.  RH_E_CAPACITY with
 * *n_out = the needed size. */
int rh_fit_sets(const double *xyz_aos, const double *nrm_aos, const int64_t *idx_1based, const int32_t *ok_or_null, int32_t k,
                int32_t drawN, const rh_params *p, int32_t f32, rh_shape *shapes_out, int32_t *set_out_or_null, int32_t cap,
                int32_t *n_out);

/* estimatescore / ConfidenceInterval (src/confidenceintervals.jl:71-74, 53-59, 1-6) */
int rh_estimatescore(int64_t S1length, int64_t Plength, int64_t sigma, int32_t score_mode,
                     double *ci_min, double *ci_max, double *ci_E);
/* prob(n, s, N, k) (src/utilities.jl:262) */
double rh_prob(double n, int64_t s, int64_t N, int64_t k);

/* ---- driver: replaces ransac(pc, params) (src/iterations.jl:35-162) ---- */
typedef struct {
    uint64_t s[4];           /* xoshiro256++ state (rh_rng_seed) */
    const uint64_t *stream;  /* optional injected raw 64-bit draws, consumed first */
    int64_t stream_len, stream_pos;
    int64_t draws;
} rh_rng;
void rh_rng_seed(rh_rng *r, uint64_t seed);
/* rand(1:n) = 1 + floor(next * n / 2^64) */
int64_t rh_rng_range(rh_rng *r, int64_t n);

/* samplepointcloud4!(pc, ..) (src/fitting.jl:383-430) k times in a row, as ONE launch: what the reference's loop does once
 * per minimal set (iterations.jl:80-99) -- first point by rejection on rand(1:n) (:388-395), the other drawN - 1 as the
 * rand(1:count)-th enabled point of the root cell with one redraw when it repeats the first (:414-423), reject when two
 * coincide (:425-428).  The draws are the caller's generator's (an injected stream first), consumed exactly as k sequential
 * calls would consume them -- same number, same order -- so a loop that samples a whole iteration's sets through this call
 * takes the same decisions as one that calls rh_rng_range / rh_select_enabled per point (the device evaluates the call
 * for every start position of a window of draws, the host follows the chain).  idx_out: k x drawN points (1-based);
 * ok_out[j]: the reference's first return value; level_out (optional): its second where a set was drawn (1: every set comes
 * from the root cell), and 0 with ok = 0.  One DEVIATION: for a set rejected because its points are not all
 * different the reference returns (false, 1) (fitting.jl:427), and (false, 0) only where fewer than drawN points are
 * enabled (:408); here level_out is 0 in both cases.  Nothing reads the level of a rejected set (iterations.jl:82 skips
 * it).  drawN: 2 .. 16 -- the draws need two points; rh_fit_sets, which fits what this call drew, takes 3 .. 16 (a plane is
 * fitted to three points).  RH_E_INVALID without an enabled point (the reference would draw for ever). */
int rh_sample_sets(rh_cloud *c, int32_t drawN, rh_rng *rng, int32_t k, int64_t *idx_out_1based, int32_t *ok_out,
                   int32_t *level_out_or_null);

typedef struct {
    rh_shape shape;
    int64_t n_inpoints;
    int64_t *inpoints;       /* ascending, 1-based; points into the result's arena (rh_result_free) */
    double score_E;
    int64_t iteration;
} rh_extracted;              /* ExtractedShape, src/fitting.jl:81-84 */

typedef struct {
    rh_extracted *shapes;
    int64_t n_shapes;
    int64_t iterations;
    int64_t candidates_scored;
    int64_t scored_left;
    double seconds;          /* wall time of the loop (src/iterations.jl:46,159; not truncated) */
    double seconds_score;    /* device time in score launches + count read-back */
    double seconds_extract;  /* refit + invalidate + candidate liveness */
    double seconds_host;     /* sampling + fit + bookkeeping */
    double seconds_to_last_extraction;   /* wall time from the start of the loop to the end of the last extraction (0: none) */
    void *arena;             /* internal: the pinned host block that holds every inpoints list */
} rh_result;

/* xyz_aos / nrm_aos: the same host arrays given to rh_cloud_create (read for the
 * minimal-set fits only).  The cloud's enabled bits are updated in place, like
 * pc.isenabled. */
int rh_ransac(rh_cloud *c, const double *xyz_aos, const double *nrm_aos, const rh_params *p,
              rh_rng *rng, rh_result *out);
/* ransac(pc, params) on a Float32 cloud (rh_cloud_create_f32; octree.jl:102-109): the minimal-set fits (plane.jl:33-57,
 * sphere.jl:29-114, cylinder.jl:34-168), scoring, candidate liveness and refit all run in binary32, the thresholds stay
 * what the caller made them (utilities.jl:488-503); extracted shapes hold binary32 numbers (cones included: rh_fit_f32).
 * rh_ransac itself accepts such a cloud when handed
 * the Float32 values as doubles; this entry takes Julia's Vector{SVector{3,Float32}} memory as is. */
int rh_ransac_f32(rh_cloud *c, const float *xyz_aos, const float *nrm_aos, const rh_params *p,
                  rh_rng *rng, rh_result *out);
void rh_result_free(rh_result *r);
/* rh_shape_extents (above) of a result's own shapes and index lists, one call for all of them; the lists are uploaded
 * from the result's pinned block */
int rh_result_extents(rh_cloud *c, const rh_result *r, rh_extent *out /* r->n_shapes */);

/* ---- one scene on several GPUs of a node (no counterpart in the reference, which is single-threaded:
 *      src/iterations.jl:35-162 run by `world` processes, one per GPU) ----
 * rh_mp_open is collective: every rank calls it with the same name (a POSIX shared-memory name, "/..."), rank 0
 * creates the segment.  slot_bytes bounds one rank's candidate list of one window (<= 0: 1 MiB).  rh_ransac_mp:
 * every rank holds a replica of the cloud in the same state and passes the same parameters and seed; the minimal sets
 * of every iteration are dealt round-robin to the ranks, the ranks exchange their windows' candidate lists through
 * the segment, and every rank returns exactly what rh_ransac returns for the same inputs.  Float64 clouds only
 * (RH_E_INVALID on a Float32 cloud: that combination has never been held against the single-GPU run). */
typedef struct rh_mp rh_mp;
int rh_mp_open(const char *shm_name, int32_t rank, int32_t world, int64_t slot_bytes, rh_mp **out);
int rh_mp_close(rh_mp *m);
/* the exchange on its own: every rank contributes `bytes` bytes (the same number everywhere), out gets world x bytes in
 * rank order; host memory only */
int rh_mp_allgather(rh_mp *m, const void *payload, int64_t bytes, void *out);
int rh_ransac_mp(rh_cloud *c, const double *xyz_aos, const double *nrm_aos, const rh_params *p,
                 rh_rng *rng, rh_mp *mp, rh_result *out);

/* ---- parameter-space bitmap + largest connected component
 *      (src/parameterspacebitmap.jl:12-60, 69-109; dead code upstream) ----
 * bitmap: xs*ys bytes, column-major like a Julia BitMatrix (pixel [x,y] at x + xs*y,
 * 0-based).  conn8 = 0: 4-connectivity (`1:ndims`), 1: `trues(3,3)`.  Writes the
 * 0-based linear indices (ascending) of the largest component. */
int rh_largestconncomp(const uint8_t *bitmap, int32_t xs, int32_t ys, int32_t conn8, int device,
                       int64_t *out, int64_t cap, int64_t *n_out);
int rh_bitmapparameters(const double *params2d, const uint8_t *compat, const int64_t *idsource_or_null,
                        int64_t n, double beta, int32_t *xs, int32_t *ys, double *betax, double *betay,
                        uint8_t *bitmap_or_null, int64_t *idxmap_or_null);

/* ---- measurement plumbing (bench.py): HIP events on the cloud's stream ---- */
/* rh_score_batch_dev twice, bracketed by HIP events on the cloud's stream: first the way
 * rh_score_batch_dev runs it (one kernel for all kinds) -> ms_out[4]; then one launch per kind
 * with an event before each and after the last -> ms_out[0..3] (0 for kinds without candidates
 * ~ an empty launch).  Waits for the batch.  ms_out[0] < 0 on entry: the first form only
 * (profiling passes that must see the product's launches alone). */
/* (a launch that takes super-tile lists, "st_cull": ms_out[4] is the score launch alone; the list launch in front of it is
 * returned by rh_last_list_launch_ms after the call, 0 when the launch took none) */
int rh_last_list_launch_ms(rh_cloud *c, float *ms_out);
int rh_score_batch_dev_timed(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p,
                             int32_t *d_counts, uint64_t *d_masks_or_null, float *ms_out /* [5] */);
/* device time of the most recent rh_refit on this cloud: the full-cloud scan kernel and the
 * compaction (popcount + scan + expansion), from HIP events on the cloud's stream */
int rh_last_refit_ms(rh_cloud *c, float *ms_scan_out, float *ms_compact_out);
/* Stream the cloud's kernels and copies are enqueued on.  By default a cloud owns a non-blocking
 * stream.  use_external = 1: use the caller's hipStream_t (0 = the null stream) from now on, so the
 * caller can order its own work (a fill before, an RCCL collective after) against a
 * rh_score_batch_dev WITHOUT host synchronisation; use_external = 0: back to the own stream.
 * Waits for the work already enqueued on the previous stream.  The caller keeps the stream alive. */
int rh_cloud_set_stream(rh_cloud *c, void *hip_stream, int use_external);
int rh_timer_start(rh_cloud *c);
int rh_timer_stop(rh_cloud *c, float *ms_out); /* synchronises the stream */
int rh_cloud_sync(rh_cloud *c);
/* device allocations on the cloud's device for the *_dev entry points */
int rh_dev_alloc(rh_cloud *c, int64_t bytes, void **d_out);
int rh_dev_free(rh_cloud *c, void *d);
int rh_dev_upload(rh_cloud *c, void *d_dst, const void *h_src, int64_t bytes);
int rh_dev_download(rh_cloud *c, void *h_dst, const void *d_src, int64_t bytes);

/* ---- multi-GPU: candidate-sharded scoring with the score all-reduce inside the library ----
 * Candidates are independent (src/fitting.jl:181-190).  One process per GPU, each with a replica of the cloud; every
 * rank scores a slice of the batch, ONE RCCL all-reduce (sum, int32[b_total]) over xGMI gives every rank every count --
 * integer sums: bit-identical to one GPU.  librccl is loaded on first use (a copy already in the process is shared).
 *   rank 0:      rh_comm_unique_id(id)          ... the host program hands the 128 bytes to the other ranks ...
 *   every rank:  rh_comm_create(cloud, rank, world, id, &comm)
 *   per batch:   rh_score_batch_allreduce_dev(cloud, comm, d_my_shapes, b, offset, b_total, &params, d_counts_total)
 *                (enqueues: zero, score into [offset, offset + b), all-reduce on the communicator's own stream -- so the
 *                next batch's scoring overlaps it when the caller alternates two count buffers: a buffer may come back two
 *                calls later, the library orders that call behind the collective that read it)
 *   then:        rh_comm_fence(comm, cloud)  (the cloud's stream waits, no host sync)  or  rh_comm_sync(comm)  (host waits) */
#define RH_COMM_ID_BYTES 128
typedef struct rh_comm rh_comm;
int rh_comm_unique_id(void *id_out /* RH_COMM_ID_BYTES */);
int rh_comm_create(rh_cloud *c, int32_t rank, int32_t world, const void *unique_id, rh_comm **out);
int rh_comm_destroy(rh_comm *m);
int rh_score_batch_allreduce_dev(rh_cloud *c, rh_comm *m, const rh_shape *d_shapes, int32_t b, int32_t offset, int32_t b_total,
                                 const rh_params *p, int32_t *d_counts_total);
int rh_comm_fence(rh_comm *m, rh_cloud *c);
int rh_comm_sync(rh_comm *m);

/* wall time of the rh_cloud_create call that made the cloud, ms: [0] total, [1] the k-d leaf order of subset 1 (what
 * gives the culled score kernel its compact 64-point groups; built on the device, a radix sort per tree level --
 * RH_KD_HOST=1 keeps the host's nth_element recursion as the A/B), [2] before it (allocations, uploads, AoS -> SoA,
 * bounding box, Morton order of the cloud on the device), [3] after it (enabled bits).  RH_CREATE_PROF=1 prints the
 * stages on stderr. */
int rh_cloud_create_ms(const rh_cloud *c, double *out4);

/* ---- the reference's octree: pc.octree (src/octree.jl:237-244 buildoctree, :158-177 OctreeRefinery / needs_refinement /
 * refine_data, :187-196 iswithinrectangle, :212-230 octreedepth, :11-22 getnthcell; utilities.jl:125-136 findAABB;
 * RegionTrees' findleaf as src/fitting.jl:397 uses it; the enabled-cell gather of fitting.jl:405-407) ----
 * Cells are numbered from 0 (the root) in creation order; depth of the root is 1 (octree.jl:240).  The tree has the
 * reference's geometry with its quirks (root = Cell(minV, maxV) with maxV read as widths; vmin < p <= vmax membership;
 * refinement while a cell holds more than 8 points, stopped at depth 48: *overflow).  It never changes what ransac()
 * returns (every sample comes from the root cell) and rh_ransac does not build it. */
typedef struct rh_octree rh_octree;
int rh_octree_build(const double *xyz_aos, int64_t n, rh_octree **out);                 /* buildoctree(vertices); host-side set-up */
/* the tree of a Float32 cloud (RANSACCloud(...; force_eltype = Float32), octree.jl:102-109): findAABB, the divisions origin +
 * widths / 2, the children's widths and the vmin < p <= vmax tests are binary32 operations there, so cells and their point lists
 * can differ from the binary64 tree of the same (widened) points.  The queries below serve both kinds of tree (the geometry
 * comes back widened to double, exactly). */
int rh_octree_build_f32(const float *xyz_aos, int64_t n, rh_octree **out);
int rh_octree_destroy(rh_octree *t);
int rh_octree_info(const rh_octree *t, int32_t *n_cells, int32_t *octreedepth, int32_t *overflow);
int rh_octree_findleaf(const rh_octree *t, const double *p3, int32_t *cell_out);        /* findleaf(pc.octree, p) */
int rh_octree_getnthcell(const rh_octree *t, int32_t cell, int32_t n, int32_t *cell_out /* -1 = nothing */);
int rh_octree_node_info(const rh_octree *t, int32_t cell, double *origin3, double *widths3, int32_t *depth, int32_t *parent,
                        int32_t *children8 /* -1: a leaf */, int64_t *npoints);
int rh_octree_node_points(const rh_octree *t, int32_t cell, int64_t *idx_out_1based, int64_t cap);   /* cell.data.incellpoints */
/* cell.data.incellpoints[pc.isenabled[cell.data.incellpoints]] (fitting.jl:405-407) on the device, against cloud c's bits */
int rh_octree_cell_enabled(rh_cloud *c, rh_octree *t, int32_t cell, int64_t *idx_out_1based, int64_t cap, int64_t *n_out);

/* ---- point normals for a cloud without them (no counterpart in the reference, which starts from clouds with
 *      normals: "If normal information is not available, there are algorithms to approximate it (PCA for example)",
 *      docs/src/ransac.md:13) ----
 * For every point p_i (0-based i):
 *  1. neighbours: p_i itself first, then the other points ordered by d^2 = (dx*dx + dy*dy) + dz*dz (binary64,
 *     dx = q.x - p.x), ties to the smaller index; the first k of that order; with radius > 0 those with
 *     d^2 > radius*radius dropped.  m = what remains (1 <= m <= min(k, n));
 *  2. C = sum (q - c)(q - c)^T / m over them, c their mean (binary64); eigenvalues l0 <= l1 <= l2;
 *  3. normal = the unit eigenvector of l0; curvature = l0 / (l0 + l1 + l2);
 *  4. degenerate (m < 3, l2 == 0 or l1 <= 1e-12 * l2): normal (0, 0, 0), curvature 0, flag 1; otherwise flag 0;
 *  5. sign: the component of largest magnitude positive (the first on a tie), then
 *     orient 0: kept; 1: negated if dot(n, viewpoint - p) < 0; 2: negated if dot(n, hint_i) < 0.
 * The same bits on every run.  A zero normal never passes isparallel (src/utilities.jl:115-117), so a degenerate
 * point never becomes an inlier; the result feeds rh_cloud_create as its nrm_aos.  hints_aos_or_null: n x 3
 * (orient = 2 only).  curv / flags outputs are optional.  RH_E_INVALID: k outside 3..64, orient outside 0..2,
 * orient = 2 without hints, radius negative or not finite, a coordinate not finite, n < 1. */
typedef struct {
    int32_t k;               /* 3..64 */
    int32_t orient;          /* 0 canonical sign, 1 towards viewpoint, 2 along hints */
    double radius;           /* 0 = no limit */
    double viewpoint[3];     /* orient = 1 */
} rh_normals_params;
int rh_estimate_normals(const double *xyz_aos, int64_t n, const rh_normals_params *p, const double *hints_aos_or_null,
                        int device, double *nrm_out_aos, double *curv_out_or_null, int32_t *flags_out_or_null);
/* Julia's Vector{SVector{3,Float32}} in and out: the binary64 result on the widened coordinates, rounded once */
int rh_estimate_normals_f32(const float *xyz_aos, int64_t n, const rh_normals_params *p, const float *hints_aos_or_null,
                            int device, float *nrm_out_aos, float *curv_out_or_null, int32_t *flags_out_or_null);

/* ---- voxel-grid downsampling of a raw cloud (no counterpart in the reference, which leaves thinning to the user) ----
 * One output row per occupied cell of a grid of width beta, and the map point -> row that carries a shape found on the
 * thinned cloud back to the scan.  n points (binary64 array-of-structures; the _f32 entry widens exactly), optional normals.
 *  1. dropped: a point with a coordinate that is not finite; with normals, also one with a normal component that is not
 *     finite or exceeds 2 in magnitude.  F = the points that are left;
 *  2. o = the componentwise minimum over F;
 *  3. per axis a = (x - o) / beta (one binary64 subtraction, one division, no contraction), c = floor(a), t = a - c
 *     (exact, 0 <= t < 1), f = (uint64) floor(t * 4294967296.0).  The cell is (cx, cy, cz).  beta must be finite and
 *     positive and no axis may have more than 2^20 cells (the rule and the 21-bit key fields of rh_refit_component):
 *     RH_E_INVALID otherwise, and for n < 1 or n >= 2^31;
 *  4. the occupied cells are numbered 1 .. M by the smallest point index they hold, ascending (first-appearance order:
 *     first[] is strictly increasing);
 *  5. per row: count; first = the 1-based index of the cell's first point; the output point --
 *     mode RH_VOX_FIRST:    the first point's coordinates (and normal) copied bit for bit;
 *     mode RH_VOX_CENTROID: per axis S = sum of f over the cell in uint64 (exact, whatever the order), then
 *                           num = (double)(S >> 32) * 4294967296.0 + (double)(S & 0xFFFFFFFF)   (one rounding),
 *                           m = (num / (double)count) * 2^-32,  x = o + ((double)c + m) * beta,
 *                           each operation rounded on its own: the centroid at a resolution of beta * 2^-32;
 *  6. normals in centroid mode: per component g = llrint(n_c * 1048576.0) (the product is exact, ties to even),
 *     G = sum of g in int64 (|G| <= 2^52: (double)G is exact), len = sqrt((Gx*Gx + Gy*Gy) + Gz*Gz), output G / len per
 *     component, (0, 0, 0) when len == 0.  With flags & RH_VOX_ALIGN_NORMALS a point's g is negated before the sum when
 *     (nx*rx + ny*ry) + nz*rz < 0, r = the normal of the cell's first point (for rh_estimate_normals with orient = 0,
 *     whose canonical sign flips inside a cell);
 *  7. row_of_point[i] = the 1-based row of point i, 0 for a dropped point;
 *  8. F empty: M = 0 and RH_OK;
 *  9. the _f32 entry: the binary64 result on the widened input, rounded once.
 * The same bits on every run; permuting the input permutes the rows and changes nothing else (except that with
 * RH_VOX_ALIGN_NORMALS the side the normals are turned to is that of the cell's first point, which a permutation changes).
 * *n_out = M.  M > cap: RH_E_CAPACITY (like rh_refit) with row_of_point still written in full; cap = n always suffices.
 * xyz_out (cap x 3) is required when cap > 0; normals out need normals in; the other outputs are optional.  Parameters
 * and pointers are checked before the first device call. */
enum { RH_VOX_FIRST = 0, RH_VOX_CENTROID = 1 };
#define RH_VOX_ALIGN_NORMALS 1
typedef struct {
    double beta;             /* cell width */
    int32_t mode;            /* RH_VOX_FIRST / RH_VOX_CENTROID */
    int32_t flags;           /* RH_VOX_ALIGN_NORMALS or 0 */
} rh_voxel_params;
int rh_voxel_downsample(const double *xyz_aos, const double *nrm_aos_or_null, int64_t n, const rh_voxel_params *p, int device,
                        double *xyz_out_aos, double *nrm_out_aos_or_null, int64_t *first_out_1based_or_null,
                        int32_t *count_out_or_null, int64_t cap, int32_t *row_of_point_out_or_null,
                        int64_t *n_out, int64_t *n_dropped_out_or_null);
int rh_voxel_downsample_f32(const float *xyz_aos, const float *nrm_aos_or_null, int64_t n, const rh_voxel_params *p, int device,
                            float *xyz_out_aos, float *nrm_out_aos_or_null, int64_t *first_out_1based_or_null,
                            int32_t *count_out_or_null, int64_t cap, int32_t *row_of_point_out_or_null,
                            int64_t *n_out, int64_t *n_dropped_out_or_null);

/* ---- exact k nearest neighbours of a raw cloud, and outlier removal on them (no counterpart in the reference, which
 *      starts from clean clouds) ----
 * The search is that of rh_estimate_normals, step 1.  For point i (0-based) the ORDER of the other points is: ascending
 * d^2 = (dx*dx + dy*dy) + dz*dz (binary64, dx = q.x - p.x, no contraction), ties to the smaller index; the point itself is
 * left out by its index, not by its distance, so a duplicate of p_i (d^2 = 0) is a neighbour.
 * rh_knn:
 *  1. k is 1 .. RH_KNN_MAX_K; the neighbours of i are the first k of its order, with radius > 0 those with
 *     d^2 > radius*radius dropped; count[i] = how many are left (0 <= count[i] <= min(k, n - 1));
 *  2. idx is int32 [n x k], row i = the neighbours' 1-based indices in that order, 0 past count[i]; d2 is double [n x k],
 *     the d^2 as computed, +inf past count[i]; count is int32 [n].  Every output is optional;
 *  3. the _f32 entry widens the coordinates exactly and searches in binary64; d2 stays double;
 *  4. RH_E_INVALID: k outside 1 .. 63, radius negative or not finite, n < 1, n >= 2^31 - 1, a null xyz -- decided before
 *     the device is touched -- and a coordinate that is not finite (found on the device, nothing is written).
 * The same bits on every run.  The array arguments of rh_knn and rh_remove_outliers may be host or device pointers (the
 * copies are hipMemcpyDefault); scalars, parameters and stats are host memory.
 *
 * rh_remove_outliers: statistical / absolute / radius outlier removal, defined so that every output is one fixed sequence of
 * IEEE binary64 operations.
 *  T(a_0 .. a_(L-1)) is the root of the perfect binary tree over ADJACENT pairs of the values, padded with +0.0 to the next
 *  power of two: b = a; while (len(b) > 1) b = { b_0 + b_1, b_2 + b_3, ... }.  (Adding zeros is exact, so the padding does not
 *  show and the result does not depend on how the device cuts the tree into lanes, waves and blocks; its blocks hold
 *  RH_OUT_BLOCK_POINTS points.)
 *  1. count_i and d2_i1 .. d2_i,count_i: rh_knn's for (k, radius);
 *  2. m_i = T(sqrt(d2_i1), .., sqrt(d2_i,count_i)) / count_i, the mean distance to the neighbours; +inf when count_i == 0;
 *  3. V = { i : count_i >= 1 }, in index order; n_valid = |V|;
 *  4. mu = T(m_i if i in V else +0.0, i = 0 .. n-1) / n_valid, 0 when V is empty;
 *  5. sigma = sqrt(T((m_i - mu)*(m_i - mu) if i in V else +0.0, i = 0 .. n-1) / (n_valid - 1)), 0 when n_valid < 2;
 *  6. mode RH_OUT_STATISTICAL: tau = mu + std_mul*sigma (product rounded, then the sum); keep_i = i in V and m_i <= tau;
 *     mode RH_OUT_ABSOLUTE:    tau = threshold, the same test;
 *     mode RH_OUT_RADIUS:      keep_i = count_i == k (at least k other points within radius; radius > 0 required);
 *                              tau = radius in the stats;
 *  7. nn_median = the lower median -- sorted position floor((n_valid - 1) / 2) -- of sqrt(d2_i1) over V, 0 when V is
 *     empty: the cloud's point spacing, from which beta and eps are chosen.
 * keep_out: uint8 [n], 1 = kept.  kept_idx_out (optional): the kept points' 1-based indices, ascending, int32;
 * *n_kept_out = their number; more than cap: RH_E_CAPACITY (like rh_refit) with *n_kept_out set and keep_out,
 * mean_dist_out and stats still written in full.  mean_dist_out (optional): m_i, double [n].  stats (optional).
 * RH_E_INVALID, before the device is touched: k outside 1 .. 63, an unknown mode, radius negative or not finite (or not
 * positive in mode RH_OUT_RADIUS), std_mul not finite (statistical), threshold NaN (absolute), n < 1, n >= 2^31 - 1, a
 * null xyz / params / keep_out / n_kept_out, cap < 0, cap > 0 without kept_idx_out; on the device: a coordinate that is
 * not finite.  The same bits on every run; a permutation of the input permutes m_i and keep_i and can change mu, sigma and
 * tau in their last bits (the tree runs over the index order). */
#define RH_KNN_MAX_K 63
#define RH_OUT_BLOCK_POINTS 1024
enum { RH_OUT_STATISTICAL = 0, RH_OUT_ABSOLUTE = 1, RH_OUT_RADIUS = 2 };
typedef struct {
    int32_t k;               /* 1 .. RH_KNN_MAX_K */
    int32_t mode;            /* RH_OUT_* */
    double std_mul;          /* RH_OUT_STATISTICAL */
    double radius;           /* 0 = no limit (RH_OUT_RADIUS: > 0) */
    double threshold;        /* RH_OUT_ABSOLUTE */
} rh_outlier_params;
typedef struct {
    int64_t n_valid;         /* |V| */
    int64_t n_kept;
    double mu, sigma, tau;
    double nn_median;
} rh_outlier_stats;
int rh_knn(const double *xyz_aos, int64_t n, int32_t k, double radius, int device, int32_t *idx_out_or_null,
           double *d2_out_or_null, int32_t *count_out_or_null);
int rh_knn_f32(const float *xyz_aos, int64_t n, int32_t k, double radius, int device, int32_t *idx_out_or_null,
               double *d2_out_or_null, int32_t *count_out_or_null);
int rh_remove_outliers(const double *xyz_aos, int64_t n, const rh_outlier_params *p, int device, uint8_t *keep_out,
                       int32_t *kept_idx_out_or_null, int64_t cap, int64_t *n_kept_out, double *mean_dist_out_or_null,
                       rh_outlier_stats *stats_or_null);
int rh_remove_outliers_f32(const float *xyz_aos, int64_t n, const rh_outlier_params *p, int device, uint8_t *keep_out,
                           int32_t *kept_idx_out_or_null, int64_t cap, int64_t *n_kept_out, double *mean_dist_out_or_null,
                           rh_outlier_stats *stats_or_null);

/* ---- density-based clustering of a raw cloud: DBSCAN, and Euclidean cluster extraction at min_pts = 1 (no counterpart in
 *      the reference, whose clouds hold one object) ----
 * Splits a cloud into its spatially connected parts: a scan into objects before rh_ransac, the points that rh_assign_points
 * left without a label into the next objects or clutter, the inpoints of one shape into its patches.
 * Points p_1 .. p_n (binary64 array-of-structures; the _f32 entry widens exactly), eps > 0, min_pts >= 1, min_size >= 1.
 *  1. d2(i, j) = (dx*dx + dy*dy) + dz*dz in binary64, no contraction: rh_knn's expression.  eps2 = eps*eps, rounded once;
 *  2. j is a neighbour of i when j != i and d2(i, j) <= eps2.  The boundary is included; i is left out by its index, so a
 *     duplicate of p_i is a neighbour at distance 0;
 *  3. i is a CORE point when 1 + (the number of its neighbours) >= min_pts: the point counts itself, as in scikit-learn and
 *     Open3D.  With min_pts = 1 every point is a core point and the result is plain Euclidean cluster extraction;
 *  4. a cluster is a connected component of the graph on the core points whose edges are the neighbour relation.  Two
 *     clusters are never joined through a point that is no core point;
 *  5. a BORDER point is no core point and has at least one core neighbour; it belongs to the cluster of its NEAREST core
 *     neighbour: smallest d2, ties to the smaller index.  Textbook DBSCAN gives a border point to whichever cluster reaches
 *     it first, which depends on the order of processing; this rule does not, and differs from it only for border points
 *     within eps of two clusters;
 *  6. every other point is NOISE, and so are, in the labels, all points of a cluster with fewer than min_size members (core
 *     and border points counted);
 *  7. order = RH_CLUSTER_BY_INDEX: the clusters that are left are numbered 1 .. M by ascending index of their smallest core
 *     point; RH_CLUSTER_BY_SIZE: by descending size, ties by the smallest core point's index.  Noise has label 0.
 * Every decision is a comparison of binary64 values of fixed expressions or integer arithmetic: the same bits on every run,
 * and a permutation of the input permutes the result (with the numbering following the indices).
 * labels_out: int32 [n].  kind_out (optional): uint8 [n], RH_PT_*; the kind of a point of a cluster dropped in step 6 is what
 * it was before the drop, core or border.  *n_clusters_out = M.
 * counts (optional): int64 [cap + 1], the points per label, label 0 first; offsets (optional): int64 [cap + 2] and idx
 * (optional): int64 [n]: the 1-based indices grouped by label, label 0 first, ascending within a label, label l at
 * idx[offsets[l] .. offsets[l + 1]) -- the lists of rh_assign_points.  The entries of the labels M + 1 .. min(cap, n) are
 * counts 0 and offsets n; nothing is written beyond min(cap, n).  M > cap with counts or offsets asked for: RH_E_CAPACITY
 * (like rh_refit) with *n_clusters_out = M and labels_out, kind_out and stats still written in full; cap = n always suffices.
 * stats (optional): n_clusters = M; n_core + n_border + n_noise = n by the kinds; n_small = the core and border points of the
 * clusters dropped in step 6 (label 0 holds n_noise + n_small points); largest = the size of the largest cluster left, 0
 * when M = 0.
 * The array arguments may be host or device pointers (the copies are hipMemcpyDefault); parameters, scalars and stats are
 * host memory.  RH_E_INVALID, before the device is touched: a null xyz / params / labels_out / n_clusters_out, n < 1,
 * n >= 2^31, eps not finite or <= 0, min_pts < 1, min_size < 1, an unknown order, cap < 0; on the device: a coordinate that
 * is not finite (nothing is written). */
enum { RH_CLUSTER_BY_INDEX = 0, RH_CLUSTER_BY_SIZE = 1 };
enum { RH_PT_NOISE = 0, RH_PT_BORDER = 1, RH_PT_CORE = 2 };
typedef struct {
    double eps;
    int32_t min_pts, min_size;
    int32_t order;           /* RH_CLUSTER_BY_* */
    int32_t reserved;        /* 0 */
} rh_cluster_params;
typedef struct {
    int64_t n_clusters, n_core, n_border, n_noise;
    int64_t n_small;         /* points of clusters below min_size */
    int64_t largest;
} rh_cluster_stats;
int rh_cluster(const double *xyz_aos, int64_t n, const rh_cluster_params *p, int device, int32_t *labels_out,
               uint8_t *kind_out_or_null, int64_t cap, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
               int64_t *idx_out_or_null, int64_t *n_clusters_out, rh_cluster_stats *stats_or_null);
int rh_cluster_f32(const float *xyz_aos, int64_t n, const rh_cluster_params *p, int device, int32_t *labels_out,
                   uint8_t *kind_out_or_null, int64_t cap, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
                   int64_t *idx_out_or_null, int64_t *n_clusters_out, rh_cluster_stats *stats_or_null);

/* ---- consistent orientation of normals without a viewpoint: sign propagation along a minimum spanning forest of the
 *      neighbour graph (Hoppe et al. 1992; no counterpart in the reference, which starts from oriented normals) ----
 * Every per-point test of the engine is sign sensitive (isparallel is dot(v1, v2) > cos(alpha), src/utilities.jl:115-117),
 * and rh_estimate_normals can fix the sign only from a viewpoint or hints.  A merged, thinned or registered cloud has
 * neither; this call turns its normals so that neighbouring normals agree.  Points p_0 .. p_(n-1) and normals n_i (binary64
 * array-of-structures, the normals used as given, not renormalised), k in 1 .. RH_KNN_MAX_K, radius (0 = none), anchor, up.
 *  1. VERTICES.  V = the points whose normal is not (0, 0, 0) (all three components == 0.0).  The degenerate points of
 *     rh_estimate_normals take no part and come back untouched;
 *  2. EDGES.  {i, j}, i < j, is an edge when both are in V and j is among rh_knn's neighbours of i for (k, radius) or i is
 *     among those of j.  The search runs over all n points, exactly rh_knn's; edges that touch a point outside V are
 *     dropped afterwards;
 *  3. WEIGHT.  dot_ij = (ni.x*nj.x + ni.y*nj.y) + ni.z*nj.z in binary64, each operation rounded on its own, no contraction
 *     (bit-symmetric in i and j).  a_ij = |dot_ij|, s_ij = (dot_ij < 0);
 *  4. ORDER.  The edges are totally ordered by descending a, then ascending i, then ascending j (Hoppe's 1 - |ni.nj|
 *     without the subtraction);
 *  5. FOREST.  F = the minimum spanning forest under that order.  The order is total, so F is unique and depends on no
 *     order of processing;
 *  6. PARITY.  Within a tree par(i) ^ par(j) = the XOR of s along the tree path from i to j;
 *  7. ANCHOR of every component (tree):
 *     RH_ORI_ANCHOR_FIRST: the component's smallest index, kept as given: want = 0;
 *     RH_ORI_ANCHOR_TOP:   the point of largest t = ((x*up.x + y*up.y) + z*up.z) + 0.0 (a NaN t counts as -inf), ties to the
 *                          smaller index; want = (((n.x*up.x + n.y*up.y) + n.z*up.z) < 0) for its normal n: the topmost
 *                          normal points up (Hoppe's rule: outward normals on a closed surface);
 *  8. FLIP.  flip_i = par(i) ^ par(anchor) ^ want.  The output normal is the input with all three components negated when
 *     flip_i is set and bit-identical otherwise;
 *  9. OUTPUTS.  nrm_out: n x 3, may be the input pointer.  flip_out (optional) int32 [n]: 1 flipped, 0 kept, -1 outside V.
 *     comp_out (optional) int32 [n]: the components numbered 1 .. M by their smallest index, 0 outside V.  stats (optional):
 *       n_vertices = |V|; n_edges; n_components = M; n_tree_edges = n_vertices - n_components; n_flipped;
 *       n_inconsistent = the edges with s_ij ^ flip_i ^ flip_j set: their ends disagree in sign AFTER the orientation, and
 *                        every one of them is a non-tree edge;
 *       largest_component = the size of the largest component (0 when V is empty);
 *       min_tree_absdot = the smallest a over F, +inf without a tree edge.
 *     The last two say how far to trust the result;
 * 10. RH_E_INVALID, decided before the device is touched: k outside 1 .. 63, radius negative or not finite, anchor outside
 *     0 .. 1, with RH_ORI_ANCHOR_TOP an up that is not finite or all zero, n < 1, n >= 2^31 - 1, n*k >= 2^31 (the directed
 *     pairs are counted in 31 bits), a null xyz / nrm / params / nrm_out; found on the device, nothing is written: a
 *     coordinate that is not finite, a normal component that is not finite or exceeds 2 in magnitude;
 * 11. the _f32 entry widens coordinates and normals exactly, decides everything in binary64 and negates the float normals:
 *     negation is exact, no rounding appears anywhere.
 * Every decision is a comparison of binary64 values of fixed expressions or integer arithmetic: the same bits on every
 * run.  The array arguments may be host or device pointers (the copies are hipMemcpyDefault); params and stats are host
 * memory.  The neighbour lists never leave the device. */
enum { RH_ORI_ANCHOR_FIRST = 0, RH_ORI_ANCHOR_TOP = 1 };
typedef struct {
    int32_t k;               /* 1 .. RH_KNN_MAX_K */
    int32_t anchor;          /* RH_ORI_ANCHOR_* */
    double radius;           /* 0 = no limit */
    double up[3];            /* RH_ORI_ANCHOR_TOP */
} rh_orient_params;
typedef struct {
    int64_t n_vertices, n_edges, n_components, n_tree_edges;
    int64_t n_flipped, n_inconsistent, largest_component;
    double min_tree_absdot;
} rh_orient_stats;
int rh_orient_normals(const double *xyz_aos, const double *nrm_aos, int64_t n, const rh_orient_params *p, int device,
                      double *nrm_out_aos, int32_t *flip_out_or_null, int32_t *comp_out_or_null, rh_orient_stats *stats_or_null);
int rh_orient_normals_f32(const float *xyz_aos, const float *nrm_aos, int64_t n, const rh_orient_params *p, int device,
                          float *nrm_out_aos, int32_t *flip_out_or_null, int32_t *comp_out_or_null, rh_orient_stats *stats_or_null);

/* ---- region growing by smoothness for a cloud with normals (Rabbani et al. 2006: the second detector of PCL and CGAL
 *      beside RANSAC; no counterpart in the reference, which finds shapes by RANSAC alone) ----
 * Splits a cloud by its SURFACES where rh_cluster splits it by gaps in space: a detector of its own for piecewise-smooth
 * scenes, a pre-segmentation with rh_ransac run per region, the points rh_assign_points left without a label into sheets.
 * The textbook algorithm grows one region after another from a sorted seed list, and its result depends on the seed order
 * and on which region reaches a point first.  This statement follows rh_cluster's three kinds and depends on no order:
 * seeds play the core points, smooth neighbour pairs play the eps-neighbourhood, the border rule is "nearest".
 * Points p_0 .. p_(n-1), normals n_i (binary64 array-of-structures, used as given, not renormalised), optional curvature
 * c_i (double [n] or null: rh_estimate_normals' curv_out), parameters below.
 *  1. V = the points whose normal is not (0, 0, 0) (all three components == 0.0).  The degenerate points of
 *     rh_estimate_normals are outside V, take no part and come back with label 0;
 *  2. NEIGHBOURS.  N(i) = rh_knn's neighbour list of i for (k, radius), searched over all n points.  i ~ j when j is in
 *     N(i) or i is in N(j): the undirected graph of rh_orient_normals, step 2;
 *  3. SMOOTH PAIR, for i ~ j with both in V.  dot = (ni.x*nj.x + ni.y*nj.y) + ni.z*nj.z, each operation rounded on its
 *     own, no contraction (bit-symmetric in i and j); a = fabs(dot) with RH_SEG_UNSIGNED, dot otherwise.  The pair is
 *     smooth when a >= cos_angle and, with dist_max > 0, both tangent-plane distances pass: with dx = pj.x - pi.x (dy, dz
 *     likewise), e_i = (ni.x*dx + ni.y*dy) + ni.z*dz and e_j = (nj.x*(-dx) + nj.y*(-dy)) + nj.z*(-dz) -- negation is
 *     exact, so the test is symmetric -- fabs(e_i) <= dist_max and fabs(e_j) <= dist_max.  The distance test is what
 *     separates parallel sheets a step apart, whose normals agree;
 *  4. SEED.  i in V is a seed when no curvature is given or c_i <= curv_max.  A NaN curvature makes no seed;
 *  5. REGION.  A region is a connected component of the graph on the seeds whose edges are the smooth pairs.  Two regions
 *     are never joined through a point that is no seed;
 *  6. BORDER.  i in V that is no seed and forms a smooth pair with at least one seed j is a border point; it belongs to
 *     the region of that j with the smallest d2(i, j) (rh_knn's expression), ties to the smaller j.  j may list i without
 *     i listing j: those pairs count;
 *  7. every other point has label 0 and kind RH_PT_NOISE.  The kinds are rh_cluster's, RH_PT_CORE meaning seed; after the
 *     min_size drop a point's kind is what it was before the drop;
 *  8. min_size and the numbering are rh_cluster's steps 6 and 7, "smallest core point" reading "smallest seed";
 *  9. labels_out, kind_out, cap, counts, offsets, idx and *n_regions_out behave as in rh_cluster, RH_E_CAPACITY included.
 *     stats (optional): n_regions = M; n_seed + n_border + n_unassigned + n_invalid = n, where n_invalid = n - |V| and
 *     n_unassigned = the points of V that are neither a seed nor have a seed to attach to; n_small = the seeds and border
 *     points of the regions dropped by min_size; largest = the size of the largest region left, 0 when M = 0;
 * 10. RH_E_INVALID, decided before the device is touched: a null xyz / nrm / params / labels_out / n_regions_out, n < 1,
 *     n >= 2^31 - 1, n*k >= 2^31, k outside 1 .. RH_KNN_MAX_K, radius negative or not finite, cos_angle not finite or
 *     outside [-1, 1], curv_max NaN, dist_max negative or not finite, min_size < 1, an unknown order or flag bit, cap < 0;
 *     found on the device, nothing is written: a coordinate that is not finite, a normal component that is not finite or
 *     exceeds 2 in magnitude;
 * 11. the _f32 entry widens coordinates, normals and curvature exactly and decides everything in binary64: its outputs
 *     equal those of the binary64 call on the widened input.
 * Every decision is a comparison of binary64 values of fixed expressions or integer arithmetic: the same bits on every run,
 * whatever the order of processing.  The caller takes the cosine: the library never calls cos().  The array arguments may
 * be host or device pointers (the copies are hipMemcpyDefault); params, scalars and stats are host memory.  The neighbour
 * lists never leave the device. */
#define RH_SEG_UNSIGNED 1
typedef struct {
    int32_t k;               /* 1 .. RH_KNN_MAX_K */
    int32_t flags;           /* RH_SEG_UNSIGNED or 0 */
    double radius;           /* 0 = no limit (rh_knn's) */
    double cos_angle;        /* finite, in [-1, 1] */
    double curv_max;         /* not NaN; ignored without curvature */
    double dist_max;         /* 0 = no distance test; otherwise finite and > 0 */
    int32_t min_size;        /* >= 1 */
    int32_t order;           /* RH_CLUSTER_BY_* */
} rh_segment_params;
typedef struct {
    int64_t n_regions, n_seed, n_border, n_unassigned, n_invalid;
    int64_t n_small;         /* points of regions below min_size */
    int64_t largest;
} rh_segment_stats;
int rh_segment_smooth(const double *xyz_aos, const double *nrm_aos, const double *curv_or_null, int64_t n,
                      const rh_segment_params *p, int device, int32_t *labels_out, uint8_t *kind_out_or_null, int64_t cap,
                      int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null,
                      int64_t *n_regions_out, rh_segment_stats *stats_or_null);
int rh_segment_smooth_f32(const float *xyz_aos, const float *nrm_aos, const float *curv_or_null, int64_t n,
                          const rh_segment_params *p, int device, int32_t *labels_out, uint8_t *kind_out_or_null, int64_t cap,
                          int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null,
                          int64_t *n_regions_out, rh_segment_stats *stats_or_null);

/* ---- nearest neighbours of query points in ANOTHER cloud, and cloud-to-cloud distances on them (no counterpart in the
 *      reference, which works on one cloud) ----
 * Carries labels, shapes and normals from one cloud to another (a thinned cloud to the full scan, one scan to the next),
 * and measures how far a scan lies from a reference cloud.  Reference points r_1 .. r_n, query points q_1 .. q_m (binary64
 * array-of-structures; the _f32 entries widen both arrays exactly and search in binary64).
 * rh_knn_query: for query j (0-based) the ORDER of the n reference points is: ascending d^2 = (dx*dx + dy*dy) + dz*dz
 * (binary64, dx = r.x - q.x, no contraction: rh_knn's expression), ties to the smaller reference index.  NO point is left
 * out: a reference point equal to the query is its first neighbour at d^2 = 0.
 *  1. k is 1 .. RH_KNN_MAX_K; the neighbours of j are the first k of its order, with radius > 0 those with
 *     d^2 > radius*radius dropped (the boundary is included); count[j] = how many are left (0 <= count[j] <= min(k, n));
 *  2. idx is int32 [m x k], row j = the neighbours' 1-based reference indices in that order, 0 past count[j]; d2 is double
 *     [m x k], the d^2 as computed, +inf past count[j]; count is int32 [m].  Rows are in the caller's query order, whatever
 *     order the device serves them in.  Every output is optional;
 *  3. d2 stays double in the _f32 entry;
 *  4. RH_E_INVALID: a null array, n < 1, n >= 2^31 - 1, m < 1, m >= 2^31, k outside 1 .. 63, radius negative or not finite
 *     -- decided before the device is touched -- and a coordinate of either cloud that is not finite (found on the device,
 *     nothing is written).
 * The same bits on every run.  The array arguments may be host or device pointers (the copies are hipMemcpyDefault);
 * parameters and stats are host memory.
 *
 * rh_cloud_distance: the distance of every query to the reference cloud and its summary, every output one fixed sequence of
 * IEEE binary64 operations.  nn_j is the first entry of the order above (k = 1, the params' radius); query j is VALID when
 * there is such an entry.  With e = q_j - r_nn componentwise:
 *  RH_DIST_POINT: d_j = sqrt(d^2), the d^2 of the order;
 *  RH_DIST_PLANE: d_j = fabs((e.x*n.x + e.y*n.y) + e.z*n.z), n the normal stored for r_nn, used as given: it is neither
 *                 normalised nor checked (the distance to the tangent plane at the nearest point when n is a unit normal).
 * dist_out: double [m], d_j, +inf when query j is not valid.  nn_idx_out (optional): int32 [m], the 1-based reference index,
 * 0 when query j is not valid.  stats (optional), with T() the tree of rh_remove_outliers over the query index order
 * j = 0 .. m-1 (blocks of RH_OUT_BLOCK_POINTS):
 *  n_valid  = the number of valid queries;
 *  mean     = T(d_j if valid else +0.0) / n_valid;
 *  rms      = sqrt(T(d_j*d_j if valid else +0.0) / n_valid);
 *  max      = the largest d_j over the valid queries: the one-sided Hausdorff distance from the queries to the reference;
 *  argmax   = the smallest 1-based j reaching max, 0 when there is none;
 *  n_within = the number of valid j with d_j <= threshold (threshold may be +inf);
 *  median   = the lower median of d_j over the valid queries -- sorted position floor((n_valid - 1) / 2), as nn_median.
 * All four doubles are 0 when n_valid == 0.  No floating-point atomics: the same bits on every run; a permutation of the
 * queries permutes d_j and can change mean and rms in their last bits.  The measures are ONE-SIDED, queries -> reference.
 * The symmetric ones are two calls composed by the caller: Hausdorff = the larger of the two max, Chamfer = the sum (or
 * mean) of the two mean (or of the two rms squared), with the roles of the clouds exchanged in the second call.
 * RH_E_INVALID, before the device is touched: a null ref / qry / params / dist_out, n and m as above, radius negative or not
 * finite, threshold NaN, an unknown metric, RH_DIST_PLANE without normals; on the device: a coordinate that is not finite. */
enum { RH_DIST_POINT = 0, RH_DIST_PLANE = 1 };
typedef struct {
    double radius;           /* 0 = no limit */
    double threshold;        /* for n_within */
    int32_t metric;          /* RH_DIST_* */
    int32_t reserved;        /* 0 */
} rh_distance_params;
typedef struct {
    int64_t n_valid, n_within;
    int64_t argmax;          /* 1-based query index, 0 = none */
    double mean, rms, max, median;
} rh_distance_stats;
int rh_knn_query(const double *ref_xyz_aos, int64_t n, const double *qry_xyz_aos, int64_t m, int32_t k, double radius,
                 int device, int32_t *idx_out_or_null, double *d2_out_or_null, int32_t *count_out_or_null);
int rh_knn_query_f32(const float *ref_xyz_aos, int64_t n, const float *qry_xyz_aos, int64_t m, int32_t k, double radius,
                     int device, int32_t *idx_out_or_null, double *d2_out_or_null, int32_t *count_out_or_null);
int rh_cloud_distance(const double *ref_xyz_aos, const double *ref_nrm_aos_or_null, int64_t n, const double *qry_xyz_aos,
                      int64_t m, const rh_distance_params *p, int device, double *dist_out, int32_t *nn_idx_out_or_null,
                      rh_distance_stats *stats_or_null);
int rh_cloud_distance_f32(const float *ref_xyz_aos, const float *ref_nrm_aos_or_null, int64_t n, const float *qry_xyz_aos,
                          int64_t m, const rh_distance_params *p, int device, double *dist_out, int32_t *nn_idx_out_or_null,
                          rh_distance_stats *stats_or_null);

/* ---- rigid registration of one cloud onto another: iterative closest point (no counterpart in the reference, which
 *      works on one cloud) ----
 * Brings the query cloud q_1 .. q_m into the frame of the reference cloud r_1 .. r_n, so that rh_knn_query,
 * rh_cloud_distance and the labels carried across mean what they say.  Every output is one fixed sequence of IEEE binary64
 * operations (+, -, *, /, sqrt; no contraction); the _f32 entry widens all arrays exactly and computes in binary64.
 * Below, S(..) = T(..) + 0.0 with T() the tree of rh_remove_outliers over the query index order j = 0 .. m-1 (the device's
 * blocks pad with +0.0, so a root of -0.0 is read as +0.0; every other value is unchanged), one tree per component.
 *  1. CENTRE.  lo_k / hi_k = the smallest / largest reference coordinate along axis k; c_k = 0.5*(lo_k + hi_k).
 *     s = r - c and y = q - c componentwise are the centred points.
 *  2. STATE.  A 3x3 matrix R (row-major R_kl) and a vector t act on centred queries:
 *         y'_k = ((R_k0*y_0 + R_k1*y_1) + R_k2*y_2) + t_k.
 *     With init = [A | u] (3x4 row-major, x' = A x + u in the caller's frame; A is used as given, it is neither checked
 *     nor made orthogonal), or A = I, u = 0 when init is null:
 *         R = A,   t_k = (((A_k0*c_0 + A_k1*c_1) + A_k2*c_2) + u_k) - c_k.
 *  3. CORRESPONDENCE, every iteration anew: p_j = y'_j + c componentwise; nn_j = the first entry of rh_knn_query's order
 *     for the query point p_j (k = 1, the params' radius, 0 = no limit); query j is VALID when there is such an entry.
 *     n_valid = the number of valid queries.
 *  4. LEAVES of a valid query, with s = r_nn - c and e = s - y' componentwise (a query that is not valid has +0.0 in
 *     every leaf):
 *     RH_DIST_PLANE, n the normal stored for r_nn, used as given:
 *         a_0 = y'_1*n_2 - y'_2*n_1,  a_1 = y'_2*n_0 - y'_0*n_2,  a_2 = y'_0*n_1 - y'_1*n_0,  a_3 = n_0, a_4 = n_1, a_5 = n_2,
 *         b = (e_0*n_0 + e_1*n_1) + e_2*n_2;
 *         the 28 leaves a_u*a_v (0 <= u <= v <= 5), a_u*b (u = 0 .. 5) and b*b.  H_uv = H_vu = S(a_u*a_v), g_u = S(a_u*b),
 *         E = S(b*b).
 *     RH_DIST_POINT (the three rows n = e_x, e_y, e_z of the plane metric, written out; no product with a literal zero
 *     is formed): the 16 leaves
 *         P_00 = y'_0*y'_0, P_11 = y'_1*y'_1, P_22 = y'_2*y'_2, P_01 = y'_0*y'_1, P_02 = y'_0*y'_2, P_12 = y'_1*y'_2,
 *         Y_k = y'_k,   X_0 = y'_1*e_2 - y'_2*e_1,  X_1 = y'_2*e_0 - y'_0*e_2,  X_2 = y'_0*e_1 - y'_1*e_0,   D_k = e_k,
 *         (e_0*e_0 + e_1*e_1) + e_2*e_2;
 *         H_00 = S(P_11) + S(P_22), H_11 = S(P_00) + S(P_22), H_22 = S(P_00) + S(P_11),
 *         H_01 = -S(P_01), H_02 = -S(P_02), H_12 = -S(P_12),
 *         H_04 = -S(Y_2), H_05 = S(Y_1), H_13 = S(Y_2), H_15 = -S(Y_0), H_23 = -S(Y_1), H_24 = S(Y_0),
 *         H_03 = H_14 = H_25 = +0.0;  H_33 = H_44 = H_55 = (double)n_valid, H_34 = H_35 = H_45 = +0.0;
 *         g_u = S(X_u), g_(3+k) = S(D_k), E = S(the last leaf).
 *     rms = sqrt(E / (double)n_valid), 0 when n_valid = 0: the residual BEFORE this iteration's step.
 *  5. n_valid < 6 (fewer residuals than unknowns, whichever metric): the call ends with status RH_REG_TOO_FEW.
 *  6. SOLVE H x = g by Cholesky, H = L L^T, row by row:
 *         for i = 0 .. 5:  for j = 0 .. i:  v = H_ji;  for k = 0 .. j-1 ascending: v = v - L_ik*L_jk;
 *                              j < i:  L_ij = v / L_jj;
 *                              j = i:  the pivot: accepted when v > 1e-10*H_ii (H_ii the original diagonal); L_ii = sqrt(v).
 *     A pivot that is not accepted (NaN included) ends the call with status RH_REG_DEGENERATE.  Then
 *         for i = 0 .. 5:       v = g_i;  for k = 0 .. i-1 ascending: v = v - L_ik*z_k;  z_i = v / L_ii;
 *         for i = 5 down to 0:  v = z_i;  for k = i+1 .. 5 ascending: v = v - L_ki*x_k;  x_i = v / L_ii.
 *  7. UPDATE.  w = (x_0, x_1, x_2), tau = (x_3, x_4, x_5), a_k = 0.5*w_k, aa = (a_0*a_0 + a_1*a_1) + a_2*a_2, d = 1.0 + aa,
 *     f = 1.0 - aa.  The rotation step is the Cayley map of a (rational: no sin, no cos):
 *         C_kk = (f + 2.0*(a_k*a_k)) / d,
 *         C_01 = (2.0*(a_0*a_1) - 2.0*a_2) / d,   C_10 = (2.0*(a_0*a_1) + 2.0*a_2) / d,
 *         C_02 = (2.0*(a_0*a_2) + 2.0*a_1) / d,   C_20 = (2.0*(a_0*a_2) - 2.0*a_1) / d,
 *         C_12 = (2.0*(a_1*a_2) - 2.0*a_0) / d,   C_21 = (2.0*(a_1*a_2) + 2.0*a_0) / d;
 *         R_kl <- (C_k0*R_0l + C_k1*R_1l) + C_k2*R_2l   (all nine from the old R),
 *         t_k  <- ((C_k0*t_0 + C_k1*t_1) + C_k2*t_2) + tau_k   (all three from the old t).
 *  8. STOP after the update: sqrt((w_0*w_0 + w_1*w_1) + w_2*w_2) <= rot_tol and sqrt((tau_0*tau_0 + tau_1*tau_1) +
 *     tau_2*tau_2) <= trans_tol: status RH_REG_CONVERGED.  Otherwise, after max_iter iterations: RH_REG_MAX_ITER.
 *  9. OUTPUTS.  transform_out: 3x4 row-major [R | t_out] in the caller's frame, x' = R x + t_out,
 *         t_out_k = (t_k + c_k) - ((R_k0*c_0 + R_k1*c_1) + R_k2*c_2)
 *     -- the state reached so far, whatever the status.  result (optional): status; iterations = the number of iterations
 *     whose steps 3 and 4 ran (each but possibly the last was followed by an update; with RH_REG_TOO_FEW and
 *     RH_REG_DEGENERATE the last was not); n_valid and rms of the last of them.  n_valid_it_out / rms_it_out (optional,
 *     int32 / double [max_iter]): n_valid and rms of iteration 0, 1, ..; 0 behind `iterations`.
 * The reference's grid is built once per call; the queries' pass (box, margin, cell keys, sort) runs on p_j every
 * iteration, and nothing that could change a neighbour is carried from one iteration to the next.  No floating-point
 * atomics: the same bits on every run; a permutation of the queries can change the result in its last bits (the trees run
 * over the query index order).  The array arguments may be host or device pointers (hipMemcpyDefault); params, init,
 * transform_out, result and the two histories are host memory.
 * The function returns RH_OK whatever the status.  RH_E_INVALID, before the device is touched: a null ref / qry / params /
 * transform_out, n and m outside the limits of rh_knn_query, radius negative or not finite, rot_tol or trans_tol negative
 * or NaN (+inf is allowed: that test always holds), max_iter outside 1 .. RH_REG_MAX_ITERATIONS, an unknown metric,
 * RH_DIST_PLANE without normals, an init entry that is not finite; on the device: a coordinate of either cloud, or of a
 * p_j, that is not finite (nothing is written). */
#define RH_REG_MAX_ITERATIONS 1000
enum { RH_REG_CONVERGED = 0, RH_REG_MAX_ITER = 1, RH_REG_DEGENERATE = 2, RH_REG_TOO_FEW = 3 };
typedef struct {
    double radius;           /* 0 = no limit */
    double rot_tol;          /* on |w|, radians to first order */
    double trans_tol;        /* on |tau|, the clouds' unit */
    int32_t metric;          /* RH_DIST_* */
    int32_t max_iter;        /* 1 .. RH_REG_MAX_ITERATIONS */
} rh_register_params;
typedef struct {
    int32_t status;          /* RH_REG_* */
    int32_t iterations;
    int64_t n_valid;         /* of the last iteration */
    double rms;              /* of the last iteration, before its step */
} rh_register_result;
int rh_register(const double *ref_xyz_aos, const double *ref_nrm_aos_or_null, int64_t n, const double *qry_xyz_aos, int64_t m,
                const rh_register_params *p, const double *init_3x4_or_null, int device, double *transform_out_3x4,
                rh_register_result *result_or_null, int32_t *n_valid_it_out_or_null, double *rms_it_out_or_null);
int rh_register_f32(const float *ref_xyz_aos, const float *ref_nrm_aos_or_null, int64_t n, const float *qry_xyz_aos, int64_t m,
                    const rh_register_params *p, const double *init_3x4_or_null, int device, double *transform_out_3x4,
                    rh_register_result *result_or_null, int32_t *n_valid_it_out_or_null, double *rms_it_out_or_null);

/* ---- global registration without a start: point descriptors, feature matching, RANSAC over correspondences (no
 *      counterpart in the reference, which works on one cloud) ----
 * rh_register needs a start within its basin; these three calls produce one for two clouds that differ by an arbitrary
 * rigid motion.  Everything is integers or one fixed sequence of IEEE binary64 operations (+, -, *, /, sqrt, floor; no
 * contraction), so host, device and a numpy restatement give the same bytes.  Below
 *     dot(x, y) = (x_0*y_0 + x_1*y_1) + x_2*y_2,   cross(a, b) = (a_1*b_2 - a_2*b_1, a_2*b_0 - a_0*b_2, a_0*b_1 - a_1*b_0).
 *
 * rh_describe: D_i, RH_DESC_DIM = 33 uint16 per point, from the points, their normals (required, used as given, not
 * renormalised), k in 1 .. RH_KNN_MAX_K and radius (0 = none).
 *  1. N(i) and count_i are the neighbour list and count of rh_knn for (k, radius).
 *  2. PAIR FEATURES of (i, j), j in N(i); i is always the source (the pair is not reordered by the normals' angles):
 *         d = p_j - p_i componentwise,  d2 = dot(d, d),  u = n_i,  s = n_j,
 *         v = cross(u, d),  v2 = dot(v, v),  w = cross(u, v),  len = sqrt(d2),  vl = sqrt(v2),
 *         f1 = dot(u, d) / len,   f2 = dot(v, s) / vl,   a = dot(w, s) / vl,   b = dot(u, s),
 *         g = |a| + |b|,   r = b / g,   psi = a >= 0 ? 1.0 - r : 3.0 + r.
 *     psi is a rational pseudo-angle in [0, 4) of the direction (b, a): monotone in the angle, no atan2.  The pair is
 *     DEGENERATE and adds nothing when d2 == 0, v2 == 0, g == 0, or one of f1, f2, psi is NaN.
 *  3. BINS, decided in binary64: bin(x) = t < 0 ? 0 : (t > 10 ? 10 : t) with t = floor(x);
 *         b1 = bin((f1 + 1.0)*5.5),   b2 = bin((f2 + 1.0)*5.5),   b3 = bin(psi*2.75).
 *     S_i, 33 counts, gets +1 at b1, at 11 + b2 and at 22 + b3 for every pair of i that is not degenerate.
 *  4. D_i[c] = count_i*S_i[c] + the sum over j in N(i) of S_j[c]: integers, at most 2*63*63 = RH_DESC_MAX, so the order of
 *     the sum does not show.
 * In exact arithmetic D is invariant under a rigid motion of points and normals together; in floating point a value on
 * a bin edge can move to the next bin.  desc_out: uint16 [n x 33]; count_out (optional): int32 [n], count_i.
 * The _f32 entry widens coordinates and normals exactly.  The same bytes on every run.  RH_E_INVALID, before the device
 * is touched: a null xyz / normals / desc_out, k outside 1 .. 63, radius negative or not finite, n < 1,
 * n > (2^31 - 1) / 33; on the device: a coordinate or a normal that is not finite (nothing is written).
 *
 * rh_match_features: for every query row the reference row of smallest sum over c of (q_c - r_c)^2 -- an exact integer,
 * at most 33 * 7938^2 < 2^31 -- ties to the smaller index.  idx_out: int32 [m], 1-based; dist_out (optional): uint32 [m],
 * that sum.  flags = RH_MATCH_MUTUAL: the same search runs from the reference side (for every reference row its best
 * query row, ties to the smaller index) and idx_out[j] = 0 where the best query of reference row idx_out[j] is not j;
 * dist_out is not changed by it.  RH_E_INVALID, before the device is touched: a null ref / qry / idx_out, unknown flags,
 * n or m outside 1 .. (2^31 - 1) / 80; on the device: a descriptor value above RH_DESC_MAX (nothing is written).
 *
 * rh_register_global: the motion x' = R x + t of the queries onto the reference that most of the c correspondences
 * (q_corr_qry[i], r_corr_ref[i]), 1-based int32 indices, agree with; trials hypotheses from three correspondences each.
 *  1. TRIPLES.  triples (int32 [trials x 3], 0-based into the correspondences) when given; otherwise rh_rng_seed(seed) and
 *     trial t = 0, 1, .. takes three draws rh_rng_range(c) - 1 in order -- always three, whatever they are.
 *  2. A trial (i0, i1, i2) is VALID when all of these hold:
 *       the three indices are distinct;
 *       for each edge (x, y) = (0, 1), (0, 2), (1, 2), with lq = dot(q_x - q_y, q_x - q_y) and lr likewise of r, ee =
 *       edge_ratio*edge_ratio and mm = min_edge*min_edge:  lq >= ee*lr,  lr >= ee*lq,  lq >= mm;
 *       the frames of (q_0, q_1, q_2) and of (r_0, r_1, r_2) exist.
 *  3. FRAME of (x0, x1, x2):  h = x1 - x0,  hh = dot(h, h),  e1 = h / sqrt(hh) componentwise,  gv = cross(e1, x2 - x0),
 *     g2 = dot(gv, gv); the frame exists when hh > 0 and g2 > 0;  e3 = gv / sqrt(g2),  e2 = cross(e3, e1).
 *     F is the matrix with columns e1, e2, e3: F_k0 = e1_k, F_k1 = e2_k, F_k2 = e3_k.
 *  4. TRANSFORM:  R_kl = (Fr_k0*Fq_l0 + Fr_k1*Fq_l1) + Fr_k2*Fq_l2;
 *         cq = ((q_0 + q_1) + q_2) / 3.0 componentwise, cr likewise;
 *         t_k = cr_k - ((R_k0*cq_0 + R_k1*cq_1) + R_k2*cq_2).
 *  5. COUNT of a valid trial: the correspondences i with dot(z, z) <= tau*tau, where for q = q_corr_qry[i], r = r_corr_ref[i]
 *         z_k = (((R_k0*q_0 + R_k1*q_1) + R_k2*q_2) + t_k) - r_k.
 *     A trial that is not valid has count -1.
 *  6. BEST: the largest count, ties to the smaller trial.
 * transform_out: 3x4 row-major [R | t] of the best trial; the identity when no trial is valid.  result (optional): status
 * RH_GLOB_OK or RH_GLOB_NO_TRIAL, best_trial (0-based) and best_count (both -1 with RH_GLOB_NO_TRIAL), n_valid_trials.
 * counts_out (optional): int32 [trials].  The function returns RH_OK with either status.  The _f32 entry widens the
 * coordinates exactly.  The array arguments of the three calls may be host or device pointers (hipMemcpyDefault); params,
 * transform_out and result are host memory.  The same bytes on every run.
 * RH_E_INVALID, before the device is touched: a null ref / qry / corr / params / transform_out, n or m outside the limits
 * of rh_knn_query, c < 3 or c > (2^31 - 1) / 6, trials outside 1 .. RH_GLOBAL_MAX_TRIALS, tau not positive or not finite,
 * edge_ratio outside (0, 1], min_edge negative or not finite; a given triple outside 0 .. c - 1; on the device: a
 * coordinate that is not finite, a correspondence outside 1 .. m / 1 .. n (nothing is written). */
#define RH_DESC_DIM 33
#define RH_DESC_MAX 7938
#define RH_MATCH_MUTUAL 1
#define RH_GLOBAL_MAX_TRIALS (1 << 20)
enum { RH_GLOB_OK = 0, RH_GLOB_NO_TRIAL = 1 };
typedef struct {
    int32_t trials;          /* 1 .. RH_GLOBAL_MAX_TRIALS */
    int32_t reserved;
    uint64_t seed;           /* of the draws; not read when triples are given */
    double tau;              /* > 0: a correspondence agrees when its residual is at most tau */
    double edge_ratio;       /* 0 < e <= 1: the shorter of a pair of edges is at least e times the longer */
    double min_edge;         /* >= 0: every query edge of a triple is at least this long */
} rh_global_params;
typedef struct {
    int32_t status;          /* RH_GLOB_* */
    int32_t best_trial;      /* 0-based; -1: none */
    int32_t best_count;
    int32_t n_valid_trials;
} rh_global_result;
int rh_describe(const double *xyz_aos, const double *nrm_aos, int64_t n, int32_t k, double radius, int device,
                uint16_t *desc_out, int32_t *count_out_or_null);
int rh_describe_f32(const float *xyz_aos, const float *nrm_aos, int64_t n, int32_t k, double radius, int device,
                    uint16_t *desc_out, int32_t *count_out_or_null);
int rh_match_features(const uint16_t *ref_desc, int64_t n, const uint16_t *qry_desc, int64_t m, int32_t flags, int device,
                      int32_t *idx_out, uint32_t *dist_out_or_null);
int rh_register_global(const double *ref_xyz_aos, int64_t n, const double *qry_xyz_aos, int64_t m, const int32_t *corr_qry,
                       const int32_t *corr_ref, int64_t c, const rh_global_params *p, const int32_t *triples_or_null, int device,
                       double *transform_out_3x4, rh_global_result *result_or_null, int32_t *counts_out_or_null);
int rh_register_global_f32(const float *ref_xyz_aos, int64_t n, const float *qry_xyz_aos, int64_t m, const int32_t *corr_qry,
                           const int32_t *corr_ref, int64_t c, const rh_global_params *p, const int32_t *triples_or_null,
                           int device, double *transform_out_3x4, rh_global_result *result_or_null,
                           int32_t *counts_out_or_null);

/* ---- tuning options ----
 * The library reads NO environment variable: what a caller may tune goes through this call, for one cloud or, with
 * cloud = NULL, process-wide (the value a cloud without its own setting sees).  value = RH_OPTION_UNSET clears a setting.
 *   "score_path"  RH_SCORE_PATH_AUTO (default: the culled kernel from 8192 subset points on) / _BRUTE / _GROUPS -- which
 *                 batched score kernel clouds created from now on use (scorecandidates!, src/fitting.jl:181-190); fixed when
 *                 a cloud is created because its internal point order depends on it: process-wide only
 *   "refit_path"  RH_REFIT_PATH_AUTO (default: the culled scan from 2^21 points on) / _SCAN / _CULLED -- which full-cloud
 *                 scan rh_refit and rh_ransac take (refit, src/shapes/plane.jl:137-143); read on every refit
 *   "s4_rows"     0 (default: by the launch's size) / 4 / 8 / 12 / 16 -- 64-candidate chunks per block row of the culled
 *                 score kernel; read on every launch
 *   "unp_words"   0 (default) or the segment width, in 64-bit words, of the pass that turns the score kernel's inlier
 *                 lists into dense subset-order mask rows (inpoints, src/shapes/plane.jl:68); read on every call
 *   "st_cull"     0 (default: by the launch's size) / 1 (whenever possible) / 2 (never) -- a small launch in front of the
 *                 culled score kernel tests every candidate against the boxes of the SUPER-TILES (16 groups of 64 points)
 *                 and leaves per super-tile the list of candidates that may meet it; the score kernel's blocks then walk
 *                 those lists instead of every candidate of the batch.  Read on every launch.
 *   "st_list_mb"  0 (default: 512) or the most MiB the candidate lists of one batch slot may take (8 bytes per super-tile of
 *                 1024 subset points and candidate); a launch that would need more, or whose allocation fails, takes no lists.
 *                 Read on every launch.
 *   "nsig"        0 (default: on) / 2 (off) -- the culled score kernel and its list launch also rule a (plane, group) pair out
 *                 when no point of the group has its normal in one of the 96 direction cells the candidate can accept (masks
 *                 per 64-point group, made once when the cloud is created).  Counts and masks do not depend on it.  Read on
 *                 every launch.
 *   "plane_order" 0 (default: by size, from 256 tiles of 256 subset points on) / 1 (whenever possible) / 2 (never) --
 *                 counts-only launches of the culled score kernel on subset 1 walk their PLANE
 *                 candidates over a second internal order of the subset: inside every node of the position tree with at most
 *                 1024 points the same points, ordered by a k-d tree on their normals, so that a group's normal-cell mask
 *                 holds fewer cells and fewer (plane, group) pairs survive (made once when the cloud is created; about 52
 *                 bytes per subset point).  Counts do not depend on it; launches that write masks never take it.  Read on every launch.
 *   "kd_align"    0 (default: by size, from 1000 tiles of 256 subset points on) / 1 (always) / 2 (never) -- the shape of the
 *                 position k-d tree whose 64-point leaves are the internal order of subset 1: aligned, a node of more than
 *                 1024 points gives its left child a multiple of 1024 points, so that the runs of 1024 consecutive points
 *                 that "st_cull" keeps candidate lists for (and the nodes "plane_order" sorts inside) are nodes of the tree,
 *                 with tighter boxes and shorter lists.  Results do not depend on it.  Read when a cloud is created and
 *                 fixed for its life, like "score_path": process-wide only; setting it on a cloud is RH_E_INVALID, and a
 *                 process-wide change leaves the clouds that exist as they are.
 *   "batches_in_flight"  1 (default) .. 4 -- with F > 1, rh_score_batch_dev calls take turns on the cloud's
 *                 stream and F - 1 more with workspaces of their own, so one batch's prepare + score launches start while
 *                 the previous batches' launches drain.  The caller keeps F count (and mask) buffers and gives call k of a
 *                 run of such calls buffer k mod F (a buffer is written again only by the stream that wrote it last; a call
 *                 that hands in a buffer another batch in flight is writing is simply run after it, alone);
 *                 every other call on the cloud, rh_cloud_sync and rh_timer_stop included, first lets the cloud's stream
 *                 wait for the others, so whatever follows sees every batch's counts.  Ignored while the cloud runs on a
 *                 caller's stream (rh_cloud_set_stream).
 * Results never depend on any of them (tests/test_parity_gpu.py runs every parity test under both score paths).
 * Unknown keys and out-of-range values: RH_E_INVALID.  The diag build (libransac_hip_diag.so, include/ransac_hip_diag.h)
 * knows more keys -- the A/B switches of the experiments -- and falls back to RH_* environment variables; the product
 * build does neither. */
#define RH_OPTION_UNSET INT64_MIN
enum { RH_SCORE_PATH_AUTO = 0, RH_SCORE_PATH_BRUTE = 1, RH_SCORE_PATH_GROUPS = 2 };
enum { RH_REFIT_PATH_AUTO = 0, RH_REFIT_PATH_SCAN = 1, RH_REFIT_PATH_CULLED = 2 };
int rh_set_option(rh_cloud *c_or_null, const char *key, int64_t value);
int rh_get_option(const rh_cloud *c_or_null, const char *key, int64_t *value_out, int32_t *is_set_out_or_null);
int rh_build_variant(void);   /* 0 = product, 1 = diag (-DRH_DIAG) */
/* what the cloud's last batch launch of the culled score kernel looked like (bench.py names the measured kernel with it):
 * out4 = { chunks of 64 candidates per block row, 1 if the rows walked super-tile lists ("st_cull") else 0, rows, tiles } */
int rh_score_launch_info(rh_cloud *c, int32_t *out4);

#ifdef __cplusplus
}
#endif
#endif
