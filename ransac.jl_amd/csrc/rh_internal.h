// rh_internal.h -- internal declarations of libransac_hip.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ransac_hip.h"
#include "dev_buf.h"
#include "enabled_state.h"

// ---- error plumbing -------------------------------------------------------
void rh_set_error(const char *fmt, ...);

#define RH_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            rh_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,   \
                         __LINE__);                                                         \
            return RH_E_NODEVICE;                                                           \
        }                                                                                   \
    } while (0)

#define RH_TRY(call)                 \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != RH_OK) return rc_; \
    } while (0)

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }   // blocks of b that cover a

// ---- options (options.cpp): what rh_set_option stores; the diag build also reads the RH_* environment ---------
enum rh_opt_id {
    RH_OPT_SCORE_PATH = 0,      // product keys (rh_set_option, include/ransac_hip.h)
    RH_OPT_S4_ROWS,
    RH_OPT_UNP_WORDS,
    RH_OPT_ST_CULL,
    RH_OPT_REFIT_PATH,
    RH_OPT_BATCHES_IN_FLIGHT,
    RH_OPT_ST_LIST_MB,
    RH_OPT_NSIG,
    RH_OPT_PLANE_ORDER,
    RH_OPT_KD_ALIGN,
    RH_OPT_N_PRODUCT,
    // A/B switches and diagnostics: alive in the diag build only (in the product build they read as unset)
    RH_OPT_CREATE_PROF = RH_OPT_N_PRODUCT, RH_OPT_AABB_HOST, RH_OPT_SUB_ORDER, RH_OPT_KD_HOST, RH_OPT_NO_SPREAD, RH_OPT_OCT_CHAIN_W,
    RH_OPT_NO_MANAGED_STORE, RH_OPT_OCT_ONE_WINDOW, RH_OPT_OCT_WINDOW_ITERS, RH_OPT_NO_FUSED_SCORE, RH_OPT_NO_PIPELINE,
    RH_OPT_NO_OCT_CHAIN, RH_OPT_REFIT_BLOCKS, RH_OPT_NO_FUSED_SAMPLER, RH_OPT_NO_CREC, RH_OPT_LONG_WINDOW_SETS, RH_OPT_NO_OCT_TAB,
    RH_OPT_NO_DRIVER_CACHE, RH_OPT_HOST_SAMPLER, RH_OPT_DRIVER_PROF, RH_OPT_G2_DBG, RH_OPT_KREFIT_DBG, RH_OPT_NO_FAST_EXTRACT,
    RH_OPT_COUNT
};
struct rh_cloud;
int64_t rh_opt(const rh_cloud *c, int id);               // cloud -> process -> (diag) environment; RH_OPTION_UNSET = nobody said
void rh_opt_init_cloud(rh_cloud *c);
#ifdef RH_DIAG
const char *rh_opt_env_string(const char *name);         // string-valued diagnostics (RH_RCCL_LIB): diag build only
static inline bool rh_opt_on(const rh_cloud *c, int id) { const int64_t v = rh_opt(c, id); return v != RH_OPTION_UNSET && v != 0; }
static inline int64_t rh_opt_int(const rh_cloud *c, int id, int64_t dflt) { const int64_t v = rh_opt(c, id); return v == RH_OPTION_UNSET ? dflt : v; }
#else
// product build: the diag ids are compile-time "unset" -- the A/B branches fold away
static inline bool rh_opt_on(const rh_cloud *c, int id) { if (id >= RH_OPT_N_PRODUCT) return false; const int64_t v = rh_opt(c, id); return v != RH_OPTION_UNSET && v != 0; }
static inline int64_t rh_opt_int(const rh_cloud *c, int id, int64_t dflt) { if (id >= RH_OPT_N_PRODUCT) return dflt; const int64_t v = rh_opt(c, id); return v == RH_OPTION_UNSET ? dflt : v; }
#endif

// ---- device-side candidate record ------------------------------------------
// Per-candidate constants hoisted out of the per-point loop.  Every hoisted value is
// a pure function of the candidate computed with the same IEEE operations the
// reference evaluates per call, so hoisting does not change a single bit.
//   plane    f[0..2]=point  f[3..5]=normal f[6..8]=normalize(normal)   (plane.jl:85)
//   sphere   f[0..2]=center f[3]=R  f[4]=sgn
//   cylinder f[0..2]=axis   f[3..5]=center f[6]=R f[7]=sgn
//   cone     f[0..2]=apex   f[3..5]=axis   f[6]=cos(-w/2) f[7]=sin(-w/2) f[8]=sgn
// sgn = +1.0 (outwards) / -1.0 (inwards); multiplying by it is exact.
struct rh_prep {
    double f[12];
};

// Per-candidate constants of the CONSERVATIVE stages (box tests, band prefilter), in the record's free slots so that
// stage 1 does not recompute them per (chunk, tile): f[11] = sum |f[0..6]| (the magnitude behind box_slack); cylinder:
// f[8] = 1 + |c0|_1, f[9] = k = 2 - |a|^2, f[10] = 1 + |k| |a|^2 (closed-form rho^2 of the prefilter, score_device.h).
__host__ __device__ inline void prep_derived(rh_prep &o, int kind)
{
    o.f[11] = (((((fabs(o.f[0]) + fabs(o.f[1])) + fabs(o.f[2])) + fabs(o.f[3])) + fabs(o.f[4])) + fabs(o.f[5])) + fabs(o.f[6]);
    if (kind == RH_CYLINDER) {
        const double a2 = (o.f[0] * o.f[0] + o.f[1] * o.f[1]) + o.f[2] * o.f[2];
        const double k = 2.0 - a2;
        o.f[8] = (1.0 + fabs(o.f[3])) + (fabs(o.f[4]) + fabs(o.f[5]));
        o.f[9] = k;
        o.f[10] = 1.0 + fabs(k) * a2;
    }
}

// the record of a shape: on the device in the prep kernels, on the host where a candidate is passed by value as a kernel
// argument (both builds: no contraction, IEEE sqrt and divide -- the same bits)
__host__ __device__ __forceinline__ void prep_one(const rh_shape &s, rh_prep &o)
{
#pragma unroll
    for (int i = 0; i < 12; i++) o.f[i] = 0.0;
    const double sgn = s.outwards ? 1.0 : -1.0;
    switch (s.kind) {
    case RH_PLANE: {
        for (int i = 0; i < 6; i++) o.f[i] = s.v[i];
        const double a = s.v[3], b = s.v[4], c = s.v[5];
        const double inv = 1.0 / sqrt((a * a + b * b) + c * c);   // o_z = normalize(plane.normal)
        o.f[6] = inv * a; o.f[7] = inv * b; o.f[8] = inv * c;
        break;
    }
    case RH_SPHERE:
        for (int i = 0; i < 4; i++) o.f[i] = s.v[i];
        o.f[4] = sgn;
        break;
    case RH_CYLINDER:
        for (int i = 0; i < 7; i++) o.f[i] = s.v[i];
        o.f[7] = sgn;
        break;
    default:
        for (int i = 0; i < 6; i++) o.f[i] = s.v[i];
        o.f[6] = s.v[7];   // cos(-opang/2)
        o.f[7] = s.v[8];   // sin(-opang/2)
        o.f[8] = sgn;
        break;
    }
    prep_derived(o, s.kind);
}
inline void rh_prep_host(const rh_shape &s, rh_prep *out) { prep_one(s, *out); }

// The float record of a candidate on a Float32 cloud, from its binary64 record: the record's leading fields are the
// shape's own numbers (+ sgn), so the casts are exact for a Float32 shape, whose fields are binary32 numbers, and one
// rounding for any other; a plane's normalised normal (f[6..8]) is recomputed in binary32 (plane.jl:85 on a Float32
// plane).  Every kernel holds rh_prep records only and derives this one where it runs the binary32 test.
struct rh_prepf {
    float f[12];
};
template <int KIND>
__host__ __device__ inline rh_prepf prepf_of(const rh_prep &P)
{
    rh_prepf o;
    for (int i = 0; i < 9; i++) o.f[i] = (float)P.f[i];
    for (int i = 9; i < 12; i++) o.f[i] = 0.0f;
    if (KIND == RH_PLANE) {
        const float a = o.f[3], b = o.f[4], c = o.f[5];
        const float inv = 1.0f / sqrtf((a * a + b * b) + c * c);
        o.f[6] = inv * a; o.f[7] = inv * b; o.f[8] = inv * c;
    }
    if (KIND == RH_SPHERE) { o.f[5] = o.f[6] = o.f[7] = o.f[8] = 0.0f; }
    if (KIND == RH_CYLINDER) { o.f[8] = 0.0f; }
    return o;
}
__host__ __device__ inline rh_prepf prepf_of_kind(const rh_prep &P, int kind)
{
    switch (kind) {
    case RH_PLANE: return prepf_of<RH_PLANE>(P);
    case RH_SPHERE: return prepf_of<RH_SPHERE>(P);
    case RH_CYLINDER: return prepf_of<RH_CYLINDER>(P);
    default: return prepf_of<RH_CONE>(P);
    }
}

// score kernel geometry (kernels.hip)
constexpr int RH_SC_THREADS = 256;
constexpr int RH_SC_PPT = 4;                             // points per lane
constexpr int RH_SC_WAVE_PTS = 64 * RH_SC_PPT;           // contiguous points per wave per tile
constexpr int RH_SC_TILE = RH_SC_THREADS * RH_SC_PPT;    // points per block per tile
constexpr int RH_SC_CT = 64;                             // candidates per block
constexpr int RH_WORDS_PER_BLOCK = 1024;                 // scan granularity (64-bit words)
constexpr int RH_G2_TG = 4;                              // 64-point groups per LDS tile of the culled score kernel
constexpr int RH_G2_TILE = RH_G2_TG * 64;
constexpr int64_t RH_G2_MIN_POINTS = 8192;               // below this the brute-force kernel is used
// ---- the shape of the position k-d tree of subset 1 (kdorder.hip, cloud.hip).  The shape depends on the
// point count alone, and this is its one statement: the device order, the host order (RH_KD_HOST) and the plane order's
// blocks all split a node of cnt > 64 points where kd_left_count says.
//   today's rule: the left child gets half of the node's whole 64-point groups, rounded up: every split is at a multiple of
//     64, only the last group of the subset is partial;
//   aligned: a node of more than RH_KD_NODE = 1024 points gives its left child half of its 1024-point runs, rounded up, so
//     every node of at most 1024 points is exactly [1024 k, min(s, 1024 (k + 1))): the runs of 16 groups that the candidate
//     lists call super-tiles ARE tree nodes, and the plane order's blocks are the super-tiles.  Below 1024 points today's rule.
// Both children are non-empty for every cnt > 64 (aligned, cnt > 1024: m = ceil(cnt / 1024) >= 2 and (m + 1) / 2 <= m - 1).
constexpr int64_t RH_KD_NODE = 1024;
// The groupings of the culled score path, stated once: 64 points per group, RH_G2_TG groups per tile (what a block stages),
// RH_S4_STG groups per super-tile (what the candidate lists are cut by).  Super-tiles are whole tiles, and a super-tile is a
// k-d node: the aligned tree and the plane order's blocks (kdorder.hip) are correct only while these agree.
constexpr int RH_S4_STG = 16;
static_assert(RH_KD_NODE == RH_S4_STG * 64, "a super-tile is one node of the aligned position tree");
static_assert(RH_S4_STG % RH_G2_TG == 0, "a super-tile is a whole number of tiles");
constexpr int64_t RH_KD_ALIGN_MIN_TILES = 1000;          // "kd_align" by size: subsets of this many 256-point tiles and more (the size from which list launches are taken with batches in flight)
static inline int64_t kd_left_count(int64_t cnt, bool aligned)
{
    if (aligned && cnt > RH_KD_NODE) return (((cnt + RH_KD_NODE - 1) / RH_KD_NODE + 1) / 2) * RH_KD_NODE;
    return ((cnt / 64 + 1) / 2) * 64;
}
// "kd_align" (0 = by size, 1 = always, 2 = never) for a subset of s points
static inline bool kd_aligned_for(int64_t s, int64_t opt)
{
    const int64_t tiles = ((s + 63) / 64 + RH_G2_TG - 1) / RH_G2_TG;
    return opt == 1 || (opt == 0 && tiles >= RH_KD_ALIGN_MIN_TILES);
}
constexpr int64_t RH_KREFIT_MIN = 1 << 21;               // clouds from this size on take the culled refit scan (korder.hip): 1M points 17 us culled against 13 us streaming, 10M 24 against 80

// ---- the cloud --------------------------------------------------------------
struct rh_oct_state;
struct rh_s4_points {   // what the v4 score kernel runs over (score4.hip): points as six planes `stride` apart, 64-point groups + their boxes
    const double *pts;
    int64_t stride, s, ngroups;
    const float *gb32;
};
// Everything that belongs to ONE batch being prepared and scored: its buffers (grown on demand: rh_dev::grow) and what the
// launchers leave in them.  A cloud has RH_MAX_IN_FLIGHT of them (rh_cloud::ws).  ws[0] is the workspace of the cloud's own
// stream: every path but the pipelined rh_score_batch_dev uses it alone.  With rh_set_option "batches_in_flight" = F > 1 the
// batches of rh_score_batch_dev take turns on ws[0 .. F-1], slot k >= 1 on a stream of its own, so one batch's prepare + score
// launches fill the chip while the previous batch's launch drains.  Whatever a launcher needs of a batch it gets as a
// `rh_batch_ws &`; a buffer that is not in here is shared by all batches of the cloud (see "shared by the batches" below).
#define RH_MAX_IN_FLIGHT 4
struct rh_batch_ws {
    // the slot in the pipeline (made by batch_slot_create for slots >= 1; null in ws[0], whose batches run on the cloud's stream)
    hipStream_t stream = nullptr;      // rh_cloud::stream is this one while the slot's batch is queued
    rh_event done, start;   // behind the slot's last batch / where `stream` was ordered behind the cloud's
    bool dirty = false;                // work on `stream` the cloud's own stream has not waited for yet
    bool started = false;              // `stream` has been ordered behind the cloud's stream since the last join
    const void *out_counts = nullptr, *out_masks = nullptr;   // (ws[0] too) the buffers the slot's batch in flight writes (null: none)
    // the bins (rh_ensure_batch) and what the prep kernels leave in them
    int64_t batch_cap = 0;
    rh_dev<rh_shape> d_shapes;         // [batch_cap]
    rh_dev<rh_prep> d_prep;            // [4 * batch_cap], kind-major
    rh_dev<int32_t> d_orig, d_counts;   // [4 * batch_cap], [batch_cap]
    rh_dev<char> d_qpre;               // [4 * batch_cap] classifier records (rh4::rh_cls, 64 B) of the bins in d_prep; culling records: d_box
    rh_dev<float> d_box;               // [RH_BOX_FIELDS][4 * batch_cap] culling records of the same bins (v4 score kernel), structure of arrays
    bool qpre_v4 = false;              // ... made by the last prep kernel (for the thresholds it was given)
    rh_dev<int32_t> d_nk2;             // [8] rh_score_batch_dev's bin sizes: two halves used alternately, each batch zeroes the other
    int nk2_flip = 0;
    bool nk2_ready = false;
    // masks in internal order, before un-permuting (rh_masks_begin / rh_masks_finish).  Culled kernel (masks4): per candidate
    // row a list of (internal word number, inlier word) entries, 16 bytes each, at most one per group (mstride4 of them), and
    // in d_occ one int32 cursor per row, zero between batches.  Brute-force kernels: dense rows.
    rh_dev<uint64_t> d_masks_int;      // (its count: 64-bit words)
    rh_dev<uint8_t> d_occ;             // (bytes)
    int64_t mstride4 = 0;              // (entries)
    bool masks4 = false;
    // per-super-tile candidate lists of the batch being scored (score4.hip, st_cull_kernel): [nst][4 kinds][stlist_cap] slots, [nst][4] counts
    rh_dev<uint16_t> d_stlist;
    rh_dev<int32_t> d_stcount;
    int64_t stlist_cap = 0, stlist_nst = 0;
    int64_t stlist_nomem = 0;          // bytes of the list allocation that failed last (0: none did): not tried again at that size or above
    // mask un-permutation of rows that span 2..16 segments (rhk_unpermute_masks4): per output segment and internal word, the bits
    // that land in the segment.  Built on the slot's own stream, so stream order alone puts it in front of the slot's readers.
    rh_dev<uint64_t> d_segmask;
    int64_t segmask_words = 0;         // ... made for this segment width (0: none yet)
};
// the four kinds' bins of a prepared batch: candidate records, original positions, classifier and culling records
struct rh_bins {
    const rh_prep *prep[4];
    const int32_t *orig[4];
    const void *cls[4];
    const float *box[4];
};
static inline rh_bins rh_bins_at(const rh_prep *prep, const int32_t *orig, const void *cls, const float *box, const int64_t off[4])
{
    rh_bins B;
    for (int k = 0; k < 4; k++) {
        B.prep[k] = prep + off[k];
        B.orig[k] = orig + off[k];
        B.cls[k] = cls ? (const char *)cls + (size_t)off[k] * 64 : nullptr;
        B.box[k] = box ? box + off[k] : nullptr;
    }
    return B;
}
// ... of a workspace the prep kernels filled: bin k at k * batch_cap, the culling records' fields 4 * batch_cap apart
static inline rh_bins rh_ws_bins(const rh_batch_ws &w)
{
    const int64_t off[4] = { 0, w.batch_cap, 2 * w.batch_cap, 3 * w.batch_cap };
    return rh_bins_at(w.d_prep, w.d_orig, w.d_qpre, w.d_box, off);
}
// Everything ONE score launch is told: the launchers below take it whole, a call site fills it in once.
struct rh_score_job {
    rh_bins bins = {};                 // the four kinds' bins ...
    int64_t bstride = 0;               // ... the fields of their culling records this far apart
    const uint64_t *en[4] = { nullptr, nullptr, nullptr, nullptr };   // per kind the enabled words of the point set (null: every point counts): rh_subset_job
    const int32_t *nk[4] = { nullptr, nullptr, nullptr, nullptr };    // per kind the bin's size, on the device
    int32_t bound = 0;                 // >= the candidates of all kinds together (sizes the culled launch)
    int32_t kind_bound[4] = { 0, 0, 0, 0 };   // >= those of each kind (brute-force kernels, the per-kind timing leg)
    const double *eps = nullptr, *cosa = nullptr;   // [4] thresholds the bins' records were made for
    int32_t *d_counts = nullptr;
    uint64_t *d_masks_int = nullptr;   // null: counts only.  Culled kernel: the workspace's entry lists (w.d_occ, w.mstride4)
    rh_s4_points points = { nullptr, 0, 0, 0, nullptr };   // pts null: subset 1 in internal order; else rhk_score4_dis' stretch of the disabled list
    const int32_t *stop = nullptr;     // chained octree windows: the window's stop flag as the score kernel sees it
    bool open_count = false;           // `bound` is a guess (windows of the candidate loop): a tail launch covers a longer list
    hipEvent_t ev_listed = nullptr;    // timed launches: recorded behind the list launch, in front of the score launch
};
struct rh_cloud {
    int64_t opt[RH_OPT_COUNT];         // rh_set_option on this cloud (RH_OPTION_UNSET: the process-wide value holds); rh_opt_init_cloud
    int device = -1;
    hipStream_t stream = nullptr;      // the stream every launch / copy of this cloud goes to (a slot's own while its batch is queued: rh_score_batch_dev)
    hipStream_t own_stream = nullptr;  // created with the cloud; `stream` is this or the caller's (rh_cloud_set_stream)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evk[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // per-kind launch brackets
    hipStream_t copy_stream = nullptr; // rh_ransac: read-back of the extracted index lists, beside the compute stream
    hipEvent_t ev_copied = nullptr;    // idx_out has been read back
    hipEvent_t ev_sync = nullptr;      // rh_ransac: the host's one wait per extraction
    int64_t n = 0, s = 0;
    int64_t n_pad = 0, s_pad = 0;      // padded to RH_SC_TILE
    int64_t nwords = 0, swords = 0;    // ceil(n/64), ceil(s/64)
    int64_t nblocks = 0;               // ceil(nwords / RH_WORDS_PER_BLOCK)

    // HBM layout: six SoA planes of n_pad (resp. s_pad) doubles: x y z nx ny nz
    rh_dev<double> full;               // full cloud, original order
    rh_dev<double> set_ws;             // sampler -> fitter hand-over: gathered minimal sets, [drawN * 6][sets]
    rh_dev<int32_t> set_level;         // per set: octree level it was drawn from, 0 = no set
    int64_t set_ws_sets = 0;
    rh_dev<double> rec;                // the same points as 64-byte records (x y z nx ny nz 0 0): one line per random gather
    rh_dev<double> sub;                // subset 1, subset order
    rh_dev<int32_t> sub_idx0;          // [s] 0-based original index of subset position j
    rh_dev<int32_t> sub_perm;          // [s] internal (k-d leaf order) position -> subset position j
    rh_dev<double> gb;                 // 7 planes x ng_pad: box centre cx cy cz, half extents hx hy hz, radius hr
    int64_t ngroups = 0, ng_pad = 0;   // 64-point groups of the subset (internal order)
    double create_ms[4] = { 0, 0, 0, 0 };   // rh_cloud_create: total, host k-d leaf order of subset 1, everything before it, everything after it
    double coord_mag = 0;              // max |coordinate| over the subset (rounding slack of the bounds)
    double nrm_mag = 0;                // max |normal component| over the subset (margins of the binary32 classifier)
    bool use_groups = false;           // culled scoring path available (s large enough)
    bool kd_aligned = false;           // the position tree of subset 1 has the aligned shape (kd_left_count; "kd_align" when the cloud was created)
    rh_dev<float> gb32;                // the same boxes in binary32, 8 floats per group (v4 score kernel: scalar loads)
    rh_dev<float> st32;                // boxes of the super-tiles (16 consecutive groups = 4 tiles of the k-d leaf order), 8 floats each
    int64_t nst = 0;
    rh_dev<float> tile32;              // boxes of the tiles (4 consecutive groups: what a block of the culled score kernel stages; the diag build's pair census reads them), 8 floats each
    int64_t ntile = 0;
    rh_dev<uint32_t> gm32;             // normal-cell masks of the groups (score4_device.h, nsig_cell): 96 bits in 4 words each, over ALL points of the group -- never rebuilt
    rh_dev<uint32_t> stm32;            // ... of the super-tiles: the OR of their 16 groups' masks, 4 words each
    double nrm_len = 0;                // largest finite normal length over the subset (0: not known), made with the masks
    // The plane order (kdorder.hip): a second internal order of subset 1 that the plane segments of
    // counts-only score launches walk -- inside every node of the position tree with at most 1024 points the same points,
    // ordered by a k-d tree on their NORMALS down to 64-point groups.  Null: the cloud has none (no culled path), planes walk
    // the leaf order.
    rh_dev<double> pl_sub;             // 6 planes x s_pad: subset 1 in plane order
    rh_dev<int32_t> pl_src;            // [s_pad] plane-order position i holds the point of leaf-order position pl_src[i]
    rh_dev<float> pl_gb32;             // binary32 boxes of the plane-order groups, 8 floats each (like gb32)
    rh_dev<uint32_t> pl_gm32;          // normal-cell masks of the plane-order groups, 4 words each (like gm32)
    rh_dev<float> pl_st32;             // boxes of the plane order's super-tiles (16 consecutive groups of ITS order: what the plane lists are cut by), like st32
    rh_dev<uint32_t> pl_stm32;         // ... and their normal-cell masks, like stm32
    rh_dev<uint64_t> pl_enabled;       // [swords] sub_enabled gathered into plane order: rewritten behind every change of sub_enabled, on its stream
    rh_dev<double> dis_gb;             // boxes of the dis segment in use (7 x ng_pad)

    // The enabled bits and what follows them: `en` says which derived structure matches the bits (enabled_state.h, DESIGN.md
    // section 3).  Only enabled.hip writes `enabled` and names block_sums / d_total.
    rh_enabled_state en;
    rh_dev<uint64_t> enabled;          // [nwords]  pc.isenabled chunks
    rh_dev<uint64_t> sub_enabled;      // [swords]  enabled bits gathered into subset order
    rh_dev<double> dis;                // disabled subset-1 points (append-only), capacity s_pad + tile
    int64_t dis_stride = 0;
    rh_dev<int32_t> d_ndis;            // device counter: entries in dis
    int64_t n_dis = 0;                 // host mirror: exact outside a run; inside rh_ransac as of the last extraction's read-back
    rh_dev<uint64_t> oct_men;          // [nwords] the Morton-order mirror of the bits (en.has_mirror; else regathered on its next use)
    rh_dev<int32_t> oct_prefix;        // [nwords + 1] its popcount prefix (rhk_oct_sync_enabled)
    rh_dev<int32_t> en_block_sums;     // [nblocks + 1] popcounts of the enabled words per block (en.has_block_sums), scanned in place by the directory
    rh_dev<int32_t> word_prefix;       // [nwords + 1] the select directory: exclusive prefix of popcount(enabled); its total is d_total (en.has_directory)
    rh_dev<int32_t> sel_list;          // sel_list[r] = 0-based index of the (r+1)-th enabled point (en.has_list; built on demand)
    rh_dev<double> crec;               // 64-byte records (8 doubles each) of the ENABLED points in rank order (en.has_records; long sampling windows)
    rh_dev<int32_t> block_sums;        // [nblocks + 1] the scan scratch, lent out by rhk_take_scan_scratch ...
    rh_dev<int32_t> d_total;           // ... and its scalar: the directory's total until somebody else takes it

    // The cloud in Morton order (korder.hip), built on the device with the cloud: the order of the linear octree of
    // octree_sampling = 1 and of the culled refit scan.
    bool k_built = false;
    double k_lo[3] = { 0, 0, 0 }, k_size = 1;   // bounding cube of the cloud (findAABB, utilities.jl:125-136)
    double k_mag = 0;                  // max |coordinate| over the cloud (rounding slack of the box tests)
    rh_dev<double> fullk;              // 6 planes x n_pad, Morton order
    rh_dev<float> fullk32;             // the same as float (Float32 clouds)
    rh_dev<double> kgb;                // 7 planes x kg_pad: box of every 64 consecutive points of fullk
    int64_t kg_pad = 0;
    rh_dev<int32_t> klist;             // [nwords] groups that survive the box test of the scan in flight
    rh_dev<int32_t> kctr;              // [2] list length (zero between scans)
    rh_dev<uint8_t> kflag;             // [n_pad] one byte per point, original order: inlier of the scan in flight (zero between scans)
    bool oct_built = false;            // depth + host twins of the octree (rh_octree_ensure)
    int oct_depth = 0, oct_max_depth = 0;
    rh_dev<uint64_t> oct_code;         // [n] sorted Morton codes (device)
    rh_dev<int32_t> oct_perm;          // [n] Morton position -> original index0
    rh_dev<int32_t> oct_pos;           // [n] original index0 -> Morton position
    rh_dev<rh_oct_state> oct_state;    // chained octree windows: the window's state,
    rh_dev<float> dis_gb32;            // binary32 twins of dis_gb
    rh_dev<unsigned long long> s4_stats;   // diag build: event counters of the score launches (rh_dbg_s4_stats), 128 x u64 on the device
    rh_dev<int32_t> oct_adv_tab;       //   the (level, slot) table of rhk_oct_advance, its bitmap (kept zero) and the sorted scores
    rh_dev<unsigned long long> oct_adv_bits;
    int64_t oct_adv_cells = 0;
    rh_dev<double> oct_adv_E;
    rh_dev<uint64_t> oct_code_o;       // [n] the Morton codes in original point order (built with oct_tab)
    rh_dev<int32_t> oct_tab;           // first Morton position of every level-oct_tab_level cell (+ n at the end)
    int oct_tab_level = 0;
    rh_dev<double> oct_P;              // level distributions of a speculation window
    std::vector<uint64_t> h_oct_code;  // host twins (host-side sampling, enabled mirror)
    std::vector<int32_t> h_oct_perm, h_oct_pos;

    // refit workspaces
    rh_dev<uint64_t> refit_mask;       // [nwords]
    rh_dev<int64_t> idx_out;           // [n] compacted indices

    // largest-connected-component filter of a refit set (component.hip): the setting rh_ransac's extractions read
    // (rh_cloud_set_component_filter; 0: off) and the workspace, grown on demand and kept between calls
    double comp_beta = 0;
    int32_t comp_conn26 = 1;
    rh_dev<char> comp_tab;             // the cell table: per slot key (8 B), parent, point count, smallest index (4 B each)
    int64_t comp_cap = 0;              // in slots
    rh_dev<uint64_t> comp_scal;        // the call's scalars on the device (minimum, maximum, |I|, winner, components) ...
    rh_pinned<uint64_t> comp_h;        // ... and where the host reads the first seven (pinned)

    // oriented extents of extracted shapes (extent.hip): workspaces, grown on demand and kept between calls
    rh_dev<double> ext_part;           // one row of partial sums / minima / maxima per chunk of list entries
    int64_t ext_part_rows = 0;
    rh_dev<int32_t> ext_flag;          // the call's error word (RH_EXT_BAD_* bits of extent.hip), raised by the kernels
    rh_dev<char> ext_in;               // the host entry's uploads: shapes, offsets, records, index lists

    // per-point labels (assign.hip): workspaces, grown on demand and kept between calls
    rh_dev<char> asg_ws;               // prepared shape records, the lists' count matrix, label totals and offsets
    rh_dev<char> asg_io;               // the host entry's shapes and its outputs on their way to the host

    // the batch workspaces: ws[0] the cloud's own, ws[1 ..] the other slots of rh_score_batch_dev's pipeline (rh_batch_ws)
    rh_batch_ws ws[RH_MAX_IN_FLIGHT];
    uint32_t pipe_k = 0;               // batches since the pipeline (re)started

    // Shared by the batches: state of the scoring path that is per CLOUD, although batches on several streams go through the
    // code that touches it.  Why each is safe to share:
    //   d_nk, d_masks, d_zero, ev_cull / last_cull_ms: only touched by calls that join the slots first and run on ws[0]
    //     (rh_score_batch, rh_score_batch_dev_timed, rh_ransac's windows) -- no other batch is in flight then.
    //   last_s4: host-side record of the last sized batch launch, whichever slot it was on (a cloud is used by one host thread at a time).
    // Whatever else a score launch is told travels in its rh_score_job.
    rh_dev<int32_t> d_nk;              // [4] bin sizes of a batch whose sizes the host uploads (rh_score_batch) or the sampler leaves (rh_ransac)
    rh_dev<uint64_t> d_masks;          // rh_score_batch: the masks in subset order on their way to the host (grown on demand)
    rh_dev<int32_t> d_zero;            // 64 zero bytes: the bin size a kind left out of a launch reads (per-kind timing leg)
    hipEvent_t ev_cull = nullptr;      // timed launches (rh_score_batch_dev_timed): behind the list launch, in front of the score launch
    float last_cull_ms = 0.f;
    int32_t last_s4[4] = { 0, 0, 0, 0 };   // the last sized batch launch of the culled score kernel: R, lists taken (0 / 1), rows, tiles (rh_score_launch_info)

    rh_dev<int64_t> d_ranks;           // select in/out

    // Float32 clouds (rh_cloud_create_f32): float copies of the two point sets (fullk32: the Morton-order twin of full32)
    bool f32 = false;
    bool f32_groups = false;           // scored by the culled kernel; else by the brute-force kernel (both: exact test in binary32)
    rh_dev<float> full32;              // 6 planes x n_pad, original order (the refit scan streams these: 24 B per point)
    rh_dev<float> sub32;               // 6 planes x s_pad, subset 1 in k-d leaf order (the brute-force batch score reads these)

    // rh_ransac_mp: this process's share of every iteration's minimal sets (set j belongs to rank j % world)
    int32_t mp_rank = 0, mp_world = 1;
#ifdef RH_DIAG
    // what the last rhk_sample_fit launched (rh_dbg_sample_fit): kernels (1 ranks-fused, 2 oct-fused, 3 two-kernel),
    // DN instantiation, CONE instantiation, select list handed over, compact records handed over, cell directory handed over
    int32_t dbg_sampler_path[6] = { 0, 0, 0, 0, 0, 0 };
#endif

    // rh_ransac's reusable buffers, parked here between calls (driver.hip owns the layout and the deleter)
    void *drv_cache = nullptr;
    void (*drv_cache_free)(rh_cloud *, void *) = nullptr;

    // rh_score_batch with host buffers: device twin of the pinned staging block of a small batch (one upload)
    rh_dev<char> d_stage;

    // pinned staging
    rh_pinned<char> h_pin;
};

// the job of scoring prepared bins (sizes: d_nk[0 .. 3]) against subset 1 with p's thresholds; the caller adds the bounds, the
// outputs and whatever else its launch is told.  The one place that says which enabled words a kind's scorer applies:
// sphere.jl:121,131 -- the sphere scorer builds `ens` and never applies it, so faithful mode counts every point
static inline rh_score_job rh_subset_job(const rh_cloud *c, const rh_params *p, const rh_bins &bins, int64_t bstride, const int32_t *d_nk)
{
    rh_score_job J;
    J.bins = bins;
    J.bstride = bstride;
    for (int k = 0; k < 4; k++) {
        J.en[k] = (k == RH_SPHERE && !p->sphere_uses_enabled) ? nullptr : c->sub_enabled.get();
        J.nk[k] = d_nk + k;
    }
    J.eps = p->eps;
    J.cosa = p->cos_alpha;
    return J;
}

// liveness pass over a small store (rhk_liveness_small): per kind the prepared candidates, their number, where
// their flags start, and the first entry of the disabled list they have to be tested against
struct rh_live_args {
    const rh_prep *prep[4];
    int32_t nk[4], base[4];
    int64_t first[4];
    double eps[4], cosa[4];
    int32_t f32 = 0;     // Float32 cloud: the binary32 tests
};

// ---- kernel launchers (kernels.hip) -----------------------------------------
int rhk_transpose_aos(rh_cloud *c, const double *d_aos_xyz, const double *d_aos_nrm, int64_t n,
                      const int32_t *d_gather_or_null, int64_t count, double *dst, int64_t dst_stride);
int rhk_fetch2_i32(rh_cloud *c, const int32_t *d_src0, const int32_t *d_src1, int32_t *h_pinned_dst);   // h[0..1] = *d0, *d1 in stream order (pinned h)
int rhk_pack_records(rh_cloud *c, const double *d_xyz, const double *d_nrm, int64_t n, double *d_rec);
// The prep launchers fill the bins of the workspace they are given (w.d_prep / w.d_orig, bin k at k * w.batch_cap); with eps +
// cosa they also leave the bins' classifier / culling records in w.d_qpre / w.d_box and say so in w.qpre_v4.
int rhk_prep_sorted(rh_cloud *c, rh_batch_ws &w, int32_t b, int32_t *d_counts_to_zero = nullptr, const double *eps = nullptr,
                    const double *cosa = nullptr);   // w.d_shapes[0 .. b), sorted by kind -> w.d_prep, slot for slot
int rhk_prep_records(rh_cloud *c, const rh_shape *d_shapes, int32_t b, rh_prep *d_prep);   // d_shapes[0 .. b) -> d_prep, slot for slot, and nothing else
struct rh_cand_entry;
struct rh_oct_state;
int rhk_prep_entries(rh_cloud *c, rh_batch_ws &w, const rh_cand_entry *d_entries, const int32_t *d_count, int32_t cap_entries,
                     int32_t launch_bound, int32_t *d_counts, int nk_is_zero, const double *eps = nullptr,
                     const double *cosa = nullptr, const rh_oct_state *ost = nullptr);   // bin sizes: c->d_nk
int rhk_prep_binned(rh_cloud *c, rh_batch_ws &w, const rh_shape *d_shapes, int32_t b, int32_t *d_nk, int32_t *d_counts_to_zero,
                    int32_t *d_nk_other, int nk_is_zero, const double *eps = nullptr, const double *cosa = nullptr,
                    int32_t *zero_extra = nullptr, int32_t zero_extra_n = 0);   // the launch also zeroes zero_extra_n ints from zero_extra
bool rh_score_v4_enabled(const rh_cloud *c);
// culled path (k-d leaf order + per-group boxes): all kinds in one launch of score4.hip's kernel over job.points.  w: the
// super-tile lists of the launch and, with masks, the entry lists they leave it as (job.d_masks_int = w.d_masks_int, cursors
// w.d_occ, rows w.mstride4 apart: rhk_unpermute_masks4).  launch_info (optional): a sized launch (not open_count) leaves its
// R, lists taken (0 / 1), rows and tiles there.
int rhk_score4_all(rh_cloud *c, rh_batch_ws &w, const rh_score_job &job, int32_t *launch_info = nullptr);
int rhk_unpermute_masks4(rh_cloud *c, rh_batch_ws &w, int32_t b, uint64_t *d_out);   // unpermute4.hip: w's entry lists -> dense rows
// (functions that only join the units of the score path are kept out of the library's dynamic symbols)
#define RH_UNIT_LOCAL __attribute__((visibility("hidden")))
RH_UNIT_LOCAL bool rhk_plane_order_wanted(const rh_cloud *c);   // score4.hip: "plane_order" -- do plane candidates walk the plane order of subset 1?
// score nk candidates of one kind; nk_host < 0: count is only known on the device (d_nk),
// launch for an upper bound of nk_bound candidates
int rhk_score_kind(rh_cloud *c, int kind, const double *pts, int64_t stride, int64_t s,
                   const uint64_t *enabled_words_or_null, const rh_prep *d_prep, const int32_t *d_orig,
                   const int32_t *d_nk, int32_t nk_bound, double eps, double cosa, int32_t *d_counts,
                   uint64_t *d_masks_or_null, int64_t mask_stride);
int rhk_score_kind(rh_cloud *c, int kind, const float *pts, int64_t stride, int64_t s,   // ... over float planes (Float32 cloud: sub32)
                   const uint64_t *enabled_words_or_null, const rh_prep *d_prep, const int32_t *d_orig,
                   const int32_t *d_nk, int32_t nk_bound, double eps, double cosa, int32_t *d_counts,
                   uint64_t *d_masks_or_null, int64_t mask_stride);
int rhk_gb32_build(rh_cloud *c);   // (boxes32.hip: gb32 / st32 / tile32 / gm32 / stm32 and nrm_len from gb and sub)
// boxes32.hip, queued on c->stream: the binary32 boxes of ng groups from their binary64 ones (7 planes c->ng_pad apart), and
// of the nruns runs of k consecutive groups of subset 1
RH_UNIT_LOCAL void rhk_gb32_of(rh_cloud *c, const double *gb, int64_t ng, float *gb32);
RH_UNIT_LOCAL void rhk_runs32_of(rh_cloud *c, const double *gb, int k, int64_t nruns, float *out);
int rhk_store_cls(rh_cloud *c, const rh_prep *const prep[4], const int32_t n[4], const int32_t pbase[5], const double eps[4],
                  const double cosa[4], void *d_cls, float *d_box, int64_t bstride);
int rhk_score4_dis(rh_cloud *c, int64_t first, int64_t cnt, rh_score_job job);   // the same over dis[first, first + cnt): fills in job.points
int rhk_cloud_aabb(rh_cloud *c, const double *d_xyz, int64_t n, double lo[3], double hi[3], bool has[3], double *mag);   // kdorder.hip
int rhk_kd_order(rh_cloud *c, const double *d_xyz, const double *d_nrm, const int32_t *d_idx0);   // kdorder.hip: subset 1's k-d leaf order on the device
int rhk_plane_order_build(rh_cloud *c);     // kdorder.hip: the plane order of subset 1 from c->sub (pl_sub, pl_src, then rhk_plane_boxes)
int rhk_plane_enabled_sync(rh_cloud *c);    // kdorder.hip: pl_enabled from sub_enabled, on the cloud's stream (no plane order: nothing)
int rhk_plane_boxes(rh_cloud *c);           // boxes32.hip: pl_gb32 / pl_gm32 / pl_st32 / pl_stm32 from pl_sub
int rhk_score_kind_dis(rh_cloud *c, int kind, int64_t first, int64_t cnt, const rh_prep *d_prep, const int32_t *d_orig,
                       const int32_t *d_nk, int32_t nk_bound, double eps, double cosa, int32_t *d_counts);
int rhk_group_bounds(rh_cloud *c);
int rhk_unpermute_masks(rh_cloud *c, const uint64_t *d_in, int32_t b, uint64_t *d_out);
// refit_mask = the shape's inliers among the enabled points (original order), by the cloud's element type; `apply`: the
// caller follows up with rhk_enabled_apply_refit, so a culled scan may clear the Morton-order enabled bits on the way
int rhk_refit_mask(rh_cloud *c, const rh_prep &P, int kind, double eps, double cosa, bool apply = false);
// korder.hip
int rhk_korder_build(rh_cloud *c, const double *d_xyz, const double *d_nrm, const double lo[3], double size, double mag);
int rhk_f32_build(rh_cloud *c);   // full32, sub32 (the caller's allocations) and fullk32 of a Float32 cloud
bool rhk_refit_is_culled(const rh_cloud *c);
int rhk_refitk_mask(rh_cloud *c, const rh_prep &P, int kind, double eps, double cosa, bool apply);
int rhk_group_bounds_of(rh_cloud *c, const double *pts, int64_t stride, int64_t count, int64_t ngroups, double *gb, int64_t gstride);
int rhk_oct_build_tab(rh_cloud *c);                                     // the sampler's cell directory (needs oct_depth)
// component.hip: refit_mask &= the largest connected component of its points on the voxel grid of size beta (one wait for
// the stream: |I| sizes the table); the number of components follows in stream order
int rhk_component_filter(rh_cloud *c, double beta, int conn26, int64_t *n_refit_out);
int rhk_component_stats(rh_cloud *c, int64_t *h_ncomp);
int rhk_liveness_small(rh_cloud *c, int64_t lo, int64_t span, const rh_live_args &A, int32_t *d_flags);   // flags must be zero on entry
int rhk_pack_live(rh_cloud *c, int32_t *d_flags, int32_t n_flags, int32_t *h_flags, int32_t *h_scalars);
uint64_t rh_rng_next_raw(rh_rng *r);   // fit.cpp: the next raw 64-bit draw (an injected stream first)
int rhk_iota(rh_cloud *c, int32_t *d, int32_t n, int32_t base);
int rhk_gather_prep(rh_cloud *c, const rh_prep *src, const int32_t *d_idx, int32_t n, rh_prep *dst);
// removeinvalidshapes! (fitting.jl:209-221) on a device-managed store (driver.hip, chained octree windows): the store's
// entries carry the host's candidate number (id); an entry dies when its liveness count is non-zero or it is the
// extracted candidate.  The survivors move to the spare arrays in order, the ids of the dead ones go to the host.
// Index space: the kinds laid end to end, each padded to a multiple of RH_STORE_PAD (pbase[q]; pbase[4] = the end).
constexpr int RH_STORE_PAD = 256;
struct rh_store_plan {
    const rh_prep *prep[4];
    rh_prep *spare[4];
    const int32_t *id[4];
    int32_t *spare_id[4];
    const double *E[4];          // the entries' scores: the first maximum over the survivors is found on the way
    double *spare_E[4];
    int32_t n[4], pbase[5];
    const int32_t *counts;       // liveness counts at pbase[q] + slot
    int32_t extracted_id;
};
// d_work: 2 * (pbase[4] / RH_STORE_PAD) + 16 ints of scratch; h_out (pinned): [0..3] the kinds' new lengths, [4] the number
// of dead entries; h_dead (pinned): their ids, in no particular order; h_best (pinned, one per block of RH_STORE_PAD
// entries): the block's best survivor -- greatest score, smallest id among equals; id < 0: none
struct rh_store_best { double E; long long id; };
// d_dead (>= the store's entries), d_best (one per block): device staging of the two lists (flushed to the pinned ones by a last small kernel)
int rhk_store_compact(rh_cloud *c, const rh_store_plan &P, int32_t *d_work, int32_t *h_out, int32_t *h_dead, rh_store_best *h_best,
                      int32_t *d_dead, rh_store_best *d_best);

int rhk_compact_generic(hipStream_t stream, const uint64_t *mask, int64_t nwords, int32_t *ws_block_sums,
                        int64_t *idx_out, int64_t cap, int32_t *d_total, int32_t *word_prefix_out = nullptr);

// ---- the enabled bits and what follows them (enabled.hip; the protocol: enabled_state.h) -------
int rhk_enabled_alloc(rh_cloud *c);
int rhk_enabled_replace(rh_cloud *c, const uint64_t *chunks);           // every word from the host's chunks (null: all ones)
int rhk_enabled_clear_list(rh_cloud *c, const int64_t *d_idx, int64_t n);   // invalidate_indexes! of a device list; waits
int rhk_enabled_apply_refit(rh_cloud *c);                               // idx_out = list of refit_mask, enabled &= ~refit_mask
int rhk_enabled_resync(rh_cloud *c);                                    // start of rh_ransac: the disabled list from scratch
void rhk_enabled_run_ended(rh_cloud *c);
const int32_t *rhk_fold_total(const rh_cloud *c);                       // (device) the list length of the last apply_refit
struct rh_scan_scratch { int32_t *sums, *total; };
rh_scan_scratch rhk_take_scan_scratch(rh_cloud *c);                     // block_sums / d_total lent to a scan that is not the directory's: reports "scratch taken"
int rhk_refit_total(rh_cloud *c, const char *who, int64_t *host_out, int64_t cap, int64_t *total_out, hipEvent_t ev = nullptr);
int rhk_ensure_select(rh_cloud *c);                                     // the select directory, built unless c->en has it
int rhk_build_sel_list(rh_cloud *c);
int rhk_enabled_total(rh_cloud *c, int32_t *count);
int rhk_select(rh_cloud *c, const int64_t *d_ranks, int32_t k, int64_t *d_out);   // (this and the next: the directory must be built)
int rhk_sample_sets_seq(rh_cloud *c, const uint64_t *d_raw, int32_t L, int32_t drawN, int64_t *d_rec);   // rh_sample_sets
int rhk_count_enabled(rh_cloud *c, int64_t *out);
int rhk_korder_sync_enabled(rh_cloud *c);                               // oct_men = enabled in Morton order, unless it is already
int rhk_oct_sync_enabled(rh_cloud *c);                                  // ... and oct_prefix

// device-side sampling + fitting (sampler.hip)
struct rh_cand_entry {
    int64_t slot;     // ((iteration - k0) * minsubsetN + set) * n_shape_types + type index
    int32_t level;    // octree level the set was drawn from (1 = root)
    int32_t pad;
    rh_shape shape;
};
// State of a CHAINED octree window on the device (driver.hip, run_streams_device): the iterations of the window are
// queued back to back -- sample, fit, prepare, score, rhk_oct_advance -- and the level scores / level distribution
// the next iteration samples from are advanced on the device, so the host is not in the loop between iterations.
struct rh_oct_state {
    double S[32], P[32];          // pc.levelscore, pc.levelweight: as the NEXT iteration of the window finds them
    double best_E;                // the best stored score (findhighestscore), has_best != 0
    long long store_count, cc2;   // stored candidates / candidates scored so far
    rh_prep *store_prep[4];       // the device store of prepared candidates (driver.hip): arrays per kind, their capacities and
    double *store_E[4];           //   (with the candidates' scores)
    int32_t *store_id[4];         //   fill -- every iteration appends its candidates' records and their numbers on the host
    long long store_cap[4];       //   (appended + the candidate's rank in candidate order)
    long long appended;
    int32_t store_n[4];
    int32_t has_best;
    int32_t stop;                 // an iteration's extraction test passed (approximately: the host decides): the rest of the window is skipped
    int32_t start;                // list position where the entries of the next iteration begin
    int32_t it_done;              // iterations of the window that ran
};
// d_P: null (root-cell sampling) or n_iters x oct_depth level distributions.  Chained octree windows launch one
// iteration at a time: n_iters = 1, it0 = its index in the window (slots, draw counters), ost = the window's state
// (d_P = ost->P; a set stop flag skips the launch).
int rhk_sample_fit(rh_cloud *c, const rh_params *prm, uint64_t seed, int64_t k0, int32_t n_iters, int32_t n_enabled,
                   const double *d_P, rh_cand_entry *d_out, int32_t cap, void *d_status, int status_is_zero,
                   int32_t *d_nk_zero, int32_t it0 = 0, const rh_oct_state *ost = nullptr);
// What the host gets per iteration of a chained window (pinned memory, written by rhk_oct_advance's kernel)
struct rh_oct_iter_hdr {
    int32_t skipped;              // the window had ended before this iteration: nothing else is valid
    int32_t overflow;             // bit 0: the candidate list is full, bit 1: the device store is: the iteration is incomplete (the window ends here)
    int32_t gave_up;              // sampling found no enabled point
    int32_t start, end;           // the iteration's entries in the list (and in the pinned copies of the list and the counts)
    int32_t stop_after;           // the device expects an extraction after this iteration (it skips the rest of the window)
    int32_t pad[2];
    unsigned long long draws;     // random numbers the iteration consumed
    double P[32];                 // the level distribution after the iteration
#ifdef RH_OCT_TIMING
    unsigned long long t[8];      // phase times of the kernel (100 MHz ticks)
#endif
};
// end of an iteration of a chained octree window: levelscore[level] += E(candidate) in candidate order (fitting.jl:184),
// updatelevelweight (octree.jl:198-205), the running best score and the (approximate) extraction test; the iteration's
// entries and counts are copied to h_entries / h_counts (same positions as in the list), h_rank gets every entry's rank
// in candidate order within the iteration, the prepared records go behind the device store (ost->store_*) with h_slot
// saying where, and h_hdr[it] is filled.
// it = index of the iteration in the window, k = its number.
int rhk_oct_window_begin(rh_cloud *c, rh_oct_state *ost);   // a window that continues from the device's state: list position 0
int rhk_oct_advance(rh_cloud *c, const rh_params *prm, rh_oct_state *ost, const rh_cand_entry *d_entries, const void *d_status,
                    int32_t cap, const int32_t *d_counts, int32_t it, int64_t k, rh_cand_entry *h_entries, int32_t *h_counts,
                    int32_t *h_rank, int32_t *h_slot, rh_oct_iter_hdr *h_hdr);
// status block, head of the list and of its counts -> pinned host memory; zeroes the status block
int rhk_pack_window(rh_cloud *c, void *d_status, int32_t n_iters, const rh_cand_entry *d_entries, const int32_t *d_counts,
                    int32_t head_cap, void *h_status, void *h_entries, int32_t *h_counts);
int rh_octree_ensure(rh_cloud *c, const double *xyz, int max_depth);   // cloud.hip

int32_t rh_spread_multiplier(int32_t b);   // t -> (t * m) mod b: a permutation of the batch that separates neighbours

// ---- host helpers (cloud.hip) -----------------------------------------------
// (a device buffer of the cloud grows through rh_dev::grow on c->stream, the stream of the workspace in use)
int rh_ensure_batch(rh_cloud *c, rh_batch_ws &w, int64_t b);
// rh_score_batch_dev whose prepare launch also zeroes zero_extra_n ints from zero_extra (null: nothing besides the counts)
int rh_score_batch_dev_zeroing(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p, int32_t *d_counts, uint64_t *d_masks,
                               int32_t *zero_extra, int32_t zero_extra_n);
int rh_join_batches(rh_cloud *c);   // the cloud's stream waits for what the other batch slots have in flight ("batches_in_flight")
int rh_cloud_join(rh_cloud *c);     // the same with the cloud's device made current first (options.cpp)
int rh_ensure_pin(rh_cloud *c, int64_t bytes);
// the level distributions of a window: room for `need` doubles, `cap` of them when the buffer has to grow
static inline int rh_ensure_oct_P(rh_cloud *c, int64_t need, int64_t cap) { return need > c->oct_P.count() ? c->oct_P.grow(c->stream, cap) : RH_OK; }
int rh_validate_params(const rh_params *p);
