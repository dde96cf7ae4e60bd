// segment.hip -- region growing by smoothness for a cloud with normals (rh_segment_smooth; include/ransac_hip.h states the
// definition in full): rh_cluster's three kinds with seeds for core points, smooth neighbour pairs for the eps-neighbourhood
// and "nearest seed" for the border rule, so that nothing depends on a seed order or on which region reaches a point first.
//   check    one thread per point: V and seed flags, the refused normals counted (as ori_check_kernel does)
//   search   the shared search (knn_grid.h / knn_device.h, lists of k + 1 entries), one wave per point, with an epilogue of
//            its own: lanes 1 .. k test their neighbour for a smooth pair and write its index into the int32 [n x k] list,
//            "smooth" in the top bit, -1 for no neighbour.  The lists never leave the device
//   unite    one lane per list slot (coalesced list reads).  Both ends seeds and the pair smooth: uf_unite on parents
//            indexed by ORIGINAL index, so that a region's root is its smallest seed.  Exactly one end a seed: the bit
//            pattern of d2 is offered to the other end, a 64-bit unsigned atomicMin (non-negative doubles order as
//            integers).  A slot is directed, the pair is not: either end may be the seed
//   pick     the same walk: the offers whose d2 equals the minimum offer the seed's index, a 32-bit atomicMin -- the
//            (d2, index) minimum without a 96-bit atomic
//   root     root[i] = uf_find(i) for a seed, uf_find(best_i) for a border point, -1 otherwise; kind[]
//   tail     root_labels.h: sizes, the min_size filter, the numbering, labels, stats and lists
// Nothing waits on another block; uf_unite's retry loop (union_find.h) is the only loop without a static bound.  No
// floating-point atomics: every output is a comparison of binary64 values or an integer.
#include "knn_device.h"
#include "root_labels.h"
#include "union_find.h"

namespace {

constexpr uint32_t SEG_NOSLOT = 0xFFFFFFFFu;    // no neighbour (an index is below 2^31 - 2: bit 31 | index never reads so)
constexpr uint32_t SEG_SMOOTH = 0x80000000u;
constexpr int32_t SEG_NONE = 0x7FFFFFFF;
constexpr uint8_t SEG_V = 1, SEG_SEED = 2;

// the call's scalars on the device, beside the tail's
struct SegScal {
    unsigned long long n_bad, n_invalid;
};

struct SegJob {
    int64_t n;
    int32_t kk;              // list slots per point
    int32_t unsgn;           // RH_SEG_UNSIGNED
    double cos_angle, dist_max;
    const double *xyz, *nrm; // [3n] by original index
    const uint8_t *state;    // [n] SEG_V | SEG_SEED
    uint32_t *list;          // [n x kk]
    int32_t *parent;         // [n] by original index
    unsigned long long *best_d2;   // [n] the smallest offer, as bits
    int32_t *best_j;         // [n] the smallest seed among the offers of that d2
    int32_t *root;           // [n] the region's smallest seed, -1 = none
    uint8_t *kind;           // [n]
};

// V, the seeds, and the components that are refused
__global__ void seg_check_kernel(const double *__restrict__ nrm, const double *__restrict__ curv, int64_t n, double curv_max,
                                 uint8_t *__restrict__ state, SegScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, out = false;
    if (i < n) {
        const double x = nrm[3 * i], y = nrm[3 * i + 1], z = nrm[3 * i + 2];
        bad = !(isfinite(x) && isfinite(y) && isfinite(z)) || fabs(x) > 2.0 || fabs(y) > 2.0 || fabs(z) > 2.0;
        const bool v = !bad && !(x == 0.0 && y == 0.0 && z == 0.0);
        const bool seed = v && (curv == nullptr || curv[i] <= curv_max);   // (a NaN compares false: no seed)
        out = !v;
        state[i] = (uint8_t)((v ? SEG_V : 0) | (seed ? SEG_SEED : 0));
    }
    const uint64_t bb = __builtin_amdgcn_ballot_w64(bad), bo = __builtin_amdgcn_ballot_w64(out);
    if ((threadIdx.x & 63) == 0) {
        if (bb) atomicAdd(&sc->n_bad, (unsigned long long)__popcll(bb));
        if (bo) atomicAdd(&sc->n_invalid, (unsigned long long)__popcll(bo));
    }
}

__global__ void seg_init_kernel(SegJob J)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= J.n) return;
    J.parent[i] = (int32_t)i;
    J.best_d2[i] = ~0ULL;
    J.best_j[i] = SEG_NONE;
}

// step 3 of the definition for the pair (i, j), p = p_i; bit-symmetric in i and j
__device__ __forceinline__ bool seg_smooth(const SegJob &J, const double p[3], int64_t i, int64_t j)
{
    const double *a = J.nrm + 3 * i, *b = J.nrm + 3 * j;
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
    const double dot = (ax * bx + ay * by) + az * bz;
    bool ok = (J.unsgn ? fabs(dot) : dot) >= J.cos_angle;
    if (J.dist_max > 0.0) {
        const double dx = J.xyz[3 * j] - p[0], dy = J.xyz[3 * j + 1] - p[1], dz = J.xyz[3 * j + 2] - p[2];
        const double ei = (ax * dx + ay * dy) + az * dz;
        const double ej = (bx * (-dx) + by * (-dy)) + bz * (-dz);
        ok = ok && fabs(ei) <= J.dist_max && fabs(ej) <= J.dist_max;
    }
    return ok;
}

// the search's epilogue: the list of wave w's point, kk slots
__global__ __launch_bounds__(NRM_BLOCK) void seg_search_kernel(Grid g, KnnQuery kq, SegJob J)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= kq.nq) return;                                       // wave-uniform
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, kq, lane, w, p, self, bd, br);
    if (self < 0 || (int64_t)self >= J.n) return;                 // (wave-uniform) nothing is addressed through a bad index
    if (lane < 1 || lane > J.kk) return;
    const double r2 = kq.radius * kq.radius;
    const bool in = br != NRM_NORANK && br >= 1u && (kq.radius <= 0.0 || bd <= r2);
    const uint32_t j = br - 1u;                                   // rank = index + 1
    uint32_t slot = SEG_NOSLOT;
    if (in && (int64_t)j < J.n && j != (uint32_t)self) {
        const bool both = (J.state[self] & SEG_V) != 0 && (J.state[j] & SEG_V) != 0;
        slot = j | ((both && seg_smooth(J, p, self, j)) ? SEG_SMOOTH : 0u);
    }
    J.list[(int64_t)self * J.kk + (lane - 1)] = slot;
}

// PICK = false: unite and the d2 offers.  PICK = true: the index offers at the smallest d2.
template <bool PICK>
__global__ __launch_bounds__(256) void seg_walk_kernel(SegJob J, int64_t nk)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nk) return;
    const uint32_t e = J.list[t];
    if (e == SEG_NOSLOT || (e & SEG_SMOOTH) == 0) return;
    const int32_t i = (int32_t)((uint32_t)t / (uint32_t)J.kk);    // (nk < 2^31)
    const int32_t j = (int32_t)(e & ~SEG_SMOOTH);
    if ((int64_t)i >= J.n || (int64_t)j >= J.n) return;           // nothing is addressed through a bad index
    const bool si = (J.state[i] & SEG_SEED) != 0, sj = (J.state[j] & SEG_SEED) != 0;
    if (si && sj) {
        if (!PICK && ld(&J.parent[i]) != ld(&J.parent[j])) uf_unite(J.parent, i, j);
        return;
    }
    if (!si && !sj) return;
    const int32_t s = si ? i : j, b = si ? j : i;                 // the seed, and the end it is offered to
    const double dx = J.xyz[3 * (int64_t)j] - J.xyz[3 * (int64_t)i], dy = J.xyz[3 * (int64_t)j + 1] - J.xyz[3 * (int64_t)i + 1],
                 dz = J.xyz[3 * (int64_t)j + 2] - J.xyz[3 * (int64_t)i + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;              // (bit-symmetric: the differences only change sign)
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
    if (!PICK) atomicMin(&J.best_d2[b], bits);
    else if (bits == J.best_d2[b]) atomicMin(&J.best_j[b], s);
}

__global__ __launch_bounds__(256) void seg_root_kernel(SegJob J)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= J.n) return;
    const uint8_t st = J.state[i];
    int32_t from = SEG_NONE;
    if (st & SEG_SEED) from = (int32_t)i;
    else if (st & SEG_V) from = J.best_j[i];
    const bool has = from >= 0 && (int64_t)from < J.n;
    J.root[i] = has ? uf_find(J.parent, from) : -1;
    J.kind[i] = (st & SEG_SEED) ? RH_PT_CORE : (has ? RH_PT_BORDER : RH_PT_NOISE);
}

template <typename T>
int segment(const char *who, const T *xyz_aos, const T *nrm_aos, const T *curv, int64_t n, const rh_segment_params *p, int device,
            int32_t *labels_out, uint8_t *kind_out, int64_t cap, int64_t *counts_out, int64_t *offsets_out, int64_t *idx_out,
            int64_t *n_regions_out, rh_segment_stats *stats)
{
    if (!xyz_aos || !nrm_aos || !p || !labels_out || !n_regions_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= (int64_t)0x7FFFFFFF) { rh_set_error("%s: n = %lld outside 1 .. 2^31 - 2", who, (long long)n); return RH_E_INVALID; }
    if (p->k < 1 || p->k > RH_KNN_MAX_K) { rh_set_error("%s: k = %d outside 1 .. %d", who, p->k, RH_KNN_MAX_K); return RH_E_INVALID; }
    if ((p->flags & ~RH_SEG_UNSIGNED) != 0) { rh_set_error("%s: flags = %d holds an unknown bit", who, p->flags); return RH_E_INVALID; }
    if (!(isfinite(p->radius) && p->radius >= 0.0)) { rh_set_error("%s: radius must be finite and >= 0", who); return RH_E_INVALID; }
    if (!(p->cos_angle >= -1.0 && p->cos_angle <= 1.0)) { rh_set_error("%s: cos_angle must lie in [-1, 1]", who); return RH_E_INVALID; }
    if (p->curv_max != p->curv_max) { rh_set_error("%s: curv_max is NaN", who); return RH_E_INVALID; }
    if (!(isfinite(p->dist_max) && p->dist_max >= 0.0)) { rh_set_error("%s: dist_max must be finite and >= 0", who); return RH_E_INVALID; }
    if (p->min_size < 1) { rh_set_error("%s: min_size = %d: it is >= 1", who, p->min_size); return RH_E_INVALID; }
    if (p->order != RH_CLUSTER_BY_INDEX && p->order != RH_CLUSTER_BY_SIZE) { rh_set_error("%s: order = %d is not a numbering", who, p->order); return RH_E_INVALID; }
    if (cap < 0) { rh_set_error("%s: cap = %lld", who, (long long)cap); return RH_E_INVALID; }
    const int k = p->k;
    const int64_t nk = n * k;
    if (nk >= ((int64_t)1 << 31)) { rh_set_error("%s: n * k = %lld list slots, the limit is 2^31 - 1", who, (long long)nk); return RH_E_INVALID; }

    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;

    // the cloud, the normals, the curvature (binary64 for every decision), V and the seeds
    double *d_xyz = nullptr, *d_nrm = nullptr, *d_curv = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.alloc(&d_nrm, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyDefault));   // (the caller's arrays may be on the device already)
    RH_TRY(S.upload(nrm_aos, d_nrm, 3 * n, hipMemcpyDefault));
    if (curv) {
        RH_TRY(S.alloc(&d_curv, n));
        RH_TRY(S.upload(curv, d_curv, n, hipMemcpyDefault));
    }
    SegScal *d_ss = nullptr, hs;
    RootScal *d_sc = nullptr;
    uint8_t *d_state = nullptr;
    RH_TRY(S.alloc(&d_ss, 1));
    RH_TRY(S.alloc(&d_sc, 1));
    RH_TRY(S.alloc(&d_state, n));
    SCOPE_HIP(S, hipMemsetAsync(d_ss, 0, sizeof(SegScal), st));
    SCOPE_HIP(S, hipMemsetAsync(d_sc, 0, sizeof(RootScal), st));
    hipLaunchKernelGGL(seg_check_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_nrm, d_curv, n, p->curv_max, d_state, d_ss);
    SCOPE_HIP(S, hipGetLastError());

    // the search (it refuses a coordinate that is not finite) and the lists
    KnnIndex ix;
    KnnQuery kq;
    RH_TRY(ix.init(S, d_xyz, n));
    RH_TRY(S.fetch(&hs, d_ss));
    if (hs.n_bad != 0) { rh_set_error("%s: a normal component is not finite or exceeds 2 in magnitude", who); return RH_E_INVALID; }
    RH_TRY(knn_index_for_k(ix, k + 1, p->radius, kq));
    SegJob J;
    J.n = n; J.kk = k; J.unsgn = (p->flags & RH_SEG_UNSIGNED) != 0;
    J.cos_angle = p->cos_angle; J.dist_max = p->dist_max;
    J.xyz = d_xyz; J.nrm = d_nrm; J.state = d_state;
    RH_TRY(S.alloc(&J.list, nk));
    RH_TRY(S.alloc(&J.parent, n)); RH_TRY(S.alloc(&J.best_d2, n)); RH_TRY(S.alloc(&J.best_j, n));
    RH_TRY(S.alloc(&J.root, n)); RH_TRY(S.alloc(&J.kind, n));
    SCOPE_HIP(S, hipMemsetAsync(J.list, 0xFF, sizeof(uint32_t) * (size_t)nk, st));
    hipLaunchKernelGGL(seg_init_kernel, dim3(blocks_for(n)), dim3(256), 0, st, J);
    hipLaunchKernelGGL(seg_search_kernel, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, J);
    SCOPE_HIP(S, hipGetLastError());

    // regions, border points, roots
    hipLaunchKernelGGL(seg_walk_kernel<false>, dim3(blocks_for(nk)), dim3(256), 0, st, J, nk);
    hipLaunchKernelGGL(seg_walk_kernel<true>, dim3(blocks_for(nk)), dim3(256), 0, st, J, nk);
    hipLaunchKernelGGL(seg_root_kernel, dim3(blocks_for(n)), dim3(256), 0, st, J);
    SCOPE_HIP(S, hipGetLastError());

    // the tail; the search is over, so both key arrays of the grid are free
    RootTail tl;
    tl.what = "regions";
    tl.d_root = J.root; tl.d_kind = J.kind; tl.n = n;
    tl.min_size = p->min_size; tl.by_size = p->order == RH_CLUSTER_BY_SIZE; tl.cap = cap;
    tl.d_sc = d_sc; tl.d_mkey = ix.d_key[0]; tl.d_msorted = ix.d_key[1];
    tl.labels_out = labels_out; tl.kind_out = kind_out; tl.counts_out = counts_out; tl.offsets_out = offsets_out; tl.idx_out = idx_out;
    return root_labels(S, tl, [&](const RootScal &r, int64_t m) {
        *n_regions_out = m;
        if (stats) {
            stats->n_regions = m;
            stats->n_seed = (int64_t)r.n_core; stats->n_border = (int64_t)r.n_border;
            stats->n_invalid = (int64_t)hs.n_invalid;
            stats->n_unassigned = (int64_t)r.n_noise - (int64_t)hs.n_invalid;   // (a point outside V has kind RH_PT_NOISE)
            stats->n_small = (int64_t)r.n_small; stats->largest = r.largest;
        }
    });
}

}  // namespace

extern "C" int rh_segment_smooth(const double *xyz_aos, const double *nrm_aos, const double *curv_or_null, int64_t n,
                                 const rh_segment_params *p, int device, int32_t *labels_out, uint8_t *kind_out_or_null, int64_t cap,
                                 int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null,
                                 int64_t *n_regions_out, rh_segment_stats *stats_or_null)
{
    return segment<double>("rh_segment_smooth", xyz_aos, nrm_aos, curv_or_null, n, p, device, labels_out, kind_out_or_null, cap,
                           counts_out_or_null, offsets_out_or_null, idx_out_or_null, n_regions_out, stats_or_null);
}

extern "C" int rh_segment_smooth_f32(const float *xyz_aos, const float *nrm_aos, const float *curv_or_null, int64_t n,
                                     const rh_segment_params *p, int device, int32_t *labels_out, uint8_t *kind_out_or_null, int64_t cap,
                                     int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null,
                                     int64_t *n_regions_out, rh_segment_stats *stats_or_null)
{
    return segment<float>("rh_segment_smooth_f32", xyz_aos, nrm_aos, curv_or_null, n, p, device, labels_out, kind_out_or_null, cap,
                          counts_out_or_null, offsets_out_or_null, idx_out_or_null, n_regions_out, stats_or_null);
}
