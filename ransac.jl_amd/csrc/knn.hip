// knn.hip -- exact k nearest neighbours of a raw cloud and outlier removal on them (rh_knn, rh_remove_outliers;
// include/ransac_hip.h states the definitions in full).  The search is the shared one of knn_grid.h / knn_device.h, the
// one rh_estimate_normals runs: a list of k + 1 entries whose first is the point itself.  This file adds
//   1. the query epilogue: lanes 1 .. k of the wave's sorted list written as idx / d2 / count in original point order, or,
//      for outlier removal, only m_i (the mean neighbour distance), count_i and sqrt(d2_i1) -- 20 bytes per point, the
//      n x k lists never exist;
//   2. the tree reductions of mu and sigma: T() of the header, stated once in tree_sum.h.  No floating-point atomics;
//   3. the flag pass and a stable compaction of the kept indices (hipcub's scan-based DeviceSelect);
//   4. the lower median of the nearest-neighbour distances: a radix sort of the bit patterns of the non-negative doubles.
// Scratch is allocated per call and freed on every way out (call_scope.h).
#include "knn_device.h"
#include "tree_sum.h"

namespace {

struct KnnOut {
    int32_t *idx;            // [n x kk] or null
    double *d2;              // [n x kk] or null
    int32_t *count;          // [n] or null
    double *mean;            // [n] or null: outlier mode, with nn1
    double *nn1;             // [n]
};

__global__ __launch_bounds__(NRM_BLOCK) void knn_query_kernel(Grid g, KnnQuery kq, KnnOut o)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= kq.nq) return;                                       // wave-uniform
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, kq, lane, w, p, self, bd, br);
    if (self < 0 || (int64_t)self >= kq.n) return;                // (wave-uniform) nothing is addressed through a bad index
    const int kk = kq.k - 1;                                      // lane 0 is the point itself: d^2 = 0 and rank 0 sort first
    const double r2 = kq.radius * kq.radius;
    // the neighbours: lanes 1 .. kk, those beyond the radius dropped (a prefix of the list)
    const bool in = lane >= 1 && lane <= kk && br != NRM_NORANK && (kq.radius <= 0.0 || bd <= r2);
    const int cnt = __popcll(__builtin_amdgcn_ballot_w64(in));
    if (lane >= 1 && lane <= kk) {
        const int64_t at = (int64_t)self * kk + (lane - 1);
        if (o.idx) o.idx[at] = in ? (int32_t)br : 0;              // rank = index + 1: 1-based already
        if (o.d2) o.d2[at] = in ? bd : INFINITY;
    }
    if (o.count && lane == 0) o.count[self] = cnt;
    if (o.mean) {
        const double v = in ? sqrt(bd) : 0.0;
        const double slot = __shfl(v, (lane + 1) & 63);           // neighbour j in tree slot j - 1 (lane 0 holds +0.0)
        const double s = tree64(slot);
        const double first = __shfl(v, 1);
        if (lane == 0) {
            o.mean[self] = cnt > 0 ? s / (double)cnt : INFINITY;
            o.nn1[self] = first;
        }
    }
}

// the call's scalars on the device
struct OutScal {
    double mu, sigma, tau, med;
    unsigned long long nvalid;
    int32_t nkept;
    int32_t pad;
};

// step 0: mu from the root of the first tree; step 1: sigma from the second's, and tau
__global__ void out_scalars_kernel(OutScal *sc, const double *root, int step, rh_outlier_params p)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long nv = sc->nvalid;
    if (step == 0) {
        sc->mu = nv ? *root / (double)nv : 0.0;
        return;
    }
    sc->sigma = nv >= 2 ? sqrt(*root / (double)(nv - 1)) : 0.0;
    if (p.mode == RH_OUT_STATISTICAL) { const double w = p.std_mul * sc->sigma; sc->tau = sc->mu + w; }
    else sc->tau = p.mode == RH_OUT_ABSOLUTE ? p.threshold : p.radius;
}

// keep flags, and the sort keys of the median: the bit pattern of sqrt(d2_i1) >= +0.0 orders like the value; points
// outside V sort behind everything
__global__ void out_flag_kernel(const double *__restrict__ mean, const double *__restrict__ nn1, const int32_t *__restrict__ count,
                                int64_t n, const OutScal *sc, int mode, int k, uint8_t *__restrict__ keep, uint64_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = count[i];
    keep[i] = mode == RH_OUT_RADIUS ? (c == k) : (c >= 1 && mean[i] <= sc->tau);
    key[i] = c >= 1 ? (uint64_t)__double_as_longlong(nn1[i]) : ~0ull;
}

__global__ void out_median_kernel(OutScal *sc, const uint64_t *sorted, int64_t n)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long nv = sc->nvalid;
    const unsigned long long at = nv ? (nv - 1) / 2 : 0;
    sc->med = (nv && at < (unsigned long long)n) ? __longlong_as_double((long long)sorted[at]) : 0.0;
}

int check_common(const char *who, const void *xyz, int64_t n, int k, double radius)
{
    if (!xyz) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= (int64_t)0x7FFFFFFF) { rh_set_error("%s: n = %lld outside 1 .. 2^31 - 2", who, (long long)n); return RH_E_INVALID; }
    if (k < 1 || k > RH_KNN_MAX_K) { rh_set_error("%s: k = %d outside 1 .. %d", who, k, RH_KNN_MAX_K); return RH_E_INVALID; }
    if (!(isfinite(radius) && radius >= 0.0)) { rh_set_error("%s: radius must be finite and >= 0", who); return RH_E_INVALID; }
    return RH_OK;
}

// upload, bounding box, grid for lists of k + 1 entries
template <typename T>
int open_search(CallScope &S, const T *xyz_aos, int64_t n, int k, double radius, KnnIndex &ix, KnnQuery &kq)
{
    double *d_xyz = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyDefault));   // (the caller's array may be on the device already)
    RH_TRY(ix.init(S, d_xyz, n));
    return knn_index_for_k(ix, k + 1, radius, kq);
}

template <typename T>
int knn(const T *xyz_aos, int64_t n, int32_t k, double radius, int device, int32_t *idx_out, double *d2_out, int32_t *count_out)
{
    static const char who[] = "rh_knn";
    RH_TRY(check_common(who, xyz_aos, n, k, radius));
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    KnnIndex ix;
    KnnQuery kq;
    RH_TRY(open_search(S, xyz_aos, n, k, radius, ix, kq));
    KnnOut o;
    memset(&o, 0, sizeof o);
    if (idx_out) RH_TRY(S.alloc(&o.idx, n * k));
    if (d2_out) RH_TRY(S.alloc(&o.d2, n * k));
    if (count_out) RH_TRY(S.alloc(&o.count, n));
    hipLaunchKernelGGL(knn_query_kernel, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, o);
    SCOPE_HIP(S, hipGetLastError());
    if (idx_out) SCOPE_HIP(S, hipMemcpyAsync(idx_out, o.idx, sizeof(int32_t) * (size_t)n * k, hipMemcpyDefault, st));
    if (d2_out) SCOPE_HIP(S, hipMemcpyAsync(d2_out, o.d2, sizeof(double) * (size_t)n * k, hipMemcpyDefault, st));
    if (count_out) SCOPE_HIP(S, hipMemcpyAsync(count_out, o.count, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}

template <typename T>
int remove_outliers(const T *xyz_aos, int64_t n, const rh_outlier_params *p, int device, uint8_t *keep_out, int32_t *kept_idx_out,
                    int64_t cap, int64_t *n_kept_out, double *mean_dist_out, rh_outlier_stats *stats)
{
    static const char who[] = "rh_remove_outliers";
    if (!p || !keep_out || !n_kept_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    RH_TRY(check_common(who, xyz_aos, n, p->k, p->radius));
    if (p->mode != RH_OUT_STATISTICAL && p->mode != RH_OUT_ABSOLUTE && p->mode != RH_OUT_RADIUS) {
        rh_set_error("%s: mode = %d is not an outlier mode", who, p->mode);
        return RH_E_INVALID;
    }
    if (p->mode == RH_OUT_RADIUS && !(p->radius > 0.0)) { rh_set_error("%s: the radius mode needs radius > 0", who); return RH_E_INVALID; }
    if (p->mode == RH_OUT_STATISTICAL && !isfinite(p->std_mul)) { rh_set_error("%s: std_mul is not finite", who); return RH_E_INVALID; }
    if (p->mode == RH_OUT_ABSOLUTE && p->threshold != p->threshold) { rh_set_error("%s: threshold is NaN", who); return RH_E_INVALID; }
    if (cap < 0 || (cap > 0 && !kept_idx_out)) { rh_set_error("%s: cap = %lld without a list to fill", who, (long long)cap); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    KnnIndex ix;
    KnnQuery kq;
    RH_TRY(open_search(S, xyz_aos, n, p->k, p->radius, ix, kq));

    // 1. m_i, count_i, sqrt(d2_i1)
    KnnOut o;
    memset(&o, 0, sizeof o);
    RH_TRY(S.alloc(&o.mean, n));
    RH_TRY(S.alloc(&o.nn1, n));
    RH_TRY(S.alloc(&o.count, n));
    hipLaunchKernelGGL(knn_query_kernel, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, o);
    SCOPE_HIP(S, hipGetLastError());

    // 2. mu, then sigma and tau
    OutScal *d_sc = nullptr;
    double *d_part[2] = { nullptr, nullptr };
    RH_TRY(S.alloc(&d_sc, 1));
    RH_TRY(tree_alloc(S, n, d_part));
    SCOPE_HIP(S, hipMemsetAsync(d_sc, 0, sizeof(OutScal), st));
    const double *d_root = nullptr;
    RH_TRY(tree_root<0>(S, o.mean, o.count, n, &d_sc->mu, &d_sc->nvalid, d_part, &d_root));
    hipLaunchKernelGGL(out_scalars_kernel, dim3(1), dim3(64), 0, st, d_sc, d_root, 0, *p);
    RH_TRY(tree_root<1>(S, o.mean, o.count, n, &d_sc->mu, &d_sc->nvalid, d_part, &d_root));
    hipLaunchKernelGGL(out_scalars_kernel, dim3(1), dim3(64), 0, st, d_sc, d_root, 1, *p);
    SCOPE_HIP(S, hipGetLastError());

    // 3. flags and the kept indices; 4. the median.  The grid's key buffers are free again: the sort's keys go there.
    uint8_t *d_keep = nullptr;
    int32_t *d_kept = nullptr;
    RH_TRY(S.alloc(&d_keep, n));
    RH_TRY(S.alloc(&d_kept, n));
    uint64_t *d_key = ix.d_key[0], *d_sorted = ix.d_key[1];
    hipLaunchKernelGGL(out_flag_kernel, dim3(blocks_for(n)), dim3(256), 0, st, o.mean, o.nn1, o.count, n, d_sc, (int)p->mode, (int)p->k,
                       d_keep, d_key);
    SCOPE_HIP(S, hipGetLastError());
    hipcub::CountingInputIterator<int32_t> one_based(1);
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceSelect::Flagged(t, b, one_based, d_keep, d_kept, &d_sc->nkept, (int)n, st); }));
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, d_key, d_sorted, (int)n, 0, 64, st); }));
    hipLaunchKernelGGL(out_median_kernel, dim3(1), dim3(64), 0, st, d_sc, d_sorted, n);
    SCOPE_HIP(S, hipGetLastError());

    OutScal h;
    SCOPE_HIP(S, hipMemcpyAsync(&h, d_sc, sizeof h, hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipMemcpyAsync(keep_out, d_keep, (size_t)n, hipMemcpyDefault, st));
    if (mean_dist_out) SCOPE_HIP(S, hipMemcpyAsync(mean_dist_out, o.mean, sizeof(double) * (size_t)n, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    *n_kept_out = h.nkept;
    if (stats) {
        stats->n_valid = (int64_t)h.nvalid;
        stats->n_kept = h.nkept;
        stats->mu = h.mu; stats->sigma = h.sigma; stats->tau = h.tau; stats->nn_median = h.med;
    }
    if (!kept_idx_out) return RH_OK;
    if ((int64_t)h.nkept > cap) {
        rh_set_error("%s: %d points are kept, the list holds %lld", who, h.nkept, (long long)cap);
        return RH_E_CAPACITY;
    }
    if (h.nkept > 0) {
        SCOPE_HIP(S, hipMemcpyAsync(kept_idx_out, d_kept, sizeof(int32_t) * (size_t)h.nkept, hipMemcpyDefault, st));
        SCOPE_HIP(S, hipStreamSynchronize(st));
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_knn(const double *xyz_aos, int64_t n, int32_t k, double radius, int device, int32_t *idx_out_or_null,
                      double *d2_out_or_null, int32_t *count_out_or_null)
{
    return knn<double>(xyz_aos, n, k, radius, device, idx_out_or_null, d2_out_or_null, count_out_or_null);
}

extern "C" int rh_knn_f32(const float *xyz_aos, int64_t n, int32_t k, double radius, int device, int32_t *idx_out_or_null,
                          double *d2_out_or_null, int32_t *count_out_or_null)
{
    return knn<float>(xyz_aos, n, k, radius, device, idx_out_or_null, d2_out_or_null, count_out_or_null);
}

extern "C" int rh_remove_outliers(const double *xyz_aos, int64_t n, const rh_outlier_params *p, int device, uint8_t *keep_out,
                                  int32_t *kept_idx_out_or_null, int64_t cap, int64_t *n_kept_out, double *mean_dist_out_or_null,
                                  rh_outlier_stats *stats_or_null)
{
    return remove_outliers<double>(xyz_aos, n, p, device, keep_out, kept_idx_out_or_null, cap, n_kept_out, mean_dist_out_or_null,
                                   stats_or_null);
}

extern "C" int rh_remove_outliers_f32(const float *xyz_aos, int64_t n, const rh_outlier_params *p, int device, uint8_t *keep_out,
                                      int32_t *kept_idx_out_or_null, int64_t cap, int64_t *n_kept_out,
                                      double *mean_dist_out_or_null, rh_outlier_stats *stats_or_null)
{
    return remove_outliers<float>(xyz_aos, n, p, device, keep_out, kept_idx_out_or_null, cap, n_kept_out, mean_dist_out_or_null,
                                  stats_or_null);
}
