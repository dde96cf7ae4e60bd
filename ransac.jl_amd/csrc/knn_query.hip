// knn_query.hip -- the nearest neighbours of the points of one cloud (the queries) among the points of another (the
// reference), and the cloud-to-cloud distances on them (rh_knn_query, rh_cloud_distance; include/ransac_hip.h states the
// definitions in full).  The search of a query point in another cloud -- the queries' own pass, the radius early-out and
// the epilogues -- is QuerySearch of knn_query_search.h, shared with rh_register.  This file adds the two entry points and
// the stats of rh_cloud_distance: T() of tree_sum.h for mean and rms; maximum and lower median from one radix sort of the
// bit patterns of the non-negative d_j; argmax and n_within by integer atomics.  No floating-point atomics.
// Scratch is allocated per call and freed on every way out (call_scope.h).
#include "knn_query_search.h"
#include "tree_sum.h"

namespace {

// the distance call's scalars on the device
struct DistScal {
    double mean, rms, max, med;
    unsigned long long nvalid, nwithin, argmax;
};

// the sort keys of maximum and median -- the bit pattern of d_j >= +0.0 orders like the value, queries that are not valid
// sort behind everything -- and the number of valid d_j <= threshold
__global__ __launch_bounds__(256) void dist_key_kernel(const double *__restrict__ dist, const int32_t *__restrict__ nn, int64_t m,
                                                       double threshold, uint64_t *__restrict__ key, DistScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool within = false;
    if (i < m) {
        const bool valid = nn[i] > 0;
        const double d = dist[i];
        key[i] = valid ? (uint64_t)__double_as_longlong(d) : ~0ull;
        within = valid && d <= threshold;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(within);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&sc->nwithin, (unsigned long long)__popcll(b));   // an integer count
}

__global__ void dist_scalars_kernel(DistScal *sc, const double *root_sum, const double *root_sq, const uint64_t *sorted, int64_t m)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long nv = sc->nvalid;
    sc->argmax = ~0ull;
    if (!nv || nv > (unsigned long long)m) { sc->mean = sc->rms = sc->max = sc->med = 0.0; return; }
    sc->mean = *root_sum / (double)nv;
    sc->rms = sqrt(*root_sq / (double)nv);
    sc->max = __longlong_as_double((long long)sorted[nv - 1]);
    sc->med = __longlong_as_double((long long)sorted[(nv - 1) / 2]);
}

// the smallest 1-based j reaching the maximum
__global__ void dist_argmax_kernel(const double *__restrict__ dist, const int32_t *__restrict__ nn, int64_t m, DistScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || nn[i] <= 0 || !sc->nvalid) return;
    if (__double_as_longlong(dist[i]) == __double_as_longlong(sc->max)) atomicMin(&sc->argmax, (unsigned long long)(i + 1));
}

template <typename T>
int knn_query(const T *ref_aos, int64_t n, const T *qry_aos, int64_t m, int32_t k, double radius, int device, int32_t *idx_out,
              double *d2_out, int32_t *count_out)
{
    static const char who[] = "rh_knn_query";
    RH_TRY(check_query(who, ref_aos, n, qry_aos, m, k, radius));
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    QuerySearch q;
    RH_TRY(q.open(S, ref_aos, n, qry_aos, m, k, radius));
    if (idx_out) RH_TRY(S.alloc(&q.a.idx, m * k));
    if (d2_out) RH_TRY(S.alloc(&q.a.d2, m * k));
    if (count_out) RH_TRY(S.alloc(&q.a.count, m));
    RH_TRY(q.run(S));
    if (idx_out) SCOPE_HIP(S, hipMemcpyAsync(idx_out, q.a.idx, sizeof(int32_t) * (size_t)m * k, hipMemcpyDefault, st));
    if (d2_out) SCOPE_HIP(S, hipMemcpyAsync(d2_out, q.a.d2, sizeof(double) * (size_t)m * k, hipMemcpyDefault, st));
    if (count_out) SCOPE_HIP(S, hipMemcpyAsync(count_out, q.a.count, sizeof(int32_t) * (size_t)m, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}

template <typename T>
int cloud_distance(const T *ref_aos, const T *nrm_aos, int64_t n, const T *qry_aos, int64_t m, const rh_distance_params *p,
                   int device, double *dist_out, int32_t *nn_out, rh_distance_stats *stats)
{
    static const char who[] = "rh_cloud_distance";
    if (!p || !dist_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    RH_TRY(check_query(who, ref_aos, n, qry_aos, m, 1, p->radius));
    if (p->metric != RH_DIST_POINT && p->metric != RH_DIST_PLANE) {
        rh_set_error("%s: metric = %d is not a distance metric", who, p->metric);
        return RH_E_INVALID;
    }
    if (p->metric == RH_DIST_PLANE && !nrm_aos) { rh_set_error("%s: the plane metric needs the reference's normals", who); return RH_E_INVALID; }
    if (p->threshold != p->threshold) { rh_set_error("%s: threshold is NaN", who); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    QuerySearch q;
    RH_TRY(q.open(S, ref_aos, n, qry_aos, m, 1, p->radius));
    q.a.metric = p->metric;
    if (p->metric == RH_DIST_PLANE) {
        double *d_nrm = nullptr;
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        RH_TRY(S.upload(nrm_aos, d_nrm, 3 * n, hipMemcpyDefault));
        q.a.nrm = d_nrm;
    }
    RH_TRY(S.alloc(&q.a.dist, m));
    RH_TRY(S.alloc(&q.a.nn, m));
    RH_TRY(q.run(S));
    SCOPE_HIP(S, hipMemcpyAsync(dist_out, q.a.dist, sizeof(double) * (size_t)m, hipMemcpyDefault, st));
    if (nn_out) SCOPE_HIP(S, hipMemcpyAsync(nn_out, q.a.nn, sizeof(int32_t) * (size_t)m, hipMemcpyDefault, st));
    if (!stats) {
        SCOPE_HIP(S, hipStreamSynchronize(st));
        return RH_OK;
    }

    // T(d_j) and T(d_j*d_j) over the valid queries, then one sort for maximum and median.  The queries' key buffers are
    // free again: the sort's keys go there.
    DistScal *d_sc = nullptr;
    double *d_part[2] = { nullptr, nullptr }, *d_part2[2] = { nullptr, nullptr };
    RH_TRY(S.alloc(&d_sc, 1));
    RH_TRY(tree_alloc(S, m, d_part));
    RH_TRY(tree_alloc(S, m, d_part2));
    SCOPE_HIP(S, hipMemsetAsync(d_sc, 0, sizeof(DistScal), st));
    const double *d_sum = nullptr, *d_sq = nullptr;
    RH_TRY(tree_root<0>(S, q.a.dist, q.a.nn, m, nullptr, &d_sc->nvalid, d_part, &d_sum));
    RH_TRY(tree_root<3>(S, q.a.dist, q.a.nn, m, nullptr, nullptr, d_part2, &d_sq));
    hipLaunchKernelGGL(dist_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, q.a.dist, q.a.nn, m, p->threshold, q.d_key[0], d_sc);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, q.d_key[0], q.d_key[1], (int)m, 0, 64, st); }));
    hipLaunchKernelGGL(dist_scalars_kernel, dim3(1), dim3(64), 0, st, d_sc, d_sum, d_sq, q.d_key[1], m);
    hipLaunchKernelGGL(dist_argmax_kernel, dim3(blocks_for(m)), dim3(256), 0, st, q.a.dist, q.a.nn, m, d_sc);
    SCOPE_HIP(S, hipGetLastError());
    DistScal h;
    RH_TRY(S.fetch(&h, d_sc));
    stats->n_valid = (int64_t)h.nvalid;
    stats->n_within = (int64_t)h.nwithin;
    stats->argmax = h.argmax == ~0ull ? 0 : (int64_t)h.argmax;
    stats->mean = h.mean; stats->rms = h.rms; stats->max = h.max; stats->median = h.med;
    return RH_OK;
}

}  // namespace

extern "C" int rh_knn_query(const double *ref_xyz_aos, int64_t n, const double *qry_xyz_aos, int64_t m, int32_t k, double radius,
                            int device, int32_t *idx_out_or_null, double *d2_out_or_null, int32_t *count_out_or_null)
{
    return knn_query<double>(ref_xyz_aos, n, qry_xyz_aos, m, k, radius, device, idx_out_or_null, d2_out_or_null, count_out_or_null);
}

extern "C" int rh_knn_query_f32(const float *ref_xyz_aos, int64_t n, const float *qry_xyz_aos, int64_t m, int32_t k, double radius,
                                int device, int32_t *idx_out_or_null, double *d2_out_or_null, int32_t *count_out_or_null)
{
    return knn_query<float>(ref_xyz_aos, n, qry_xyz_aos, m, k, radius, device, idx_out_or_null, d2_out_or_null, count_out_or_null);
}

extern "C" int rh_cloud_distance(const double *ref_xyz_aos, const double *ref_nrm_aos_or_null, int64_t n, const double *qry_xyz_aos,
                                 int64_t m, const rh_distance_params *p, int device, double *dist_out, int32_t *nn_idx_out_or_null,
                                 rh_distance_stats *stats_or_null)
{
    return cloud_distance<double>(ref_xyz_aos, ref_nrm_aos_or_null, n, qry_xyz_aos, m, p, device, dist_out, nn_idx_out_or_null,
                                  stats_or_null);
}

extern "C" int rh_cloud_distance_f32(const float *ref_xyz_aos, const float *ref_nrm_aos_or_null, int64_t n, const float *qry_xyz_aos,
                                     int64_t m, const rh_distance_params *p, int device, double *dist_out,
                                     int32_t *nn_idx_out_or_null, rh_distance_stats *stats_or_null)
{
    return cloud_distance<float>(ref_xyz_aos, ref_nrm_aos_or_null, n, qry_xyz_aos, m, p, device, dist_out, nn_idx_out_or_null,
                                 stats_or_null);
}
