// knn_query.hip -- the nearest neighbours of the points of one cloud (the queries) among the points of another (the
// reference), and the cloud-to-cloud distances on them (rh_knn_query, rh_cloud_distance; include/ransac_hip.h states the
// definitions in full).  The search is the shared one of knn_grid.h / knn_device.h with the query point handed in and
// self = -1: the grid holds the reference only, no point is left out.  This file adds
//   1. the queries' own pass: their bounding box and finiteness (cloud_box), the margin of the distance bounds widened to
//      the box of both clouds, and a radix sort of (clamped reference-cell key, query index), so that the four waves of a
//      block walk the same cells; results are written at the caller's query index;
//   2. the radius early-out: a query farther than the radius from the reference's box ends with an empty list before any
//      shell is walked or the table scanned;
//   3. the epilogues: lanes 0 .. k - 1 of the wave's sorted list as idx / d2 / count, or, for rh_cloud_distance, a list of
//      one turned into d_j / nn_j -- 12 bytes per query, the m x k lists never exist;
//   4. the stats of rh_cloud_distance: T() of tree_sum.h for mean and rms; maximum and lower median from one radix sort of
//      the bit patterns of the non-negative d_j; argmax and n_within by integer atomics.  No floating-point atomics.
// Scratch is allocated per call and freed on every way out (call_scope.h).
#include "knn_device.h"
#include "tree_sum.h"

namespace {

struct XqArgs {
    const double *qxyz;      // the queries, AoS, caller's order
    const int32_t *order;    // wave w serves query order[w]
    double rhi[3];           // the reference box's maximum (its minimum is the grid's origin)
    int32_t *idx;            // list mode: [m x k] or null
    double *d2;              //            [m x k] or null
    int32_t *count;          //            [m] or null
    double *dist;            // distance mode (not null): [m]
    int32_t *nn;             //            [m]
    const double *nrm;       //            the reference's normals, AoS (RH_DIST_PLANE)
    int metric;
};

// the queries' keys: the reference cell nearest to each (cell_of clamps), and their indices
__global__ void xq_key_kernel(Grid g, const double *__restrict__ qxyz, int64_t m, uint64_t *__restrict__ key, int32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t cx = cell_of(qxyz[3 * i], g.o[0], g.h, g.dim[0]);
    const int64_t cy = cell_of(qxyz[3 * i + 1], g.o[1], g.h, g.dim[1]);
    const int64_t cz = cell_of(qxyz[3 * i + 2], g.o[2], g.h, g.dim[2]);
    key[i] = (uint64_t)(cx + g.dim[0] * (cy + g.dim[1] * cz));
    idx[i] = (int32_t)i;
}

__global__ __launch_bounds__(NRM_BLOCK) void xq_kernel(Grid g, KnnQuery kq, XqArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= kq.nq) return;                                       // wave-uniform
    const int64_t j = a.order[w];
    if (j < 0 || j >= kq.nq) return;                              // (wave-uniform) nothing is addressed through a bad index
    const double p[3] = { a.qxyz[3 * j], a.qxyz[3 * j + 1], a.qxyz[3 * j + 2] };
    const int k = kq.k;
    const double radius = kq.radius, r2 = radius * radius;
    double bd = INFINITY;
    uint32_t br = NRM_NORANK;
    bool far = false;
    if (radius > 0.0) {   // farther than the radius from the reference's box: nothing to find, no shell is walked
        double s = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            const double e = p[ax] < g.o[ax] ? g.o[ax] - p[ax] : (p[ax] > a.rhi[ax] ? p[ax] - a.rhi[ax] : 0.0);
            s += e * e;
        }
        far = sqrt(s) - g.margin > radius;
    }
    if (!far) knn_search_point(g, kq, lane, p, -1, bd, br);
    // the list: a prefix of the order, the entries beyond the radius dropped
    const bool in = lane < k && br != NRM_NORANK && (radius <= 0.0 || bd <= r2);
    if (a.dist) {
        if (lane != 0) return;
        double d = INFINITY;
        if (in) {
            d = sqrt(bd);
            if (a.metric == RH_DIST_PLANE) {
                const int64_t ri = (int64_t)br - 1;
                const double ex = p[0] - g.xyz[3 * ri], ey = p[1] - g.xyz[3 * ri + 1], ez = p[2] - g.xyz[3 * ri + 2];
                d = fabs((ex * a.nrm[3 * ri] + ey * a.nrm[3 * ri + 1]) + ez * a.nrm[3 * ri + 2]);
            }
        }
        a.dist[j] = d;
        a.nn[j] = in ? (int32_t)br : 0;                            // rank = index + 1: 1-based already
        return;
    }
    const int cnt = __popcll(__builtin_amdgcn_ballot_w64(in));
    if (lane < k) {
        const int64_t at = j * k + lane;
        if (a.idx) a.idx[at] = in ? (int32_t)br : 0;
        if (a.d2) a.d2[at] = in ? bd : INFINITY;
    }
    if (a.count && lane == 0) a.count[j] = cnt;
}

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

int check_query(const char *who, const void *ref, int64_t n, const void *qry, int64_t m, int k, double radius)
{
    if (!ref || !qry) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= (int64_t)0x7FFFFFFF) { rh_set_error("%s: n = %lld outside 1 .. 2^31 - 2", who, (long long)n); return RH_E_INVALID; }
    if (m < 1 || m > (int64_t)0x7FFFFFFF) { rh_set_error("%s: m = %lld outside 1 .. 2^31 - 1", who, (long long)m); return RH_E_INVALID; }
    if (k < 1 || k > RH_KNN_MAX_K) { rh_set_error("%s: k = %d outside 1 .. %d", who, k, RH_KNN_MAX_K); return RH_E_INVALID; }
    if (!(isfinite(radius) && radius >= 0.0)) { rh_set_error("%s: radius must be finite and >= 0", who); return RH_E_INVALID; }
    return RH_OK;
}

// What a cross query runs on: both clouds on the device and finite, the grid over the reference for lists of k entries
// (no self entry: k, not k + 1), its margin widened to the box of both clouds, the queries in the order of their cells.
struct QuerySearch {
    KnnIndex ix;
    KnnQuery kq;
    Grid g;
    XqArgs a;
    uint64_t *d_key[2] = { nullptr, nullptr };   // the queries' sort buffers, free again after open()
    uint8_t *d_tmp = nullptr;
    size_t tmp_bytes = 0;

    template <typename T>
    int open(CallScope &S, const T *ref_aos, int64_t n, const T *qry_aos, int64_t m, int k, double radius)
    {
        const hipStream_t st = S.st;
        double *d_ref = nullptr, *d_qry = nullptr;
        RH_TRY(S.alloc(&d_ref, 3 * n));
        RH_TRY(S.upload(ref_aos, d_ref, 3 * n, hipMemcpyDefault));   // (the caller's arrays may be on the device already)
        RH_TRY(ix.init(S, d_ref, n));
        RH_TRY(S.alloc(&d_qry, 3 * m));
        RH_TRY(S.upload(qry_aos, d_qry, 3 * m, hipMemcpyDefault));
        double qlo[3], qhi[3];
        RH_TRY(cloud_box(S, d_qry, m, qlo, qhi));
        RH_TRY(knn_index_for_k(ix, k, radius, kq));
        kq.nq = m;
        g = ix.g;
        // p - face and the d^2 of a query are rounded at the magnitude of the query: the margin covers the box of both clouds
        double amax = ix.omax, span = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            amax = std::max(amax, std::max(fabs(qlo[ax]), fabs(qhi[ax])));
            span = std::max(span, std::max(ix.hi[ax], qhi[ax]) - std::min(ix.lo[ax], qlo[ax]));
        }
        g.margin = 1e-12 * (amax + span + g.h);
        memset(&a, 0, sizeof a);
        a.qxyz = d_qry;
        for (int ax = 0; ax < 3; ax++) a.rhi[ax] = ix.hi[ax];

        int32_t *d_idx[2] = { nullptr, nullptr };
        RH_TRY(S.alloc(&d_key[0], m)); RH_TRY(S.alloc(&d_key[1], m));
        RH_TRY(S.alloc(&d_idx[0], m)); RH_TRY(S.alloc(&d_idx[1], m));
        size_t pair_bytes = 0, key_bytes = 0;
        SCOPE_HIP(S, hipcub::DeviceRadixSort::SortPairs(nullptr, pair_bytes, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)m, 0, 64, st));
        SCOPE_HIP(S, hipcub::DeviceRadixSort::SortKeys(nullptr, key_bytes, d_key[0], d_key[1], (int)m, 0, 64, st));
        tmp_bytes = std::max(pair_bytes, key_bytes);
        RH_TRY(S.alloc(&d_tmp, (int64_t)tmp_bytes));
        const uint64_t cells = (uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2];
        int bits = 1;
        while (bits < 64 && (cells - 1) >> bits) bits++;
        hipLaunchKernelGGL(xq_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, g, d_qry, m, d_key[0], d_idx[0]);
        SCOPE_HIP(S, hipGetLastError());
        size_t tb = tmp_bytes;
        SCOPE_HIP(S, hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)m, 0, bits, st));
        a.order = d_idx[1];
        return RH_OK;
    }

    int run(CallScope &S)
    {
        hipLaunchKernelGGL(xq_kernel, dim3(blocks_for(kq.nq, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, S.st, g, kq, a);
        SCOPE_HIP(S, hipGetLastError());
        return RH_OK;
    }
};

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
    size_t tb = q.tmp_bytes;
    SCOPE_HIP(S, hipcub::DeviceRadixSort::SortKeys(q.d_tmp, tb, q.d_key[0], q.d_key[1], (int)m, 0, 64, st));
    hipLaunchKernelGGL(dist_scalars_kernel, dim3(1), dim3(64), 0, st, d_sc, d_sum, d_sq, q.d_key[1], m);
    hipLaunchKernelGGL(dist_argmax_kernel, dim3(blocks_for(m)), dim3(256), 0, st, q.a.dist, q.a.nn, m, d_sc);
    SCOPE_HIP(S, hipGetLastError());
    DistScal h;
    SCOPE_HIP(S, hipMemcpyAsync(&h, d_sc, sizeof h, hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
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
