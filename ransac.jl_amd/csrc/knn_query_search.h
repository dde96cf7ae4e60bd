// knn_query_search.h -- the search of a query point in ANOTHER cloud, stated once for rh_knn_query, rh_cloud_distance
// (knn_query.hip) and rh_register (register.hip).  The search itself is the shared one of knn_grid.h / knn_device.h with
// the query point handed in and self = -1: the grid holds the reference only, no point is left out.  Here are
//   1. the queries' own pass: their bounding box and finiteness (cloud_box), the margin of the distance bounds widened to
//      the box of both clouds, and a radix sort of (clamped reference-cell key, query index), so that the four waves of a
//      block walk the same cells; results are written at the caller's query index;
//   2. the radius early-out: a query farther than the radius from the reference's box ends with an empty list before any
//      shell is walked or the table scanned;
//   3. the epilogues: lanes 0 .. k - 1 of the wave's sorted list as idx / d2 / count, or a list of one turned into
//      d_j / nn_j -- 12 bytes per query, the m x k lists never exist.
// QuerySearch opens the reference once (upload, grid) and binds a query array as often as the caller likes (box, margin,
// keys, sort): rh_register binds the moved queries of every iteration to one grid.
// Everything lives in an anonymous namespace: each translation unit that includes the header gets its own kernels.
#pragma once

#include "knn_device.h"

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

inline int check_query(const char *who, const void *ref, int64_t n, const void *qry, int64_t m, int k, double radius)
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
//   open_reference()  once: the reference on the device, its box, the grid;
//   reserve()         once: the buffers of a query pass over m points;
//   bind()            per query array of those m points: box, margin, keys, sort -- nothing is allocated (the first sort sizes the
//                     scope's scratch block, CallScope::cub);
//   run()             the search of the bound queries.
// open() is the four in a row for a call with one query array.
struct QuerySearch {
    KnnIndex ix;
    KnnQuery kq;
    Grid g;
    XqArgs a;
    int64_t m = 0;
    uint64_t *d_key[2] = { nullptr, nullptr };   // the queries' sort buffers, free again after bind()
    int32_t *d_idx[2] = { nullptr, nullptr };
    unsigned long long *d_box = nullptr;

    template <typename T>
    int open_reference(CallScope &S, const T *ref_aos, int64_t n, int k, double radius)
    {
        double *d_ref = nullptr;
        RH_TRY(S.alloc(&d_ref, 3 * n));
        RH_TRY(S.upload(ref_aos, d_ref, 3 * n, hipMemcpyDefault));   // (the caller's arrays may be on the device already)
        RH_TRY(ix.init(S, d_ref, n));
        RH_TRY(knn_index_for_k(ix, k, radius, kq));
        memset(&a, 0, sizeof a);
        for (int ax = 0; ax < 3; ax++) a.rhi[ax] = ix.hi[ax];
        return RH_OK;
    }

    int reserve(CallScope &S, int64_t m_)
    {
        m = m_;
        RH_TRY(S.alloc(&d_box, cloud_box_words(m)));
        RH_TRY(S.alloc(&d_key[0], m)); RH_TRY(S.alloc(&d_key[1], m));
        RH_TRY(S.alloc(&d_idx[0], m)); RH_TRY(S.alloc(&d_idx[1], m));
        return RH_OK;
    }

    int bind(CallScope &S, const double *d_qry)
    {
        const hipStream_t st = S.st;
        double qlo[3], qhi[3];
        RH_TRY(cloud_box(S, d_qry, m, qlo, qhi, d_box));
        kq.nq = m;
        g = ix.g;
        // p - face and the d^2 of a query are rounded at the magnitude of the query: the margin covers the box of both clouds
        double amax = ix.omax, span = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            amax = std::max(amax, std::max(fabs(qlo[ax]), fabs(qhi[ax])));
            span = std::max(span, std::max(ix.hi[ax], qhi[ax]) - std::min(ix.lo[ax], qlo[ax]));
        }
        g.margin = 1e-12 * (amax + span + g.h);
        a.qxyz = d_qry;
        const int bits = sort_bits((uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2]);
        hipLaunchKernelGGL(xq_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, g, d_qry, m, d_key[0], d_idx[0]);
        SCOPE_HIP(S, hipGetLastError());
        RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)m, 0, bits, st); }));
        a.order = d_idx[1];
        return RH_OK;
    }

    template <typename T>
    int open(CallScope &S, const T *ref_aos, int64_t n, const T *qry_aos, int64_t m_, int k, double radius)
    {
        RH_TRY(open_reference(S, ref_aos, n, k, radius));
        double *d_qry = nullptr;
        RH_TRY(S.alloc(&d_qry, 3 * m_));
        RH_TRY(S.upload(qry_aos, d_qry, 3 * m_, hipMemcpyDefault));
        RH_TRY(reserve(S, m_));
        return bind(S, d_qry);
    }

    int run(CallScope &S)
    {
        hipLaunchKernelGGL(xq_kernel, dim3(blocks_for(kq.nq, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, S.st, g, kq, a);
        SCOPE_HIP(S, hipGetLastError());
        return RH_OK;
    }
};

}  // namespace
