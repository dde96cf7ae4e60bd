// knn_device.h -- the exact k-nearest-neighbour query over the grid of knn_grid.h, one wave per query point:
//   lane j holds the j-th best (d^2, rank) pair, rank 0 = the point itself (a self query), rank i + 1 = point i (so ties
//   go to the smaller index), d^2 = (dx*dx + dy*dy) + dz*dz in binary64.  The cells of shell s (Chebyshev distance s from the query's cell)
//   stream their points in 64 at a time; a batch with a candidate below the k-th best is sorted (bitonic, __shfl_xor) and
//   merged with the best list.  The search stops when the k-th best d^2 is below the squared distance to the faces of the
//   cube searched so far (or beyond the radius), so the result is exact.  A point whose next shell would enumerate more
//   cells than the hash table has slots scans the table instead (every occupied cell not yet visited, pruned by its box
//   distance): isolated points end, and end exact.
// knn_search_point() is that loop, for any query point; knn_search() runs it for a point of the cloud itself.  A kernel
// calls one of them and goes on with its own epilogue over the wave's sorted list (the PCA of normals.hip, the lists and
// mean distances of knn.hip, the cross-cloud lists and distances of knn_query.hip).  knn_index_for_k() chooses the cell
// width for a list length.
#pragma once

#include "knn_grid.h"

namespace {

__device__ inline bool key_less(double ad, uint32_t ar, double bd, uint32_t br)
{
    return ad < bd || (ad == bd && ar < br);
}

// one compare-exchange of a bitonic network across lanes lane and lane ^ j
__device__ inline void cmpx(double &d, uint32_t &r, int j, bool take_min)
{
    const double od = __shfl_xor(d, j);
    const uint32_t orr = (uint32_t)__shfl_xor((int)r, j);
    if (key_less(od, orr, d, r) == take_min) { d = od; r = orr; }
}

// merge one batch (d, r per lane; NRM_NORANK = none) into the ascending best list (bd, br per lane)
__device__ inline void merge_batch(int lane, int k, double d, uint32_t r, double &bd, uint32_t &br)
{
    const double kd = __shfl(bd, k - 1);
    const uint32_t kr = (uint32_t)__shfl((int)br, k - 1);
    const bool keep = r != NRM_NORANK && key_less(d, r, kd, kr);
    if (__builtin_amdgcn_ballot_w64(keep) == 0) return;
    if (!keep) { d = INFINITY; r = NRM_NORANK; }
    for (int sz = 2; sz <= 64; sz <<= 1)
        for (int j = sz >> 1; j > 0; j >>= 1)
            cmpx(d, r, j, ((lane & j) == 0) == ((lane & sz) == 0));
    const double rd = __shfl(d, 63 - lane);
    const uint32_t rr = (uint32_t)__shfl((int)r, 63 - lane);
    if (key_less(rd, rr, bd, br)) { bd = rd; br = rr; }
    for (int j = 32; j > 0; j >>= 1) cmpx(bd, br, j, (lane & j) == 0);
}

// every lane brings one cell's [st, st + cnt); their points go through merge_batch 64 at a time
__device__ void stream_cells(const Grid &g, int lane, int k, int32_t st, int32_t cnt, const double p[3], int32_t self,
                             double &bd, uint32_t &br)
{
    int32_t inc = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t v = __shfl_up(inc, d);
        if (lane >= d) inc += v;
    }
    const int32_t total = __shfl(inc, 63);
    const int32_t pre = inc - cnt;
    for (int32_t b = 0; b < total; b += 64) {
        const int32_t gi = b + lane;
        int lo = 0;                                  // the last cell whose prefix is <= gi (all lanes shuffle)
        for (int step = 32; step > 0; step >>= 1) {
            const int32_t v = __shfl(pre, lo + step < 64 ? lo + step : 63);
            if (lo + step < 64 && v <= gi) lo += step;
        }
        const int32_t cst = __shfl(st, lo), cpre = __shfl(pre, lo);
        double d = INFINITY;
        uint32_t r = NRM_NORANK;
        if (gi < total) {
            const int32_t q = cst + (gi - cpre);
            const double dx = g.sx[q] - p[0], dy = g.sy[q] - p[1], dz = g.sz[q] - p[2];
            d = (dx * dx + dy * dy) + dz * dz;
            const int32_t oi = g.sidx[q];
            r = oi == self ? 0u : (uint32_t)oi + 1u;
        }
        merge_batch(lane, k, d, r, bd, br);
    }
}

__device__ inline void hash_find(const Grid &g, uint64_t key, int32_t &st, int32_t &cnt)
{
    const int64_t sl = table_find(g.hkey, (uint32_t)g.mask, key);
    if (sl < 0) { st = 0; cnt = 0; return; }
    st = g.hrange[2 * sl];
    cnt = g.hrange[2 * sl + 1] - st;
}

// lower bound of the distance from p to the box of cell (cx, cy, cz), lowered by the margin
__device__ __forceinline__ double cell_lb(const Grid &g, const double p[3], const int64_t c[3])
{
    double s = 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = g.o[a] + (double)c[a] * g.h, hi = g.o[a] + (double)(c[a] + 1) * g.h;
        const double e = p[a] < lo ? lo - p[a] : (p[a] > hi ? p[a] - hi : 0.0);
        s += e * e;
    }
    const double d = sqrt(s) - g.margin;
    return d > 0.0 ? d : 0.0;
}

__device__ inline bool skip_cell(double lb, double kd, double radius)
{
    return lb * lb > kd || (radius > 0.0 && lb > radius);
}

struct KnnQuery {
    int64_t nq;              // query points (waves)
    int64_t n;
    int k;                   // length of the list, the point itself included (<= 64)
    int sample;              // 1: query w is sorted point w*n/nq (the cell-width sample); 0: sorted point w
    double radius;
    int smax;                // last shell enumerated cell by cell; beyond it the hash table is scanned
};

// The search for query point p (wave-uniform): on return lane j holds the j-th entry of p's order in (bd, br) -- br =
// NRM_NORANK where the cloud has fewer points.  self is the index of the reference point that is p itself and ranks first
// (rank 0) whatever its d^2; self = -1: p is no point of the grid's cloud (a cross query, knn_query.hip), nothing is
// excluded and rank = index + 1 throughout.
// p need not lie inside the grid's box: cell_of clamps, so c is the cell nearest to p along every axis.  cell_lb is the
// distance to a cell's box wherever p is.  The bound `inner` below stays a lower bound for a clamped cell: along an axis
// where p lies below the box, c = 0, so the cube's lower face is the grid's boundary and is not used (no point lies beyond
// it), and its upper face o + (s + 1) h lies above p, so every unseen point beyond that face is at least face - p away;
// above the box the same holds with the sides exchanged.  g.margin must cover the rounding of p - face at p's magnitude:
// a cross query enlarges it by the query box (enlarging the margin never changes a result, it only prunes less).
__device__ inline void knn_search_point(const Grid &g, const KnnQuery &a, int lane, const double p[3], int32_t self,
                                        double &bd, uint32_t &br)
{
    int64_t c[3];
    for (int ax = 0; ax < 3; ax++) c[ax] = cell_of(p[ax], g.o[ax], g.h, g.dim[ax]);
    const int k = a.k;
    const double radius = a.radius;
    bd = INFINITY;
    br = NRM_NORANK;

    for (int s = 0;; s++) {
        if (s > a.smax) {   // scan every occupied cell outside the cube already searched
            const double kd0 = __shfl(bd, k - 1);
            for (uint64_t base = 0; base <= g.mask; base += 64) {
                const uint64_t sl = base + lane;
                int32_t st = 0, cnt = 0;
                const uint64_t key = g.hkey[sl];
                if (key != GRID_EMPTY) {
                    const int64_t q[3] = { (int64_t)(key % (uint64_t)g.dim[0]), (int64_t)((key / (uint64_t)g.dim[0]) % (uint64_t)g.dim[1]),
                                           (int64_t)(key / (uint64_t)(g.dim[0] * g.dim[1])) };
                    int64_t cheb = 0;
                    for (int ax = 0; ax < 3; ax++) { const int64_t e = q[ax] > c[ax] ? q[ax] - c[ax] : c[ax] - q[ax]; cheb = e > cheb ? e : cheb; }
                    if (cheb > a.smax && !skip_cell(cell_lb(g, p, q), kd0, radius)) {
                        st = g.hrange[2 * sl];
                        cnt = g.hrange[2 * sl + 1] - st;
                    }
                }
                stream_cells(g, lane, k, st, cnt, p, self, bd, br);
            }
            break;
        }
        const int side = 2 * s + 1, total = side * side * side;   // (2 smax + 1)^3 <= hash slots < 2^31
        const double kd0 = __shfl(bd, k - 1);
        for (int base = 0; base < total; base += 64) {
            const int t = base + lane;
            int32_t st = 0, cnt = 0;
            if (t < total) {
                const int64_t q[3] = { c[0] + t % side - s, c[1] + (t / side) % side - s, c[2] + t / (side * side) - s };
                int64_t cheb = 0;
                bool inside = true;
                for (int ax = 0; ax < 3; ax++) {
                    const int64_t e = q[ax] > c[ax] ? q[ax] - c[ax] : c[ax] - q[ax];
                    cheb = e > cheb ? e : cheb;
                    inside = inside && q[ax] >= 0 && q[ax] < g.dim[ax];
                }
                if (cheb == s && inside && !skip_cell(cell_lb(g, p, q), kd0, radius))
                    hash_find(g, (uint64_t)(q[0] + g.dim[0] * (q[1] + g.dim[1] * q[2])), st, cnt);
            }
            stream_cells(g, lane, k, st, cnt, p, self, bd, br);
        }
        // unseen points lie outside the cube of cells c - s .. c + s: done when the k-th best is closer than its faces
        const double kd = __shfl(bd, k - 1);
        double inner = INFINITY;
        for (int ax = 0; ax < 3; ax++) {
            if (c[ax] - s > 0) inner = fmin(inner, p[ax] - (g.o[ax] + (double)(c[ax] - s) * g.h));
            if (c[ax] + s < g.dim[ax] - 1) inner = fmin(inner, (g.o[ax] + (double)(c[ax] + s + 1) * g.h) - p[ax]);
        }
        if (inner == INFINITY) break;                             // the cube holds the whole grid
        inner -= g.margin;
        if (inner > 0.0 && (inner * inner > kd || (radius > 0.0 && inner > radius))) break;
    }
}

// The self query of wave w (wave-uniform; the caller has checked w < a.nq): the query point is a point of the sorted
// arrays; on return p is the point and self its original index, (bd, br) as above.
__device__ inline void knn_search(const Grid &g, const KnnQuery &a, int lane, int64_t w, double p[3], int32_t &self,
                                  double &bd, uint32_t &br)
{
    const int64_t sp = a.sample ? w * a.n / a.nq : w;
    p[0] = g.sx[sp]; p[1] = g.sy[sp]; p[2] = g.sz[sp];
    self = g.sidx[sp];
    knn_search_point(g, a, lane, p, self, bd, br);
}

// the cell-width sample: only the k-th best d^2 of every query
__global__ __launch_bounds__(NRM_BLOCK) void knn_sample_kernel(Grid g, KnnQuery a, double *__restrict__ kth_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= a.nq) return;                                        // wave-uniform
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, a, lane, w, p, self, bd, br);
    const double kd = __shfl(bd, a.k - 1);
    if (lane == 0) kth_out[w] = kd;
}

// The grid a search for lists of k entries (the point itself included) runs on; fills in q for the full query:
//  1. coarse grid: k points per cell of the box's mean density (thin extents floored at 1e-3 of the largest);
//  2. the k-th neighbour distance of a sample of points, exact, on that grid; the cell width is twice its median;
//  3. the grid of that width.
inline int knn_index_for_k(KnnIndex &ix, int k, double radius, KnnQuery &q)
{
    const int64_t n = ix.n;
    memset(&q, 0, sizeof q);
    q.n = n;
    q.k = k;
    q.radius = radius;
    double vol = 1.0;
    for (int ax = 0; ax < 3; ax++) vol *= std::max(ix.ext[ax], 1e-3 * ix.L);
    RH_TRY(ix.build(cbrt(vol * k / (double)n)));
    const double h0 = ix.g.h;
    const int64_t ns = std::min<int64_t>(n, NRM_SAMPLE);
    double *d_kth = nullptr;
    RH_TRY(ix.S->alloc(&d_kth, ns));
    q.nq = ns;
    q.sample = 1;
    q.smax = ix.smax();
    hipLaunchKernelGGL(knn_sample_kernel, dim3(blocks_for(ns, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, ix.S->st, ix.g, q, d_kth);
    SCOPE_HIP(*ix.S, hipGetLastError());
    std::vector<double> kth((size_t)ns);
    RH_TRY(ix.S->fetch(kth.data(), d_kth, (size_t)ns));
    std::nth_element(kth.begin(), kth.begin() + ns / 2, kth.end());
    const double med = kth[(size_t)(ns / 2)];
    const double h = (med > 0.0 && isfinite(med)) ? 2.0 * sqrt(med) : h0;
    RH_TRY(ix.build(h));
    q.nq = n;
    q.sample = 0;
    q.smax = ix.smax();
    return RH_OK;
}

}  // namespace
