// normals.hip -- oriented point normals for a cloud that has none (rh_estimate_normals, include/ransac_hip.h).
// The reference starts from clouds with normals and names the missing step: "If normal information is not available,
// there are algorithms to approximate it (PCA for example)" (docs/src/ransac.md:13).  This is that PCA, exact in its
// neighbours:
//   1. a uniform grid: cell width from the k-th neighbour distance of a sample of points (found exactly on a first,
//      coarse grid whose width comes from the bounding box), points radix-sorted by cell key, an open-addressing hash
//      table key -> [start, end) of the occupied cells only (empty space costs nothing);
//   2. one wave per query point, k <= 64 = the wave width: lane j holds the j-th best (d^2, rank) pair, rank 0 = the
//      point itself, rank i + 1 = point i (so ties go to the smaller index).  The cells of shell s (Chebyshev distance s
//      from the query's cell) stream their points in 64 at a time; a batch with a candidate below the k-th best is
//      sorted (bitonic, __shfl_xor) and merged with the best list.  The search stops when the k-th best d^2 is below
//      the squared distance to the faces of the cube searched so far (or beyond the radius), so the result is exact.
//      A point whose next shell would enumerate more cells than the hash table has slots scans the table instead
//      (every occupied cell not yet visited, pruned by its box distance): isolated points end, and end exact;
//   3. two-pass mean and covariance in binary64 (fixed butterfly order: the same bits on every run), cyclic Jacobi on
//      the 3x3 matrix (accurate when lambda0 ~ lambda1), degenerate rule, canonical sign, orientation.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "jacobi3.h"
#include "rh_internal.h"

namespace {

constexpr uint64_t NRM_EMPTY = ~0ull;
constexpr int NRM_BLOCK = 256;           // 4 waves = 4 query points per block
constexpr int NRM_SAMPLE = 2048;         // points whose k-th neighbour distance sets the cell width
constexpr int NRM_BBOX_BLOCKS = 1024;
constexpr int64_t NRM_MAX_DIM = 1 << 20; // cells per axis: 3 x 21 bits of key
constexpr uint32_t NRM_NORANK = 0xFFFFFFFFu;

struct Grid {
    double o[3];             // bounding-box minimum
    double h;                // cell width
    double margin;           // distance bounds are lowered by this (cell assignment and face positions are rounded)
    int64_t dim[3];
    const uint64_t *hkey;    // hash table: cell key (NRM_EMPTY = free slot) ...
    const int32_t *hrange;   // ... and [start, end) of its points in the sorted arrays (2 ints per slot)
    uint64_t mask;           // slots - 1
    const double *sx, *sy, *sz;
    const int32_t *sidx;     // original index of each sorted point
    const double *xyz;       // original AoS coordinates
};

__host__ __device__ inline int64_t cell_of(double v, double o, double h, int64_t dim)
{
    const double t = floor((v - o) / h);
    int64_t c = t < 0.0 ? 0 : (t >= (double)dim ? dim - 1 : (int64_t)t);
    return c;
}

__device__ inline uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------ grid build ----
template <typename T>
__global__ void nrm_widen_kernel(const T *__restrict__ in, double *__restrict__ out, int64_t cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) out[i] = (double)in[i];
}

// per block: min xyz, max xyz, 1 if a coordinate is not finite
__global__ void nrm_bbox_kernel(const double *__restrict__ xyz, int64_t n, double *__restrict__ part)
{
    double mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    double bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        for (int a = 0; a < 3; a++) {
            const double v = xyz[3 * i + a];
            if (!isfinite(v)) bad = 1.0;
            mn[a] = v < mn[a] ? v : mn[a];
            mx[a] = v > mx[a] ? v : mx[a];
        }
    for (int j = 32; j > 0; j >>= 1)
        for (int a = 0; a < 3; a++) {
            const double u = __shfl_xor(mn[a], j), w = __shfl_xor(mx[a], j);
            mn[a] = u < mn[a] ? u : mn[a];
            mx[a] = w > mx[a] ? w : mx[a];
        }
    for (int j = 32; j > 0; j >>= 1) { const double b = __shfl_xor(bad, j); bad = b > bad ? b : bad; }
    __shared__ double red[NRM_BLOCK / 64][7];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; a++) { red[wv][a] = mn[a]; red[wv][3 + a] = mx[a]; }
        red[wv][6] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int f = threadIdx.x;
        double r = red[0][f];
        for (int w = 1; w < NRM_BLOCK / 64; w++) {
            const double v = red[w][f];
            r = (f < 3) ? (v < r ? v : r) : (v > r ? v : r);
        }
        part[7 * blockIdx.x + f] = r;
    }
}

__global__ void nrm_key_kernel(Grid g, int64_t n, uint64_t *__restrict__ key, int32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t cx = cell_of(g.xyz[3 * i], g.o[0], g.h, g.dim[0]);
    const int64_t cy = cell_of(g.xyz[3 * i + 1], g.o[1], g.h, g.dim[1]);
    const int64_t cz = cell_of(g.xyz[3 * i + 2], g.o[2], g.h, g.dim[2]);
    key[i] = (uint64_t)(cx + g.dim[0] * (cy + g.dim[1] * cz));
    idx[i] = (int32_t)i;
}

__global__ void nrm_gather_kernel(const double *__restrict__ xyz, const int32_t *__restrict__ idx, int64_t n,
                                  double *__restrict__ sx, double *__restrict__ sy, double *__restrict__ sz)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    sx[i] = xyz[3 * j]; sy[i] = xyz[3 * j + 1]; sz[i] = xyz[3 * j + 2];
}

// number of occupied cells = runs of equal sorted keys
__global__ void nrm_runs_kernel(const uint64_t *__restrict__ key, int64_t n, unsigned long long *count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool start = i < n && (i == 0 || key[i] != key[i - 1]);
    const uint64_t b = __builtin_amdgcn_ballot_w64(start);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// the first point of a run writes its start, the last its end, into the slot of the run's key
__global__ void nrm_hash_kernel(const uint64_t *__restrict__ key, int64_t n, uint64_t *hkey, int32_t *hrange, uint64_t mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i];
    const bool start = i == 0 || key[i - 1] != k, end = i == n - 1 || key[i + 1] != k;
    if (!start && !end) return;
    uint64_t sl = mix64(k) & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS((unsigned long long *)&hkey[sl], (unsigned long long)NRM_EMPTY,
                                                  (unsigned long long)k);
        if (prev == NRM_EMPTY || prev == k) break;
        sl = (sl + 1) & mask;
    }
    if (start) hrange[2 * sl] = (int32_t)i;
    if (end) hrange[2 * sl + 1] = (int32_t)(i + 1);
}

// ---------------------------------------------------------------------- query ----
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
    uint64_t sl = mix64(key) & g.mask;
    for (;;) {
        const uint64_t kk = g.hkey[sl];
        if (kk == key) { st = g.hrange[2 * sl]; cnt = g.hrange[2 * sl + 1] - st; return; }
        if (kk == NRM_EMPTY) { st = 0; cnt = 0; return; }
        sl = (sl + 1) & g.mask;
    }
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

__device__ inline double wsum(double v)
{
    for (int j = 32; j > 0; j >>= 1) v += __shfl_xor(v, j);   // butterfly: every lane ends with the same bits
    return v;
}

struct QueryArgs {
    int64_t nq;              // query points (waves)
    int64_t n;
    int k;
    int orient;              // 0 canonical, 1 viewpoint, 2 hints
    int sample;              // 1: only the k-th best d^2 -> kth_out (the cell-width sample), query w = sorted point w*n/nq
    double radius;
    double view[3];
    int smax;                // last shell enumerated cell by cell; beyond it the hash table is scanned
    const double *hints;     // AoS, original order
    double *kth_out;
};

template <typename OutT>
__global__ __launch_bounds__(NRM_BLOCK) void nrm_query_kernel(Grid g, QueryArgs a, OutT *__restrict__ nrm,
                                                              OutT *__restrict__ curv, int32_t *__restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= a.nq) return;                                        // wave-uniform
    const int64_t sp = a.sample ? w * a.n / a.nq : w;
    const double p[3] = { g.sx[sp], g.sy[sp], g.sz[sp] };
    const int32_t self = g.sidx[sp];
    int64_t c[3];
    for (int ax = 0; ax < 3; ax++) c[ax] = cell_of(p[ax], g.o[ax], g.h, g.dim[ax]);
    const int k = a.k;
    const double radius = a.radius;
    double bd = INFINITY;
    uint32_t br = NRM_NORANK;

    for (int s = 0;; s++) {
        if (s > a.smax) {   // scan every occupied cell outside the cube already searched
            const double kd0 = __shfl(bd, k - 1);
            for (uint64_t base = 0; base <= g.mask; base += 64) {
                const uint64_t sl = base + lane;
                int32_t st = 0, cnt = 0;
                const uint64_t key = g.hkey[sl];
                if (key != NRM_EMPTY) {
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

    if (a.sample) {
        const double kd = __shfl(bd, k - 1);
        if (lane == 0) a.kth_out[w] = kd;
        return;
    }

    // the neighbourhood: the first k of the order, those beyond the radius dropped (a prefix of the list)
    const double r2 = radius * radius;
    const bool in = lane < k && br != NRM_NORANK && (radius <= 0.0 || bd <= r2);
    const int m = __popcll(__builtin_amdgcn_ballot_w64(in));
    double q[3] = { 0.0, 0.0, 0.0 };
    if (in) {
        const int64_t qi = br == 0 ? (int64_t)self : (int64_t)br - 1;
        for (int ax = 0; ax < 3; ax++) q[ax] = g.xyz[3 * qi + ax];
    }
    double mean[3], e[3];
    for (int ax = 0; ax < 3; ax++) mean[ax] = wsum(q[ax]) / (double)m;
    for (int ax = 0; ax < 3; ax++) e[ax] = in ? q[ax] - mean[ax] : 0.0;
    double A[3][3];
    A[0][0] = wsum(e[0] * e[0]) / m; A[0][1] = wsum(e[0] * e[1]) / m; A[0][2] = wsum(e[0] * e[2]) / m;
    A[1][1] = wsum(e[1] * e[1]) / m; A[1][2] = wsum(e[1] * e[2]) / m; A[2][2] = wsum(e[2] * e[2]) / m;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    if (lane != 0) return;

    double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    rh_jacobi3(A, V);
    int i0 = 0, i1 = 1, i2 = 2;                                    // ascending eigenvalues
    if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
    if (A[i2][i2] < A[i1][i1]) { const int t = i1; i1 = i2; i2 = t; }
    if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
    const double l0 = A[i0][i0], l1 = A[i1][i1], l2 = A[i2][i2];
    double nv[3] = { V[0][i0], V[1][i0], V[2][i0] };
    const double nn = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    for (int ax = 0; ax < 3; ax++) nv[ax] /= nn;
    double cv = l0 / ((l0 + l1) + l2);
    bool degenerate = m < 3 || l2 == 0.0 || l1 <= 1e-12 * l2 || !(isfinite(nv[0]) && isfinite(nv[1]) && isfinite(nv[2]))
                      || !isfinite(cv);
    if (degenerate) {
        nv[0] = nv[1] = nv[2] = 0.0;
        cv = 0.0;
    } else {
        int im = 0;                                                // canonical sign: the largest component positive
        if (fabs(nv[1]) > fabs(nv[im])) im = 1;
        if (fabs(nv[2]) > fabs(nv[im])) im = 2;
        double sg = nv[im] < 0.0 ? -1.0 : 1.0;
        double dot = 0.0;
        if (a.orient == 1)
            dot = (sg * nv[0] * (a.view[0] - p[0]) + sg * nv[1] * (a.view[1] - p[1])) + sg * nv[2] * (a.view[2] - p[2]);
        else if (a.orient == 2) {
            const double *hv = a.hints + 3 * (int64_t)self;
            dot = (sg * nv[0] * hv[0] + sg * nv[1] * hv[1]) + sg * nv[2] * hv[2];
        }
        if (dot < 0.0) sg = -sg;
        for (int ax = 0; ax < 3; ax++) nv[ax] = sg * nv[ax] + 0.0;   // (+ 0.0: no negative zero)
    }
    for (int ax = 0; ax < 3; ax++) nrm[3 * (int64_t)self + ax] = (OutT)nv[ax];
    if (curv) curv[self] = (OutT)cv;
    if (flags) flags[self] = degenerate ? 1 : 0;
}

inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// device buffers of one call, freed on every way out
struct Buffers {
    std::vector<void *> ptrs;
    ~Buffers() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T>
    int alloc(T **p, int64_t count)
    {
        *p = nullptr;
        const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
        const hipError_t e = hipMalloc((void **)p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rh_set_error("rh_estimate_normals: hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? RH_E_NOMEM : RH_E_NODEVICE;
        }
        ptrs.push_back(*p);
        return RH_OK;
    }
    void release(void *p)
    {
        for (auto &q : ptrs)
            if (q == p) { (void)hipFree(q); q = nullptr; }
    }
};

struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};

template <typename T>
int estimate(const T *xyz_aos, int64_t n, const rh_normals_params *p, const T *hints, int device, T *nrm_out,
             T *curv_out, int32_t *flags_out)
{
    if (!xyz_aos || !p || !nrm_out) { rh_set_error("rh_estimate_normals: NULL argument"); return RH_E_INVALID; }
    if (n < 1 || n > (int64_t)0x7FFFF000) { rh_set_error("rh_estimate_normals: n = %lld outside 1 .. 2^31 - 4096", (long long)n); return RH_E_INVALID; }
    if (p->k < 3 || p->k > 64) { rh_set_error("rh_estimate_normals: k = %d outside 3 .. 64", p->k); return RH_E_INVALID; }
    if (p->orient < 0 || p->orient > 2) { rh_set_error("rh_estimate_normals: orient = %d outside 0 .. 2", p->orient); return RH_E_INVALID; }
    if (p->orient == 2 && !hints) { rh_set_error("rh_estimate_normals: orient = 2 needs hints"); return RH_E_INVALID; }
    if (!(isfinite(p->radius) && p->radius >= 0.0)) { rh_set_error("rh_estimate_normals: radius must be finite and >= 0"); return RH_E_INVALID; }
    if (p->orient == 1 && !(isfinite(p->viewpoint[0]) && isfinite(p->viewpoint[1]) && isfinite(p->viewpoint[2]))) {
        rh_set_error("rh_estimate_normals: the viewpoint is not finite");
        return RH_E_INVALID;
    }
    int ndev = 0;
    RH_TRY(rh_device_count(&ndev));
    if (ndev <= 0) { rh_set_error("no HIP device is visible; libransac_hip has no CPU fallback"); return RH_E_NODEVICE; }
    if (device < 0 || device >= ndev) { rh_set_error("device %d out of range (%d visible)", device, ndev); return RH_E_INVALID; }
#define NH(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { rh_set_error("rh_estimate_normals: %s", hipGetErrorString(e_)); return RH_E_NODEVICE; } } while (0)
    NH(hipSetDevice(device));
    StreamHolder sh;
    NH(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t st = sh.s;
    Buffers B;
    const int k = p->k;

    double *d_xyz = nullptr, *d_hints = nullptr;
    RH_TRY(B.alloc(&d_xyz, 3 * n));
    auto upload = [&](const T *src, double *dst) -> int {
        if (sizeof(T) == sizeof(double)) {
            NH(hipMemcpyAsync(dst, src, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
            return RH_OK;
        }
        T *d_in = nullptr;
        RH_TRY(B.alloc(&d_in, 3 * n));
        NH(hipMemcpyAsync(d_in, src, sizeof(T) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(nrm_widen_kernel<T>, dim3(nblk(3 * n, 256)), dim3(256), 0, st, d_in, dst, 3 * n);
        NH(hipGetLastError());
        NH(hipStreamSynchronize(st));
        B.release(d_in);
        return RH_OK;
    };
    RH_TRY(upload(xyz_aos, d_xyz));
    if (p->orient == 2) {
        RH_TRY(B.alloc(&d_hints, 3 * n));
        RH_TRY(upload(hints, d_hints));
    }

    // bounding box and the finiteness of every coordinate
    double *d_part = nullptr;
    RH_TRY(B.alloc(&d_part, 7 * NRM_BBOX_BLOCKS));
    hipLaunchKernelGGL(nrm_bbox_kernel, dim3(NRM_BBOX_BLOCKS), dim3(NRM_BLOCK), 0, st, d_xyz, n, d_part);
    NH(hipGetLastError());
    std::vector<double> part(7 * NRM_BBOX_BLOCKS);
    NH(hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
    NH(hipStreamSynchronize(st));
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int b = 0; b < NRM_BBOX_BLOCKS; b++) {
        if (part[7 * b + 6] != 0.0) { rh_set_error("rh_estimate_normals: a coordinate is not finite"); return RH_E_INVALID; }
        for (int ax = 0; ax < 3; ax++) { lo[ax] = std::min(lo[ax], part[7 * b + ax]); hi[ax] = std::max(hi[ax], part[7 * b + 3 + ax]); }
    }
    double ext[3], L = 0.0, omax = 0.0;
    for (int ax = 0; ax < 3; ax++) {
        ext[ax] = hi[ax] - lo[ax];
        L = std::max(L, ext[ax]);
        omax = std::max(omax, std::max(fabs(lo[ax]), fabs(hi[ax])));
    }

    uint64_t *d_key[2] = { nullptr, nullptr };
    int32_t *d_idx[2] = { nullptr, nullptr };
    double *d_s[3] = { nullptr, nullptr, nullptr };
    unsigned long long *d_count = nullptr;
    RH_TRY(B.alloc(&d_key[0], n)); RH_TRY(B.alloc(&d_key[1], n));
    RH_TRY(B.alloc(&d_idx[0], n)); RH_TRY(B.alloc(&d_idx[1], n));
    for (int ax = 0; ax < 3; ax++) RH_TRY(B.alloc(&d_s[ax], n));
    RH_TRY(B.alloc(&d_count, 1));
    size_t tmp_bytes = 0;
    NH(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)n, 0, 64, st));
    uint8_t *d_tmp = nullptr;
    RH_TRY(B.alloc(&d_tmp, (int64_t)tmp_bytes));
    uint64_t *d_hkey = nullptr;
    int32_t *d_hrange = nullptr;
    uint64_t hcap = 0;

    Grid g;
    // grid of width h: sort by cell, gather, hash table of the occupied cells
    auto build_grid = [&](double h) -> int {
        h = std::max(h, L / (double)NRM_MAX_DIM);
        if (!(h > 0.0) || !isfinite(h)) h = 1.0;
        for (int ax = 0; ax < 3; ax++) {
            g.o[ax] = lo[ax];
            g.dim[ax] = std::min((int64_t)floor(ext[ax] / h) + 1, NRM_MAX_DIM + 1);
        }
        g.h = h;
        g.margin = 1e-12 * (omax + L + h);
        g.xyz = d_xyz;
        const uint64_t cells = (uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2];
        int bits = 1;
        while (bits < 64 && (cells - 1) >> bits) bits++;
        hipLaunchKernelGGL(nrm_key_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, g, n, d_key[0], d_idx[0]);
        NH(hipGetLastError());
        NH(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)n, 0, bits, st));
        hipLaunchKernelGGL(nrm_gather_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_xyz, d_idx[1], n, d_s[0], d_s[1], d_s[2]);
        NH(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(nrm_runs_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_key[1], n, d_count);
        NH(hipGetLastError());
        unsigned long long occupied = 0;
        NH(hipMemcpyAsync(&occupied, d_count, sizeof occupied, hipMemcpyDeviceToHost, st));
        NH(hipStreamSynchronize(st));
        uint64_t cap = 64;
        while (cap < 2 * occupied) cap <<= 1;
        if (cap > hcap) {
            B.release(d_hkey);
            B.release(d_hrange);
            RH_TRY(B.alloc(&d_hkey, (int64_t)cap));
            RH_TRY(B.alloc(&d_hrange, 2 * (int64_t)cap));
            hcap = cap;
        }
        NH(hipMemsetAsync(d_hkey, 0xFF, sizeof(uint64_t) * cap, st));
        hipLaunchKernelGGL(nrm_hash_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_key[1], n, d_hkey, d_hrange, cap - 1);
        NH(hipGetLastError());
        g.hkey = d_hkey; g.hrange = d_hrange; g.mask = cap - 1;
        g.sx = d_s[0]; g.sy = d_s[1]; g.sz = d_s[2]; g.sidx = d_idx[1];
        return RH_OK;
    };
    auto smax_of = [&]() {   // the last shell whose cube enumerates no more cells than the hash table has slots
        int s = 1;
        while ((double)(2 * s + 3) * (2 * s + 3) * (2 * s + 3) <= (double)(g.mask + 1)) s++;
        return s;
    };

    QueryArgs qa;
    memset(&qa, 0, sizeof qa);
    qa.n = n;
    qa.k = k;
    qa.orient = p->orient;
    qa.radius = p->radius;
    for (int ax = 0; ax < 3; ax++) qa.view[ax] = p->viewpoint[ax];
    qa.hints = d_hints;

    // 1. coarse grid: k points per cell of the box's mean density (thin extents floored at 1e-3 of the largest)
    double vol = 1.0;
    for (int ax = 0; ax < 3; ax++) vol *= std::max(ext[ax], 1e-3 * L);
    RH_TRY(build_grid(cbrt(vol * k / (double)n)));
    const double h0 = g.h;
    // 2. the k-th neighbour distance of a sample of points, exact, on that grid; the cell width is twice its median
    const int64_t ns = std::min<int64_t>(n, NRM_SAMPLE);
    double *d_kth = nullptr;
    RH_TRY(B.alloc(&d_kth, ns));
    qa.nq = ns;
    qa.sample = 1;
    qa.smax = smax_of();
    qa.kth_out = d_kth;
    hipLaunchKernelGGL(nrm_query_kernel<double>, dim3(nblk(ns, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, g, qa,
                       (double *)nullptr, (double *)nullptr, (int32_t *)nullptr);
    NH(hipGetLastError());
    std::vector<double> kth((size_t)ns);
    NH(hipMemcpyAsync(kth.data(), d_kth, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, st));
    NH(hipStreamSynchronize(st));
    std::nth_element(kth.begin(), kth.begin() + ns / 2, kth.end());
    const double med = kth[(size_t)(ns / 2)];
    const double h = (med > 0.0 && isfinite(med)) ? 2.0 * sqrt(med) : h0;
    // 3. the grid of that width, every point's neighbours and normal
    RH_TRY(build_grid(h));
    T *d_nrm = nullptr, *d_curv = nullptr;
    int32_t *d_flags = nullptr;
    RH_TRY(B.alloc(&d_nrm, 3 * n));
    if (curv_out) RH_TRY(B.alloc(&d_curv, n));
    if (flags_out) RH_TRY(B.alloc(&d_flags, n));
    qa.nq = n;
    qa.sample = 0;
    qa.smax = smax_of();
    qa.kth_out = nullptr;
    hipLaunchKernelGGL(nrm_query_kernel<T>, dim3(nblk(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, g, qa, d_nrm, d_curv, d_flags);
    NH(hipGetLastError());
    NH(hipMemcpyAsync(nrm_out, d_nrm, sizeof(T) * 3 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (curv_out) NH(hipMemcpyAsync(curv_out, d_curv, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (flags_out) NH(hipMemcpyAsync(flags_out, d_flags, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    NH(hipStreamSynchronize(st));
#undef NH
    return RH_OK;
}

}  // namespace

extern "C" int rh_estimate_normals(const double *xyz_aos, int64_t n, const rh_normals_params *p, const double *hints_aos_or_null,
                                   int device, double *nrm_out_aos, double *curv_out_or_null, int32_t *flags_out_or_null)
{
    return estimate<double>(xyz_aos, n, p, hints_aos_or_null, device, nrm_out_aos, curv_out_or_null, flags_out_or_null);
}

extern "C" int rh_estimate_normals_f32(const float *xyz_aos, int64_t n, const rh_normals_params *p, const float *hints_aos_or_null,
                                       int device, float *nrm_out_aos, float *curv_out_or_null, int32_t *flags_out_or_null)
{
    return estimate<float>(xyz_aos, n, p, hints_aos_or_null, device, nrm_out_aos, curv_out_or_null, flags_out_or_null);
}
