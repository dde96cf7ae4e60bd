// cell_grid.h -- the pieces every grid of cells over a point set is made of (the component filter's voxels, the
// downsampler's, the kNN search's): the bounding box as order-preserving integers, cell keys of 3 x 21 bits, an
// open-addressing table of keys, and the block-level minimum / maximum / count reduction with its one-block fold.
// The table here is the key array and its mask only: what hangs on a slot (parents, counts, rows, ranges) stays with its
// owner, and so do the loops over the points.  The integer part compiles under a plain host compiler.
// Everything lives in an anonymous namespace: each translation unit that includes the header gets its own fold kernel.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RH_GRID_HD __host__ __device__ inline
#else
#define RH_GRID_HD inline
#endif

namespace {

constexpr uint64_t GRID_EMPTY = ~0ULL;          // (no key: cells are below 2^20 per axis, bit 63 of a key is never set)
constexpr uint64_t GRID_FIELD = 0x1FFFFFULL;    // one axis of a key
constexpr int GRID_MM_BLOCKS = 4096;            // blocks of a minimum pass at most, 8 words of partial results each
enum { MM_MIN = 0, MM_MAX = 3, MM_COUNT = 6, MM_WORDS = 8 };

// doubles as unsigned integers in the same order (finite values; -0.0 sorts below +0.0, which no cell formula can tell apart)
RH_GRID_HD uint64_t ord_of(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
RH_GRID_HD double ord_back(uint64_t u)
{
    u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFULL) : ~u;
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// the key of cell (cx, cy, cz), each in 0 .. 2^20 - 1: x in the highest field.  bias 1 keeps the -1 neighbours of cell 0
// inside their fields (key arithmetic on neighbours: the component filter), bias 0 is the plain cell.  Every field is
// masked, which the component filter's own formula was not: the same bits for all cells that pass grid_axis_fits
RH_GRID_HD uint64_t grid_pack(long long cx, long long cy, long long cz, int bias)
{
    return (((uint64_t)(cx + bias) & GRID_FIELD) << 42) | (((uint64_t)(cy + bias) & GRID_FIELD) << 21) | ((uint64_t)(cz + bias) & GRID_FIELD);
}
// field `axis` (0 = x) of a key, bias included
RH_GRID_HD uint64_t grid_field(uint64_t key, int axis) { return (key >> (21 * (2 - axis))) & GRID_FIELD; }

// cells of width beta between lo and hi along one axis, minus one; false: more than 2^20, they do not fit a field
RH_GRID_HD bool grid_axis_fits(double lo, double hi, double beta, double *cells_out)
{
    *cells_out = floor((hi - lo) / beta);
    return *cells_out < 1048576.0;
}

#if defined(__HIPCC__)

__device__ __forceinline__ uint32_t slot_hash(uint64_t k)
{
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDULL; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ULL; k ^= k >> 33;
    return (uint32_t)k;
}

// the slot of `key`, -1 where the table does not hold it (a table is at most half full: an empty slot ends every probe
// sequence); for tables that nobody inserts into any more
__device__ __forceinline__ int64_t table_find(const uint64_t *keys, uint32_t mask, uint64_t key)
{
    uint32_t h = slot_hash(key) & mask;
    for (;;) {
        const uint64_t k = keys[h];
        if (k == key) return (int64_t)h;
        if (k == GRID_EMPTY) return -1;
        h = (h + 1) & mask;
    }
}

// the slot of `key`, taken if nobody has: key loaded first, CAS only into an empty slot (a dense cell sends its CAS only
// until the key stands there)
__device__ __forceinline__ uint32_t table_insert(uint64_t *keys, uint32_t mask, uint64_t key)
{
    uint32_t h = slot_hash(key) & mask;
    for (;;) {
        const unsigned long long k = __hip_atomic_load((const unsigned long long *)&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == key) return h;
        if (k == GRID_EMPTY) {
            const unsigned long long old = atomicCAS((unsigned long long *)&keys[h], (unsigned long long)GRID_EMPTY, (unsigned long long)key);
            if (old == GRID_EMPTY || old == key) return h;
        }
        h = (h + 1) & mask;
    }
}

// Minimum, maximum and number of the points a thread adds; store() meets the block's 256 threads (all of them call it):
// a wave shuffle, the four waves through LDS, then MM_WORDS words in part[MM_WORDS * blockIdx.x ..] as ord_of() words, a
// block without points ~0 / 0.  Partial results and one folding block, no atomics: 4096 blocks x 7 atomics on one cache
// line took 0.34 ms, ten times the rest of such a pass.
struct MinMaxCount {
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    long long cnt = 0;

    __device__ __forceinline__ void add(double x, double y, double z)
    {
        const double p[3] = { x, y, z };
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = p[a] < lo[a] ? p[a] : lo[a];
            hi[a] = p[a] > hi[a] ? p[a] : hi[a];
        }
        cnt++;
    }

    __device__ __forceinline__ void store(unsigned long long *__restrict__ part)
    {
#pragma unroll
        for (int a = 0; a < 3; a++)
            for (int off = 32; off > 0; off >>= 1) {
                const double l = __shfl_down(lo[a], off), h = __shfl_down(hi[a], off);
                lo[a] = l < lo[a] ? l : lo[a];
                hi[a] = h > hi[a] ? h : hi[a];
            }
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
        __shared__ double s_lo[4][3], s_hi[4][3];
        __shared__ long long s_cnt[4];
        if ((threadIdx.x & 63) == 0) {
            const int wv = threadIdx.x >> 6;
#pragma unroll
            for (int a = 0; a < 3; a++) { s_lo[wv][a] = lo[a]; s_hi[wv][a] = hi[a]; }
            s_cnt[wv] = cnt;
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
        for (int wv = 1; wv < 4; wv++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = s_lo[wv][a] < lo[a] ? s_lo[wv][a] : lo[a];
                hi[a] = s_hi[wv][a] > hi[a] ? s_hi[wv][a] : hi[a];
            }
            cnt += s_cnt[wv];
        }
        unsigned long long *o = part + MM_WORDS * (size_t)blockIdx.x;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            o[MM_MIN + a] = cnt > 0 ? (unsigned long long)ord_of(lo[a]) : ~0ULL;
            o[MM_MAX + a] = cnt > 0 ? (unsigned long long)ord_of(hi[a]) : 0ULL;
        }
        o[MM_COUNT] = (unsigned long long)cnt;
    }
};

// ... folded by one block of 256 threads into scal[0 .. 6]; the words from 7 up to nwords_out (<= 256) are zeroed: a
// caller's further scalars of the call start from 0
__global__ void __launch_bounds__(256)
grid_minmax_fold_kernel(const unsigned long long *__restrict__ part, int nparts, unsigned long long *__restrict__ scal, int nwords_out)
{
    __shared__ unsigned long long sh[256][7];
    unsigned long long v[7] = { ~0ULL, ~0ULL, ~0ULL, 0ULL, 0ULL, 0ULL, 0ULL };
    for (int b = threadIdx.x; b < nparts; b += 256) {
        const unsigned long long *o = part + MM_WORDS * (size_t)b;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v[MM_MIN + a] = o[MM_MIN + a] < v[MM_MIN + a] ? o[MM_MIN + a] : v[MM_MIN + a];
            v[MM_MAX + a] = o[MM_MAX + a] > v[MM_MAX + a] ? o[MM_MAX + a] : v[MM_MAX + a];
        }
        v[MM_COUNT] += o[MM_COUNT];
    }
#pragma unroll
    for (int k = 0; k < 7; k++) sh[threadIdx.x][k] = v[k];
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const unsigned long long l = sh[threadIdx.x + step][MM_MIN + a], h = sh[threadIdx.x + step][MM_MAX + a];
                if (l < sh[threadIdx.x][MM_MIN + a]) sh[threadIdx.x][MM_MIN + a] = l;
                if (h > sh[threadIdx.x][MM_MAX + a]) sh[threadIdx.x][MM_MAX + a] = h;
            }
            sh[threadIdx.x][MM_COUNT] += sh[threadIdx.x + step][MM_COUNT];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nwords_out) scal[threadIdx.x] = threadIdx.x < 7 ? sh[0][threadIdx.x] : 0ULL;
}

#endif  // __HIPCC__

}  // namespace
