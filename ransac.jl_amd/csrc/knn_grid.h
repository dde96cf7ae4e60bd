// knn_grid.h -- the uniform grid of the exact k-nearest-neighbour search (knn_device.h has the query), shared by
// normals.hip (rh_estimate_normals), knn.hip (rh_knn, rh_remove_outliers), orient.hip (rh_orient_normals), segment.hip (rh_segment_smooth), knn_query.hip and register.hip (rh_knn_query,
// rh_cloud_distance, rh_register: the grid holds the reference cloud) and cluster.hip (rh_cluster, which walks the cells itself):
//   points radix-sorted by cell key, an open-addressing hash table key -> [start, end) of the occupied cells only (empty
//   space costs nothing; table and bounding box are cell_grid.h's), the coordinates gathered into cell order.  KnnIndex
//   holds the grid's buffers in the call's scope (call_scope.h) and rebuilds the grid for any cell width.
// Everything here lives in an anonymous namespace: each translation unit that includes the header gets its own kernels.
#pragma once

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "call_scope.h"
#include "cell_grid.h"
#include "rh_internal.h"

namespace {

constexpr int NRM_BLOCK = 256;           // 4 waves = 4 query points per block
constexpr int NRM_SAMPLE = 2048;         // points whose k-th neighbour distance sets the cell width
constexpr int64_t NRM_MAX_DIM = 1 << 20; // cells per axis: 3 x 21 bits of key
constexpr uint32_t NRM_NORANK = 0xFFFFFFFFu;

struct Grid {
    double o[3];             // bounding-box minimum
    double h;                // cell width
    double margin;           // distance bounds are lowered by this (cell assignment and face positions are rounded)
    int64_t dim[3];
    const uint64_t *hkey;    // hash table: cell key (GRID_EMPTY = free slot) ...
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

// ------------------------------------------------------------------ grid build ----
// bounding box and number of the points whose coordinates are all finite: per block, the fold of cell_grid.h follows
__global__ void __launch_bounds__(256) nrm_minmax_kernel(const double *__restrict__ xyz, int64_t n, unsigned long long *__restrict__ part)
{
    MinMaxCount acc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) acc.add(x, y, z);
    }
    acc.store(part);
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
    const uint32_t sl = table_insert(hkey, (uint32_t)mask, k);
    if (start) hrange[2 * (size_t)sl] = (int32_t)i;
    if (end) hrange[2 * (size_t)sl + 1] = (int32_t)(i + 1);
}

// the words cloud_box folds through for a cloud of n points
inline int64_t cloud_box_words(int64_t n) { return MM_WORDS * (1 + std::min<int64_t>(blocks_for(n), GRID_MM_BLOCKS)); }

// the bounding box of the n points of d_xyz; RH_E_INVALID on a coordinate that is not finite (one round trip to the host).
// d_scal: cloud_box_words(n) words of the caller's (a call that asks again and again), or null: allocated here.
inline int cloud_box(CallScope &S, const double *d_xyz, int64_t n, double lo[3], double hi[3], unsigned long long *d_scal = nullptr)
{
    const hipStream_t st = S.st;
    const int64_t nb = std::min<int64_t>(blocks_for(n), GRID_MM_BLOCKS);
    unsigned long long h_scal[MM_COUNT + 1];
    if (!d_scal) RH_TRY(S.alloc(&d_scal, cloud_box_words(n)));
    hipLaunchKernelGGL(nrm_minmax_kernel, dim3((unsigned)nb), dim3(256), 0, st, d_xyz, n, d_scal + MM_WORDS);
    hipLaunchKernelGGL(grid_minmax_fold_kernel, dim3(1), dim3(256), 0, st, d_scal + MM_WORDS, (int)nb, d_scal, (int)MM_WORDS);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.fetch(h_scal, d_scal, MM_COUNT + 1));
    if ((int64_t)h_scal[MM_COUNT] != n) { rh_set_error("%s: a coordinate is not finite", S.who); return RH_E_INVALID; }
    for (int ax = 0; ax < 3; ax++) { lo[ax] = ord_back(h_scal[MM_MIN + ax]); hi[ax] = ord_back(h_scal[MM_MAX + ax]); }
    return RH_OK;
}

// The grid over the n points of one call: init() finds the bounding box (RH_E_INVALID on a coordinate that is not finite)
// and allocates, build(h) makes the grid of cell width h (again and again: the buffers are re-used).
struct KnnIndex {
    CallScope *S = nullptr;    // the call's buffers and its stream
    int64_t n = 0;
    double *d_xyz = nullptr;
    double lo[3], hi[3], ext[3], L = 0.0, omax = 0.0;
    uint64_t *d_key[2] = { nullptr, nullptr };
    int32_t *d_idx[2] = { nullptr, nullptr };
    double *d_s[3] = { nullptr, nullptr, nullptr };
    unsigned long long *d_count = nullptr;
    uint64_t *d_hkey = nullptr;
    int32_t *d_hrange = nullptr;
    uint64_t hcap = 0;
    Grid g;

    int init(CallScope &S_, double *d_xyz_, int64_t n_)
    {
        S = &S_; d_xyz = d_xyz_; n = n_;
        RH_TRY(cloud_box(*S, d_xyz, n, lo, hi));
        L = 0.0; omax = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            ext[ax] = hi[ax] - lo[ax];
            L = std::max(L, ext[ax]);
            omax = std::max(omax, std::max(fabs(lo[ax]), fabs(hi[ax])));
        }
        RH_TRY(S->alloc(&d_key[0], n)); RH_TRY(S->alloc(&d_key[1], n));
        RH_TRY(S->alloc(&d_idx[0], n)); RH_TRY(S->alloc(&d_idx[1], n));
        for (int ax = 0; ax < 3; ax++) RH_TRY(S->alloc(&d_s[ax], n));
        RH_TRY(S->alloc(&d_count, 1));
        return RH_OK;
    }

    // grid of width h: sort by cell, gather, hash table of the occupied cells
    int build(double h)
    {
        const hipStream_t st = S->st;
        h = std::max(h, L / (double)NRM_MAX_DIM);
        if (!(h > 0.0) || !isfinite(h)) h = 1.0;
        for (int ax = 0; ax < 3; ax++) {
            g.o[ax] = lo[ax];
            g.dim[ax] = std::min((int64_t)floor(ext[ax] / h) + 1, NRM_MAX_DIM + 1);
        }
        g.h = h;
        g.margin = 1e-12 * (omax + L + h);
        g.xyz = d_xyz;
        const int bits = sort_bits((uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2]);
        hipLaunchKernelGGL(nrm_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, g, n, d_key[0], d_idx[0]);
        SCOPE_HIP(*S, hipGetLastError());
        RH_TRY(S->cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)n, 0, bits, st); }));
        hipLaunchKernelGGL(nrm_gather_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_xyz, d_idx[1], n, d_s[0], d_s[1], d_s[2]);
        SCOPE_HIP(*S, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(nrm_runs_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_key[1], n, d_count);
        SCOPE_HIP(*S, hipGetLastError());
        unsigned long long occupied = 0;
        RH_TRY(S->fetch(&occupied, d_count));
        uint64_t cap = 64;
        while (cap < 2 * occupied) cap <<= 1;
        if (cap > hcap) {
            S->release(d_hkey);
            S->release(d_hrange);
            RH_TRY(S->alloc(&d_hkey, (int64_t)cap));
            RH_TRY(S->alloc(&d_hrange, 2 * (int64_t)cap));
            hcap = cap;
        }
        SCOPE_HIP(*S, hipMemsetAsync(d_hkey, 0xFF, sizeof(uint64_t) * cap, st));
        hipLaunchKernelGGL(nrm_hash_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_key[1], n, d_hkey, d_hrange, cap - 1);
        SCOPE_HIP(*S, hipGetLastError());
        g.hkey = d_hkey; g.hrange = d_hrange; g.mask = cap - 1;
        g.sx = d_s[0]; g.sy = d_s[1]; g.sz = d_s[2]; g.sidx = d_idx[1];
        return RH_OK;
    }

    // the last shell whose cube enumerates no more cells than the hash table has slots
    int smax() const
    {
        int s = 1;
        while ((double)(2 * s + 3) * (2 * s + 3) * (2 * s + 3) <= (double)(g.mask + 1)) s++;
        return s;
    }
};

}  // namespace
