// voxel.hip -- voxel-grid downsampling of a raw cloud (rh_voxel_downsample, include/ransac_hip.h states the definition in
// full): one output point per occupied cell of a grid of width beta, rows in first-appearance order, and the map
// point -> row that carries a shape found on the thinned cloud back to the scan.  The reference leaves thinning to the
// user.  Everything order-dependent is an integer: cells live in an open-addressing table (cell_grid.h), counts,
// first indices and the 32-bit fixed-point offsets of the centroid are integer atomics, so the same bits come out
// whatever order the points arrive in.
//   1. minimum:    o = componentwise minimum of the points that are kept (+ maximum for the extent check, + |F|); every
//                  point leaves 1 / 0 (kept / dropped) in its row_of_point word -- one read-back
//   2. insert:     table_insert; count += 1, first = min(first, i); the slot of every
//                  point is kept (4 bytes) so that no later pass probes again.  A wave whose points all share a cell
//                  sends one probe and one pair of atomics
//   3. ranks:      a point flags itself when it is its cell's first; exclusive scan; second read-back (M)
//   4. rows:       the first points write row -> slot, first, count and key of their rows
//   5. accumulate: row_of_point; in centroid mode the offsets f and the fixed-point normals g are added into M x 6
//                  64-bit integers, lanes of a wave that share a row combined first
//   6. finish:     one thread per row
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "call_scope.h"
#include "cell_grid.h"
#include "rh_internal.h"

namespace {

constexpr int VOX_COMBINE_ROUNDS = 4;  // distinct rows per wave that are looked at for lanes to combine
constexpr int VOX_COMBINE_MIN = 8;     // lanes that share a row before a wave reduction beats their own atomics

struct vox_table {
    uint64_t *key;      // [cap] cell key, GRID_EMPTY: free
    int32_t *count;     // [cap] points in the cell
    int32_t *first;     // [cap] smallest 0-based point index
    int32_t *row;       // [cap] 1-based output row (written by the rows pass)
    uint32_t mask;      // cap - 1 (cap is a power of two)
};

struct vox_grid {
    double o[3];
    double beta;
};

// cell and 32-bit fixed-point offset inside it along one axis: a = (x - o) / beta, c = floor(a), t = a - c (exact),
// f = floor(t * 2^32)
__device__ __forceinline__ void cell_axis(double x, double o, double beta, uint64_t *c, uint64_t *f)
{
    const double a = (x - o) / beta;
    const double fl = floor(a);
    *c = (uint64_t)(long long)fl;
    *f = (uint64_t)floor((a - fl) * 4294967296.0);
}

__device__ __forceinline__ uint64_t cell_key(const double *__restrict__ p, const vox_grid &g)
{
    uint64_t c[3], f;
#pragma unroll
    for (int a = 0; a < 3; a++) cell_axis(p[a], g.o[a], g.beta, &c[a], &f);
    return grid_pack((long long)c[0], (long long)c[1], (long long)c[2], 0);
}

// ---- 1. minimum, maximum and number of the points that are kept; valid[i] = 1 / 0.  Every block (256 threads) leaves
// its partial result in `part`, the fold of cell_grid.h follows
__global__ void __launch_bounds__(256)
vox_minmax_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm, int64_t n, int32_t *__restrict__ valid,
                  unsigned long long *__restrict__ part)
{
    MinMaxCount acc;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double p[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
        bool ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        if (nrm) {
#pragma unroll
            for (int a = 0; a < 3; a++) ok = ok && fabs(nrm[3 * i + a]) <= 2.0;   // (false for NaN and infinities)
        }
        valid[i] = ok ? 1 : 0;
        if (ok) acc.add(p[0], p[1], p[2]);
    }
    acc.store(part);
}

// ---- 2. the cell table
__global__ void __launch_bounds__(256) vox_init_kernel(vox_table T)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > T.mask) return;
    T.key[s] = GRID_EMPTY;
    T.count[s] = 0;
    T.first[s] = 0x7FFFFFFF;
    T.row[s] = 0;
}

// (no thread leaves before the end: the ballots and shuffles count on whole waves; the grid covers n rounded up to 256)
__global__ void __launch_bounds__(256)
vox_insert_kernel(const double *__restrict__ xyz, int64_t n, const int32_t *__restrict__ valid, vox_grid g, vox_table T,
                  uint32_t *__restrict__ slot)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool v = i < n && valid[i] != 0;
    uint64_t key = GRID_EMPTY;
    if (v) key = cell_key(xyz + 3 * i, g);
    const uint64_t act = __builtin_amdgcn_ballot_w64(v);
    if (act == 0) return;   // (the whole wave)
    const int lead = __ffsll((unsigned long long)act) - 1;
    const uint64_t klead = __shfl(key, lead);
    if (__builtin_amdgcn_ballot_w64(v && key == klead) == act) {
        // one cell for the whole wave: its lowest lane holds the smallest index
        uint32_t h = 0;
        if (lane == lead) {
            h = table_insert(T.key, T.mask, key);
            atomicAdd(&T.count[h], (int32_t)__popcll(act));
            atomicMin(&T.first[h], (int32_t)i);
        }
        h = __shfl(h, lead);
        if (v) slot[i] = h;
        return;
    }
    if (v) {
        const uint32_t h = table_insert(T.key, T.mask, key);
        atomicAdd(&T.count[h], 1);
        atomicMin(&T.first[h], (int32_t)i);
        slot[i] = h;
    }
}

// ---- 3. a point is its cell's first
__global__ void __launch_bounds__(256)
vox_flag_kernel(int64_t n, const int32_t *__restrict__ valid, const uint32_t *__restrict__ slot, vox_table T, int32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t f = 0;
    if (valid[i] != 0) {
        const uint32_t s = slot[i];
        f = s <= T.mask && (int64_t)T.first[s] == i;
    }
    flag[i] = f;
}

// ---- 4. the rows: first (1-based), count and key; row -> slot
__global__ void __launch_bounds__(256)
vox_rows_kernel(int64_t n, const int32_t *__restrict__ flag, const int32_t *__restrict__ rank, const uint32_t *__restrict__ slot,
                vox_table T, int64_t M, int64_t *__restrict__ first, int32_t *__restrict__ count, uint64_t *__restrict__ rkey)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || flag[i] == 0) return;
    const int64_t r = rank[i];
    const uint32_t s = slot[i];
    if (r < 0 || r >= M || s > T.mask) return;
    T.row[s] = (int32_t)(r + 1);
    first[r] = i + 1;
    count[r] = T.count[s];
    rkey[r] = T.key[s];
}

// ---- 5. row_of_point (in place of the 1 / 0 of pass 1) and, in centroid mode, the integer sums: 3 offsets, then 3
// fixed-point normal components (NV = 3 or 6 values per point), M x 6 words
template <int NV>
__global__ void __launch_bounds__(256)
vox_accum_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm, int64_t n, int32_t *__restrict__ rowof,
                 const uint32_t *__restrict__ slot, vox_grid g, vox_table T, int64_t M, int centroid, int align,
                 unsigned long long *__restrict__ sums)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool v = i < n && rowof[i] != 0;
    int64_t row = 0;
    int32_t fi = -1;
    if (v) {
        const uint32_t s = slot[i];
        if (s <= T.mask) { row = T.row[s]; fi = T.first[s]; }
        v = row >= 1 && row <= M;
        rowof[i] = v ? (int32_t)row : 0;
    }
    if (!centroid) return;   // (the whole grid)
    unsigned long long val[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) val[k] = 0ULL;
    if (v) {
        uint64_t c;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            uint64_t f;
            cell_axis(xyz[3 * i + a], g.o[a], g.beta, &c, &f);
            val[a] = f;
        }
        if (NV == 6) {
            const double q[3] = { nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2] };
            bool neg = false;
            if (align && fi >= 0 && (int64_t)fi < n) {
                const double *r = nrm + 3 * (int64_t)fi;
                neg = (q[0] * r[0] + q[1] * r[1]) + q[2] * r[2] < 0.0;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const long long gq = llrint(q[a] * 1048576.0);
                val[3 + a] = (unsigned long long)(neg ? -gq : gq);
            }
        }
    }
    // lanes that share a row add up inside the wave before they touch memory: a dense cell would otherwise queue all
    // its points on six addresses.  Only the first few distinct rows of a wave are looked at, and a row with few lanes
    // is cheaper served by their own atomics than by a reduction over 64
    uint64_t todo = __builtin_amdgcn_ballot_w64(v);
    bool done = !v;
    for (int round = 0; round < VOX_COMBINE_ROUNDS && todo != 0; round++) {
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const int64_t rl = __shfl(row, lead);
        const bool mine = !done && row == rl;
        const uint64_t mb = __builtin_amdgcn_ballot_w64(mine);
        if (__popcll(mb) >= VOX_COMBINE_MIN) {
#pragma unroll
            for (int k = 0; k < NV; k++) {
                unsigned long long x = mine ? val[k] : 0ULL;
                for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
                if (lane == lead) atomicAdd(&sums[6 * (size_t)(rl - 1) + k], x);
            }
            if (mine) done = true;
        }
        todo &= ~mb;
    }
    if (!done) {
#pragma unroll
        for (int k = 0; k < NV; k++) atomicAdd(&sums[6 * (size_t)(row - 1) + k], val[k]);
    }
}

// ---- 6. one thread per row
template <typename OutT>
__global__ void __launch_bounds__(256)
vox_finish_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm, int64_t n, int64_t M, vox_grid g, int centroid,
                  const int64_t *__restrict__ first, const int32_t *__restrict__ count, const uint64_t *__restrict__ rkey,
                  const unsigned long long *__restrict__ sums, OutT *__restrict__ xyz_out, OutT *__restrict__ nrm_out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    if (!centroid) {
        const int64_t fi = first[r] - 1;
        if (fi < 0 || fi >= n) return;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            xyz_out[3 * r + a] = (OutT)xyz[3 * fi + a];
            if (nrm_out) nrm_out[3 * r + a] = (OutT)nrm[3 * fi + a];
        }
        return;
    }
    const uint64_t key = rkey[r];
    const double cnt = (double)count[r];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const unsigned long long S = sums[6 * (size_t)r + a];
        const double c = (double)grid_field(key, a);
        const double num = (double)(S >> 32) * 4294967296.0 + (double)(S & 0xFFFFFFFFULL);
        const double m = (num / cnt) * (1.0 / 4294967296.0);
        xyz_out[3 * r + a] = (OutT)(g.o[a] + (c + m) * g.beta);
    }
    if (nrm_out) {
        double G[3];
#pragma unroll
        for (int a = 0; a < 3; a++) G[a] = (double)(long long)sums[6 * (size_t)r + 3 + a];
        const double len = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
#pragma unroll
        for (int a = 0; a < 3; a++) nrm_out[3 * r + a] = (OutT)(len == 0.0 ? 0.0 : G[a] / len);
    }
}

template <typename T>
int downsample(const T *xyz_aos, const T *nrm_aos, int64_t n, const rh_voxel_params *p, int device, T *xyz_out, T *nrm_out,
               int64_t *first_out, int32_t *count_out, int64_t cap, int32_t *rowof_out, int64_t *n_out, int64_t *n_dropped_out)
{
    if (n_out) *n_out = 0;
    if (n_dropped_out) *n_dropped_out = 0;
    if (!xyz_aos || !p || !n_out) { rh_set_error("rh_voxel_downsample: NULL argument"); return RH_E_INVALID; }
    if (n < 1 || n >= ((int64_t)1 << 31)) { rh_set_error("rh_voxel_downsample: n = %lld outside 1 .. 2^31 - 1", (long long)n); return RH_E_INVALID; }
    if (!(p->beta > 0.0) || !(p->beta <= 1.7976931348623157e308)) { rh_set_error("rh_voxel_downsample: beta must be finite and > 0"); return RH_E_INVALID; }
    if (p->mode != RH_VOX_FIRST && p->mode != RH_VOX_CENTROID) { rh_set_error("rh_voxel_downsample: mode = %d outside 0 .. 1", p->mode); return RH_E_INVALID; }
    if (p->flags & ~RH_VOX_ALIGN_NORMALS) { rh_set_error("rh_voxel_downsample: unknown flags %d", p->flags); return RH_E_INVALID; }
    if (cap < 0 || (cap > 0 && !xyz_out)) { rh_set_error("rh_voxel_downsample: no output for %lld rows", (long long)cap); return RH_E_INVALID; }
    if (nrm_out && !nrm_aos) { rh_set_error("rh_voxel_downsample: normals out without normals in"); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open("rh_voxel_downsample", device));
    const hipStream_t st = S.st;
    const int centroid = p->mode == RH_VOX_CENTROID;
    const dim3 blk(256), gp(blocks_for(n));

    double *d_xyz = nullptr, *d_nrm = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyHostToDevice));
    if (nrm_aos) {
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        RH_TRY(S.upload(nrm_aos, d_nrm, 3 * n, hipMemcpyHostToDevice));
    }

    // 1. o, the extent and |F|
    int32_t *d_rowof = nullptr;
    unsigned long long *d_scal = nullptr;
    RH_TRY(S.alloc(&d_rowof, n));
    RH_TRY(S.alloc(&d_scal, MM_WORDS * (1 + GRID_MM_BLOCKS)));
    {
        const int64_t b = std::min<int64_t>((n + 255) / 256, GRID_MM_BLOCKS);
        hipLaunchKernelGGL(vox_minmax_kernel, dim3((unsigned)b), blk, 0, st, d_xyz, d_nrm, n, d_rowof, d_scal + MM_WORDS);
        hipLaunchKernelGGL(grid_minmax_fold_kernel, dim3(1), blk, 0, st, d_scal + MM_WORDS, (int)b, d_scal, (int)MM_WORDS);
        SCOPE_HIP(S, hipGetLastError());
    }
    unsigned long long h_scal[MM_WORDS];
    RH_TRY(S.fetch(h_scal, d_scal, MM_WORDS));
    const int64_t nf = (int64_t)h_scal[MM_COUNT];
    if (n_dropped_out) *n_dropped_out = n - nf;
    auto download_map = [&]() -> int {
        if (rowof_out) SCOPE_HIP(S, hipMemcpyAsync(rowof_out, d_rowof, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        SCOPE_HIP(S, hipStreamSynchronize(st));
        return RH_OK;
    };
    if (nf == 0) return download_map();   // (every word of the map is 0)
    vox_grid g;
    g.beta = p->beta;
    double box_cells = 1.0;
    for (int a = 0; a < 3; a++) {
        g.o[a] = ord_back(h_scal[MM_MIN + a]);
        double cells;
        if (!grid_axis_fits(g.o[a], ord_back(h_scal[MM_MAX + a]), g.beta, &cells)) {
            rh_set_error("rh_voxel_downsample: the points span more than 2^20 cells of size %g along axis %d", g.beta, a);
            return RH_E_INVALID;
        }
        box_cells *= cells + 1.0;
    }

    // 2. the table: 2 min(|F|, cells of the box) slots or more
    uint64_t tcap = 64;
    while ((double)tcap < 2.0 * std::min((double)nf, box_cells)) tcap <<= 1;
    uint8_t *d_tab = nullptr;
    RH_TRY(S.alloc(&d_tab, (int64_t)(tcap * 20)));
    vox_table tab;
    tab.key = (uint64_t *)d_tab;
    tab.count = (int32_t *)(tab.key + tcap);
    tab.first = tab.count + tcap;
    tab.row = tab.first + tcap;
    tab.mask = (uint32_t)(tcap - 1);
    uint32_t *d_slot = nullptr;
    int32_t *d_flag = nullptr, *d_rank = nullptr;
    RH_TRY(S.alloc(&d_slot, n));
    RH_TRY(S.alloc(&d_flag, n));
    RH_TRY(S.alloc(&d_rank, n));
    hipLaunchKernelGGL(vox_init_kernel, dim3(blocks_for((int64_t)tcap)), blk, 0, st, tab);
    hipLaunchKernelGGL(vox_insert_kernel, gp, blk, 0, st, d_xyz, n, d_rowof, g, tab, d_slot);
    // 3. ranks of the first points
    hipLaunchKernelGGL(vox_flag_kernel, gp, blk, 0, st, n, d_rowof, d_slot, tab, d_flag);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_flag, d_rank, (int)n, st); }));
    int32_t last[2] = { 0, 0 };
    SCOPE_HIP(S, hipMemcpyAsync(&last[0], d_rank + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipMemcpyAsync(&last[1], d_flag + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    const int64_t M = (int64_t)last[0] + last[1];
    if (M < 1 || M > nf) { rh_set_error("rh_voxel_downsample: %lld rows from %lld points", (long long)M, (long long)nf); return RH_E_INTERNAL; }
    *n_out = M;
    const bool fits = M <= cap;
    const int sum_mode = fits && centroid;

    // 4. rows, 5. the map and the sums
    int64_t *d_first = nullptr;
    int32_t *d_count = nullptr;
    uint64_t *d_rkey = nullptr;
    unsigned long long *d_sums = nullptr;
    RH_TRY(S.alloc(&d_first, M));
    RH_TRY(S.alloc(&d_count, M));
    RH_TRY(S.alloc(&d_rkey, M));
    if (sum_mode) {
        RH_TRY(S.alloc(&d_sums, 6 * M));
        SCOPE_HIP(S, hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * 6 * (size_t)M, st));
    }
    hipLaunchKernelGGL(vox_rows_kernel, gp, blk, 0, st, n, d_flag, d_rank, d_slot, tab, M, d_first, d_count, d_rkey);
    const int align = (p->flags & RH_VOX_ALIGN_NORMALS) ? 1 : 0;
    if (d_nrm) hipLaunchKernelGGL(vox_accum_kernel<6>, gp, blk, 0, st, d_xyz, d_nrm, n, d_rowof, d_slot, g, tab, M, sum_mode, align, d_sums);
    else hipLaunchKernelGGL(vox_accum_kernel<3>, gp, blk, 0, st, d_xyz, d_nrm, n, d_rowof, d_slot, g, tab, M, sum_mode, align, d_sums);
    SCOPE_HIP(S, hipGetLastError());
    if (!fits) {
        RH_TRY(download_map());
        rh_set_error("rh_voxel_downsample: %lld occupied cells, capacity %lld", (long long)M, (long long)cap);
        return RH_E_CAPACITY;
    }

    // 6. the output rows
    T *d_xout = nullptr, *d_nout = nullptr;
    RH_TRY(S.alloc(&d_xout, 3 * M));
    if (nrm_out) RH_TRY(S.alloc(&d_nout, 3 * M));
    hipLaunchKernelGGL(vox_finish_kernel<T>, dim3(blocks_for(M)), blk, 0, st, d_xyz, d_nrm, n, M, g, centroid, d_first, d_count, d_rkey,
                       d_sums, d_xout, d_nout);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(xyz_out, d_xout, sizeof(T) * 3 * (size_t)M, hipMemcpyDeviceToHost, st));
    if (nrm_out) SCOPE_HIP(S, hipMemcpyAsync(nrm_out, d_nout, sizeof(T) * 3 * (size_t)M, hipMemcpyDeviceToHost, st));
    if (first_out) SCOPE_HIP(S, hipMemcpyAsync(first_out, d_first, sizeof(int64_t) * (size_t)M, hipMemcpyDeviceToHost, st));
    if (count_out) SCOPE_HIP(S, hipMemcpyAsync(count_out, d_count, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, st));
    RH_TRY(download_map());
    return RH_OK;
}

}  // namespace

extern "C" int rh_voxel_downsample(const double *xyz_aos, const double *nrm_aos_or_null, int64_t n, const rh_voxel_params *p, int device,
                                   double *xyz_out_aos, double *nrm_out_aos_or_null, int64_t *first_out_1based_or_null,
                                   int32_t *count_out_or_null, int64_t cap, int32_t *row_of_point_out_or_null,
                                   int64_t *n_out, int64_t *n_dropped_out_or_null)
{
    return downsample<double>(xyz_aos, nrm_aos_or_null, n, p, device, xyz_out_aos, nrm_out_aos_or_null, first_out_1based_or_null,
                              count_out_or_null, cap, row_of_point_out_or_null, n_out, n_dropped_out_or_null);
}

extern "C" int rh_voxel_downsample_f32(const float *xyz_aos, const float *nrm_aos_or_null, int64_t n, const rh_voxel_params *p, int device,
                                       float *xyz_out_aos, float *nrm_out_aos_or_null, int64_t *first_out_1based_or_null,
                                       int32_t *count_out_or_null, int64_t cap, int32_t *row_of_point_out_or_null,
                                       int64_t *n_out, int64_t *n_dropped_out_or_null)
{
    return downsample<float>(xyz_aos, nrm_aos_or_null, n, p, device, xyz_out_aos, nrm_out_aos_or_null, first_out_1based_or_null,
                             count_out_or_null, cap, row_of_point_out_or_null, n_out, n_dropped_out_or_null);
}
