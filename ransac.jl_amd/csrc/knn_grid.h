// knn_grid.h -- the uniform grid of the exact k-nearest-neighbour search (knn_device.h has the query), shared by
// normals.hip (rh_estimate_normals) and knn.hip (rh_knn, rh_remove_outliers):
//   points radix-sorted by cell key, an open-addressing hash table key -> [start, end) of the occupied cells only (empty
//   space costs nothing), the coordinates gathered into cell order.  KnnIndex owns the buffers of one call and rebuilds the
//   grid for any cell width.
// Everything here lives in an anonymous namespace: each translation unit that includes the header gets its own kernels.
#pragma once

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

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

inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// device buffers of one call, freed on every way out
struct Buffers {
    const char *who;         // the entry point, for error texts
    std::vector<void *> ptrs;
    explicit Buffers(const char *who_) : who(who_) {}
    ~Buffers() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T>
    int alloc(T **p, int64_t count)
    {
        *p = nullptr;
        const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
        const hipError_t e = hipMalloc((void **)p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rh_set_error("%s: hipMalloc(%zu bytes) failed: %s", who, bytes, hipGetErrorString(e));
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

#define KNN_HIP(who_, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { rh_set_error("%s: %s", (who_), hipGetErrorString(e_)); return RH_E_NODEVICE; } } while (0)

// the usable device and a stream of the call's own
inline int knn_open_device(const char *who, int device, StreamHolder &sh)
{
    int ndev = 0;
    RH_TRY(rh_device_count(&ndev));
    if (ndev <= 0) { rh_set_error("no HIP device is visible; libransac_hip has no CPU fallback"); return RH_E_NODEVICE; }
    if (device < 0 || device >= ndev) { rh_set_error("device %d out of range (%d visible)", device, ndev); return RH_E_INVALID; }
    KNN_HIP(who, hipSetDevice(device));
    KNN_HIP(who, hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    return RH_OK;
}

// cnt values of T from the caller's array into doubles on the device, widened exactly
template <typename T>
int knn_upload(Buffers &B, hipStream_t st, const T *src, double *dst, int64_t cnt, hipMemcpyKind kind)
{
    if (sizeof(T) == sizeof(double)) {
        KNN_HIP(B.who, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)cnt, kind, st));
        return RH_OK;
    }
    T *d_in = nullptr;
    RH_TRY(B.alloc(&d_in, cnt));
    KNN_HIP(B.who, hipMemcpyAsync(d_in, src, sizeof(T) * (size_t)cnt, kind, st));
    hipLaunchKernelGGL(nrm_widen_kernel<T>, dim3(nblk(cnt, 256)), dim3(256), 0, st, d_in, dst, cnt);
    KNN_HIP(B.who, hipGetLastError());
    KNN_HIP(B.who, hipStreamSynchronize(st));
    B.release(d_in);
    return RH_OK;
}

// The grid over the n points of one call: init() finds the bounding box (RH_E_INVALID on a coordinate that is not finite)
// and allocates, build(h) makes the grid of cell width h (again and again: the buffers are re-used).
struct KnnIndex {
    Buffers *B = nullptr;
    hipStream_t st = nullptr;
    int64_t n = 0;
    double *d_xyz = nullptr;
    double lo[3], hi[3], ext[3], L = 0.0, omax = 0.0;
    uint64_t *d_key[2] = { nullptr, nullptr };
    int32_t *d_idx[2] = { nullptr, nullptr };
    double *d_s[3] = { nullptr, nullptr, nullptr };
    unsigned long long *d_count = nullptr;
    uint8_t *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    uint64_t *d_hkey = nullptr;
    int32_t *d_hrange = nullptr;
    uint64_t hcap = 0;
    Grid g;

    int init(Buffers &B_, hipStream_t st_, double *d_xyz_, int64_t n_)
    {
        B = &B_; st = st_; d_xyz = d_xyz_; n = n_;
        const char *who = B->who;
        // bounding box and the finiteness of every coordinate
        double *d_part = nullptr;
        RH_TRY(B->alloc(&d_part, 7 * NRM_BBOX_BLOCKS));
        hipLaunchKernelGGL(nrm_bbox_kernel, dim3(NRM_BBOX_BLOCKS), dim3(NRM_BLOCK), 0, st, d_xyz, n, d_part);
        KNN_HIP(who, hipGetLastError());
        std::vector<double> part(7 * NRM_BBOX_BLOCKS);
        KNN_HIP(who, hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
        KNN_HIP(who, hipStreamSynchronize(st));
        for (int ax = 0; ax < 3; ax++) { lo[ax] = INFINITY; hi[ax] = -INFINITY; }
        for (int b = 0; b < NRM_BBOX_BLOCKS; b++) {
            if (part[7 * b + 6] != 0.0) { rh_set_error("%s: a coordinate is not finite", who); return RH_E_INVALID; }
            for (int ax = 0; ax < 3; ax++) { lo[ax] = std::min(lo[ax], part[7 * b + ax]); hi[ax] = std::max(hi[ax], part[7 * b + 3 + ax]); }
        }
        L = 0.0; omax = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            ext[ax] = hi[ax] - lo[ax];
            L = std::max(L, ext[ax]);
            omax = std::max(omax, std::max(fabs(lo[ax]), fabs(hi[ax])));
        }
        RH_TRY(B->alloc(&d_key[0], n)); RH_TRY(B->alloc(&d_key[1], n));
        RH_TRY(B->alloc(&d_idx[0], n)); RH_TRY(B->alloc(&d_idx[1], n));
        for (int ax = 0; ax < 3; ax++) RH_TRY(B->alloc(&d_s[ax], n));
        RH_TRY(B->alloc(&d_count, 1));
        KNN_HIP(who, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)n, 0, 64, st));
        RH_TRY(B->alloc(&d_tmp, (int64_t)tmp_bytes));
        return RH_OK;
    }

    // grid of width h: sort by cell, gather, hash table of the occupied cells
    int build(double h)
    {
        const char *who = B->who;
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
        KNN_HIP(who, hipGetLastError());
        KNN_HIP(who, hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_key[0], d_key[1], d_idx[0], d_idx[1], (int)n, 0, bits, st));
        hipLaunchKernelGGL(nrm_gather_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_xyz, d_idx[1], n, d_s[0], d_s[1], d_s[2]);
        KNN_HIP(who, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(nrm_runs_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_key[1], n, d_count);
        KNN_HIP(who, hipGetLastError());
        unsigned long long occupied = 0;
        KNN_HIP(who, hipMemcpyAsync(&occupied, d_count, sizeof occupied, hipMemcpyDeviceToHost, st));
        KNN_HIP(who, hipStreamSynchronize(st));
        uint64_t cap = 64;
        while (cap < 2 * occupied) cap <<= 1;
        if (cap > hcap) {
            B->release(d_hkey);
            B->release(d_hrange);
            RH_TRY(B->alloc(&d_hkey, (int64_t)cap));
            RH_TRY(B->alloc(&d_hrange, 2 * (int64_t)cap));
            hcap = cap;
        }
        KNN_HIP(who, hipMemsetAsync(d_hkey, 0xFF, sizeof(uint64_t) * cap, st));
        hipLaunchKernelGGL(nrm_hash_kernel, dim3(nblk(n, 256)), dim3(256), 0, st, d_key[1], n, d_hkey, d_hrange, cap - 1);
        KNN_HIP(who, hipGetLastError());
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
