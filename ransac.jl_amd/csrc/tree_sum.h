// tree_sum.h -- T() of include/ransac_hip.h, the order-fixed sum of rh_remove_outliers (knn.hip), rh_cloud_distance
// (knn_query.hip) and rh_register (register.hip, whose kernels fold many components in this very tree): the root of the perfect binary tree over ADJACENT pairs of the leaves, padded with +0.0.  A lane's four
// values, a butterfly over lanes with xor 1, 2, .. 32, adjacent pairs of the four wave sums and then the same kernel over
// the block partials are that very tree, so the bits do not depend on the launch geometry.  No floating-point atomics.
// Everything lives in an anonymous namespace: each translation unit that includes the header gets its own kernels.
#pragma once

#include "call_scope.h"
#include "rh_internal.h"

namespace {

constexpr int OUT_THREADS = 256;
constexpr int OUT_PER_THREAD = 4;
constexpr int OUT_BLOCK_POINTS = OUT_THREADS * OUT_PER_THREAD;
static_assert(OUT_BLOCK_POINTS == RH_OUT_BLOCK_POINTS, "the header names the block size of the reduction tree");
static_assert(OUT_THREADS == 4 * 64, "the block's last two tree levels are written out for four waves");

// the sum of the 64 lanes' values as the tree over adjacent pairs; every lane ends with the same bits
__device__ inline double tree64(double v)
{
    for (int j = 1; j < 64; j <<= 1) v += __shfl_xor(v, j);
    return v;
}

// One level of the tree: block b leaves T() of its OUT_BLOCK_POINTS leaves (+0.0 past n) in part[b].  V = the i with
// count_i >= 1.  MODE 0: leaf i = v_i for i in V, and V is counted into *nvalid (an integer count); 1: (v_i - *mu)*(v_i - *mu)
// for i in V; 2: v_i as it is; 3: v_i*v_i for i in V.
template <int MODE>
__global__ __launch_bounds__(OUT_THREADS) void out_tree_kernel(const double *__restrict__ v, const int32_t *__restrict__ count,
                                                              int64_t n, const double *mu_in, unsigned long long *nvalid,
                                                              double *__restrict__ part)
{
    const int64_t base = ((int64_t)blockIdx.x * OUT_THREADS + threadIdx.x) * OUT_PER_THREAD;
    double a[OUT_PER_THREAD];
    int nv = 0;
    const double mu = MODE == 1 ? *mu_in : 0.0;
    for (int j = 0; j < OUT_PER_THREAD; j++) {
        const int64_t i = base + j;
        a[j] = 0.0;
        if (i >= n) continue;
        if (MODE == 2) { a[j] = v[i]; continue; }
        if (count[i] < 1) continue;
        nv++;
        const double x = v[i];
        if (MODE == 0) a[j] = x;
        else if (MODE == 3) a[j] = x * x;
        else { const double d = x - mu; a[j] = d * d; }
    }
    const double s = tree64((a[0] + a[1]) + (a[2] + a[3]));
    __shared__ double ws[OUT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    if (MODE == 0) {
        for (int j = 1; j < 64; j <<= 1) nv += __shfl_xor(nv, j);
        if ((threadIdx.x & 63) == 0 && nv) atomicAdd(nvalid, (unsigned long long)nv);
    }
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// the two buffers a tree of n leaves folds through
inline int tree_alloc(CallScope &S, int64_t n, double *d_part[2])
{
    const int64_t len1 = (n + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS;
    RH_TRY(S.alloc(&d_part[0], len1));
    RH_TRY(S.alloc(&d_part[1], (len1 + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS));
    return RH_OK;
}

// T() over the leaves of MODE (0 / 1 / 3) of the n points: level after level until one value is left; *root_out points at it
template <int MODE>
int tree_root(CallScope &S, const double *d_v, const int32_t *d_count, int64_t n, const double *d_mu, unsigned long long *d_nvalid,
              double *d_part[2], const double **root_out)
{
    int64_t len = (n + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS;
    hipLaunchKernelGGL(out_tree_kernel<MODE>, dim3((unsigned)len), dim3(OUT_THREADS), 0, S.st, d_v, d_count, n, d_mu, d_nvalid, d_part[0]);
    SCOPE_HIP(S, hipGetLastError());
    int cur = 0;
    while (len > 1) {
        const int64_t nb = (len + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS;
        hipLaunchKernelGGL(out_tree_kernel<2>, dim3((unsigned)nb), dim3(OUT_THREADS), 0, S.st, d_part[cur], (const int32_t *)nullptr, len,
                           (const double *)nullptr, (unsigned long long *)nullptr, d_part[cur ^ 1]);
        SCOPE_HIP(S, hipGetLastError());
        cur ^= 1;
        len = nb;
    }
    *root_out = d_part[cur];
    return RH_OK;
}

}  // namespace
