// boxes32.hip -- the binary32 twins of an ordering of subset 1, made once per cloud: what stage 1 of the v4 score kernel
// (score4.hip) and the list launch in front of it read instead of the points.  Per 64-point group its box and its normal-cell
// mask, per super-tile (S4_STG groups) the same, per tile (S4_TG groups) a box, and the largest normal length of the subset.
// The leaf order's twins live on the cloud next to its binary64 boxes (rhk_gb32_build); the plane order's (kdorder.hip) have
// their binary64 boxes as a temporary (rhk_plane_boxes).
#include "rh_internal.h"
#include "score_device.h"
#include "score4_device.h"
#include "score4_shared.h"

namespace {

using namespace rhdev;
using namespace rh4;

// binary32 boxes of the groups from the binary64 ones (7 planes of gstride doubles): 8 floats per group
__global__ void gb32_kernel(const double *__restrict__ gb, int64_t gstride, int64_t ngroups, float *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    const double c[3] = { gb[g], gb[gstride + g], gb[2 * gstride + g] };
    const double h[3] = { gb[3 * gstride + g], gb[4 * gstride + g], gb[5 * gstride + g] };
    float o[8];
    box_to_f32(c, h, o);
#pragma unroll
    for (int k = 0; k < 8; k++) out[g * 8 + k] = o[k];
}

// boxes of runs of k consecutive groups (k = S4_STG: the super-tiles, k = S4_TG: the tiles): the union of the groups' boxes,
// widened by what the unions' own arithmetic can lose, then made binary32 like a group's.  A group box that is not finite
// makes the union's NaN: never skipped.
__global__ void st32_kernel(const double *__restrict__ gb, int64_t gstride, int64_t ngroups, int k_groups, int64_t nst, float *__restrict__ out)
{
    const int64_t st = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (st >= nst) return;
    double lo[3] = { __builtin_inf(), __builtin_inf(), __builtin_inf() }, hi[3] = { -__builtin_inf(), -__builtin_inf(), -__builtin_inf() };
    bool bad = false;
    for (int64_t g = st * k_groups; g < (st + 1) * k_groups && g < ngroups; g++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double cc = gb[k * gstride + g], hh = gb[(3 + k) * gstride + g];
            bad |= !(fabs(cc) < __builtin_inf()) || !(fabs(hh) < __builtin_inf());
            lo[k] = fmin(lo[k], cc - hh);
            hi[k] = fmax(hi[k], cc + hh);
        }
    double c3[3], h3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c3[k] = 0.5 * lo[k] + 0.5 * hi[k];
        // (cc -+ hh above and the two differences below each round once: a few ulps of the LARGEST magnitude involved, not of h)
        h3[k] = fmax(hi[k] - c3[k], c3[k] - lo[k]) * 1.000000000001 + (fabs(lo[k]) + fabs(hi[k])) * 1e-15;
        bad |= !(fabs(c3[k]) < __builtin_inf()) || !(h3[k] < __builtin_inf());
    }
    float o[8];
    box_to_f32(c3, h3, o);
#pragma unroll
    for (int k = 0; k < 8; k++) out[st * 8 + k] = bad ? __builtin_nanf("") : o[k];
}

// normal-cell masks of the groups (score4_device.h): a wave per group, lane = point; every point of the group counts, enabled
// or not.  out: 4 words per group (96 bits + 0).  maxlen: the largest finite normal length seen (bits of a non-negative double).
__global__ void __launch_bounds__(256)
nsig_kernel(const double *__restrict__ pts, int64_t stride, int64_t s, int64_t ngroups, uint32_t *__restrict__ out, unsigned long long *__restrict__ maxlen)
{
    __shared__ uint32_t m[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 4 + wv;
    if (lane < 4) m[wv][lane] = 0u;
    __syncthreads();
    const int64_t i = g * 64 + lane;
    double len = 0.0;
    if (g < ngroups && i < s) {
        const double nx = pts[3 * stride + i], ny = pts[4 * stride + i], nz = pts[5 * stride + i];
        uint32_t w[3];
        nsig_point_bits(nx, ny, nz, w);
        if (w[0] != 0u) atomicOr(&m[wv][0], w[0]);
        if (w[1] != 0u) atomicOr(&m[wv][1], w[1]);
        if (w[2] != 0u) atomicOr(&m[wv][2], w[2]);
        const double l = sqrt((nx * nx + ny * ny) + nz * nz);
        if (l < __builtin_inf()) len = l;   // (NaN and inf: not a length; such a normal sets no bit or all of them)
    }
    unsigned long long lb = __builtin_bit_cast(unsigned long long, len);
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long v = __shfl_down(lb, off); lb = v > lb ? v : lb; }
    if (lane == 0 && lb != 0ULL) atomicMax(maxlen, lb);
    __syncthreads();
    if (g < ngroups && lane < 4) out[g * 4 + lane] = m[wv][lane];
}

// ... of the super-tiles: the OR of their groups' masks
__global__ void nsig_st_kernel(const uint32_t *__restrict__ gm, int64_t ngroups, int k_groups, int64_t nst, uint32_t *__restrict__ out)
{
    const int64_t st = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (st >= nst) return;
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    for (int64_t g = st * k_groups; g < (st + 1) * k_groups && g < ngroups; g++)
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] |= gm[g * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; k++) out[st * 4 + k] = w[k];
}

// one ordering of subset 1 and where its twins go
struct Twins32 {
    const double *pts;               // the points in that order, six planes c->s_pad apart
    const double *gb;                // the binary64 boxes of its groups, 7 planes c->ng_pad apart
    float *gb32, *st32, *tile32;     // boxes of the groups, the super-tiles, the tiles (st32 / tile32 null: none)
    uint32_t *gm32, *stm32;          // normal-cell masks of the groups and the super-tiles (either null: none)
};

// The twins of T on c->stream: the boxes, then the masks.  The points' normals never change and the masks do not look at the
// enabled bits, so once per cloud is enough.  With masks the call waits for the stream -- *nrm_len (optional) comes back with
// them, the largest finite normal length of the subset; without masks it only queues.
int twins32_build(rh_cloud *c, const Twins32 &T, double *nrm_len)
{
    rhk_gb32_of(c, T.gb, c->ngroups, T.gb32);
    if (T.st32 != nullptr && c->nst > 0) rhk_runs32_of(c, T.gb, S4_STG, c->nst, T.st32);
    if (T.tile32 != nullptr && c->ntile > 0) rhk_runs32_of(c, T.gb, S4_TG, c->ntile, T.tile32);
    RH_HIP(hipGetLastError());
    if (nrm_len != nullptr) *nrm_len = 0.0;
    if (T.gm32 == nullptr || T.stm32 == nullptr || c->s <= 0) return RH_OK;
    rh_dev<unsigned long long> d_len;
    RH_TRY(d_len.alloc(1));
    RH_HIP(hipMemsetAsync(d_len, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(nsig_kernel, dim3(cdiv4(c->ngroups, 4)), dim3(256), 0, c->stream, T.pts, c->s_pad, c->s, c->ngroups, T.gm32, d_len);
    hipLaunchKernelGGL(nsig_st_kernel, dim3(cdiv4(c->nst, 64)), dim3(64), 0, c->stream, T.gm32, c->ngroups, S4_STG, c->nst, T.stm32);
    RH_HIP(hipGetLastError());
    unsigned long long h_len = 0;
    if (nrm_len != nullptr) RH_HIP(hipMemcpyAsync(&h_len, d_len, sizeof h_len, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    if (nrm_len != nullptr) *nrm_len = __builtin_bit_cast(double, h_len);
    return RH_OK;
}

}  // namespace

// the binary32 boxes of ng groups from their binary64 ones (7 planes c->ng_pad apart); queued on c->stream
void rhk_gb32_of(rh_cloud *c, const double *gb, int64_t ng, float *gb32)
{
    hipLaunchKernelGGL(gb32_kernel, dim3(cdiv4(ng, 256)), dim3(256), 0, c->stream, gb, c->ng_pad, ng, gb32);
}

// the binary32 boxes of the nruns runs of k consecutive groups of subset 1 (st32_kernel) from the groups' binary64 boxes; queued on c->stream
void rhk_runs32_of(rh_cloud *c, const double *gb, int k, int64_t nruns, float *out)
{
    hipLaunchKernelGGL(st32_kernel, dim3(cdiv4(nruns, 64)), dim3(64), 0, c->stream, gb, c->ng_pad, c->ngroups, k, nruns, out);
}

// the leaf order: from c->gb, onto the cloud.  Waits for the stream only when it makes masks (one wait, at creation).
int rhk_gb32_build(rh_cloud *c)
{
    if (c->ngroups == 0 || c->gb32 == nullptr) return RH_OK;
    return twins32_build(c, { c->sub, c->gb, c->gb32, c->st32, c->tile32, c->gm32, c->stm32 }, &c->nrm_len);
}

// the plane order (kdorder.hip): boxes and normal-cell masks of the 64-point groups of c->pl_sub and of its super-tiles -- 16
// consecutive groups of the plane order are another point set than 16 of the leaf order.  No tile boxes: the launch cuts its
// lists by super-tiles.  The binary64 boxes are a temporary of the call: it always makes masks (pl_gm32 and pl_stm32 come with
// pl_sub, and a group means a point), so twins32_build has waited for the stream when it returns.
int rhk_plane_boxes(rh_cloud *c)
{
    if (c->pl_sub == nullptr || c->pl_gm32 == nullptr || c->pl_stm32 == nullptr || c->ngroups == 0) return RH_OK;
    rh_dev<double> gb;
    RH_TRY(gb.alloc(7 * c->ng_pad));
    RH_HIP(hipMemsetAsync(gb, 0, sizeof(double) * 7 * (size_t)c->ng_pad, c->stream));
    RH_HIP(hipMemsetAsync(c->pl_gb32, 0, sizeof(float) * 8 * (size_t)c->ng_pad, c->stream));
    RH_HIP(hipMemsetAsync(c->pl_gm32, 0, sizeof(uint32_t) * 4 * (size_t)c->ng_pad, c->stream));
    RH_TRY(rhk_group_bounds_of(c, c->pl_sub, c->s_pad, c->s, c->ngroups, gb, c->ng_pad));
    return twins32_build(c, { c->pl_sub, gb, c->pl_gb32, c->pl_st32, nullptr, c->pl_gm32, c->pl_stm32 }, nullptr);
}
