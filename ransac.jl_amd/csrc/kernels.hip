// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the RANSAC hot path.
//
// Numerics contract: IEEE binary64, the reference's operation order, NO fused
// multiply-add (built with -ffp-contract=off), correctly rounded sqrt and divide.
// Each per-point test cites the reference function it restates (paths under
// /root/reference/src).  StaticArrays semantics: dot = (a1*b1 + a2*b2) + a3*b3,
// norm = sqrt of the same sum of squares, normalize(a) = (1/norm(a)) * a.
//
// Layout: points are structure-of-arrays, six planes (x y z nx ny nz) of `stride`
// doubles; lane i of a wave reads element base+i of each plane (512-B coalesced
// loads).  Candidate constants are wave-uniform: they are read with scalar loads
// into SGPRs, the per-point math runs on the FP64 vector ALU, inlier counts come
// from 64-bit wave ballots + s_bcnt1 (no cross-lane reduction tree).

#include <stdlib.h>

#include <type_traits>

#include "rh_internal.h"
#include "score_device.h"
#include "score4_device.h"

namespace {

using namespace rhdev;

// -------------------------------------------------------------- prep ------
// (the record makers themselves: prep_one / prep_derived, rh_internal.h)
// thresholds and magnitudes behind the classifier / culling records (rh4::cls_make) the prep kernels leave beside the bins
struct PreArgs { double eps[4]; double cosa[4]; double coord_mag, nrm_mag, nrm_len; int f32; float *box; int64_t bstride; };

__global__ void prep_sorted_kernel(const rh_shape *__restrict__ shapes, int32_t b, rh_prep *__restrict__ prep,
                                   int32_t *__restrict__ counts_zero, rh4::rh_cls *__restrict__ cls, const PreArgs QA)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b) {
        rh_prep P;
        const int kind = shapes[i].kind;
        prep_one(shapes[i], P);
        prep[i] = P;
        if (counts_zero != nullptr) counts_zero[i] = 0;
        if (cls != nullptr && kind >= 0 && kind <= 3)
            rh4::cls_make(P, kind, QA.eps[kind], QA.cosa[kind], QA.coord_mag, QA.nrm_mag, cls[i], QA.box + i, QA.bstride, nullptr, QA.f32 != 0, QA.nrm_len);
    }
}

// unknown kinds (device-resident batch): bin by kind, one atomic per (wave, kind)
// counts_zero (optional): the batch's counts array, zeroed here; nk_other (optional): the OTHER half of a
// double-buffered bin-size array, zeroed for the next batch -- a scoring step then needs no memset at all
// `spread`: thread t takes candidate (t * spread) mod b (spread coprime to b, rh_spread_multiplier): neighbours
// in the batch -- often hypotheses of the same primitive -- end up in different 64-candidate chunks.  A chunk of
// near-identical candidates makes the tiles it touches 64 x heavier than the rest (measured on the cfg3 batch
// sorted by primitive: 0.231 ms instead of 0.180).
// cls (optional): the binary32 classifier record (rh4::rh_cls, score4_device.h) of every binned candidate, slot for slot,
// and its culling record in QA.box -- what the culled score kernel (score4.hip) reads

__global__ void prep_binned_kernel(const rh_shape *__restrict__ shapes, int32_t b, rh_prep *__restrict__ prep,
                                   int32_t *__restrict__ orig, int32_t *__restrict__ nk, int64_t cap,
                                   int32_t *__restrict__ counts_zero, int32_t *__restrict__ nk_other, int32_t spread,
                                   rh4::rh_cls *__restrict__ cls, const PreArgs QA, int32_t *__restrict__ zero_extra, int32_t zero_extra_n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    // (a wider range of counts to zero: the other ranks' slices of a sharded batch, rh_score_batch_allreduce_dev)
    for (int i = t; i < zero_extra_n; i += gridDim.x * blockDim.x) zero_extra[i] = 0;
    const int lane = threadIdx.x & 63;
    rh_shape s;
    int kind = -1;
    if (t < 4 && nk_other != nullptr) nk_other[t] = 0;
    const int i = t < b ? (int)(((int64_t)t * spread) % b) : 0;
    if (t < b) {
        if (counts_zero != nullptr) counts_zero[t] = 0;
        s = shapes[i];
        if (s.kind >= 0 && s.kind <= 3) kind = s.kind;   // anything else: counts[i] stays 0
    }
    // slot in the kind's bin: the first lane of every kind present in the wave reserves the wave's share -- ONE atomic
    // instruction (up to four lanes, four counters), one round trip
    int slot = 0;
    {
        uint64_t mk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t m = WB(kind == k);
            if (kind == k) mk = m;
        }
        const int leader = mk != 0 ? __builtin_ctzll(mk) : lane;
        int base = 0;
        if (kind >= 0 && lane == leader) base = atomicAdd(&nk[kind], __popcll(mk));
        base = __shfl(base, leader);
        slot = base + __popcll(mk & ((1ULL << lane) - 1ULL));
    }
    if (kind < 0) return;
    rh_prep P;
    prep_one(s, P);
    prep[(int64_t)kind * cap + slot] = P;
    orig[(int64_t)kind * cap + slot] = i;
    if (cls != nullptr)
        rh4::cls_make(P, kind, QA.eps[kind], QA.cosa[kind], QA.coord_mag, QA.nrm_mag, cls[(int64_t)kind * cap + slot],
                      QA.box + ((int64_t)kind * cap + slot), QA.bstride, nullptr, QA.f32 != 0, QA.nrm_len);
}

// the sampler's candidate list (count on the device): bin by kind like prep_binned_kernel, zero the counts
__global__ void prep_entries_kernel(const rh_cand_entry *__restrict__ entries, const int32_t *__restrict__ count_ptr,
                                    int32_t cap_entries, rh_prep *__restrict__ prep, int32_t *__restrict__ orig,
                                    int32_t *__restrict__ nk, int64_t cap, int32_t *__restrict__ counts,
                                    rh4::rh_cls *__restrict__ cls, const PreArgs QA, const rh_oct_state *__restrict__ ost)
{
    // (an iteration of a chained octree window takes the entries from its start in the list on; nothing after a stop)
    if (ost != nullptr && ost->stop != 0) return;
    const int i = (ost != nullptr ? ost->start : 0) + blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int b = min(*count_ptr, cap_entries);
    rh_shape s;
    int kind = -1;
    if (i < b) {
        s = entries[i].shape;
        counts[i] = 0;
        if (s.kind >= 0 && s.kind <= 3) kind = s.kind;
    }
    // slot in the kind's bin: the first lane of every kind present in the wave reserves the wave's share -- ONE atomic
    // instruction (up to four lanes, four counters), one round trip
    int slot = 0;
    {
        uint64_t mk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t m = WB(kind == k);
            if (kind == k) mk = m;
        }
        const int leader = mk != 0 ? __builtin_ctzll(mk) : lane;
        int base = 0;
        if (kind >= 0 && lane == leader) base = atomicAdd(&nk[kind], __popcll(mk));
        base = __shfl(base, leader);
        slot = base + __popcll(mk & ((1ULL << lane) - 1ULL));
    }
    if (kind < 0) return;
    rh_prep P;
    prep_one(s, P);
    prep[(int64_t)kind * cap + slot] = P;
    orig[(int64_t)kind * cap + slot] = i;
    if (cls != nullptr)
        rh4::cls_make(P, kind, QA.eps[kind], QA.cosa[kind], QA.coord_mag, QA.nrm_mag, cls[(int64_t)kind * cap + slot],
                      QA.box + ((int64_t)kind * cap + slot), QA.bstride, nullptr, QA.f32 != 0, QA.nrm_len);
}

// ------------------------------------------------------------- score ------
// grid.x = point splits, grid.y = candidate tiles of RH_SC_CT.  A wave owns
// RH_SC_WAVE_PTS contiguous points per tile (PPT x 64, PPT points per lane in
// registers) and walks the block's candidates; per candidate it issues PPT tests per
// lane, PPT ballots, and one LDS atomic with the wave's popcount.
// F32: the points are a Float32 cloud's (exactly converted), the test is the binary32 one on the float record that follows
// from the candidate's binary64 record (prepf_of, rh_internal.h) -- every brute-force score of such a cloud.  T: how the
// points are stored -- doubles (the disabled list, rh_ransac's subsets), or the float copy of subset 1 (batches)
template <int KIND, bool MASK, bool F32 = false, typename T = double>
__global__ void __launch_bounds__(RH_SC_THREADS)
score_kernel(const T *__restrict__ pts, int64_t stride, int64_t s,
             const uint64_t *__restrict__ enabled_words, const rh_prep *__restrict__ prep,
             const int32_t *__restrict__ orig, const int32_t *__restrict__ nk_ptr, double eps, double cosa,
             int32_t *__restrict__ counts, uint64_t *__restrict__ masks, int64_t mask_stride)
{
    const int nk = *nk_ptr;
    const int c0 = blockIdx.y * RH_SC_CT;
    if (c0 >= nk) return;
    const int nc = min(RH_SC_CT, nk - c0);

    __shared__ int32_t lcnt[RH_SC_CT];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < RH_SC_CT) lcnt[tid] = 0;
    __syncthreads();

    const T *__restrict__ X = pts, *__restrict__ Y = pts + stride, *__restrict__ Z = pts + 2 * stride;
    const T *__restrict__ NX = pts + 3 * stride, *__restrict__ NY = pts + 4 * stride, *__restrict__ NZ = pts + 5 * stride;
    const int64_t ntiles = (s + RH_SC_TILE - 1) / RH_SC_TILE;
    const int64_t swords = (s + 63) >> 6;
    static_assert(RH_SC_CT == 64, "one lane per candidate of the tile");
    static_assert(F32 || sizeof(T) == sizeof(double), "float points are a Float32 cloud's");
    int acc = 0;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t wbase = tile * RH_SC_TILE + (int64_t)wave * RH_SC_WAVE_PTS;
        T px[RH_SC_PPT], py[RH_SC_PPT], pz[RH_SC_PPT], qx[RH_SC_PPT], qy[RH_SC_PPT], qz[RH_SC_PPT];
        uint64_t en[RH_SC_PPT];
#pragma unroll
        for (int p = 0; p < RH_SC_PPT; p++) {
            const int64_t i = wbase + p * 64 + lane;
            px[p] = X[i]; py[p] = Y[i]; pz[p] = Z[i];
            qx[p] = NX[i]; qy[p] = NY[i]; qz[p] = NZ[i];
            const int64_t gb = wbase + p * 64;
            uint64_t v = valid_mask(gb, s);
            if (enabled_words != nullptr && v != 0) v &= enabled_words[gb >> 6];
            en[p] = v;
        }
        // candidate constants: scalar loads, software-prefetched one candidate ahead
        rh_prep P = prep[c0];
        for (int c = 0; c < nc; c++) {
            const rh_prep Pn = prep[c0 + min(c + 1, nc - 1)];
            uint64_t bw[RH_SC_PPT];
            int n = 0;
#pragma unroll
            for (int p = 0; p < RH_SC_PPT; p++) {
                if (F32) bw[p] = test_point<KIND>(prepf_of<KIND>(P), (float)px[p], (float)py[p], (float)pz[p], (float)qx[p], (float)qy[p],
                                                  (float)qz[p], eps, cosa) & en[p];
                else bw[p] = test_point<KIND>(P, px[p], py[p], pz[p], qx[p], qy[p], qz[p], eps, cosa) & en[p];
                n += __popcll(bw[p]);
            }
            acc += (lane == c) ? n : 0;   // lane c keeps candidate c0+c's count (RH_SC_CT == 64)
            if (MASK) {
                const int64_t w0 = wbase >> 6;
                if (lane < RH_SC_PPT && w0 + lane < swords) {
                    uint64_t v = bw[0];
#pragma unroll
                    for (int p = 1; p < RH_SC_PPT; p++) v = (lane == p) ? bw[p] : v;
                    masks[(int64_t)orig[c0 + c] * mask_stride + w0 + lane] = v;
                }
            }
            P = Pn;
        }
    }
    if (acc != 0) atomicAdd(&lcnt[lane], acc);
    __syncthreads();
    if (tid < nc) {
        const int v = lcnt[tid];
        if (v != 0) atomicAdd(&counts[orig[c0 + tid]], v);
    }
}

// one wave per 64-point group: axis-aligned box of its valid points
__global__ void __launch_bounds__(256)
group_bounds_kernel(const double *__restrict__ pts, int64_t stride, int64_t s, int64_t ngroups,
                    double *__restrict__ gb, int64_t gstride)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const int64_t i = (g << 6) + lane;
    const bool valid = i < s;
    const int64_t ii = valid ? i : (g << 6);   // the first point of a group is always valid
    double mn[3], mx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v = pts[k * stride + ii];
        mn[k] = v; mx[k] = v;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fmin(mn[k], __shfl_xor(mn[k], off));
            mx[k] = fmax(mx[k], __shfl_xor(mx[k], off));
        }
    }
    if (lane == 0) {
        double h2 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double c = 0.5 * mn[k] + 0.5 * mx[k];
            const double h = fmax(mx[k] - c, c - mn[k]) * 1.0000000000000009;
            gb[k * gstride + g] = c;
            gb[(3 + k) * gstride + g] = h;
            h2 += h * h;
        }
        gb[6 * gstride + g] = sqrt(h2) * 1.0000000000000009;
    }
}

// masks in internal (k-d leaf) order -> subset order.  One block per (candidate row, output segment): the segment of
// the output row is assembled in LDS -- every set bit of the row's input words is one LDS atomicOr at its subset
// position -- and written out once, coalesced, so the output needs neither a memset nor global atomics (the first
// version issued one global atomicOr per inlier: 12.4M of them on the cfg3 batch, 0.48 ms).
constexpr int RH_UNPERM_SEG_WORDS = 16384;   // 128 KB of LDS per block of 1024 threads (one block per CU then: 16 waves)

__global__ void __launch_bounds__(1024)
unpermute_masks_kernel(const uint64_t *__restrict__ in, const int32_t *__restrict__ perm, int64_t swords,
                       uint64_t *__restrict__ out)
{
    extern __shared__ unsigned long long seg[];
    const int64_t row = blockIdx.x;
    const int64_t w0 = (int64_t)blockIdx.y * RH_UNPERM_SEG_WORDS;
    const int nw = (int)(swords - w0 < RH_UNPERM_SEG_WORDS ? swords - w0 : RH_UNPERM_SEG_WORDS);
    for (int t = threadIdx.x; t < nw; t += 1024) seg[t] = 0ULL;
    __syncthreads();
    const uint64_t *__restrict__ src = in + row * swords;
    const int64_t lo = w0 << 6, hi = lo + ((int64_t)nw << 6);
    for (int64_t w = threadIdx.x; w < swords; w += 1024) {
        uint64_t m = src[w];
        while (m != 0) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t j = perm[(w << 6) + b];
            if (j >= lo && j < hi) atomicOr(&seg[(j - lo) >> 6], 1ULL << (j & 63));
        }
    }
    __syncthreads();
    uint64_t *__restrict__ dst = out + row * swords + w0;
    for (int t = threadIdx.x; t < nw; t += 1024) dst[t] = seg[t];
}

// the same for rows too long for one LDS segment (cfg5: 24 415 words): one thread per input word, one global atomicOr per
// inlier into the zeroed output (at that size the masks are sparse and two full passes over the rows cost more)
__global__ void unpermute_masks_atomic_kernel(const uint64_t *__restrict__ in, const int32_t *__restrict__ perm, int64_t swords,
                                              int64_t total_words, uint64_t *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_words) return;
    uint64_t m = in[t];
    const int64_t row = t / swords, w = t - row * swords;
    while (m != 0) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t j = perm[(w << 6) + b];
        atomicOr((unsigned long long *)&out[row * swords + (j >> 6)], 1ULL << (j & 63));
    }
}

// ------------------------------------------------------------- refit ------
// One candidate (kernarg -> SGPRs), the whole cloud in original order.  Each wave owns
// 64-point words; mask word = ballot & enabled word; all-disabled words are skipped
// without touching the point planes.  Per-1024-word popcount sums feed the compaction.
// 64-point words per wave per iteration (12 loads in flight per lane).  Measured on the plane scan, 10M / 50M points
// (real clouds, bench.py): 4 words 0.0804 / 0.369 ms, 2 words 0.0764 / 0.355, 1 word 0.0792 / 0.345 -- fewer words per
// wave mean more waves in flight, and with one word the compiler sinks the second half of the loads below the
// wave-level early-out of the exact test (a word whose 64 points all fail the first half never fetches the other
// three planes: 0.048 ms on a cloud of random normals).
// The float scan of a Float32 cloud (24 B per point) keeps 4 words per wave: 24 loads in flight per lane.
template <typename T> constexpr int RH_RF_WPW = 2;
template <> constexpr int RH_RF_WPW<float> = 4;

template <int KIND, typename T, typename REC, int WPW>
__global__ void __launch_bounds__(256)
refit_mask_kernel(const T *__restrict__ pts, int64_t stride, int64_t n, int64_t nwords,
                  const uint64_t *__restrict__ enabled, const REC P, double eps, double cosa,
                  uint64_t *__restrict__ mask_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const T *__restrict__ X = pts, *__restrict__ Y = pts + stride, *__restrict__ Z = pts + 2 * stride;
    const T *__restrict__ NX = pts + 3 * stride, *__restrict__ NY = pts + 4 * stride, *__restrict__ NZ = pts + 5 * stride;
    const int64_t ngroups = (nwords + WPW - 1) / WPW;
    for (int64_t g = wave0; g < ngroups; g += nwaves) {
        const int64_t w0 = g * WPW;
        uint64_t en[WPW];
        T px[WPW], py[WPW], pz[WPW], qx[WPW], qy[WPW], qz[WPW];
#pragma unroll
        for (int k = 0; k < WPW; k++) {
            const int64_t w = w0 + k;
            en[k] = w < nwords ? (enabled[w] & valid_mask(w << 6, n)) : 0ULL;
        }
#pragma unroll
        for (int k = 0; k < WPW; k++) {
            // an all-disabled word re-reads the (L2-hot) first line of the planes instead of streaming its 3 KB
            const int64_t i = (en[k] != 0 ? ((w0 + k) << 6) : (int64_t)0) + lane;
            px[k] = X[i]; py[k] = Y[i]; pz[k] = Z[i];
            qx[k] = NX[i]; qy[k] = NY[i]; qz[k] = NZ[i];
        }
#pragma unroll
        for (int k = 0; k < WPW; k++) {
            const uint64_t b = test_point<KIND>(P, px[k], py[k], pz[k], qx[k], qy[k], qz[k], eps, cosa) & en[k];
            if (lane == 0 && w0 + k < nwords) mask_out[w0 + k] = b;
        }
    }
}

// ---- liveness of a SMALL candidate store after an extraction: removeinvalidshapes! (fitting.jl:209-221)
// recomputed as "does the candidate contain one of the points that were just disabled".  All kinds in one
// launch; the end of the disabled list is read from device memory (the host has not seen it yet), the grid
// is sized for the longest list possible and the blocks beyond the end leave at once.  A wave keeps
// RH_SC_WAVE_PTS points in registers and walks every stored candidate; flags[base[kind] + slot] = 1 marks
// a dead one (the flags are all zero on entry, pack_live_kernel re-zeroes them).  grid.y splits the candidates
// of every kind into rows of RH_LIVE_CH: the walk is a chain of dependent scalar loads, so it is kept short.
constexpr int RH_LIVE_CH = 4;   // candidates of each kind per block row

template <int KIND>
__device__ __forceinline__ void live_kind(const rh_live_args &A, const double (&px)[RH_SC_PPT], const double (&py)[RH_SC_PPT],
                                          const double (&pz)[RH_SC_PPT], const double (&qx)[RH_SC_PPT],
                                          const double (&qy)[RH_SC_PPT], const double (&qz)[RH_SC_PPT], int64_t wbase,
                                          int64_t nd, int lane, int32_t *__restrict__ flags)
{
    const int nk = A.nk[KIND];
    if (nk == 0) return;
    uint64_t vm[RH_SC_PPT];
    bool any = false;
#pragma unroll
    for (int p = 0; p < RH_SC_PPT; p++) {
        const int64_t gb = wbase + p * 64;   // bits of the points in [first, nd)
        const int64_t skip = (int64_t)A.first[KIND] - gb;
        vm[p] = valid_mask(gb, nd) & (skip <= 0 ? ~0ULL : (skip >= 64 ? 0ULL : ~((1ULL << skip) - 1ULL)));
        any = any || vm[p] != 0;
    }
    if (!any) return;
    const rh_prep *__restrict__ prep = A.prep[KIND];
    const double eps = A.eps[KIND], cosa = A.cosa[KIND];
    const int c_lo = blockIdx.y * RH_LIVE_CH, c_hi = min(nk, c_lo + RH_LIVE_CH);   // this block row's candidates
    for (int c = c_lo; c < c_hi; c++) {
        const rh_prep P = prep[c];
        uint64_t hit = 0;
        if (A.f32) {   // Float32 cloud: the binary32 test on the float record the stored one implies
            const rh_prepf Pf = prepf_of<KIND>(P);
#pragma unroll
            for (int p = 0; p < RH_SC_PPT; p++)
                hit |= test_point<KIND>(Pf, (float)px[p], (float)py[p], (float)pz[p], (float)qx[p], (float)qy[p], (float)qz[p], eps, cosa) & vm[p];
        } else {
#pragma unroll
            for (int p = 0; p < RH_SC_PPT; p++)
                hit |= test_point<KIND>(P, px[p], py[p], pz[p], qx[p], qy[p], qz[p], eps, cosa) & vm[p];
        }
        if (hit != 0 && lane == 0) flags[A.base[KIND] + c] = 1;
    }
}

__global__ void __launch_bounds__(RH_SC_THREADS)
liveness_small_kernel(const double *__restrict__ dis, int64_t stride, const int32_t *__restrict__ ndis_ptr, int64_t lo,
                      const rh_live_args A, int32_t *__restrict__ flags)
{
    const int64_t nd = *ndis_ptr;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wbase = lo + (int64_t)blockIdx.x * RH_SC_TILE + (int64_t)wave * RH_SC_WAVE_PTS;
    if (wbase >= nd) return;
    double px[RH_SC_PPT], py[RH_SC_PPT], pz[RH_SC_PPT], qx[RH_SC_PPT], qy[RH_SC_PPT], qz[RH_SC_PPT];
#pragma unroll
    for (int p = 0; p < RH_SC_PPT; p++) {   // (the list has a tile of slack behind its capacity)
        const int64_t i = wbase + p * 64 + lane;
        px[p] = dis[i]; py[p] = dis[stride + i]; pz[p] = dis[2 * stride + i];
        qx[p] = dis[3 * stride + i]; qy[p] = dis[4 * stride + i]; qz[p] = dis[5 * stride + i];
    }
    live_kind<RH_PLANE>(A, px, py, pz, qx, qy, qz, wbase, nd, lane, flags);
    live_kind<RH_SPHERE>(A, px, py, pz, qx, qy, qz, wbase, nd, lane, flags);
    live_kind<RH_CYLINDER>(A, px, py, pz, qx, qy, qz, wbase, nd, lane, flags);
    live_kind<RH_CONE>(A, px, py, pz, qx, qy, qz, wbase, nd, lane, flags);
}

// the extraction's read-back in one small kernel: liveness flags (re-zeroed behind the copy) and the two list
// lengths, straight into pinned host memory
__global__ void __launch_bounds__(256)
pack_live_kernel(int32_t *__restrict__ flags, int32_t n_flags, int32_t *__restrict__ h_flags,
                 const int32_t *__restrict__ d_total, const int32_t *__restrict__ d_ndis, int32_t *__restrict__ h_scalars)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_flags) {
        h_flags[i] = flags[i];
        flags[i] = 0;
    }
    if (i == 0) {
        h_scalars[0] = *d_total;
        h_scalars[1] = *d_ndis;
    }
}

// AoS (Vector{SVector{3,Float64}}) -> SoA planes, optionally gathering through an index list
__global__ void transpose_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm,
                                 const int32_t *__restrict__ gather, int64_t count, double *__restrict__ dst,
                                 int64_t stride)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int64_t i = gather ? gather[j] : j;
    dst[j] = xyz[3 * i];
    dst[stride + j] = xyz[3 * i + 1];
    dst[2 * stride + j] = xyz[3 * i + 2];
    dst[3 * stride + j] = nrm[3 * i];
    dst[4 * stride + j] = nrm[3 * i + 1];
    dst[5 * stride + j] = nrm[3 * i + 2];
}

// 64-byte point records for the sampler's random gathers (one HBM line per point instead of six)
__global__ void pack_records_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm, int64_t n,
                                    rh_f64x2 *__restrict__ rec)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    rh_f64x2 a, b, c, d;
    a.x = xyz[3 * j]; a.y = xyz[3 * j + 1];
    b.x = xyz[3 * j + 2]; b.y = nrm[3 * j];
    c.x = nrm[3 * j + 1]; c.y = nrm[3 * j + 2];
    d.x = 0.0; d.y = 0.0;
    rec[4 * j] = a; rec[4 * j + 1] = b; rec[4 * j + 2] = c; rec[4 * j + 3] = d;
}

__global__ void iota_kernel(int32_t *d, int32_t n, int32_t base)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = base + i;
}

__global__ void gather_prep_kernel(const rh_prep *__restrict__ src, const int32_t *__restrict__ idx, int32_t n,
                                   rh_prep *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// the one spelling of "which kind": f is a generic lambda that gets the kind as an integral constant
template <typename F>
int with_kind(int kind, F &&f)
{
    switch (kind) {
    case RH_PLANE: return f(std::integral_constant<int, RH_PLANE>());
    case RH_SPHERE: return f(std::integral_constant<int, RH_SPHERE>());
    case RH_CYLINDER: return f(std::integral_constant<int, RH_CYLINDER>());
    case RH_CONE: return f(std::integral_constant<int, RH_CONE>());
    }
    rh_set_error("unknown shape kind %d", kind);
    return RH_E_INVALID;
}

template <int KIND, typename T>
int launch_score(rh_cloud *c, const T *pts, int64_t stride, int64_t s, const uint64_t *en,
                 const rh_prep *prep, const int32_t *orig, const int32_t *nk, int32_t nk_bound, double eps,
                 double cosa, int32_t *counts, uint64_t *masks, int64_t mask_stride)
{
    const int ctiles = cdiv(nk_bound, RH_SC_CT);
    const int64_t ntiles = (s + RH_SC_TILE - 1) / RH_SC_TILE;
    if (ctiles == 0 || ntiles == 0) return RH_OK;
    if (ctiles > 65535) {   // grid.y limit: 4M candidates of one kind per launch
        rh_set_error("batch of %d candidates is too large for one launch (max %d per kind)", nk_bound, 65535 * RH_SC_CT);
        return RH_E_INVALID;
    }
    // Blocks that
    // share a candidate tile differ in blockIdx.x, so consecutive ids (dealt round-robin over the
    // XCDs) stream different point tiles against the same SGPR-resident candidates.
    int64_t splits = 65536 / ctiles;   // one tile per block unless the grid gets huge: best balance (measured)
    if (splits < 1) splits = 1;
    if (splits > ntiles) splits = ntiles;
    dim3 grid((unsigned)splits, (unsigned)ctiles);
    constexpr bool FLT = sizeof(T) == sizeof(float);
    if (FLT || c->f32) {
        if (masks)
            hipLaunchKernelGGL((score_kernel<KIND, true, true, T>), grid, dim3(RH_SC_THREADS), 0, c->stream, pts, stride, s, en,
                               prep, orig, nk, eps, cosa, counts, masks, mask_stride);
        else
            hipLaunchKernelGGL((score_kernel<KIND, false, true, T>), grid, dim3(RH_SC_THREADS), 0, c->stream, pts, stride, s, en,
                               prep, orig, nk, eps, cosa, counts, masks, mask_stride);
    } else if (masks)
        hipLaunchKernelGGL((score_kernel<KIND, true, FLT, T>), grid, dim3(RH_SC_THREADS), 0, c->stream, pts, stride, s, en,
                           prep, orig, nk, eps, cosa, counts, masks, mask_stride);
    else
        hipLaunchKernelGGL((score_kernel<KIND, false, FLT, T>), grid, dim3(RH_SC_THREADS), 0, c->stream, pts, stride, s, en,
                           prep, orig, nk, eps, cosa, counts, masks, mask_stride);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

template <typename T, typename... A>
int score_kind(rh_cloud *c, int kind, const T *pts, A... a)
{
    return with_kind(kind, [&](auto K) { return launch_score<K.value>(c, pts, a...); });
}

}  // namespace

int rhk_transpose_aos(rh_cloud *c, const double *d_xyz, const double *d_nrm, int64_t n, const int32_t *d_gather,
                      int64_t count, double *dst, int64_t dst_stride)
{
    (void)n;
    if (count == 0) return RH_OK;
    hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(count, 256)), dim3(256), 0, c->stream, d_xyz, d_nrm, d_gather,
                       count, dst, dst_stride);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// two int32 from device memory into (pinned) host memory, in stream order, without a copy-engine transfer
__global__ void fetch_i32_kernel(const int32_t *__restrict__ src0, const int32_t *__restrict__ src1,
                                 int32_t *__restrict__ h_dst)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        h_dst[0] = *src0;
        h_dst[1] = *src1;
    }
}

int rhk_fetch2_i32(rh_cloud *c, const int32_t *d_src0, const int32_t *d_src1, int32_t *h_pinned_dst)
{
    hipLaunchKernelGGL(fetch_i32_kernel, dim3(1), dim3(64), 0, c->stream, d_src0, d_src1, h_pinned_dst);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// `span`: an upper bound of the list entries behind `lo` (the true end is read on the device)
int rhk_liveness_small(rh_cloud *c, int64_t lo, int64_t span, const rh_live_args &A, int32_t *d_flags)
{
    if (span <= 0) return RH_OK;
    int nk_max = 0;
    for (int q = 0; q < 4; q++) nk_max = std::max(nk_max, (int)A.nk[q]);
    if (nk_max == 0) return RH_OK;
    hipLaunchKernelGGL(liveness_small_kernel, dim3(cdiv(span, RH_SC_TILE), cdiv(nk_max, RH_LIVE_CH)), dim3(RH_SC_THREADS), 0,
                       c->stream, c->dis, c->dis_stride, c->d_ndis, lo, A, d_flags);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_pack_live(rh_cloud *c, int32_t *d_flags, int32_t n_flags, int32_t *h_flags, int32_t *h_scalars)
{
    hipLaunchKernelGGL(pack_live_kernel, dim3(std::max(1, cdiv(n_flags, 256))), dim3(256), 0, c->stream, d_flags, n_flags,
                       h_flags, rhk_fold_total(c), c->d_ndis, h_scalars);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_pack_records(rh_cloud *c, const double *d_xyz, const double *d_nrm, int64_t n, double *d_rec)
{
    if (n == 0) return RH_OK;
    hipLaunchKernelGGL(pack_records_kernel, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, d_xyz, d_nrm, n, (rh_f64x2 *)d_rec);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// The culled score path (score4.hip) is there for this cloud: a subset of RH_G2_MIN_POINTS points or more, in k-d leaf order
// with group boxes.  Smaller subsets are scored by the brute-force kernel (score_kernel).
bool rh_score_v4_enabled(const rh_cloud *c)
{
    return c->f32 ? c->f32_groups : c->use_groups;
}

// eps + cosa given: the prep kernel also leaves the classifier and culling records of the workspace's bins in
// w.d_qpre / w.d_box; w.qpre_v4 says so to the score dispatch
static PreArgs pre_args(rh_cloud *c, rh_batch_ws &w, const double *eps, const double *cosa)
{
    PreArgs QA;
    for (int k = 0; k < 4; k++) { QA.eps[k] = eps ? eps[k] : 0.0; QA.cosa[k] = cosa ? cosa[k] : 0.0; }
    QA.coord_mag = c->coord_mag;
    QA.nrm_mag = c->nrm_mag;
    QA.nrm_len = c->nrm_len;
    QA.f32 = c->f32 ? 1 : 0;
    QA.box = w.d_box;
    QA.bstride = 4 * w.batch_cap;
    w.qpre_v4 = eps != nullptr && cosa != nullptr && rh_score_v4_enabled(c) && w.d_box != nullptr && w.d_qpre != nullptr;
    return QA;
}

int rhk_prep_sorted(rh_cloud *c, rh_batch_ws &w, int32_t b, int32_t *d_counts_to_zero, const double *eps, const double *cosa)
{
    const bool both = eps != nullptr && cosa != nullptr;
    const PreArgs QA = pre_args(c, w, both ? eps : nullptr, both ? cosa : nullptr);
    if (b == 0) return RH_OK;
    hipLaunchKernelGGL(prep_sorted_kernel, dim3(cdiv(b, 256)), dim3(256), 0, c->stream, (const rh_shape *)w.d_shapes, b, w.d_prep,
                       d_counts_to_zero, w.qpre_v4 ? (rh4::rh_cls *)w.d_qpre.get() : (rh4::rh_cls *)nullptr, QA);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// the records alone of shapes that are binned nowhere (rh_cloud_assign: assign.hip): no workspace, no classifier records
int rhk_prep_records(rh_cloud *c, const rh_shape *d_shapes, int32_t b, rh_prep *d_prep)
{
    rh_batch_ws none;
    const PreArgs QA = pre_args(c, none, nullptr, nullptr);
    if (b == 0) return RH_OK;
    hipLaunchKernelGGL(prep_sorted_kernel, dim3(cdiv(b, 256)), dim3(256), 0, c->stream, d_shapes, b, d_prep, (int32_t *)nullptr,
                       (rh4::rh_cls *)nullptr, QA);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// prep + bin the first min(*d_count, cap_entries) entries into w.d_prep / w.d_orig / c->d_nk (w.batch_cap >= cap_entries)
int rhk_prep_entries(rh_cloud *c, rh_batch_ws &w, const rh_cand_entry *d_entries, const int32_t *d_count, int32_t cap_entries,
                     int32_t launch_bound, int32_t *d_counts, int nk_is_zero, const double *eps, const double *cosa,
                     const rh_oct_state *ost)
{
    if (!nk_is_zero) RH_HIP(hipMemsetAsync(c->d_nk, 0, 4 * sizeof(int32_t), c->stream));
    const PreArgs QA = pre_args(c, w, eps, cosa);
    if (launch_bound <= 0) return RH_OK;
    hipLaunchKernelGGL(prep_entries_kernel, dim3(cdiv(launch_bound, 256)), dim3(256), 0, c->stream, d_entries, d_count,
                       cap_entries, w.d_prep, w.d_orig, c->d_nk, w.batch_cap, d_counts,
                       w.qpre_v4 ? (rh4::rh_cls *)w.d_qpre.get() : (rh4::rh_cls *)nullptr, QA, ost);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// a multiplier near 0.618 b that is coprime to b: t -> (t * m) mod b is a permutation that sends neighbours far apart
int32_t rh_spread_multiplier(int32_t b)
{
    if (b < 4) return 1;
    auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t r = x % y; x = y; y = r; } return x; };
    int64_t m = (int64_t)(0.6180339887498949 * b) | 1;
    while (gcd(m, b) != 1) m += 2;
    return (int32_t)(m % b);
}

int rhk_prep_binned(rh_cloud *c, rh_batch_ws &w, const rh_shape *d_shapes, int32_t b, int32_t *d_nk, int32_t *d_counts_to_zero,
                    int32_t *d_nk_other, int nk_is_zero, const double *eps, const double *cosa, int32_t *zero_extra, int32_t zero_extra_n)
{
    if (!nk_is_zero) RH_HIP(hipMemsetAsync(d_nk, 0, 4 * sizeof(int32_t), c->stream));
    PreArgs QA = pre_args(c, w, eps, cosa);
    if (b == 0) return RH_OK;
    const int no_spread = rh_opt_on(c, RH_OPT_NO_SPREAD) ? 1 : 0;
#ifndef RH_PREP_BLOCK
#define RH_PREP_BLOCK 64   // (one wave per block: the launch is a latency chain -- shape, bin reservation, divisions, records -- and 64 blocks spread it over 64 CUs: cfg3 step 0.0860 -> 0.0846 ms, cfg2 0.0431 -> 0.0421; 128: the same; 256: round 4)
#endif
    hipLaunchKernelGGL(prep_binned_kernel, dim3(cdiv(b, RH_PREP_BLOCK)), dim3(RH_PREP_BLOCK), 0, c->stream, d_shapes, b, w.d_prep, w.d_orig,
                       d_nk, w.batch_cap, d_counts_to_zero, d_nk_other, no_spread ? 1 : rh_spread_multiplier(b),
                       w.qpre_v4 ? (rh4::rh_cls *)w.d_qpre.get() : (rh4::rh_cls *)nullptr, QA, zero_extra, zero_extra_n);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_score_kind(rh_cloud *c, int kind, const double *pts, int64_t stride, int64_t s, const uint64_t *en,
                   const rh_prep *d_prep, const int32_t *d_orig, const int32_t *d_nk, int32_t nk_bound, double eps,
                   double cosa, int32_t *d_counts, uint64_t *d_masks, int64_t mask_stride)
{
    return score_kind(c, kind, pts, stride, s, en, d_prep, d_orig, d_nk, nk_bound, eps, cosa, d_counts, d_masks, mask_stride);
}

int rhk_score_kind(rh_cloud *c, int kind, const float *pts, int64_t stride, int64_t s, const uint64_t *en,
                   const rh_prep *d_prep, const int32_t *d_orig, const int32_t *d_nk, int32_t nk_bound, double eps,
                   double cosa, int32_t *d_counts, uint64_t *d_masks, int64_t mask_stride)
{
    return score_kind(c, kind, pts, stride, s, en, d_prep, d_orig, d_nk, nk_bound, eps, cosa, d_counts, d_masks, mask_stride);
}

// the streaming scan over the planes of the cloud's element type, with the candidate's record in that type
template <typename T, typename REC>
static int launch_refit(rh_cloud *c, const T *pts, const REC &P, int kind, double eps, double cosa)
{
    constexpr int WPW = RH_RF_WPW<T>;
    const int env_blocks = (int)rh_opt_int(c, RH_OPT_REFIT_BLOCKS, 0);
    int64_t blocks = cdiv(c->nwords, 4 * WPW);
    // one group of words per wave up to 32768 blocks, a grid-stride loop beyond (measured with 4-word groups, plane
    // scan: 10M points 0.0771 ms at 2048 blocks, 0.0743 at 4096-9766; 50M points 0.364 ms at 2048, 0.350 at 32768+)
    const int64_t cap = env_blocks > 0 ? env_blocks : 32768;
    if (blocks > cap) blocks = cap;
    RH_TRY(with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((refit_mask_kernel<K.value, T, REC, WPW>), dim3((unsigned)blocks), dim3(256), 0, c->stream, pts, c->n_pad, c->n,
                           c->nwords, c->enabled, P, eps, cosa, c->refit_mask);
        return RH_OK;
    }));
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_refit_mask(rh_cloud *c, const rh_prep &P, int kind, double eps, double cosa, bool apply)
{
    const bool culled = c->nwords > 0 && rhk_refit_is_culled(c);
    int rc = RH_OK;
    if (culled) rc = rhk_refitk_mask(c, P, kind, eps, cosa, apply);
    else if (c->nwords > 0)
        rc = c->f32 ? launch_refit(c, c->full32.get(), prepf_of_kind(P, kind), kind, eps, cosa) : launch_refit(c, c->full.get(), P, kind, eps, cosa);
    c->en.scan_started(culled && rc == RH_OK, apply);
    return rc;
}

int rhk_iota(rh_cloud *c, int32_t *d, int32_t n, int32_t base)
{
    if (n == 0) return RH_OK;
    hipLaunchKernelGGL(iota_kernel, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, d, n, base);
    RH_HIP(hipGetLastError());
    return RH_OK;
}


// ---- device-managed candidate store: compaction after an extraction (rh_internal.h, rh_store_plan) ----------------------
namespace {
__device__ __forceinline__ bool store_alive(const rh_store_plan &P, int64_t g, int &q_out, int32_t &slot_out, bool &valid)
{
    int q = 0;
#pragma unroll
    for (int k = 1; k < 4; k++) q += g >= P.pbase[k] ? 1 : 0;
    const int32_t slot = (int32_t)(g - P.pbase[q]);
    q_out = q; slot_out = slot;
    valid = slot < P.n[q];
    return valid && P.counts[g] == 0 && P.id[q][slot] != P.extracted_id;
}

__global__ void __launch_bounds__(RH_STORE_PAD)
store_count_kernel(const rh_store_plan P, int32_t *__restrict__ blk_cnt)
{
    __shared__ int32_t wc[RH_STORE_PAD / 64];
    const int64_t g = (int64_t)blockIdx.x * RH_STORE_PAD + threadIdx.x;
    int q; int32_t slot; bool valid;
    const bool alive = store_alive(P, g, q, slot, valid);
    const uint64_t bm = __builtin_amdgcn_ballot_w64(alive);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(bm);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0;
        for (int w = 0; w < RH_STORE_PAD / 64; w++) a += wc[w];
        blk_cnt[blockIdx.x] = a;
    }
}

// one block: exclusive scan of the block counts; the kinds' offsets and new lengths; the dead-list counter back to zero
__global__ void __launch_bounds__(1024)
store_scan_kernel(const rh_store_plan P, const int32_t *__restrict__ blk_cnt, int32_t nblocks, int32_t *__restrict__ blk_off,
                  int32_t *__restrict__ kind_off, int32_t *__restrict__ dead_counter, int32_t *__restrict__ h_out)
{
    __shared__ int32_t part[1024];
    const int tid = threadIdx.x;
    const int32_t per = (nblocks + 1023) / 1024;
    const int32_t b0 = min(nblocks, tid * per), b1 = min(nblocks, b0 + per);
    int32_t a = 0;
    for (int32_t b = b0; b < b1; b++) a += blk_cnt[b];
    // exclusive scan of the 1024 partial sums: shuffles inside the waves, then over the 16 wave totals
    const int lane = tid & 63, wv = tid >> 6;
    int32_t incl = a;
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int w = 0; w < 16; w++) { const int32_t v = part[w]; part[w] = run; run += v; }
    }
    __syncthreads();
    int32_t run = part[wv] + incl - a;
    for (int32_t b = b0; b < b1; b++) { blk_off[b] = run; run += blk_cnt[b]; }
    if (tid == 1023) blk_off[nblocks] = run;   // (the last thread's range ends the array: the total)
    __syncthreads();
    if (tid == 0) {
        int32_t total_old = 0, total_new = 0;
        for (int q = 0; q < 4; q++) {
            const int32_t lo = blk_off[P.pbase[q] / RH_STORE_PAD], hi = blk_off[P.pbase[q + 1] / RH_STORE_PAD];
            kind_off[q] = lo;
            h_out[q] = hi - lo;
            total_old += P.n[q];
            total_new += hi - lo;
        }
        h_out[4] = total_old - total_new;
        *dead_counter = total_old - total_new;   // (the length of the dead list: store_move_kernel places its entries by rank, no atomics)
    }
}

__global__ void __launch_bounds__(RH_STORE_PAD)
store_move_kernel(const rh_store_plan P, const int32_t *__restrict__ blk_off, const int32_t *__restrict__ kind_off,
                  int32_t *__restrict__ dead_counter, int32_t *__restrict__ h_dead, rh_store_best *__restrict__ h_best)
{
    __shared__ int32_t wc[RH_STORE_PAD / 64];
    __shared__ double wE[RH_STORE_PAD / 64];
    __shared__ long long wI[RH_STORE_PAD / 64];
    const int64_t g = (int64_t)blockIdx.x * RH_STORE_PAD + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int q; int32_t slot; bool valid;
    const bool alive = store_alive(P, g, q, slot, valid);
    const uint64_t bm = __builtin_amdgcn_ballot_w64(alive);
    if (lane == 0) wc[wv] = __popcll(bm);
    __syncthreads();
    // alive entries before this one, over the whole index space
    int32_t apos = blk_off[blockIdx.x] + __popcll(bm & ((1ULL << lane) - 1ULL));
    for (int w = 0; w < wv; w++) apos += wc[w];
    if (alive) {
        const int32_t pos = apos - kind_off[q];
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 *src = (const u32x4 *)(P.prep[q] + slot);
        u32x4 *dst = (u32x4 *)(P.spare[q] + pos);
        u32x4 v[sizeof(rh_prep) / 16];
#pragma unroll
        for (int i = 0; i < (int)(sizeof(rh_prep) / 16); i++) v[i] = src[i];
#pragma unroll
        for (int i = 0; i < (int)(sizeof(rh_prep) / 16); i++) dst[i] = v[i];
        P.spare_id[q][pos] = P.id[q][slot];
        P.spare_E[q][pos] = P.E[q][slot];
    } else if (valid) {
        // dead: its place in the dead list = valid entries before it - alive entries before it (returning atomics on one
        // counter, one per wave, serialised in L2: 30 of the kernel's 40 us on a 100 000-entry store)
        int32_t vbefore = slot;
        for (int k = 0; k < q; k++) vbefore += P.n[k];
        h_dead[vbefore - apos] = P.id[q][slot];
    }
    // the block's best survivor: greatest score, smallest id among equals
    double bE = 0.0;
    long long bI = -1;
    if (alive) { bE = P.E[q][slot]; bI = P.id[q][slot]; }
    auto better = [](double e1, long long i1, double e2, long long i2) { return i1 >= 0 && (i2 < 0 || e1 > e2 || (e1 == e2 && i1 < i2)); };
    for (int off = 32; off > 0; off >>= 1) {
        const double oE = __shfl_xor(bE, off);
        const long long oI = __shfl_xor(bI, off);
        if (better(oE, oI, bE, bI)) { bE = oE; bI = oI; }
    }
    if (lane == 0) { wE[wv] = bE; wI[wv] = bI; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RH_STORE_PAD / 64; w++)
            if (better(wE[w], wI[w], bE, bI)) { bE = wE[w]; bI = wI[w]; }
        h_best[blockIdx.x].E = bE;
        h_best[blockIdx.x].id = bI;
    }
}
}  // namespace

namespace {
// the dead list and the blocks' best entries -> pinned host memory, as coalesced stores (scattered 4-byte stores from
// store_move_kernel's waves crossed PCIe one by one: 40 us per compaction of a 100 000-entry store)
__global__ void __launch_bounds__(1024)
store_flush_kernel(const int32_t *__restrict__ d_dead, const int32_t *__restrict__ dead_counter, int32_t cap, const rh_store_best *__restrict__ d_best,
                   int32_t nblocks, int32_t *__restrict__ h_dead, rh_store_best *__restrict__ h_best)
{
    const int32_t n = min(*dead_counter, cap);
    for (int32_t i = threadIdx.x; i < n; i += 1024) h_dead[i] = d_dead[i];
    for (int32_t i = threadIdx.x; i < nblocks; i += 1024) h_best[i] = d_best[i];
}
}  // namespace

int rhk_store_compact(rh_cloud *c, const rh_store_plan &P, int32_t *d_work, int32_t *h_out, int32_t *h_dead, rh_store_best *h_best,
                      int32_t *d_dead, rh_store_best *d_best)
{
    const int32_t nblocks = P.pbase[4] / RH_STORE_PAD;
    if (nblocks <= 0) { for (int i = 0; i < 5; i++) h_out[i] = 0; return RH_OK; }
    int32_t *blk_cnt = d_work, *blk_off = d_work + nblocks, *kind_off = d_work + 2 * nblocks + 1, *counter = d_work + 2 * nblocks + 8;
    hipLaunchKernelGGL(store_count_kernel, dim3((unsigned)nblocks), dim3(RH_STORE_PAD), 0, c->stream, P, blk_cnt);
    hipLaunchKernelGGL(store_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P, blk_cnt, nblocks, blk_off, kind_off, counter, h_out);
    hipLaunchKernelGGL(store_move_kernel, dim3((unsigned)nblocks), dim3(RH_STORE_PAD), 0, c->stream, P, blk_off, kind_off, counter, d_dead, d_best);
    int32_t total = 0;
    for (int q = 0; q < 4; q++) total += P.n[q];
    hipLaunchKernelGGL(store_flush_kernel, dim3(1), dim3(1024), 0, c->stream, d_dead, counter, total, d_best, nblocks, h_dead, h_best);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_gather_prep(rh_cloud *c, const rh_prep *src, const int32_t *d_idx, int32_t n, rh_prep *dst)
{
    if (n == 0) return RH_OK;
    hipLaunchKernelGGL(gather_prep_kernel, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, src, d_idx, n, dst);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// liveness pass of a cloud without the culled path: candidates against dis[first, first + cnt) (counts only), brute force
int rhk_score_kind_dis(rh_cloud *c, int kind, int64_t first, int64_t cnt, const rh_prep *d_prep, const int32_t *d_orig,
                       const int32_t *d_nk, int32_t nk_bound, double eps, double cosa, int32_t *d_counts)
{
    if (cnt <= 0 || nk_bound <= 0) return RH_OK;
    return rhk_score_kind(c, kind, c->dis + first, c->dis_stride, cnt, nullptr, d_prep, d_orig, d_nk, nk_bound, eps,
                          cosa, d_counts, nullptr, 0);
}

int rhk_group_bounds_of(rh_cloud *c, const double *pts, int64_t stride, int64_t count, int64_t ngroups, double *gb, int64_t gstride)
{
    if (ngroups == 0) return RH_OK;
    hipLaunchKernelGGL(group_bounds_kernel, dim3(cdiv(ngroups, 4)), dim3(256), 0, c->stream, pts, stride, count, ngroups, gb, gstride);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_group_bounds(rh_cloud *c)
{
    if (c->ngroups == 0) return RH_OK;
    hipLaunchKernelGGL(group_bounds_kernel, dim3(cdiv(c->ngroups, 4)), dim3(256), 0, c->stream, c->sub, c->s_pad, c->s,
                       c->ngroups, c->gb, c->ng_pad);
    RH_HIP(hipGetLastError());
    return rhk_gb32_build(c);   // the binary32 twins (v4 score kernel)
}

int rhk_unpermute_masks(rh_cloud *c, const uint64_t *d_in, int32_t b, uint64_t *d_out)
{
    if (b == 0 || c->swords == 0) return RH_OK;
    if (c->swords > RH_UNPERM_SEG_WORDS) {
        const int64_t total = (int64_t)b * c->swords;
        RH_HIP(hipMemsetAsync(d_out, 0, sizeof(uint64_t) * (size_t)total, c->stream));
        hipLaunchKernelGGL(unpermute_masks_atomic_kernel, dim3(cdiv(total, 256)), dim3(256), 0, c->stream, d_in, c->sub_perm,
                           c->swords, total, d_out);
        RH_HIP(hipGetLastError());
        return RH_OK;
    }
    const int nseg = cdiv(c->swords, RH_UNPERM_SEG_WORDS);
    const size_t lds = sizeof(uint64_t) * (size_t)std::min<int64_t>(c->swords, RH_UNPERM_SEG_WORDS);
    static bool attr_set = false;
    if (!attr_set) {   // more than the default 64 KB of dynamic LDS
        RH_HIP(hipFuncSetAttribute((const void *)unpermute_masks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(uint64_t) * RH_UNPERM_SEG_WORDS)));
        attr_set = true;
    }
    for (int32_t r0 = 0; r0 < b; r0 += 65535 * 32) {   // grid.x limit (2^31 - 1) is far away; keep launches bounded anyway
        const int32_t rows = std::min<int32_t>(b - r0, 65535 * 32);
        hipLaunchKernelGGL(unpermute_masks_kernel, dim3((unsigned)rows, (unsigned)nseg), dim3(1024), lds, c->stream,
                           d_in + (int64_t)r0 * c->swords, c->sub_perm, c->swords, d_out + (int64_t)r0 * c->swords);
    }
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// tab[k] = first Morton position whose code is >= k << shift (k = entries - 1: n): the cell directory of the octree
// sampler (fit_shared.h, OctView::cell_bounds)
__global__ void __launch_bounds__(256)
oct_tab_kernel(const uint64_t *__restrict__ code, int64_t n, int shift, int64_t entries, int32_t *__restrict__ tab)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= entries) return;
    int64_t lo = 0, hi = n;
    if (k == entries - 1) lo = n;
    else {
        const uint64_t key = (uint64_t)k << shift;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (code[mid] < key) lo = mid + 1; else hi = mid;
        }
    }
    tab[k] = (int32_t)lo;
}

__global__ void __launch_bounds__(256)
oct_code_o_kernel(const uint64_t *__restrict__ code, const int32_t *__restrict__ perm, int64_t n, uint64_t *__restrict__ code_o)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) code_o[perm[q]] = code[q];
}

int rhk_oct_build_tab(rh_cloud *c)
{
    c->oct_tab.reset();
    c->oct_code_o.reset();
    c->oct_tab_level = 0;
    if (c->n == 0) return RH_OK;
    RH_TRY(c->oct_code_o.alloc(c->n));
    hipLaunchKernelGGL(oct_code_o_kernel, dim3(cdiv(c->n, 256)), dim3(256), 0, c->stream, c->oct_code, c->oct_perm, c->n, c->oct_code_o);
    const int level = c->oct_depth < 8 ? c->oct_depth : 8;   // 8^7 + 1 entries at most (8 MB)
    const int64_t entries = ((int64_t)1 << (3 * (level - 1))) + 1;
    RH_TRY(c->oct_tab.alloc(entries));
    hipLaunchKernelGGL(oct_tab_kernel, dim3(cdiv(entries, 256)), dim3(256), 0, c->stream, c->oct_code, c->n, 3 * (21 - (level - 1)),
                       entries, c->oct_tab);
    RH_HIP(hipGetLastError());
    c->oct_tab_level = level;
    return RH_OK;
}
