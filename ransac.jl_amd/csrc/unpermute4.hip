// unpermute4.hip -- the inlier masks of a v4 score launch (score4.hip) in subset order: an independent pass behind the launch,
// from the entry lists the kernel left in the workspace.
#include <algorithm>

#include "rh_internal.h"
#include "score_device.h"
#include "score4_shared.h"
#include "wave_keys.h"

namespace {

using namespace rhdev;

// ---- masks -> subset order, from the entry lists the score kernel left (round 4; round 3 wrote the words into sparse
// internal-order rows with an occupancy byte each, and the un-permutation searched them: 1.0 ms at cfg5, a chain of
// dependent loads per block -- occupancy -> list -> words -> positions -- at two blocks per CU).  One block per (candidate
// row, output segment): the segment of the output row is assembled in LDS and written out once, coalesced.  The block
// streams the row's entries (coalesced 16-byte loads, several per thread in flight), keeps of each word the bits that
// land in ITS segment (segmask[segment][word], made once per cloud; without it -- more than 8 segments -- a range test
// after the look-up), and its waves look the surviving bits' positions up 64 at a time through a per-wave ring.
// a row of up to 8192 words (524 288 subset points) is ONE segment (64 KB of LDS); longer rows are cut into segments of 3072
// words (cfg5, 24 415 words per row, masks step: 8192 -> 0.883 ms, 6144 0.851, 4096 0.848, 3072 0.828, 2560 0.839, 2048 0.847,
// 1536 0.891: smaller segments mean more blocks per CU for a chain of dependent loads, and more passes over the entries)
#ifndef RH_UNP_BLOCK
#define RH_UNP_BLOCK 512      // threads per block of the multi-segment form
#endif
#ifndef RH_UNP_MULTI
#define RH_UNP_MULTI 3072     // words per output segment of rows that need several
#endif
constexpr int S4_UNP_WORDS = 8192, S4_UNP_WORDS_MULTI = RH_UNP_MULTI;
constexpr int S6_UNROLL = 4;

// WAVEWORD (rows of one segment): a wave per entry, a lane per bit -- the word's 64 positions are one coalesced load and
// every set bit lands in the block's segment; four entries in flight per wave (round 3's inner loop, fed from the list)
template <bool WAVEWORD, int BLK = 512>
__global__ void __launch_bounds__(BLK)
unpermute6_kernel(const rh_u64x2 *__restrict__ ent, const int32_t *__restrict__ cursor, int64_t mstride, const int32_t *__restrict__ perm,
                  int64_t swords, int64_t seg_words, const uint64_t *__restrict__ segmask, int64_t smstride, uint64_t *__restrict__ out)
{
    extern __shared__ unsigned long long seg[];
    __shared__ uint32_t ring[BLK / 64][128];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const int64_t w0 = (int64_t)blockIdx.y * seg_words;
    const int nw = (int)(swords - w0 < seg_words ? swords - w0 : seg_words);
    for (int t = threadIdx.x; t < nw; t += BLK) seg[t] = 0ULL;
    const int n = min(cursor[row], (int32_t)mstride);
    __syncthreads();
    const int32_t lo = (int32_t)(w0 << 6), span = nw << 6;
    const rh_u64x2 *__restrict__ src = ent + row * mstride;
    const uint64_t *__restrict__ sm = segmask != nullptr ? segmask + (int64_t)blockIdx.y * smstride : nullptr;
    if (WAVEWORD) {
        for (int i0 = wv * 4; i0 < n; i0 += (BLK / 64) * 4) {
            rh_u64x2 e[4];
            int32_t j[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                e[k] = src[min(i0 + k, n - 1)];
                j[k] = perm[((int64_t)e[k].x << 6) + lane] - lo;
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i0 + k < n && ((e[k].y >> lane) & 1ULL) && j[k] >= 0 && j[k] < span) atomicOr(&seg[j[k] >> 6], 1ULL << (j[k] & 63));
        }
        __syncthreads();
        uint64_t *__restrict__ dstw = out + row * swords + w0;
        for (int t = threadIdx.x; t < nw; t += BLK) dstw[t] = seg[t];
        return;
    }
    int head = 0, fill = 0;   // the wave's ring (wave-uniform)
    auto drain = [&](int k) {
        wave_lds_sync();
        if (lane < k) {
            const uint32_t e = ring[wv][(head + lane) & 127];
            const int32_t j = perm[e] - lo;
            if (j >= 0 && j < span) atomicOr(&seg[j >> 6], 1ULL << (j & 63));
        }
        head = (head + k) & 127;
        fill -= k;
    };
    for (int i0 = threadIdx.x; i0 - lane < n; i0 += BLK * S6_UNROLL) {   // (whole waves stay in the loop: ballots)
        rh_u64x2 e[S6_UNROLL];
#pragma unroll
        for (int k = 0; k < S6_UNROLL; k++) {
            const int i = i0 + k * BLK;
            e[k].x = 0; e[k].y = 0;
            if (i < n) e[k] = src[i];
        }
        uint64_t m[S6_UNROLL];
#pragma unroll
        for (int k = 0; k < S6_UNROLL; k++) m[k] = (sm != nullptr && e[k].y != 0) ? (e[k].y & sm[e[k].x]) : e[k].y;
#pragma unroll
        for (int k = 0; k < S6_UNROLL; k++) {
            const uint32_t gbase = (uint32_t)e[k].x << 6;
            uint64_t mm = m[k];
            for (;;) {
                const bool has = mm != 0;
                const uint64_t hm = WB(has);
                if (hm == 0) break;
                const int bit = has ? __builtin_ctzll(mm) : 0;
                mm &= mm - 1;
                const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0));
                if (has) ring[wv][(head + fill + rank) & 127] = gbase + (uint32_t)bit;
                fill += __popcll(hm);
                if (fill >= 64) drain(64);
            }
        }
    }
    if (fill > 0) drain(fill);
    __syncthreads();
    uint64_t *__restrict__ dst = out + row * swords + w0;
    for (int t = threadIdx.x; t < nw; t += BLK) dst[t] = seg[t];
}

__global__ void clear_cursors_kernel(int32_t *__restrict__ cursor, int32_t b)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b) cursor[i] = 0;
}

// segmask[seg * smstride + g]: bit b set <=> point b of internal word g has its subset position in output segment seg
__global__ void segmask_kernel(const int32_t *__restrict__ perm, int64_t s, int64_t ngroups, int64_t seg_bits, int nseg, int64_t smstride,
                               uint64_t *__restrict__ segmask)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    for (int sgi = 0; sgi < nseg; sgi++) {
        uint64_t m = 0;
        for (int b = 0; b < 64; b++) {
            const int64_t i = (g << 6) + b;
            if (i < s && (int64_t)perm[i] / seg_bits == sgi) m |= 1ULL << b;
        }
        segmask[(int64_t)sgi * smstride + g] = m;
    }
}

}  // namespace

// the entry lists the v4 score kernel left in the workspace (rows of mstride4 16-byte entries, one cursor per row in d_occ) ->
// dense rows in subset order; the cursors are zero again afterwards
int rhk_unpermute_masks4(rh_cloud *c, rh_batch_ws &w, int32_t b, uint64_t *d_out)
{
    if (b == 0 || c->swords == 0) return RH_OK;
    const uint64_t *d_in = w.d_masks_int;
    uint8_t *d_occ = w.d_occ;
    const int64_t mstride = w.mstride4;
    const int env_words = (int)rh_opt_int(c, RH_OPT_UNP_WORDS, 0);   // rh_set_option(.., "unp_words", n) (tests; read per call): segments of n words, so that a small cloud's rows span several / many
    const int64_t seg_words = std::min<int64_t>(c->swords, env_words > 0 ? std::min(env_words, 16384) : (c->swords <= S4_UNP_WORDS ? S4_UNP_WORDS : S4_UNP_WORDS_MULTI));
    const int nseg = cdiv4(c->swords, seg_words);
    static bool attr_set = false;
    if (!attr_set) {
        RH_HIP(hipFuncSetAttribute((const void *)unpermute6_kernel<false, RH_UNP_BLOCK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(uint64_t) * 16384)));
        RH_HIP(hipFuncSetAttribute((const void *)unpermute6_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(uint64_t) * 16384)));
        attr_set = true;
    }
    const uint64_t *sm = nullptr;
    if (nseg > 1 && nseg <= 16) {   // which bits of a word belong to which segment: made once per workspace and segment width, on its stream
        if (w.d_segmask == nullptr || w.segmask_words != seg_words) {
            w.segmask_words = 0;
            RH_TRY(w.d_segmask.grow(c->stream, (int64_t)nseg * c->ng_pad));
            w.segmask_words = seg_words;
            hipLaunchKernelGGL(segmask_kernel, dim3((unsigned)cdiv4(c->ngroups, 256)), dim3(256), 0, c->stream, c->sub_perm, c->s, c->ngroups,
                               seg_words * 64, nseg, c->ng_pad, w.d_segmask);
            RH_HIP(hipGetLastError());
        }
        sm = w.d_segmask;
    }
    const bool waveword = nseg == 1;
    if (waveword)
        hipLaunchKernelGGL(unpermute6_kernel<true>, dim3((unsigned)b, (unsigned)nseg), dim3(512), sizeof(uint64_t) * (size_t)seg_words, c->stream,
                           (const rh_u64x2 *)d_in, (const int32_t *)d_occ, mstride, c->sub_perm, c->swords, seg_words, sm, c->ng_pad, d_out);
    else
        hipLaunchKernelGGL((unpermute6_kernel<false, RH_UNP_BLOCK>), dim3((unsigned)b, (unsigned)nseg), dim3(RH_UNP_BLOCK), sizeof(uint64_t) * (size_t)seg_words, c->stream,
                           (const rh_u64x2 *)d_in, (const int32_t *)d_occ, mstride, c->sub_perm, c->swords, seg_words, sm, c->ng_pad, d_out);
    hipLaunchKernelGGL(clear_cursors_kernel, dim3((unsigned)cdiv4(b, 256)), dim3(256), 0, c->stream, (int32_t *)d_occ, b);
    RH_HIP(hipGetLastError());
    return RH_OK;
}
