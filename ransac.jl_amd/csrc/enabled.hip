// enabled.hip -- the enabled bits of a cloud (pc.isenabled), what is derived from them, and the mask scans they share with
// rhk_compact_generic: the one unit that writes rh_cloud::enabled and names block_sums / d_total (protocol: DESIGN.md §3)
#include "rh_internal.h"
#include "score_device.h"

namespace {

using namespace rhdev;

// popcount sums per RH_WORDS_PER_BLOCK words (used for the select directory)
__global__ void __launch_bounds__(256)
block_popc_kernel(const uint64_t *__restrict__ words, int64_t nwords, int32_t *__restrict__ block_sums)
{
    __shared__ int32_t red[4];
    const int64_t base = (int64_t)blockIdx.x * RH_WORDS_PER_BLOCK;
    int acc = 0;
    for (int k = threadIdx.x; k < RH_WORDS_PER_BLOCK; k += 256) {
        const int64_t w = base + k;
        if (w < nwords) acc += __popcll(words[w]);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// single-block exclusive scan of block_sums[0..nb) in place; block_sums[nb] and *total = grand total
__global__ void __launch_bounds__(1024)
scan_block_sums_kernel(int32_t *__restrict__ block_sums, int64_t nb, int32_t *__restrict__ total)
{
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int v = i < nb ? block_sums[i] : 0;
        int inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (lane >= off) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < wave; k++) woff += wsum[k];
        const int carry = carry_s;
        if (i < nb) block_sums[i] = carry + woff + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_sums[nb] = carry_s;
        *total = carry_s;
    }
}

// block b expands mask words [b*1024, (b+1)*1024): ascending 1-based indices.  Each thread owns
// 4 consecutive words: block-wide exclusive scan of their popcounts, then every thread writes the
// set bits of its own words (shape masks are sparse: a few bits per word).
// With `andnot_words` the block also clears the mask's bits there (invalidate_indexes! as enabled &= ~mask)
// and leaves the popcount of its updated words in andnot_sums[block]: the next select directory starts
// from those instead of a pass of its own.
__global__ void __launch_bounds__(256)
expand_mask_kernel(const uint64_t *__restrict__ mask, int64_t nwords, const int32_t *__restrict__ block_prefix,
                   int64_t *__restrict__ idx_out, int64_t cap, int32_t *__restrict__ word_prefix_out,
                   uint64_t *__restrict__ andnot_words, int32_t *__restrict__ andnot_sums,
                   int32_t *__restrict__ raw_total = nullptr)
{
    __shared__ int32_t wsum[4];
    __shared__ int32_t esum[4];
    __shared__ int32_t psum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * RH_WORDS_PER_BLOCK;
    // raw_total: block_prefix holds the blocks' popcounts, not their scan -- the block sums up its predecessors itself
    // (a few hundred values) and the last block leaves the grand total: one launch less than scanning them first
    int before = 0;
    if (raw_total != nullptr) {
        for (int k = threadIdx.x; k < (int)blockIdx.x; k += 256) before += block_prefix[k];
        for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off);
        if (lane == 0) psum[wave] = before;
    }
    uint64_t m[4];
    int pc[4], tsum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t w = base + threadIdx.x * 4 + k;
        m[k] = w < nwords ? mask[w] : 0ULL;
        pc[k] = __popcll(m[k]);
        tsum += pc[k];
    }
    if (andnot_words != nullptr) {
        int left = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t w = base + threadIdx.x * 4 + k;
            if (w < nwords) {
                const uint64_t e = andnot_words[w] & ~m[k];
                if (m[k] != 0) andnot_words[w] = e;
                left += __popcll(e);
            }
        }
        for (int off = 32; off > 0; off >>= 1) left += __shfl_down(left, off);
        if (lane == 0) esum[wave] = left;
    }
    int inc = tsum;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (andnot_words != nullptr && threadIdx.x == 0) andnot_sums[blockIdx.x] = esum[0] + esum[1] + esum[2] + esum[3];
    int woff = 0;
    for (int k = 0; k < wave; k++) woff += wsum[k];
    const int32_t bpre = raw_total != nullptr ? (psum[0] + psum[1] + psum[2] + psum[3]) : block_prefix[blockIdx.x];
    if (raw_total != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) *raw_total = bpre + woff + inc;
    int64_t run = (int64_t)bpre + woff + inc - tsum;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t w = base + threadIdx.x * 4 + k;
        if (word_prefix_out != nullptr && w < nwords) word_prefix_out[w] = (int32_t)run;
        if (idx_out != nullptr) {
            uint64_t bits = m[k];
            while (bits) {
                const int b = __builtin_ctzll(bits);
                bits &= bits - 1;
                if (run < cap) idx_out[run] = (w << 6) + b + 1;
                run++;
            }
        } else {
            run += pc[k];
        }
    }
}

// ------------------------------------------------- enabled maintenance ----
__global__ void invalidate_idx_kernel(const int64_t *__restrict__ idx, int64_t n, int64_t npoints,
                                      uint64_t *__restrict__ enabled, const int32_t *__restrict__ pos,
                                      uint64_t *__restrict__ men)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t i0 = idx[k] - 1;
    if (i0 < 0 || i0 >= npoints) return;
    atomicAnd((unsigned long long *)&enabled[i0 >> 6], ~(1ULL << (i0 & 63)));
    if (men != nullptr) {
        const int32_t mp = pos[i0];
        atomicAnd((unsigned long long *)&men[mp >> 6], ~(1ULL << (mp & 63)));
    }
}

// One launch per change of the enabled bits: sub_enabled bit j = enabled[sub_idx0[j]], and the subset points
// whose bit went 1 -> 0 (with `reset`: every disabled one) are appended to `dis`, the list the liveness
// pass scores.  A wave regathers RH_SUBUPD_WPW consecutive words; a block reserves the range of its points
// with ONE atomicAdd on the list length, so the ranges of different blocks follow each other in arbitrary
// order (the liveness counts are sums over the points: only the culling boxes see the order), while the
// points of a block stay in internal (k-d leaf) order, i.e. spatially compact.
constexpr int RH_SUBUPD_WPW = 8;

__global__ void __launch_bounds__(256)
update_sub_enabled_kernel(const uint64_t *__restrict__ enabled, const int32_t *__restrict__ sub_idx0, int64_t s,
                          int64_t swords, uint64_t *__restrict__ sub_enabled, int reset,
                          const double *__restrict__ sub, int64_t sub_stride, double *__restrict__ dis,
                          int64_t dis_stride, int32_t *__restrict__ ndis)
{
    __shared__ int32_t wtot[4];
    __shared__ int32_t base_s;
    __shared__ uint16_t lst[4][RH_SUBUPD_WPW * 64];   // per wave: positions (relative to its first word) of the gone points
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + wave) * RH_SUBUPD_WPW;
    // all the loads of the wave's words first (the two gathers are dependent; the words are not)
    int32_t i0[RH_SUBUPD_WPW];
    uint64_t ew[RH_SUBUPD_WPW];
#pragma unroll
    for (int k = 0; k < RH_SUBUPD_WPW; k++) {
        const int64_t j = ((w0 + k) << 6) + lane;
        i0[k] = j < s ? sub_idx0[j] : -1;
    }
#pragma unroll
    for (int k = 0; k < RH_SUBUPD_WPW; k++) ew[k] = i0[k] >= 0 ? enabled[i0[k] >> 6] : 0ULL;
    const bool own = lane < RH_SUBUPD_WPW && w0 + lane < swords;   // lane k keeps word w0 + k
    const uint64_t oldv = (own && !reset) ? sub_enabled[w0 + lane] : 0ULL;
    uint64_t newv = 0;
    int tot = 0;
#pragma unroll
    for (int k = 0; k < RH_SUBUPD_WPW; k++) {
        const bool bit = i0[k] >= 0 && ((ew[k] >> (i0[k] & 63)) & 1ULL);
        const uint64_t neww = __builtin_amdgcn_ballot_w64(bit);
        const uint64_t valid = w0 + k < swords ? valid_mask((w0 + k) << 6, s) : 0ULL;
        const uint64_t oldw = reset ? valid : (uint64_t)__shfl((unsigned long long)oldv, k);
        const uint64_t g = oldw & ~neww & valid;
        if (lane == k) newv = neww;
        if ((g >> lane) & 1ULL) lst[wave][tot + __popcll(g & ((1ULL << lane) - 1ULL))] = (uint16_t)(k * 64 + lane);
        tot += __popcll(g);
    }
    if (own) sub_enabled[w0 + lane] = newv;
    if (lane == 0) wtot[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        base_s = t > 0 ? atomicAdd(ndis, t) : 0;
    }
    __syncthreads();
    int64_t run = base_s;
    for (int k = 0; k < wave; k++) run += wtot[k];
    for (int e = lane; e < tot; e += 64) {
        const int64_t j = (w0 << 6) + lst[wave][e];
        const int64_t dst = run + e;
#pragma unroll
        for (int q = 0; q < 6; q++) dis[q * dis_stride + dst] = sub[q * sub_stride + j];
    }
}

// (ranks / out may be pinned host memory: a call with a few ranks is then this one launch, nothing else)
__global__ void select_kernel(const uint64_t *__restrict__ enabled, const int32_t *__restrict__ word_prefix,
                              int64_t nwords, const int32_t *__restrict__ total_ptr, const int64_t *__restrict__ ranks,
                              int32_t k, int64_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const int32_t total = *total_ptr;   // the select directory's count of enabled points
    const int64_t r = ranks[i];
    if (r < 1 || r > total) { out[i] = 0; return; }
    // last word w with word_prefix[w] < r
    int64_t lo = 0, hi = nwords;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (word_prefix[mid] < r) lo = mid; else hi = mid;
    }
    uint64_t m = enabled[lo];
    int rem = (int)(r - word_prefix[lo]);
    for (int t = 1; t < rem; t++) m &= m - 1;
    out[i] = (lo << 6) + __ffsll((unsigned long long)m);
}

// samplepointcloud4! (fitting.jl:383-430) on the root cell for EVERY start position of a stream of raw 64-bit draws: thread
// p plays the call that would begin at raw[p] -- first point by rejection on rand(1:n) (:388-395), the others as the
// rand(1:count)-th enabled point with one redraw when it repeats the first (:414-423), all-different test (:425-428) -- and
// leaves the points, whether the set is usable and how many draws the call consumed.  The host then follows the chain
// p -> p + consumed[p]: k calls in a row cost one launch, and the result is what k sequential calls give, draw for draw.
// rec[p]: drawN points (1-based int64; 0 = none), then consumed (0 = the draws ran out before the call finished) and ok.
__global__ void __launch_bounds__(256)
sample_sets_seq_kernel(const uint64_t *__restrict__ enabled, const int32_t *__restrict__ word_prefix, int64_t nwords, int64_t n,
                       const int32_t *__restrict__ total_ptr, const uint64_t *__restrict__ raw, int32_t L, int32_t drawN,
                       int64_t *__restrict__ rec)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= L) return;
    const int64_t count = *total_ptr;
    int64_t *o = rec + (int64_t)p * (drawN + 2);
    for (int q = 0; q < drawN + 2; q++) o[q] = 0;
    auto range = [](uint64_t u, int64_t m) { return 1 + (int64_t)__umul64hi(u, (uint64_t)m); };   // rand(1:m), rh_rng_range
    auto select = [&](int64_t r) -> int64_t {
        int64_t lo = 0, hi = nwords;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (word_prefix[mid] < r) lo = mid; else hi = mid;
        }
        uint64_t m = enabled[lo];
        const int rem = (int)(r - word_prefix[lo]);
        for (int t = 1; t < rem; t++) m &= m - 1;
        return (lo << 6) + __ffsll((unsigned long long)m);
    };
    int q = p;
    int64_t sd[16];
    if (count <= 0) return;
    int64_t r1;
    for (;;) {
        if (q >= L) return;                                  // ran out: consumed stays 0
        r1 = range(raw[q++], n);
        if ((enabled[(r1 - 1) >> 6] >> ((r1 - 1) & 63)) & 1ULL) break;
    }
    if (count < drawN) { o[drawN] = q - p; return; }          // (false, ..): fitting.jl:409-411
    sd[0] = r1;
    for (int i = 1; i < drawN; i++) {
        if (q >= L) return;
        int64_t pick = select(range(raw[q++], count));
        if (pick == sd[0]) {
            if (q >= L) return;
            pick = select(range(raw[q++], count));
        }
        sd[i] = pick;
    }
    bool distinct = true;
    for (int a = 1; a < drawN; a++)
        for (int b = 0; b < a; b++) distinct = distinct && sd[a] != sd[b];
    for (int i = 0; i < drawN; i++) o[i] = sd[i];
    o[drawN] = q - p;
    o[drawN + 1] = distinct ? 1 : 0;
}

// men[pos[i]] = enabled[i] for every point: one thread per Morton position
__global__ void oct_gather_enabled_kernel(const uint64_t *__restrict__ enabled, const int32_t *__restrict__ perm,
                                          int64_t n, uint64_t *__restrict__ men)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (j < n) {
        const int32_t i0 = perm[j];
        bit = (enabled[i0 >> 6] >> (i0 & 63)) & 1ULL;
    }
    const uint64_t w = __builtin_amdgcn_ballot_w64(bit);
    if ((threadIdx.x & 63) == 0 && (j >> 6) < (n + 63) / 64) men[j >> 6] = w;
}

}  // namespace

// one thread per bit: the set bits of word w land at word_prefix[w] + (rank inside the word);
// a wave owns one word, so the writes of a dense mask are coalesced
static __global__ void __launch_bounds__(256)
expand_dense_kernel(const uint64_t *__restrict__ mask, int64_t nwords, const int32_t *__restrict__ word_prefix,
                    int32_t *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = g >> 6;
    if (w >= nwords) return;
    const int lane = threadIdx.x & 63;
    const uint64_t m = mask[w];
    if ((m >> lane) & 1ULL) out[word_prefix[w] + __popcll(m & ((1ULL << lane) - 1ULL))] = (int32_t)g;
}

int rhk_enabled_alloc(rh_cloud *c)
{
    RH_TRY(c->enabled.alloc(c->nwords));
    RH_TRY(c->sub_enabled.alloc(c->swords));
    RH_TRY(c->d_ndis.alloc(1));
    RH_TRY(c->block_sums.alloc(std::max<int64_t>(c->nblocks, (c->swords + RH_WORDS_PER_BLOCK - 1) / RH_WORDS_PER_BLOCK) + 2));
    RH_TRY(c->en_block_sums.alloc(c->nblocks + 2));
    RH_TRY(c->word_prefix.alloc(c->nwords + 1));
    RH_TRY(c->d_total.alloc(1));
    RH_HIP(hipMemsetAsync(c->d_total, 0, sizeof(int32_t), c->stream));
    return RH_OK;
}

rh_scan_scratch rhk_take_scan_scratch(rh_cloud *c) { c->en.scratch_taken(); return { c->block_sums.get(), c->d_total.get() }; }
const int32_t *rhk_fold_total(const rh_cloud *c) { return c->d_total; }   // where rhk_enabled_apply_refit leaves its list's length
void rhk_enabled_run_ended(rh_cloud *c) { c->en.scratch_taken(); }   // (the scratch total was the extractions' while rh_ransac ran)

// mask -> ascending 1-based set-bit positions (idx_out) and / or every word's popcount prefix; ws_block_sums: nb+2 ints
int rhk_compact_generic(hipStream_t stream, const uint64_t *mask, int64_t nwords, int32_t *ws_block_sums,
                        int64_t *idx_out, int64_t cap, int32_t *d_total, int32_t *word_prefix_out)
{
    const int64_t nb = (nwords + RH_WORDS_PER_BLOCK - 1) / RH_WORDS_PER_BLOCK;
    if (nb > 0) hipLaunchKernelGGL(block_popc_kernel, dim3((unsigned)nb), dim3(256), 0, stream, mask, nwords, ws_block_sums);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(1024), 0, stream, ws_block_sums, nb, d_total);
    if (nb > 0)
        hipLaunchKernelGGL(expand_mask_kernel, dim3((unsigned)nb), dim3(256), 0, stream, mask, nwords, ws_block_sums,
                           idx_out, cap, word_prefix_out, (uint64_t *)nullptr, (int32_t *)nullptr);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// subset bits + disabled list after any change of the bits (one launch; reset_list: the list from every disabled point)
static int rebuild_sub_enabled(rh_cloud *c, bool reset_list)
{
    if (reset_list) RH_HIP(hipMemsetAsync(c->d_ndis, 0, sizeof(int32_t), c->stream));
    if (c->s == 0) return RH_OK;
    hipLaunchKernelGGL(update_sub_enabled_kernel, dim3(cdiv(c->swords, 4 * RH_SUBUPD_WPW)), dim3(256), 0, c->stream,
                       c->enabled, c->sub_idx0, c->s, c->swords, c->sub_enabled, reset_list ? 1 : 0, c->sub, c->s_pad,
                       c->dis, c->dis_stride, c->d_ndis);
    RH_HIP(hipGetLastError());
    // The plane-order twin of the words follows at once, on the same stream: whoever is ordered behind sub_enabled is ordered
    // behind it.  (Not lazily at the first plane launch: that launch may sit on a batch slot's stream, and the other slots
    // are ordered behind the cloud's stream only.)
    return rhk_plane_enabled_sync(c);
}

static int read_ndis(rh_cloud *c)   // n_dis = the list's length as the device has it (waits for the stream)
{
    int32_t ndis = 0;
    RH_HIP(hipMemcpyAsync(&ndis, c->d_ndis, sizeof ndis, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    c->n_dis = ndis;
    return RH_OK;
}

// chunks == null: all ones, which are as valid in Morton order (the mirror is a copy away, the list is empty, nothing
// waits); the caller's words leave the mirror to be regathered, and the list's length is read back
int rhk_enabled_replace(rh_cloud *c, const uint64_t *chunks)
{
    const bool all = chunks == nullptr;
    const bool mirror = all && c->k_built && c->nwords > 0;
    if (c->nwords > 0) {
        if (all) RH_HIP(hipMemsetAsync(c->enabled, 0xFF, sizeof(uint64_t) * (size_t)c->nwords, c->stream));
        else RH_HIP(hipMemcpyAsync(c->enabled, chunks, sizeof(uint64_t) * (size_t)c->nwords, hipMemcpyHostToDevice, c->stream));
        if (c->n % 64) {   // BitVector keeps the unused tail bits zero; enforce it
            const uint64_t last = (all ? ~0ULL : chunks[c->nwords - 1]) & ((~0ULL) >> (64 - c->n % 64));
            RH_HIP(hipMemcpyAsync(c->enabled + (c->nwords - 1), &last, sizeof last, hipMemcpyHostToDevice, c->stream));
        }
        if (!all || c->n % 64) RH_HIP(hipStreamSynchronize(c->stream));
        if (mirror) RH_HIP(hipMemcpyAsync(c->oct_men, c->enabled, sizeof(uint64_t) * (size_t)c->nwords, hipMemcpyDeviceToDevice, c->stream));
    }
    c->en.bits_replaced(mirror);
    RH_TRY(rebuild_sub_enabled(c, true));
    c->n_dis = 0;
    return all ? RH_OK : read_ndis(c);
}

int rhk_enabled_clear_list(rh_cloud *c, const int64_t *d_idx, int64_t n)
{
    if (n == 0) return RH_OK;
    const bool both = c->k_built && c->en.has_mirror();   // keep the Morton-order bits in step (else they are regathered later)
    hipLaunchKernelGGL(invalidate_idx_kernel, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, d_idx, n, c->n, c->enabled,
                       both ? c->oct_pos : (const int32_t *)nullptr, both ? c->oct_men : (uint64_t *)nullptr);
    RH_HIP(hipGetLastError());
    c->en.bits_cleared_by_list(both);
    RH_TRY(rebuild_sub_enabled(c, false));
    return read_ndis(c);
}

// refit list + invalidate_indexes! in one compaction: idx_out = the set bits of refit_mask, enabled &= ~refit_mask, the new
// bits' block popcounts left for the directory; nothing waits (rhk_fold_total and n_dis come with the caller's read-back)
int rhk_enabled_apply_refit(rh_cloud *c)
{
    if (c->nblocks > 0 && !c->en.scan_left_sums())
        hipLaunchKernelGGL(block_popc_kernel, dim3((unsigned)c->nblocks), dim3(256), 0, c->stream, c->refit_mask, c->nwords,
                           c->block_sums);
    const bool raw = c->nblocks > 0 && c->nblocks <= 2048;   // the expansion sums the blocks before it itself
    if (!raw) hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(1024), 0, c->stream, c->block_sums, c->nblocks, c->d_total);
    if (c->nblocks > 0)
        hipLaunchKernelGGL(expand_mask_kernel, dim3((unsigned)c->nblocks), dim3(256), 0, c->stream, c->refit_mask, c->nwords,
                           c->block_sums, c->idx_out, c->n, (int32_t *)nullptr, c->enabled, c->en_block_sums,
                           raw ? c->d_total : (int32_t *)nullptr);
    RH_HIP(hipGetLastError());
    c->en.scan_folded(c->nblocks > 0);
    return rebuild_sub_enabled(c, false);
}

int rhk_enabled_resync(rh_cloud *c)   // (the run's extractions read their lists' lengths from the scratch total)
{
    c->en.scratch_taken();
    RH_TRY(rebuild_sub_enabled(c, true));
    return read_ndis(c);
}

// select directory: word_prefix + d_total.  The block popcounts come from the extraction that left them, else from a pass here.
int rhk_ensure_select(rh_cloud *c)
{
    if (c->en.has_directory()) return RH_OK;
    if (c->nwords > 0) {
        if (!c->en.has_block_sums())
            hipLaunchKernelGGL(block_popc_kernel, dim3((unsigned)c->nblocks), dim3(256), 0, c->stream, c->enabled, c->nwords,
                               c->en_block_sums);
        hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(1024), 0, c->stream, c->en_block_sums, c->nblocks, c->d_total);
        hipLaunchKernelGGL(expand_mask_kernel, dim3((unsigned)c->nblocks), dim3(256), 0, c->stream, c->enabled, c->nwords,
                           c->en_block_sums, (int64_t *)nullptr, (int64_t)0, c->word_prefix, (uint64_t *)nullptr,
                           (int32_t *)nullptr);
        RH_HIP(hipGetLastError());
    }
    c->en.directory_built();
    return RH_OK;
}

// flat select list (sel_list[r] = the (r + 1)-th enabled point) for long sampling windows: 4 B per point, so on demand
int rhk_build_sel_list(rh_cloud *c)
{
    RH_TRY(rhk_ensure_select(c));
    if (c->en.has_list()) return RH_OK;
    if (c->nwords > 0) {
        hipLaunchKernelGGL(expand_dense_kernel, dim3((unsigned)cdiv(c->nwords * 64, 256)), dim3(256), 0, c->stream, c->enabled,
                           c->nwords, c->word_prefix, c->sel_list);
        RH_HIP(hipGetLastError());
    }
    c->en.list_built();
    return RH_OK;
}

int rhk_enabled_total(rh_cloud *c, int32_t *count)   // the directory's total on the host (built if need be; waits)
{
    RH_TRY(rhk_ensure_select(c));
    RH_HIP(hipMemcpyAsync(count, c->d_total, sizeof *count, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}

int rhk_select(rh_cloud *c, const int64_t *d_ranks, int32_t k, int64_t *d_out)
{
    if (k == 0) return RH_OK;
    if (!c->en.has_directory()) { rh_set_error("rhk_select: the select directory is not built"); return RH_E_INTERNAL; }
    hipLaunchKernelGGL(select_kernel, dim3(cdiv(k, 256)), dim3(256), 0, c->stream, c->enabled, c->word_prefix,
                       c->nwords, c->d_total, d_ranks, k, d_out);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_sample_sets_seq(rh_cloud *c, const uint64_t *d_raw, int32_t L, int32_t drawN, int64_t *d_rec)
{
    if (L == 0) return RH_OK;
    if (!c->en.has_directory()) { rh_set_error("rhk_sample_sets_seq: the select directory is not built"); return RH_E_INTERNAL; }
    hipLaunchKernelGGL(sample_sets_seq_kernel, dim3(cdiv(L, 256)), dim3(256), 0, c->stream, c->enabled, c->word_prefix, c->nwords,
                       c->n, c->d_total, d_raw, L, drawN, d_rec);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

int rhk_count_enabled(rh_cloud *c, int64_t *out)
{
    *out = 0;
    if (c->nwords == 0) return RH_OK;
    const rh_scan_scratch s = rhk_take_scan_scratch(c);
    hipLaunchKernelGGL(block_popc_kernel, dim3((unsigned)c->nblocks), dim3(256), 0, c->stream, c->enabled, c->nwords, s.sums);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(1024), 0, c->stream, s.sums, c->nblocks, s.total);
    RH_HIP(hipGetLastError());
    int32_t total = 0;
    RH_HIP(hipMemcpyAsync(&total, s.total, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    *out = total;
    return RH_OK;
}

// compact refit_mask through the scan scratch and read the total; who (null: only count): the entry whose caller gets the
// list in host_out[0 .. cap); ev (optional) is recorded behind the compaction
int rhk_refit_total(rh_cloud *c, const char *who, int64_t *host_out, int64_t cap, int64_t *total_out, hipEvent_t ev)
{
    const rh_scan_scratch s = rhk_take_scan_scratch(c);
    RH_TRY(rhk_compact_generic(c->stream, c->refit_mask, c->nwords, s.sums, who ? c->idx_out.get() : nullptr, who ? c->n : 0, s.total));
    if (ev) RH_HIP(hipEventRecord(ev, c->stream));
    int32_t total = 0;
    RH_HIP(hipMemcpyAsync(&total, s.total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    *total_out = total;
    if (who && total > cap) { rh_set_error("%s: the list has %d points, capacity %lld", who, total, (long long)cap); return RH_E_CAPACITY; }
    if (who && total > 0) {
        RH_HIP(hipMemcpyAsync(host_out, c->idx_out, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipStreamSynchronize(c->stream));
    }
    return RH_OK;
}

int rhk_korder_sync_enabled(rh_cloud *c)   // the mirror follows `enabled` lazily: regathered unless it was kept in step
{
    if (!c->k_built || c->en.has_mirror()) return RH_OK;
    if (c->n > 0) {
        hipLaunchKernelGGL(oct_gather_enabled_kernel, dim3(cdiv(c->nwords * 64, 256)), dim3(256), 0, c->stream, c->enabled,
                           c->oct_perm, c->n, c->oct_men);
        RH_HIP(hipGetLastError());
    }
    c->en.mirror_built();
    return RH_OK;
}

int rhk_oct_sync_enabled(rh_cloud *c)   // the octree sampler's view: the mirror and its popcount prefix (+ total at [nwords])
{
    if (c->n == 0) return RH_OK;
    RH_TRY(rhk_korder_sync_enabled(c));
    const rh_scan_scratch s = rhk_take_scan_scratch(c);
    RH_TRY(rhk_compact_generic(c->stream, c->oct_men, c->nwords, s.sums, nullptr, 0, s.total, c->oct_prefix));
    RH_HIP(hipMemcpyAsync(c->oct_prefix + c->nwords, s.total, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    return RH_OK;
}
