// score4.hip -- the v4 batched score kernel: scorecandidates! / scorecandidate (/root/reference/src/fitting.jl:181-190,
// shapes/plane.jl:61-71, sphere.jl:118-134, cylinder.jl:172-183, cone.jl:155-167) for a whole batch in one launch.
//
// Subset 1 in k-d leaf order, 64-point groups with boxes (kernels.hip), a block per tile of RH_G2_TG groups.
//
//  * The scalar unit is the scarce resource (measured, tools/ubench/valu_rates.hip: a scalar instruction costs a SIMD
//    ~4.2 cycles -- one scalar ALU per CU -- as much as a binary64 vector instruction; a binary32 one costs ~2.3).  The
//    older kernel walks (candidate, group) pairs with lane = point: per visit a dozen scalar instructions of loop
//    control, ballots and popcounts around 15 vector ones.  Here a LANE OWNS A PAIR.  Stage 1 (lane = candidate,
//    binary32 box tests against the tile's boxes held in scalar registers) appends the surviving (candidate, group)
//    pairs to the wave's ring in LDS; whenever 64 are queued, stage 2 takes them one per lane and every lane loops
//    over the 64 points of ITS group (LDS reads at per-lane addresses: at most RH_G2_TG distinct rows per
//    instruction, padded apart in the banks) with its candidate's record and its counters in vector registers: no
//    scalar instruction in the loop but its control, no ballot, no reduction, no divergence.
//  * The per-point work is the two-sided binary32 classifier of score4_device.h on a binary32 tile (24 B per point):
//    u = max(ua, ub) per point with sure <=> u < 0 and undecided <=> 0 <= u < 1 (plane; sphere and cylinder in the squared
//    quantities |q|^2 and qn |qn|: no root, no division).  The point loops evaluate u' = 2 u from the record doubled in
//    registers, so that both verdicts are the top two bits of u' and one v_alignbit_b32 per point keeps the pair's books
//    (score4_device.h, "Two-bit books").  The undecided POINTS of a pair -- those within the rounding margin of a
//    threshold -- are read off the owning lane's books and go through a per-wave ring to the reference's binary64 test
//    (score_device.h, unchanged; lane = ring entry, the points from global memory) one by one, whatever pair they belong
//    to; the classifier is never evaluated twice.  Cones are classified the same way (the closed form of project2cone's
//    frame, score4_device.h) with a "sure" and an "undecided" word per pair (a redo of a whole group would cost 247
//    binary64 instructions).
//  * A block's waves never wait for each other between staging and the end of a kind: each walks its own chunks
//    (culling records prefetched one chunk ahead); only the partial last batches of the waves are merged.
//
// Bit-exactness does not depend on the classifier's margins being tight, only on their being upper bounds (proof
// obligations and the audit kernel: score4_device.h).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rh_internal.h"
#include "score_device.h"
#include "score4_device.h"
#include "score4_shared.h"
#include "wave_keys.h"

namespace {

using namespace rhdev;
using namespace rh4;

// (S4_TG groups per tile, S4_STG per super-tile: score4_shared.h)
constexpr int S4_GB = 2;                 // bits of the group in a pair-list entry
constexpr unsigned S4_GM = (1u << S4_GB) - 1u;
constexpr int S4_ROW = 65;               // padded row length of the tile arrays (bank spread of the per-lane rows)
constexpr int S4_W = 4;                  // waves per block
// R: 64-candidate chunks per block row -- 16 / 12 / 4 / 2 by the size of the grid (rhk_score4_all holds the rule and the
// measurements behind it)
template <int R, bool MASK = false, bool LIST = false>
struct S4Shared {
    static_assert(S4_TG == (1 << S4_GB) && R * 64 * S4_TG <= 65536 && (R % S4_W == 0 || R < S4_W), "entry encoding: S4_GB bits of group, the rest of 16 for the candidate");
    rh_f32x4 pa[S4_TG][S4_ROW];          // (x, y, z, nx); zeros for a disabled / out-of-range point
    rh_f32x2 pb[S4_TG][S4_ROW];          // (ny, nz)
    uint64_t len[S4_TG];                 // enabled & valid bits of the groups
    rh_f32x4 gbox[S4_TG][2];             // the groups' binary32 boxes (cx cy cz hx | hy hz hr 0): stage 1 reads them as broadcasts
    rh_u32x4 gmask[S4_TG];               // the groups' normal-cell masks (96 bits; all ones without masks: another point set, "nsig" off)
    uint16_t plist[R * 64 * S4_TG + 2];  // the block's surviving pairs: candidate of the row << S4_GB | group (+ a dump slot)
    uint16_t ctab[LIST ? R * 64 : 2];    // LIST: the bin slot of every candidate of the row (the row walks its super-tile's list)
    int32_t cntb[S4_W][64];              // cone: per-wave inlier counts of the batch's pairs
    unsigned long long maskb[S4_W][64];  // cone, masks wanted: per-wave inlier words of the batch's pairs
    uint16_t qb[S4_W][128];              // cone: per-wave ring (slot-in-batch << 6 | point-in-group) for the exact test
    int weirdw[S4_TG];                   // per group: an enabled point with a non-finite value
    int npairs, next_batch;
};

struct S4KindArgs {
    const rh_cls *cls;      // classifier records of the bin
    const float *box;       // culling records of the bin: field f of slot i at box[f * bstride + i]
    const rh_prep *prep;    // binary64 records of the bin
    const int32_t *orig, *nk;
    const uint64_t *en;
    double eps, cosa;
    // the kind's point set (planes may walk the cloud's plane order while the other kinds walk the k-d leaf order: same
    // points tile by super-tile, another grouping): six planes `stride` apart, the groups' binary32 boxes (8 floats each) and
    // their normal-cell masks (4 words each; null: no pair is ruled out by its normals); `en` is in the set's order
    const double *pts;
    int64_t stride;
    const float *gb32;
    const uint32_t *gm32;
};
struct S4AllArgs {
    const int32_t *stop;   // chained octree windows: non-zero = the window has ended, nothing to score (else null)
    int row0;              // TAIL launch: first row that the sized launch did not cover
    int rows;              // sized launch: > 0 = a one-dimensional grid of (tiles padded to 8) x rows blocks in XCD order (score4_kernel)
    S4KindArgs k[4];
    int64_t ntiles, bstride, ngroups;
    // masks wanted: per candidate (as the caller numbers it) a LIST of its non-zero inlier words in internal (k-d leaf)
    // order -- entries of 16 bytes (word number, word), mstride of them per row at most; occ = one int32 cursor per row
    // (zero on entry)
    uint64_t *masks;
    uint8_t *occ;
    int64_t mstride;
    unsigned long long *stats;   // diag build: event counters of the launch (rh_dbg_s4_stats; layout at S4_STAT), else null
    // LIST launches: per super-tile (S4_STG groups) and kind the bin slots of the candidates whose culling record does not
    // rule the super-tile's box out, ascending (st_cull_kernel), stcap apart, and their numbers
    const uint16_t *stlist;
    const int32_t *stcount;
    int64_t stcap;
};

// ---- event counters (diag build only; tools/isa_account.py multiplies them with the static instruction histogram of the
// kernel's regions): one add per WAVE-level event.  Per kind k at 24 k + ...: 0 segments entered, 1..4 chunk visits of the
// wave's 1st..4th chunk, 5 candidates box-tested, 6 chunk visits without a survivor, 7 surviving pairs, 8 batches, 9 pairs
// with an undecided point (the wave-uniform loop that queues them: the "second pass" of the tools), 10 undecided points
// queued for the exact test, 11 full ring drains, 12 final drains,
// 13 points the exact test accepted, 14 pairs with a count > 0, 15 cone: compaction rounds.  Global at 96 + ...: 0 waves of
// blocks with a tile, 1 stagings (per wave), 2 re-used stagings, 3 waves whose tile has no enabled point.
#ifdef RH_DIAG
#define S4_STAT(stats, idx, val) do { const unsigned long long v_ = (unsigned long long)(val); if ((stats) != nullptr && (threadIdx.x & 63) == 0) atomicAdd((stats) + (idx), v_); } while (0)
#else
#define S4_STAT(stats, idx, val) do { } while (0)
#endif

#define RH4_CONST_AS __attribute__((address_space(4)))
// score4_kernel's explicit arguments as they lie in its kernarg segment (each at its natural alignment)
struct S4KernArgs {
    int64_t s;
    S4AllArgs A;
    int32_t *counts;
    int dbg;
};
static_assert(offsetof(S4KernArgs, A) == 8 && alignof(S4AllArgs) == 8 && offsetof(S4KernArgs, counts) == 8 + sizeof(S4AllArgs), "kernarg layout of score4_kernel");

// lane i <- lane i - 1 (lane 0 <- 0) / lane i <- lane i + 1 (lane 63 <- 0): DPP moves across the whole wave, no trip through LDS
static __device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
static __device__ __forceinline__ int wave_shl1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }

// segmented sum over runs of equal keys in adjacent lanes (runs of up to S4_TG = 4: the groups of one candidate): the
// LAST lane of a run gets the run's total, the others 0
static __device__ __forceinline__ int run_total(int v, int key, int lane)
{
    static_assert(S4_TG <= 4, "two steps cover runs of four");
    // (every move with all lanes active: a DPP move reads nothing from a lane that is switched off)
    const int k1 = wave_shr1(key), u1 = wave_shr1(v);
    v += (lane >= 1 && k1 == key) ? u1 : 0;
    const int k2 = wave_shr1(k1), u2 = wave_shr1(wave_shr1(v));
    v += (lane >= 2 && k2 == key) ? u2 : 0;
    const int kn = wave_shl1(key);
    return (lane == 63 || kn != key) ? v : 0;
}

// one batch: the 64 pairs of the block's list from `head` on (n of them valid), one per lane
template <int KIND, int R, bool MASK, bool F32, bool LIST>
static __device__ __forceinline__ void
score4_batch(S4Shared<R, MASK, LIST> &sh, const int wv, const int lane, const int pil, const int head, const int n, const int cbase, const double *__restrict__ pts,
             int64_t stride, const int64_t p0, const rh_prep *__restrict__ prep, const rh_cls *__restrict__ cls,
             const int32_t *__restrict__ orig, double eps, double cosa, int32_t *__restrict__ counts, const bool weird,
             uint64_t *__restrict__ masks, uint8_t *__restrict__ occ, const int64_t mstride, const int64_t g0, unsigned long long *__restrict__ stats)
{
    (void)stats;
    S4_STAT(stats, 24 * KIND + 8, 1);
    const bool act = lane < n;
    const uint32_t e = sh.plist[head + (act ? lane : 0)];
    const int g = (int)(e & S4_GM), ci = LIST ? (int)sh.ctab[e >> S4_GB] : cbase + (int)(e >> S4_GB);
    const rh_f32x4 *__restrict__ rowa = &sh.pa[g][0];
    const rh_f32x2 *__restrict__ rowb = &sh.pb[g][0];
    const rh_cls *__restrict__ rec = &cls[ci];
    int total = 0;
    uint64_t word = 0;   // MASK: the inlier word of the lane's pair
    // Undecided POINTS go to the exact test through a per-wave ring of (pair of the batch << 6 | point of its group), 64 at a
    // time, lane = ring entry: the reference's test of the cloud's element type on the entry's own record; what it accepts is
    // added to the pair's count (and word) in LDS.  (Float32 cloud: the staged floats are the points; Float64: global memory.)
    int qbh = 0, qbn = 0;   // ring head / fill (wave-uniform)
    auto drain_b = [&](int k) {
        wave_lds_sync();
        const bool on = lane < k;
        const unsigned e2 = on ? sh.qb[wv][(qbh + lane) & 127] : 0u;
        const int slot = (int)(e2 >> 6);
        const uint32_t pe = sh.plist[head + slot];
        const int64_t gi = p0 + (int)(pe & S4_GM) * 64 + (int)(e2 & 63u);
        uint64_t r;
        if (F32) {
            const rh_prepf Pv = prepf_of<KIND>(prep[LIST ? (int)sh.ctab[pe >> S4_GB] : cbase + (int)(pe >> S4_GB)]);
            const rh_f32x4 a = sh.pa[pe & S4_GM][e2 & 63u];
            const rh_f32x2 b = sh.pb[pe & S4_GM][e2 & 63u];
            r = test_point<KIND>(Pv, a.x, a.y, a.z, a.w, b.x, b.y, eps, cosa);
        } else {
            const rh_prep Pv = prep[LIST ? (int)sh.ctab[pe >> S4_GB] : cbase + (int)(pe >> S4_GB)];
            r = test_point<KIND>(Pv, pts[gi], pts[stride + gi], pts[2 * stride + gi], pts[3 * stride + gi], pts[4 * stride + gi],
                                 pts[5 * stride + gi], eps, cosa);
        }
        S4_STAT(stats, 24 * KIND + (k == 64 ? 11 : 12), 1);
        S4_STAT(stats, 24 * KIND + 13, __popcll(r & (k >= 64 ? ~0ULL : ((1ULL << k) - 1ULL))));
        if (on && ((r >> lane) & 1ULL)) {
            atomicAdd(&sh.cntb[wv][slot], 1);
            if (MASK) atomicOr(&sh.maskb[wv][slot], 1ULL << (e2 & 63u));
        }
        qbh = (qbh + k) & 127;
        qbn -= k;
    };
    if (KIND != RH_CONE) {
        constexpr int NF = KIND == RH_PLANE ? 9 : (KIND == RH_SPHERE ? 8 : 11);
        rh_cls C;
#pragma unroll
        for (int f = 0; f < NF; f++) C.f[f] = rec->f[f];
        const bool exact_only = weird || is_nan_bits(rec->f[RH_CLS_FLAG]);
        // The books of the pair over its 64 points (score4_device.h, "Two-bit books"): the record is doubled in registers, so a
        // point's verdict sits in the top two bits of its u' = 2 u -- sign: surely an inlier; neither bit: undecided -- and ONE
        // v_alignbit_b32 per point shifts both into the pair's books, 16 points per word.  No compare, no carry chain, no
        // running minimum; four loops over consecutive points, so that the LDS reads keep their pairing.
        cls_double<KIND>(C);
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll 8
            for (int j = 0; j < 16; j++) {
                const rh_f32x4 a = rowa[16 * q + j];
                const rh_f32x2 b = rowb[16 * q + j];
                w[q] = books2_push(w[q], cls_u2<KIND>(C, a.x, a.y, a.z, a.w, b.x, b.y));
            }
        }
        // (a disabled or out-of-range point is staged as zeros and surely out by cls_make's guards: no mask by the group's
        // enabled word here.  u' = 2 exactly -- u = 1, surely outside by the margins -- is out; a NaN u' can only come from a
        // non-finite record or point, and those pairs ignore their books: exact_only, weird)
        const bool amb = act && (exact_only || books2_any_undecided(w));
        total = (act && !exact_only) ? books2_sure_count(w) : 0;
        if (MASK) word = (act && !exact_only) ? books2_sure64(w) : 0ULL;
        // Pairs with an undecided point (a percent of them): the owning lane's books say WHICH points are undecided; a
        // wave-uniform loop over those pairs puts them on the ring, a lane per bit of the word -- two v_readlane of the owner's word, a
        // rank, a store; no record, no point and no classifier a second time -- and only they take the exact test, 64 at a
        // time, whatever pair they belong to.  (Until round 12 the loop evaluated the classifier again with lane = point to
        // find them: 36-48 vector and 53-56 scalar instructions per pair behind a scalar-load round trip.  Round 3 ran the
        // exact test on the whole group of every such pair: 40 binary64 instructions per wave and pair.)
        uint64_t redo = WB(amb);
        S4_STAT(stats, 24 * KIND + 9, __popcll(redo));
        if (redo != 0) {
            uint64_t und;   // (read of the amb lanes only)
            if (MASK) {
                const uint64_t lg = sh.len[g];
                und = exact_only ? lg : (books2_und64(w) & lg);   // (exact-only: every enabled point; point order, as the inlier words are)
            } else {
                // Counts-only: the books' own bit order (score4_device.h, "Books in place") -- bit L of the word is point pil
                // of lane L, four instructions instead of four compressions.  No mask by the group's enabled word: a disabled
                // or out-of-range point is staged as zeros, and cls_make's guards make the zero point surely out for every
                // record whose books are read (the note behind the point loops) -- its two bits never read "undecided".
                und = books2_und64_inplace(w);
                // pairs that ignore their books take every enabled point: the enabled word, deposited into the books' order
                // (wave-uniform branch: rare -- an exact-only record or a tile with a non-finite value)
                if (WB(amb && exact_only) != 0) { if (exact_only) und = books2_deposit64(sh.len[g]); }
            }
            const uint32_t undlo = (uint32_t)und, undhi = (uint32_t)(und >> 32);
            sh.cntb[wv][lane] = 0;
            if (MASK) sh.maskb[wv][lane] = 0ULL;
            while (redo != 0) {
                const int k = __builtin_ctzll(redo);
                redo &= redo - 1;
                const uint32_t ulo = __builtin_amdgcn_readlane(undlo, k), uhi = __builtin_amdgcn_readlane(undhi, k);
                const uint64_t uk = ((uint64_t)uhi << 32) | ulo;
                const bool has = (uk >> lane) & 1ULL;
                const int rank = __builtin_amdgcn_mbcnt_hi(uhi, __builtin_amdgcn_mbcnt_lo(ulo, 0));
                if (has) sh.qb[wv][(qbh + qbn + rank) & 127] = (uint16_t)((k << 6) | pil);   // (pil: the point lane's bit stands for)
                qbn += __popcll(uk);
                S4_STAT(stats, 24 * KIND + 10, __popcll(uk));
                if (qbn >= 64) drain_b(64);
            }
            if (qbn > 0) drain_b(qbn);
            wave_lds_sync();
            total += sh.cntb[wv][lane];
            if (MASK) word |= sh.maskb[wv][lane];
        }
    } else {
        rh_cls C;
#pragma unroll
        for (int f = 0; f < 13; f++) C.f[f] = rec->f[f];
        const bool exact_only = weird || is_nan_bits(rec->f[RH_CLS_FLAG]);
        // two words per pair, sign bits shifted in from the right and un-reversed afterwards: s = surely an inlier (u < 0),
        // m = not surely out (u < 1, the sign of u - 1); undecided = m & ~s
        uint32_t slo = 0, shi = 0, mlo = 0, mhi = 0;
#pragma unroll 4
        for (int j = 0; j < 32; j++) {
            const rh_f32x4 a = rowa[j];
            const rh_f32x2 b = rowb[j];
            const float u = cls_cone_u(C, a.x, a.y, a.z, a.w, b.x, b.y);
            slo = __builtin_amdgcn_alignbit(slo, __builtin_bit_cast(uint32_t, u), 31);
            mlo = __builtin_amdgcn_alignbit(mlo, __builtin_bit_cast(uint32_t, u - 1.0f), 31);
        }
#pragma unroll 4
        for (int j = 0; j < 32; j++) {
            const rh_f32x4 a = rowa[32 + j];
            const rh_f32x2 b = rowb[32 + j];
            const float u = cls_cone_u(C, a.x, a.y, a.z, a.w, b.x, b.y);
            shi = __builtin_amdgcn_alignbit(shi, __builtin_bit_cast(uint32_t, u), 31);
            mhi = __builtin_amdgcn_alignbit(mhi, __builtin_bit_cast(uint32_t, u - 1.0f), 31);
        }
        mlo &= ~slo; mhi &= ~shi;
        slo = __brev(slo); shi = __brev(shi); mlo = __brev(mlo); mhi = __brev(mhi);
        const uint64_t lg = sh.len[g];
        // (a disabled point is staged as zeros: whatever the classifier makes of it, its bit is masked out here)
        uint64_t sure = exact_only ? 0ULL : ((((uint64_t)shi << 32) | slo) & lg);
        uint64_t mask = exact_only ? lg : ((((uint64_t)mhi << 32) | mlo) & lg);
        if (!act) { mask = 0; sure = 0; }
        sh.cntb[wv][lane] = 0;
        if (MASK) sh.maskb[wv][lane] = 0ULL;
        // the set bits of the 64 masks, one per lane and round, compacted onto the ring
        while (WB(mask != 0) != 0) {
            const bool has = mask != 0;
            const int j = has ? __builtin_ctzll(mask) : 0;
            mask &= mask - 1;
            const uint64_t mm = WB(has);
            const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0));
            if (has) sh.qb[wv][(qbh + qbn + rank) & 127] = (uint16_t)((lane << 6) | j);
            qbn += __popcll(mm);
            S4_STAT(stats, 24 * KIND + 15, 1);
            S4_STAT(stats, 24 * KIND + 10, __popcll(mm));
            if (qbn >= 64) drain_b(64);
        }
        if (qbn > 0) drain_b(qbn);
        wave_lds_sync();
        total = sh.cntb[wv][lane] + __popcll(sure);
        if (MASK) word = sh.maskb[wv][lane] | sure;
    }
    if (MASK) {
        // the pairs' inlier words join their candidates' LISTS (any order): entry = (internal word number, word), 16 bytes.  The
        // pairs of a candidate sit in adjacent lanes: the first lane of such a run reserves the run's places with ONE add on
        // the row's cursor.  (Measured, cfg3 launch, against round 3's two plain stores into sparse rows, 94 us: an add per
        // entry at the end of the batch 116; places for every pair reserved at the start of the batch, the round trip behind
        // the point loop, 287 -- the cursors' adds serialise; words parked in LDS and flushed once per segment 128.)
        const bool nz = act && word != 0;
        const uint64_t nzm = WB(nz);
        if (nzm != 0) {
            const int keyp = wave_shr1(act ? ci : -1 - lane);   // (wave-uniform branch: all lanes active)
            const uint64_t starts = WB(lane == 0 || keyp != (act ? ci : -1 - lane));
            const uint64_t below = lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL);          // lanes 0 .. lane
            const int rs = 63 - __builtin_clzll(starts & below);                            // first lane of my run
            const uint64_t after = lane == 63 ? 0ULL : (starts >> (lane + 1));
            const int re = after != 0 ? lane + __builtin_ctzll(after) : 63;               // last lane of my run
            const uint64_t runm = (re == 63 ? ~0ULL : ((2ULL << re) - 1ULL)) & ~((1ULL << rs) - 1ULL);
            const int tot = __popcll(nzm & runm);
            int base = 0;
            int64_t mrow = 0;
            if (nz || (lane == rs && tot > 0)) mrow = orig[ci];
            if (lane == rs && tot > 0) base = atomicAdd((int32_t *)occ + mrow, tot);
            base = __shfl(base, rs);
            if (nz) {
                const int rank = __popcll(nzm & runm & ((1ULL << lane) - 1ULL));
                rh_u64x2 ent;
                ent.x = (uint64_t)(g0 + g);
                ent.y = word;
                ((rh_u64x2 *)masks)[mrow * mstride + base + rank] = ent;
            }
        }
    }
    S4_STAT(stats, 24 * KIND + 14, __popcll(WB(act && total > 0)));
    // one global atomic per (candidate, tile) with inliers: the pairs of a candidate sit in adjacent lanes
    const int v = run_total(act ? total : 0, act ? ci : -1 - lane, lane);
    if (v != 0) atomicAdd(&counts[orig[ci]], v);
}

// one kind segment of the block's row: chunks [lo, hi) of the kind (at most S4_R).  Stage 1: the waves share the
// chunks out, lane = candidate, box tests, survivors -> the block's pair list.  Stage 2: the waves take batches of 64
// pairs from the list until it is empty.
template <int KIND, int R, bool MASK, bool F32, bool LIST>
static __device__ __forceinline__ void
score4_segment(S4Shared<R, MASK, LIST> &sh, const RH4_CONST_AS S4KindArgs *K, const int pil, const int32_t *__restrict__ nkp, const uint16_t *__restrict__ list, const int64_t bstride, const int lo, const int hi,
               const double *__restrict__ pts, int64_t stride, const int64_t g0, const unsigned live, const bool weird,
               int32_t *__restrict__ counts, int dbg, uint64_t *__restrict__ masks, uint8_t *__restrict__ occ, const int64_t mstride,
               unsigned long long *__restrict__ stats)
{
    (void)stats;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nk = *nkp;
    S4_STAT(stats, 24 * KIND + 0, 1);
    constexpr int NB = S4Fields<KIND>::NBOX;
    // (the culling records of the wave's chunks are requested together, before the first box test)
    constexpr int CPW = (R + S4_W - 1) / S4_W;   // (rows of 1 or 2 chunks: the waves without a chunk of their own go straight to the batches)
    float B[2][RH_BOX_FIELDS];
    // (unconditional loads from a clamped slot: a lane without a candidate reads slot 0 and is masked out below -- a
    // guarded load per field costs a scalar exec-mask save / branch / restore each, ~20 scalar instructions per chunk)
    // LIST: the row's candidates come from the super-tile's list -- the bin slots of ALL the wave's chunks are requested
    // together (one round trip in front of the record loads instead of one per chunk) and kept in LDS for stage 2
    int slot[LIST ? CPW : 1];
    auto clamped = [&](int h) { const int ci = ((lo + wv + h * S4_W) << 6) + lane; return (lo + wv + h * S4_W < hi && ci < nk) ? ci : 0; };
    if (LIST) {
#pragma unroll
        for (int h = 0; h < CPW; h++) slot[h] = (int)list[clamped(h)];
#pragma unroll
        for (int h = 0; h < CPW; h++) {
            const int ci = ((lo + wv + h * S4_W) << 6) + lane;
            if (lo + wv + h * S4_W < hi && ci < nk) sh.ctab[ci - (lo << 6)] = (uint16_t)slot[h];
        }
    }
    {
        const int cil = LIST ? slot[0] : clamped(0);
#pragma unroll
        for (int f = 0; f < NB; f++) B[0][f] = K->box[(int64_t)f * bstride + cil];
    }
#pragma unroll
    for (int h = 0; h < CPW; h++) {
        const int c = lo + wv + h * S4_W;
        if (c >= hi) break;
        const int ci = (c << 6) + lane;
        if (h + 1 < CPW) {   // the next chunk's records: in flight during this chunk's tests
            const int cinl = LIST ? slot[h + 1 < CPW ? h + 1 : 0] : clamped(h + 1);
#pragma unroll
            for (int f = 0; f < NB; f++) B[(h + 1) & 1][f] = K->box[(int64_t)f * bstride + cinl];
        }
        unsigned surv = 0;
#pragma unroll
        for (int g = 0; g < S4_TG; g++) {
            // (the boxes come from LDS, wave-uniform addresses: kept in scalar registers across the four per-kind bodies
            // of the kernel they were spilled lane by lane into vector registers -- 30 spilled registers, 217 lane moves)
            const rh_f32x4 g0v = sh.gbox[g][0], g1v = sh.gbox[g][1];
            rh_box32 G;
            G.cx = g0v.x; G.cy = g0v.y; G.cz = g0v.z; G.hx = g0v.w; G.hy = g1v.x; G.hz = g1v.y; G.hr = g1v.z;
            bool skip = box_skip32<KIND>(B[h & 1], G);
            if (KIND == RH_PLANE) skip |= !nsig_meet(B[h & 1], sh.gmask[g]);   // (no point of the group has a normal the candidate accepts)
            surv |= skip ? 0u : (1u << g);
        }
        if (dbg == 2) surv = (1u << S4_TG) - 1u;
        surv &= live;
        if (ci >= nk || dbg == 1) surv = 0;
        // positions candidate-major: all lanes before me, then my own lower groups
        const int k = __popc(surv);
        const uint64_t b0 = WB(k & 1), b1 = WB(k & 2), b2 = WB(k & 4), b3 = WB(k & 8);
        const int tot = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2) + 8 * __popcll(b3);
        S4_STAT(stats, 24 * KIND + 1 + (h < 3 ? h : 3), 1);
        S4_STAT(stats, 24 * KIND + 5, __popcll(WB(ci < nk)));
        S4_STAT(stats, 24 * KIND + 7, tot);
        if (tot == 0) { S4_STAT(stats, 24 * KIND + 6, 1); continue; }
        int base = 0;
        if (lane == 0) base = atomicAdd(&sh.npairs, tot);
        base = __builtin_amdgcn_readfirstlane(base);
        auto mb = [&](uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0)); };
        int pos = base + mb(b0) + 2 * mb(b1) + 4 * mb(b2) + 8 * mb(b3);
        // (branch-free: a group that did not survive writes to the dump slot behind the list -- a predicated store costs a
        // scalar exec-mask save / branch / restore per group)
#pragma unroll
        for (int g = 0; g < S4_TG; g++) {
            const bool on = (surv >> g) & 1u;
            sh.plist[on ? pos : R * 64 * S4_TG] = (uint16_t)(((ci - (lo << 6)) << S4_GB) | g);
            pos += on ? 1 : 0;
        }
    }
    __syncthreads();
    const int npairs = sh.npairs;
    for (;;) {
        int bt = 0;
        if (lane == 0) bt = atomicAdd(&sh.next_batch, 1);
        bt = __builtin_amdgcn_readfirstlane(bt);
        if (bt * 64 >= npairs) break;
        score4_batch<KIND, R, MASK, F32, LIST>(sh, wv, lane, pil, bt * 64, min(64, npairs - bt * 64), lo << 6, pts, stride, g0 * 64, K->prep, K->cls, K->orig,
                                         K->eps, K->cosa, counts, weird, masks, occ, mstride, g0, stats);
    }
}

// the tile as binary32 with the enabled words of one kind applied (one point per thread)
template <class SH>
static __device__ __forceinline__ void s4_stage(SH &sh, const double *__restrict__ pts, int64_t stride, int64_t s,
                                                const uint64_t *__restrict__ enabled_words, const int64_t p0, const float *__restrict__ gb32,
                                                const uint32_t *__restrict__ gm32, const int64_t ngroups)
{
    static_assert(S4_TG % S4_W == 0, "every wave stages S4_TG / S4_W groups");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int GPW = S4_TG / S4_W;
    // (the loads of all the wave's groups go out before any enabled word is looked at: one round trip)
    double x[GPW], y[GPW], z[GPW], nx[GPW], ny[GPW], nz[GPW];
#pragma unroll
    for (int q = 0; q < GPW; q++) {
        const int64_t gi = p0 + (int64_t)(wv + q * S4_W) * 64 + lane;
        x[q] = pts[gi]; y[q] = pts[stride + gi]; z[q] = pts[2 * stride + gi];
        nx[q] = pts[3 * stride + gi]; ny[q] = pts[4 * stride + gi]; nz[q] = pts[5 * stride + gi];
    }
#pragma unroll
    for (int q = 0; q < GPW; q++) {
        const int g = wv + q * S4_W;
        const int64_t gi = p0 + (int64_t)g * 64 + lane;
        uint64_t v = valid_mask((gi >> 6) << 6, s);
        if (enabled_words != nullptr && v != 0) v &= enabled_words[gi >> 6];
        const bool on = (v >> (gi & 63)) & 1ULL;
        rh_f32x4 a = { 0.f, 0.f, 0.f, 0.f };
        rh_f32x2 b = { 0.f, 0.f };
        bool bad = false;
        if (on) {
            a.x = (float)x[q]; a.y = (float)y[q]; a.z = (float)z[q]; a.w = (float)nx[q]; b.x = (float)ny[q]; b.y = (float)nz[q];
            const float sum = (fabsf(a.x) + fabsf(a.y)) + (fabsf(a.z) + fabsf(a.w)) + (fabsf(b.x) + fabsf(b.y));
            bad = !(sum < __builtin_inff());   // an infinite or NaN value (binary32 overflow included)
        }
        sh.pa[g][lane] = a;
        sh.pb[g][lane] = b;
        const uint64_t wb = WB(bad);
        if (lane == 0) { sh.weirdw[g] = wb != 0 ? 1 : 0; sh.len[g] = v; }   // v is the group's word
    }
    if (tid == 0) { sh.npairs = 0; sh.next_batch = 0; }
    if (tid < 2 * S4_TG) {   // the boxes, 32 bytes each
        const int64_t g = p0 / 64 + (tid >> 1);
        sh.gbox[tid >> 1][tid & 1] = ((const rh_f32x4 *)gb32)[(g < ngroups ? g : ngroups - 1) * 2 + (tid & 1)];
    }
    if (tid >= 64 && tid < 64 + S4_TG) {   // the normal-cell masks, 16 bytes each (the second wave: not behind the boxes' loads)
        const int64_t g = p0 / 64 + (tid - 64);
        rh_u32x4 m = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u };
        if (gm32 != nullptr) m = ((const rh_u32x4 *)gm32)[g < ngroups ? g : ngroups - 1];
        sh.gmask[tid - 64] = m;
    }
}

// grid: (tiles padded to a multiple of 8, rows).  The 64-candidate chunks of the four kind bins are laid end to end,
// the expensive kinds first (cone, cylinder, sphere, plane), and cut into rows of R; a block runs the per-kind
// segment(s) of its row (almost always one) on its tile.
// TAIL: the launch that picks up what a sized-before-the-count-was-known launch leaves over (rhk_score4_all, `open`):
// its blocks walk the rows from A.row0 on grid-stride.  A separate instantiation -- the loop around the four per-kind
// bodies costs the register allocation dearly (10 to 17 vector registers spilled; until the bodies read their arguments where
// they start, 114 to 192 scalar ones as well), the one-row form none.
template <int R, bool MASK, bool F32, bool TAIL = false, bool LIST = false>
// 7 blocks of four waves per CU = 7 waves per SIMD = 72 vector registers (measured against 8 / 64 registers: cfg3 0.0816 ->
// 0.0807 ms, cfg5 0.3006 -> 0.2973; 6 / 80 registers is slower: profiles/r4/experiments.txt)
#ifndef RH_S4_MINBLK
#define RH_S4_MINBLK 7
#endif
__global__ void __launch_bounds__(64 * S4_W, (F32 && !(LIST && R == 16)) ? 8 : RH_S4_MINBLK)   // (the Float32 instantiations: 8 / 64 registers, 0.0916 -> see experiments.txt; LIST rows of 16: 20.8 KB of LDS, seven blocks)
score4_kernel(int64_t s, const S4AllArgs A, int32_t *__restrict__ counts, int dbg_arg)
{
#ifdef RH_DIAG
    const int dbg = dbg_arg;   // diag build: 1 = no pair survives stage 1 (the skeleton alone), 2 = every pair does
#else
    constexpr int dbg = 0;     // the product kernel has no such switch
    (void)dbg_arg;
#endif
    __shared__ S4Shared<R, MASK, LIST> sh;
    // Blocks go to the 8 XCDs round-robin by their linear id, each XCD with an L2 of its own.  With rows > 0 the id is
    // read as ((tile / 8) x rows + row) x 8 + tile % 8: the rows of one tile follow each other on ONE XCD, so the tile is
    // fetched from HBM once and staged from L2 by the other rows (cfg5, 9 rows over a 75-MB subset: the (tile, row) grid
    // fetched every tile once per row -- 724 MB per launch, profiles/r3).
    int64_t tile = blockIdx.x;
    int rowy = (int)blockIdx.y;
    if (!TAIL && A.rows > 0) {
        const int64_t k = blockIdx.x >> 3;
        rowy = (int)(k % A.rows);
        tile = ((k / A.rows) << 3) + (blockIdx.x & 7);
    }
    if (tile >= A.ntiles) return;
    if (A.stop != nullptr && *A.stop != 0) return;
    const int64_t g0 = tile * S4_TG;
    S4_STAT(A.stats, 96 + 0, 1);
    static_assert(!(TAIL && LIST), "the row-walking launch takes its candidates in bin order");
    int nch[4], total = 0;
    const int64_t st4 = LIST ? (tile / (S4_STG / S4_TG)) * 4 : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { nch[k] = ((LIST ? A.stcount[st4 + k] : *A.k[k].nk) + 63) >> 6; total += nch[k]; }
    bool ran = false, weird = false;
    unsigned live = 0;
    const uint64_t *staged_en = nullptr;
    const double *staged_pts = nullptr;
    (void)staged_en;
    (void)staged_pts;
    const RH4_CONST_AS S4KernArgs *const kargs = (const RH4_CONST_AS S4KernArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    // counts-only: the point that this lane's bit of a pair's undecided word stands for (score4_device.h, "Books in place")
    const int pil = MASK ? (int)(threadIdx.x & 63) : books2_point_of_bit((int)(threadIdx.x & 63));
    // Every per-kind body takes its arguments from the kernarg segment where it starts, through a constant-address-space pointer
    // behind an empty asm: the loads can neither be hoisted to the kernel's start nor merged across the bodies.  (Read from the
    // by-value A they were all requested in the prologue and stayed live across the four bodies -- 37 to 52 scalar registers of
    // the list instantiations spilled into vector lanes, 30 v_writelane per wave up front and a v_readlane wherever one was used.)
#define RH_S4_BODY(K)                                                                                                  \
    {                                                                                                                  \
        const int slo = max(lo, base) - base, shi = min(hi, base + nch[K]) - base;                                     \
        if (slo < shi) {                                                                                               \
            const RH4_CONST_AS S4KernArgs *ka = kargs;                                                                 \
            asm volatile("" : "+s"(ka));                                                                               \
            const RH4_CONST_AS S4KindArgs *Kb = &ka->A.k[K];                                                           \
            const uint64_t *const en_k = Kb->en;                                                                       \
            const double *const pts_k = Kb->pts;                                                                       \
            if (ran) __syncthreads();   /* the previous segment's waves are done with the tile and the list */        \
            if (!ran || en_k != staged_en || pts_k != staged_pts) {   /* (another point set: its own boxes and masks too) */ \
                s4_stage(sh, pts_k, Kb->stride, s, en_k, g0 * 64, Kb->gb32, Kb->gm32, ka->A.ngroups);                  \
                staged_en = en_k;                                                                                      \
                staged_pts = pts_k;                                                                                    \
                S4_STAT(A.stats, 96 + 1, 1);                                                                           \
            } else { S4_STAT(A.stats, 96 + 2, 1); if (threadIdx.x == 0) { sh.npairs = 0; sh.next_batch = 0; } }   /* same tile, same enabled words */   \
            __syncthreads();                                                                                           \
            live = 0;                                                                                                  \
            for (int g = 0; g < S4_TG; g++) live |= sh.len[g] != 0 ? (1u << g) : 0u;                                   \
            live = __builtin_amdgcn_readfirstlane(live);                                                               \
            { int ww = 0; for (int g = 0; g < S4_TG; g++) ww |= sh.weirdw[g]; weird = __builtin_amdgcn_readfirstlane(ww) != 0; }  \
            if (live != 0) score4_segment<K, R, MASK, F32, LIST>(sh, Kb, pil, LIST ? ka->A.stcount + (st4 + K) : Kb->nk, LIST ? ka->A.stlist + (st4 + K) * ka->A.stcap : nullptr, ka->A.bstride, slo, shi, pts_k, Kb->stride, g0, live, weird, counts, dbg, ka->A.masks, ka->A.occ, ka->A.mstride, A.stats); \
            else S4_STAT(A.stats, 96 + 3, 1);                                                                         \
            ran = true;                                                                                                \
        }                                                                                                              \
        base += nch[K];                                                                                                \
    }
    if (!TAIL) {
        const int lo = rowy * R, hi = min(total, lo + R);
        if (lo >= hi) return;
        int base = 0;
        RH_S4_BODY(RH_CONE)
        RH_S4_BODY(RH_CYLINDER)
        RH_S4_BODY(RH_SPHERE)
        RH_S4_BODY(RH_PLANE)
    } else {
        for (int lo = (A.row0 + (int)blockIdx.y) * R; lo < total; lo += (int)gridDim.y * R) {
            const int hi = min(total, lo + R);
            int base = 0;
            RH_S4_BODY(RH_CONE)
            RH_S4_BODY(RH_CYLINDER)
            RH_S4_BODY(RH_SPHERE)
            RH_S4_BODY(RH_PLANE)
        }
    }
#undef RH_S4_BODY
}

// ---- the super-tile lists of a batch.  One block per (super-tile, kind): the kind's candidates in bin order, 256 at a time,
// lane = candidate, the culling record against the super-tile's box with the very test of stage 1 (box_skip32: a box that
// holds all the points of its groups may be skipped only when none of them can pass) -- the survivors' bin slots, in order.
struct StCullArgs {
    const float *box[4];
    const int32_t *nk[4];
    int64_t bstride, stcap;
    const float *st32, *st32_plane;   // boxes of the super-tiles of the order the kind walks (planes: maybe the plane order's)
    const uint32_t *stm32;   // normal-cell masks of the planes' super-tiles (the OR of their groups'), 4 words each; null: not looked at
    uint16_t *stlist;
    int32_t *stcount;
};

template <int KIND>
static __device__ __forceinline__ void st_cull_kind(const StCullArgs &A, const int64_t st)
{
    constexpr int Q = 4;                       // candidates per thread and round: 1024 per round, their records requested together
    __shared__ int32_t wsum[2][Q * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nk = *A.nk[KIND];
    int32_t *cnt = A.stcount + st * 4 + KIND;
    if (nk <= 0) { if (tid == 0) *cnt = 0; return; }
    rh_box32 G;
    {
        const float *b = (KIND == RH_PLANE ? A.st32_plane : A.st32) + st * 8;
        G.cx = b[0]; G.cy = b[1]; G.cz = b[2]; G.hx = b[3]; G.hy = b[4]; G.hz = b[5]; G.hr = b[6];
    }
    rh_u32x4 GM = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u };
    if (KIND == RH_PLANE && A.stm32 != nullptr) GM = ((const rh_u32x4 *)A.stm32)[st];
    uint16_t *__restrict__ list = A.stlist + (st * 4 + KIND) * A.stcap;
    constexpr int NB = S4Fields<KIND>::NBOX;
    const float *__restrict__ box = A.box[KIND];
    int base = 0, it = 0;
    for (int j0 = 0; j0 < nk; j0 += Q * 256, it++) {
        float B[Q][RH_BOX_FIELDS];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int cand = j0 + q * 256 + tid, cl = cand < nk ? cand : 0;
#pragma unroll
            for (int f = 0; f < NB; f++) B[q][f] = box[(int64_t)f * A.bstride + cl];
        }
        uint64_t m[Q];
        bool keep[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            keep[q] = j0 + q * 256 + tid < nk && !box_skip32<KIND>(B[q], G);
            if (KIND == RH_PLANE) keep[q] = keep[q] && nsig_meet(B[q], GM);   // (no group of the super-tile holds a normal the candidate accepts)
            m[q] = WB(keep[q]);
            if (lane == 0) wsum[it & 1][q * 4 + wv] = __popcll(m[q]);
        }
        __syncthreads();   // (the sums alternate between two rows: one barrier per round)
        int run = base;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            int off = run;
#pragma unroll
            for (int w = 0; w < 4; w++) { const int v = wsum[it & 1][q * 4 + w]; off += w < wv ? v : 0; run += v; }
            if (keep[q]) list[off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[q], 0))] = (uint16_t)(j0 + q * 256 + tid);
        }
        base = run;
    }
    if (tid == 0) *cnt = base;
}

__global__ void __launch_bounds__(256)
st_cull_kernel(const StCullArgs A)
{
    const int64_t st = blockIdx.x;
    switch (blockIdx.y) {
    case RH_PLANE: st_cull_kind<RH_PLANE>(A, st); break;
    case RH_SPHERE: st_cull_kind<RH_SPHERE>(A, st); break;
    case RH_CYLINDER: st_cull_kind<RH_CYLINDER>(A, st); break;
    default: st_cull_kind<RH_CONE>(A, st); break;
    }
}

}  // namespace

// "plane_order" (read on every launch; 0 = by size, 1 = whenever the cloud has the order, 2 = never): do plane candidates walk
// the plane order of subset 1?  By size: from RH_PLANE_ORDER_MIN_TILES tiles on.  The order removes plane pairs -- vector
// instructions -- and pays where the launch is bound by their issue, not where a small grid's time is set by its heaviest block
// and by launch latency (and a row with cylinders and planes stages its tile twice).  Measured (profiles/r13/experiments.txt,
// section 7; three batches in flight, the order forced on against forced off in one process): cfg2's 123 tiles +0.2 % (inside the
// sweep's range), cfg3's mix on 305 tiles -3.4 %, on 610 tiles -4.8 %, cfg3's 1221 tiles -3.5 %, cfg5's 6104 -2.6 %.  The rule sits
// between the largest size without a gain and the smallest with one.
#ifndef RH_PLANE_ORDER_MIN_TILES
#define RH_PLANE_ORDER_MIN_TILES 256
#endif
bool rhk_plane_order_wanted(const rh_cloud *c)
{
    if (c->pl_sub == nullptr) return false;
    const int64_t opt = rh_opt_int(c, RH_OPT_PLANE_ORDER, 0);
    return opt == 1 || (opt == 0 && (c->ngroups + S4_TG - 1) / S4_TG >= RH_PLANE_ORDER_MIN_TILES);
}

// the super-tile lists of the workspace's batch: [nst][4][cap] bin slots + [nst][4] counts
static inline int64_t stlist_bytes(const rh_cloud *c, int64_t cap) { return (int64_t)sizeof(uint16_t) * c->nst * 4 * cap; }
static int ensure_stlists(rh_cloud *c, rh_batch_ws &w, int64_t cap)
{
    if (w.d_stlist != nullptr && cap <= w.stlist_cap && w.stlist_nst == c->nst) return RH_OK;
    const int64_t ncap = std::max<int64_t>(cap, 1024);
    w.stlist_cap = 0;
    RH_TRY(w.d_stcount.grow(c->stream, c->nst * 4));
    RH_TRY(w.d_stlist.grow(c->stream, c->nst * 4 * ncap));
    w.stlist_cap = ncap;
    w.stlist_nst = c->nst;
    return RH_OK;
}

// the v4 launch: job.bins' cls[k] / box[k] = the classifier / culling records of bin prep[k], slot for slot, made for eps / cosa.
int rhk_score4_all(rh_cloud *c, rh_batch_ws &w, const rh_score_job &job, int32_t *launch_info)
{
    const rh_bins &B = job.bins;
    const int32_t nk_total_bound = job.bound;
    int32_t *const d_counts = job.d_counts;
    uint64_t *const d_masks_int = job.d_masks_int;
    const bool open_count = job.open_count;
    const bool f32cloud = c->f32;   // the exact tests in binary32, on float records derived from `prep`
    // the points: subset 1 in internal order, or the set rhk_score4_dis put in place (a segment of the disabled list)
    const bool on_subset = job.points.pts == nullptr;
    const rh_s4_points PS = on_subset ? rh_s4_points{ c->sub, c->s_pad, c->s, c->ngroups, c->gb32 } : job.points;
    const int64_t ntiles = (PS.ngroups + S4_TG - 1) / S4_TG;
    const int nchunks = cdiv4(nk_total_bound, 64) + 3;   // every bin may end in a partial chunk
    if (ntiles == 0 || nk_total_bound <= 0) return RH_OK;
    if (B.cls[0] == nullptr || B.box[0] == nullptr || !rh_score_v4_enabled(c) || PS.gb32 == nullptr || (d_masks_int != nullptr && !w.masks4)) {
        rh_set_error("internal: the culled score kernel without its records (classifier, culling, group boxes, mask lists)");
        return RH_E_INTERNAL;
    }
    const int dbg = (int)rh_opt_int(c, RH_OPT_G2_DBG, 0);   // (diag build only -- 1: no pair survives stage 1, the skeleton alone: tools/region_counters.sh)
    // "nsig" (read on every launch; 0 = on, 2 = off): plane pairs are also ruled out by the groups' normal-cell masks -- on subset 1,
    // whose masks the cloud holds; any other point set is walked by its boxes alone.  Counts and masks do not depend on it.
    const bool nsig_on = on_subset && c->gm32 != nullptr && rh_opt_int(c, RH_OPT_NSIG, 0) != 2;
    S4AllArgs A;
    for (int k = 0; k < 4; k++)
        A.k[k] = { (const rh_cls *)B.cls[k], B.box[k], B.prep[k], B.orig[k], job.nk[k], job.en[k], job.eps[k], job.cosa[k],
                   PS.pts, PS.stride, PS.gb32, nsig_on ? (const uint32_t *)c->gm32 : nullptr };
    // "plane_order" (rhk_plane_order_wanted: by size, always, never): the plane candidates of a counts-only launch on subset 1 walk the
    // cloud's plane order (kdorder.hip) -- the same points, inside every node of the position tree with at most 1024 points
    // grouped by their normals, so that a group's normal-cell mask holds 8 cells instead of 18 (cfg3) and a third fewer (plane,
    // group) pairs survive stage 1.  The culling rules are sound for ANY grouping of the points and a count is a sum over
    // points: the counts are the same, bit for bit.  The plane lists of the launch (st_cull_kernel) are cut by the boxes and
    // masks of the plane order's own super-tiles.  Mask launches keep the leaf order (their inlier words are numbered by it),
    // and so do the diag build's skeleton modes.  The enabled words: the cloud's plane-order twin of sub_enabled, or none.
    const bool plane_on = on_subset && d_masks_int == nullptr && dbg == 0 && rhk_plane_order_wanted(c) &&
                          (job.en[RH_PLANE] == nullptr || job.en[RH_PLANE] == c->sub_enabled.get());
    if (plane_on) {
        S4KindArgs &P = A.k[RH_PLANE];
        P.pts = c->pl_sub;
        P.gb32 = c->pl_gb32;
        if (nsig_on) P.gm32 = c->pl_gm32;
        if (P.en != nullptr) P.en = c->pl_enabled;
    }
    A.stop = job.stop;
    A.ntiles = ntiles;
    A.bstride = job.bstride;
    A.ngroups = PS.ngroups;
    A.masks = d_masks_int;
    A.occ = d_masks_int ? w.d_occ : nullptr;
    A.mstride = d_masks_int ? w.mstride4 : 0;
    A.stats = nullptr;
#ifdef RH_DIAG
    A.stats = c->s4_stats;  // (rh_dbg_s4_stats switched the counters on)
#endif
    // Super-tile lists (round 5): a candidate meets only ~13 / 3 / 10 % of the groups (plane / sphere / cylinder at cfg3), yet
    // every block of every tile walks ALL the candidates of its row through stage 1 -- loads of their culling records, four box
    // tests, the list bookkeeping: a third of the launch's issue cycles.  One small launch first tests every candidate against
    // the boxes of the SUPER-TILES (16 groups = 4 tiles: 1/16 of the tests) and leaves per super-tile and kind the list of
    // the candidates that may meet it (42 / 7 / 35 % of them at cfg3, 24 / 6 / 21 % at cfg5); the rows of a tile are then cut
    // from its super-tile's lists.  Same culling rule, so the same counts and masks: a candidate the super-tile's box rules out
    // has no inlier in any of its groups.  For launches whose candidate count the host knows, on subset 1.
    A.stlist = nullptr; A.stcount = nullptr; A.stcap = 0;
    const int64_t st_opt = rh_opt_int(c, RH_OPT_ST_CULL, 0);   // 0 = by size, 1 = whenever possible, 2 = never
    bool use_lists = !open_count && on_subset && dbg == 0 && c->st32 != nullptr && c->nst >= 2 && nk_total_bound <= 16384 && st_opt != 2;
    // By size (measured, cfg3's mix on 10M / 20M / 30M / cfg5's on 50M points = 1221 / 2442 / 3662 / 6104 tiles, a batch of 4096): the
    // lists cut the launch's instructions by a fifth, but its blocks become three times fewer and heavier, and a small grid then
    // ends in a long tail (and the list launch sits between the prepare and the score launch) -- one batch at a time +17 % / +0 % /
    // -8 % / -13 %; with two batches in flight, where the next batch fills the tail, -8 % / -15 % / -15 % / -24 %; cfg2's 123
    // tiles +50 % either way.
    if (use_lists && st_opt == 0)
        use_lists = nk_total_bound >= 1024 && ntiles >= (rh_opt_int(c, RH_OPT_BATCHES_IN_FLIGHT, 1) > 1 ? 1000 : 3000);
    // The lists are a workspace of 8 bytes per (super-tile, candidate of the batch's capacity) and batch slot: 10 MB at cfg3,
    // 50 MB at cfg5, but 3.2 GB for 16384 candidates on a subset of 25M points.  Budget: 512 MiB per slot ("st_list_mb" changes
    // it) -- it holds the largest batch (16384) on subsets up to 4M points and cfg5's cloud four times over, and the four slots
    // of the most batches in flight together stay below 1 % of the card's HBM.  Beyond the budget, or when the allocation
    // fails, the launch takes no lists: the plain instantiation computes the same counts (it ran every such launch before there
    // were lists), and a size that failed is not tried again.
    const int64_t lcap = std::max<int64_t>(((int64_t)nk_total_bound + 63) / 64 * 64, 1024);
    if (use_lists) {
        const int64_t mb = rh_opt_int(c, RH_OPT_ST_LIST_MB, 0);
        const int64_t need = stlist_bytes(c, lcap);
        if (need > ((mb > 0 ? mb : 512) << 20) || (w.stlist_nomem > 0 && need >= w.stlist_nomem)) use_lists = false;
    }
    if (use_lists) {
        const int rc = ensure_stlists(c, w, lcap);
        if (rc == RH_E_NOMEM) {
            (void)hipGetLastError();
            rh_set_error("%s", "");
            w.stlist_nomem = stlist_bytes(c, lcap);
            use_lists = false;
        } else if (rc != RH_OK) return rc;
    }
    if (use_lists) {
        StCullArgs SA;
        for (int k = 0; k < 4; k++) { SA.box[k] = B.box[k]; SA.nk[k] = job.nk[k]; }
        SA.bstride = job.bstride; SA.stcap = w.stlist_cap; SA.st32 = c->st32; SA.st32_plane = plane_on ? c->pl_st32 : c->st32;
        SA.stm32 = nsig_on && c->stm32 != nullptr ? (const uint32_t *)(plane_on ? c->pl_stm32 : c->stm32) : nullptr; SA.stlist = w.d_stlist; SA.stcount = w.d_stcount;
        hipLaunchKernelGGL(st_cull_kernel, dim3((unsigned)c->nst, 4), dim3(256), 0, c->stream, SA);
        A.stlist = w.d_stlist; A.stcount = w.d_stcount; A.stcap = w.stlist_cap;
        if (job.ev_listed != nullptr) RH_HIP(hipEventRecord(job.ev_listed, c->stream));
    }
    const int env_r = (int)rh_opt_int(c, RH_OPT_S4_ROWS, 0);   // rh_set_option(.., "s4_rows", ..), read on every launch: the fuzzers vary it from case to case
    // R = chunks of 64 candidates per block row.  A block's fixed work -- prologue, staging its tile, the four kinds' dispatch --
    // is a third of the launch's issue cycles at cfg3 and nearly half at cfg5 (profiles/r4/region_counters*.txt): longer rows pay
    // it less often, as long as the grid still has a few blocks per slot -- and as long as the HEAVIEST block does not set the
    // launch's time: on few tiles every candidate of a row meets the same dense tiles, and the time grows linearly with R
    // (round 5, cfg2's 123 tiles: R = 1 / 2 / 4 / 8 / 16 -> 0.0428 / 0.0432 / 0.0588 / 0.0898 / 0.158 ms; the same 123 tiles of a
    // sparse 1M-point scene 0.0383 / 0.0323 / 0.0334 / 0.0442; 367 tiles R = 2 / 4 / 8 / 12 -> 0.0589 / 0.0492 / 0.0576 / 0.0616;
    // cfg3's 1221 tiles 4 / 8 / 12 / 16 -> 0.0969 / 0.0866 / 0.0855 / 0.0873; cfg5's 6104 tiles 8 / 12 / 16 / 24 / 32 -> 0.367 / 0.330 /
    // 0.319 / 0.343 / 0.328).  Open-ended windows keep 4 / 8 (their tail launch walks the same rows).
    int R;
    if (env_r == 4 || env_r == 8 || ((env_r == 1 || env_r == 2 || env_r == 12 || env_r == 16) && !open_count)) R = env_r;
    else if (open_count) R = ntiles * ((nchunks + 7) / 8) < 3000 ? 4 : 8;
    else if (ntiles * ((nchunks + 15) / 16) >= 16384) R = 16;
    else if (ntiles * ((nchunks + 11) / 12) >= 3000) R = use_lists ? 16 : 12;   // (round 6, cfg3 with lists, three in flight, R = 8 / 12 / 16 -> 0.0668 / 0.0641 / 0.0629 ms)
    else if (ntiles * ((nchunks + 3) / 4) >= 4000) R = 4;
    else R = 2;
    int64_t rows = (nchunks + R - 1) / R;
    if (!open_count && launch_info != nullptr) { launch_info[0] = R; launch_info[1] = use_lists ? 1 : 0; launch_info[2] = (int32_t)rows; launch_info[3] = (int32_t)ntiles; }
    if (rows > 65535) { rh_set_error("batch of %d candidates is too large for one launch", nk_total_bound); return RH_E_INVALID; }
    // XCD-aware grid: the hardware deals consecutive block ids round-robin to the 8 XCDs, each with an L2 of its own; with grid.x
    // padded to a multiple of 8 a tile meets the same XCD in every row (only with >= 128 tiles per XCD: cfg2's 15 per XCD unbalance)
    const bool pad8 = ntiles >= 1024;
    dim3 grid((unsigned)(pad8 ? ((ntiles + 7) / 8) * 8 : ntiles), (unsigned)rows);
    const unsigned tiles_x = grid.x;   // the tail / loop launches keep the (tile, row) grid
    A.row0 = 0;
    A.rows = 0;
    // (measured, round 4: cfg2 -- 123 tiles x 17 rows -- 0.0753 -> 0.0663 ms; cfg3 -- 1221 x 9 -- 0.0927 -> 0.1041: with every row
    // in flight at once the record gathers of stage 2 spread over all 4096 candidates instead of a row's 512; cfg5 0.388
    // either way.  So: small launches only.)
#ifndef RH_S4_XROW_MAX
#define RH_S4_XROW_MAX 4096
#endif
    if (rows > 1 && ((ntiles + 7) / 8) * 8 * rows <= RH_S4_XROW_MAX) {
        A.rows = (int)rows;
        grid = dim3((unsigned)(((ntiles + 7) / 8) * 8 * rows), 1);
    }
    // the candidate loop's windows with few candidates (octree sampling: ~1000 local shapes per iteration, few pairs
    // survive the boxes): one block per tile walks ALL the rows -- the tile is staged once instead of once per row
    // (measured on the cfg3 octree leg, 18 chunks: 27 us against 39 + 7 for rows + tail; from ~40 chunks on the rows win:
    // sweep of the threshold 32 / 40 / 48 / 64 -> 0.0491 / 0.0498 / 0.0498 / 0.0499 s for the leg)
    const int loop_max = open_count ? 32 : 0;
    auto launch_tail = [&](unsigned ny) {   // the TAIL instantiations (open-ended windows: R = 4 / 8, no masks) on a (tile, ny) grid
        const dim3 gt(tiles_x, ny);
        if (f32cloud) {
            if (R == 4) hipLaunchKernelGGL((score4_kernel<4, false, true, true>), gt, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg);
            else hipLaunchKernelGGL((score4_kernel<8, false, true, true>), gt, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg);
        } else {
            if (R == 4) hipLaunchKernelGGL((score4_kernel<4, false, false, true>), gt, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg);
            else hipLaunchKernelGGL((score4_kernel<8, false, false, true>), gt, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg);
        }
    };
    if (loop_max > 0 && d_masks_int == nullptr && nchunks <= loop_max) {
        launch_tail(1);
        RH_HIP(hipGetLastError());
        return RH_OK;
    }
#define RH_S4_LAUNCH(RR, MM, FF)                                                                                                              \
    do {                                                                                                                                      \
        if (use_lists) hipLaunchKernelGGL((score4_kernel<RR, MM, FF, false, true>), grid, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg); \
        else hipLaunchKernelGGL((score4_kernel<RR, MM, FF>), grid, dim3(64 * S4_W), 0, c->stream, PS.s, A, d_counts, dbg);  \
    } while (0)
#define RH_S4_LAUNCH_R(MM, FF)                                                                                         \
    do {                                                                                                               \
        if (R == 4) RH_S4_LAUNCH(4, MM, FF);                                                                           \
        else if (R == 1) RH_S4_LAUNCH(1, MM, FF);                                                                      \
        else if (R == 2) RH_S4_LAUNCH(2, MM, FF);                                                                      \
        else if (R == 12) RH_S4_LAUNCH(12, MM, FF);                                                                    \
        else if (R == 16) RH_S4_LAUNCH(16, MM, FF);                                                                    \
        else RH_S4_LAUNCH(8, MM, FF);                                                                                  \
    } while (0)
    if (f32cloud) {   // Float32 cloud: c->sub (and the disabled list) hold the exactly converted values
        if (d_masks_int != nullptr) RH_S4_LAUNCH_R(true, true); else RH_S4_LAUNCH_R(false, true);
    } else if (d_masks_int != nullptr) RH_S4_LAUNCH_R(true, false);
    else RH_S4_LAUNCH_R(false, false);
#undef RH_S4_LAUNCH_R
#undef RH_S4_LAUNCH
    if (open_count) {
        // nk_total_bound was a guess (a window of the candidate loop is queued before its list length is known): whatever
        // lies beyond the rows above is scored by a second, small launch that walks the remaining rows grid-stride --
        // its blocks return at once when there is nothing (the usual case)
        if (d_masks_int != nullptr) { rh_set_error("rhk_score4_all: masks need an exact candidate count"); return RH_E_INTERNAL; }
        A.row0 = (int)rows;
        launch_tail(2);
    }
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// the prepared candidates of a device store (driver.hip) -> classifier + culling records for the v4 kernel, made on the
// fly for a liveness pass: index space = the kinds laid end to end from pbase[q] on, fields of the culling records bstride apart
namespace {
__global__ void __launch_bounds__(256)
store_cls_kernel(const rh_prep *p0, const rh_prep *p1, const rh_prep *p2, const rh_prep *p3, int32_t n0, int32_t n1, int32_t n2, int32_t n3,
                 int32_t b1, int32_t b2, int32_t b3, int32_t total, double e0, double e1, double e2, double e3, double c0, double c1, double c2,
                 double c3, double M, double Nm, double Ln, rh_cls *__restrict__ cls, float *__restrict__ box, int64_t bstride)
{
    const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int q = (g >= b1 ? 1 : 0) + (g >= b2 ? 1 : 0) + (g >= b3 ? 1 : 0);
    const int32_t slot = g - (q == 0 ? 0 : (q == 1 ? b1 : (q == 2 ? b2 : b3)));
    const int32_t n = q == 0 ? n0 : (q == 1 ? n1 : (q == 2 ? n2 : n3));
    if (slot >= n) return;
    const rh_prep *pp = q == 0 ? p0 : (q == 1 ? p1 : (q == 2 ? p2 : p3));
    const double eps = q == 0 ? e0 : (q == 1 ? e1 : (q == 2 ? e2 : e3)), cosa = q == 0 ? c0 : (q == 1 ? c1 : (q == 2 ? c2 : c3));
    const rh_prep P = pp[slot];
    cls_make(P, q, eps, cosa, M, Nm, cls[g], box + g, bstride, nullptr, false, Ln);
}
}  // namespace

int rhk_store_cls(rh_cloud *c, const rh_prep *const prep[4], const int32_t n[4], const int32_t pbase[5], const double eps[4],
                  const double cosa[4], void *d_cls, float *d_box, int64_t bstride)
{
    if (pbase[4] <= 0) return RH_OK;
    hipLaunchKernelGGL(store_cls_kernel, dim3((unsigned)cdiv4(pbase[4], 256)), dim3(256), 0, c->stream, prep[0], prep[1], prep[2], prep[3], n[0], n[1],
                       n[2], n[3], pbase[1], pbase[2], pbase[3], pbase[4], eps[0], eps[1], eps[2], eps[3], cosa[0], cosa[1], cosa[2], cosa[3],
                       c->coord_mag, c->nrm_mag, c->nrm_len, (rh_cls *)d_cls, d_box, bstride);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// the v4 kernel on cnt points of the disabled list from `first` on (every one counts: the job comes without enabled words)
int rhk_score4_dis(rh_cloud *c, int64_t first, int64_t cnt, rh_score_job job)
{
    if (cnt <= 0 || job.bound <= 0) return RH_OK;
    const int64_t ng = (cnt + 63) / 64;
    if (ng > c->ng_pad) { rh_set_error("rhk_score4_dis: %lld groups", (long long)ng); return RH_E_INTERNAL; }
    RH_TRY(rhk_group_bounds_of(c, c->dis + first, c->dis_stride, cnt, ng, c->dis_gb, c->ng_pad));
    rhk_gb32_of(c, c->dis_gb, ng, c->dis_gb32);
    RH_HIP(hipGetLastError());
    job.points = { c->dis + first, c->dis_stride, cnt, ng, c->dis_gb32 };
    return rhk_score4_all(c, c->ws[0], job);   // (no lists over another set than subset 1: w is not touched)
}
