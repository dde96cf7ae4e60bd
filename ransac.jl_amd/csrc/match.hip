// match.hip -- nearest descriptor of every query row among the reference rows (rh_match_features; include/ransac_hip.h
// states the definition).  All-pairs integer work, n * m * 33 multiply-adds:
//   1. match_pack_kernel: a row of 33 uint16 becomes MT_ROW_WORDS = 20 dwords -- 17 hold two values each (the 34th is 0),
//      three pad the row to 80 bytes so that a row is five 16-byte LDS reads.  A value above RH_DESC_MAX raises a flag
//      the host reads before anything is searched;
//   2. match_kernel: one query per lane, its 17 packed dwords in registers.  A block's share of the reference streams
//      through LDS in tiles of MT_TILE rows; every lane reads the same row at the same time (a wave-wide broadcast, no
//      bank conflict), subtracts packed (v_pk_sub_i16: |q - r| <= 7938 fits 16 bits) and accumulates with the 16-bit
//      dot product (v_dot2_i32_i16): 17 + 17 vector instructions per pair, plus the compare and two selects.  The sum
//      is at most 33 * 7938^2 = 2 079 390 852 < 2^31, exact in the 32-bit accumulator.  Rows come in ascending index, so
//      a strict `<` keeps the smaller index on a tie.  grid.y cuts the reference into chunks when the queries alone do
//      not fill the device; a block folds its best into the query's 64-bit key (distance << 32 | 1-based index) with an
//      integer atomicMin, whose result does not depend on the order;
//   3. with RH_MATCH_MUTUAL the same kernel runs with the roles exchanged; match_finish_kernel unpacks the keys and
//      zeroes the entries whose partner prefers another query.
// An f32 MFMA form of |q|^2 + |r|^2 - 2 q.r is exact only below 2^24, which this range exceeds: not taken.
#include "call_scope.h"

namespace {

constexpr int MT_ROW_WORDS = 20;         // dwords per packed row: 17 used, 80 bytes
constexpr int MT_PAIRS = 17;
constexpr int MT_TILE = 256;             // reference rows per LDS tile: 20 KiB
constexpr int MT_BLOCK = 256;            // queries per block
constexpr int MT_MIN_BLOCKS = 1024;      // the reference is cut until the grid has about this many blocks

typedef short mt_short2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void match_pack_kernel(const uint16_t *__restrict__ desc, int64_t rows, uint32_t *__restrict__ packed,
                                                         int32_t *__restrict__ bad)
{
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= rows * MT_ROW_WORDS) return;
    const int64_t i = at / MT_ROW_WORDS;
    const int wd = (int)(at - i * MT_ROW_WORDS);
    uint32_t lo = 0, hi = 0;
    if (2 * wd < RH_DESC_DIM) lo = desc[i * RH_DESC_DIM + 2 * wd];
    if (2 * wd + 1 < RH_DESC_DIM) hi = desc[i * RH_DESC_DIM + 2 * wd + 1];
    if (lo > RH_DESC_MAX || hi > RH_DESC_MAX) atomicOr(bad, 1);
    packed[at] = lo | (hi << 16);
}

__device__ __forceinline__ int match_acc(uint32_t q, uint32_t r, int acc)
{
    const mt_short2 d = __builtin_bit_cast(mt_short2, q) - __builtin_bit_cast(mt_short2, r);
    return __builtin_amdgcn_sdot2(d, d, acc, false);
}

// best[j] = min(best[j], key of the nearest of rows [blockIdx.y * chunk, .. + chunk) of r to row j of q)
__global__ __launch_bounds__(MT_BLOCK) void match_kernel(const uint32_t *__restrict__ q, int64_t m, const uint32_t *__restrict__ r,
                                                         int64_t n, int64_t chunk, unsigned long long *__restrict__ best)
{
    __shared__ uint4 tile[MT_TILE * (MT_ROW_WORDS / 4)];
    const int64_t j = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
    uint32_t qv[MT_PAIRS];
    for (int c = 0; c < MT_PAIRS; c++) qv[c] = j < m ? q[j * MT_ROW_WORDS + c] : 0u;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
    uint32_t bd = 0xFFFFFFFFu, bi = 0;
    for (int64_t base = r0; base < r1; base += MT_TILE) {
        const int cnt = (int)(r1 - base < MT_TILE ? r1 - base : MT_TILE);
        __syncthreads();                                          // the previous tile has been read by every wave
        const uint4 *src = (const uint4 *)(r + base * MT_ROW_WORDS);
        for (int t = threadIdx.x; t < cnt * (MT_ROW_WORDS / 4); t += MT_BLOCK) tile[t] = src[t];
        __syncthreads();
#pragma unroll 2
        for (int row = 0; row < cnt; row++) {
            const uint4 a = tile[row * 5], b = tile[row * 5 + 1], c = tile[row * 5 + 2], d = tile[row * 5 + 3];
            const uint32_t e = ((const uint32_t *)tile)[row * MT_ROW_WORDS + 16];
            int acc = 0;
            acc = match_acc(qv[0], a.x, acc); acc = match_acc(qv[1], a.y, acc); acc = match_acc(qv[2], a.z, acc); acc = match_acc(qv[3], a.w, acc);
            acc = match_acc(qv[4], b.x, acc); acc = match_acc(qv[5], b.y, acc); acc = match_acc(qv[6], b.z, acc); acc = match_acc(qv[7], b.w, acc);
            acc = match_acc(qv[8], c.x, acc); acc = match_acc(qv[9], c.y, acc); acc = match_acc(qv[10], c.z, acc); acc = match_acc(qv[11], c.w, acc);
            acc = match_acc(qv[12], d.x, acc); acc = match_acc(qv[13], d.y, acc); acc = match_acc(qv[14], d.z, acc); acc = match_acc(qv[15], d.w, acc);
            acc = match_acc(qv[16], e, acc);
            if ((uint32_t)acc < bd) { bd = (uint32_t)acc; bi = (uint32_t)(base + row) + 1u; }
        }
    }
    if (j < m && bi != 0u) atomicMin(&best[j], ((unsigned long long)bd << 32) | bi);
}

// idx / dist of every query from its key; mutual: 0 where the partner's own best is another query
__global__ __launch_bounds__(256) void match_finish_kernel(const unsigned long long *__restrict__ best_q, int64_t m,
                                                           const unsigned long long *__restrict__ best_r_or_null, int64_t n,
                                                           int32_t *__restrict__ idx, uint32_t *__restrict__ dist)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const unsigned long long key = best_q[j];
    int64_t i = (int64_t)(key & 0xFFFFFFFFull);
    if (i < 1 || i > n) i = 0;                                     // (cannot happen: n >= 1 and every distance is below 2^32 - 1)
    if (dist) dist[j] = (uint32_t)(key >> 32);
    if (i && best_r_or_null && (int64_t)(best_r_or_null[i - 1] & 0xFFFFFFFFull) != j + 1) i = 0;
    idx[j] = (int32_t)i;
}

int match_launch(CallScope &S, const uint32_t *q, int64_t m, const uint32_t *r, int64_t n, unsigned long long *best)
{
    SCOPE_HIP(S, hipMemsetAsync(best, 0xFF, sizeof(unsigned long long) * (size_t)m, S.st));
    const int64_t bx = (m + MT_BLOCK - 1) / MT_BLOCK, tiles = (n + MT_TILE - 1) / MT_TILE;
    int64_t by = std::min<int64_t>(std::min<int64_t>(tiles, (MT_MIN_BLOCKS + bx - 1) / bx), 65535);
    const int64_t chunk = ((tiles + by - 1) / by) * MT_TILE;       // whole tiles per chunk
    by = (n + chunk - 1) / chunk;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)bx, (unsigned)by), dim3(MT_BLOCK), 0, S.st, q, m, r, n, chunk, best);
    SCOPE_HIP(S, hipGetLastError());
    return RH_OK;
}

}  // namespace

extern "C" int rh_match_features(const uint16_t *ref_desc, int64_t n, const uint16_t *qry_desc, int64_t m, int32_t flags, int device,
                                 int32_t *idx_out, uint32_t *dist_out_or_null)
{
    static const char who[] = "rh_match_features";
    if (!ref_desc || !qry_desc || !idx_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    const int64_t lim = (int64_t)0x7FFFFFFF / (MT_ROW_WORDS * 4);
    if (n < 1 || n > lim || m < 1 || m > lim) {
        rh_set_error("%s: n = %lld, m = %lld outside 1 .. %lld", who, (long long)n, (long long)m, (long long)lim);
        return RH_E_INVALID;
    }
    if (flags & ~RH_MATCH_MUTUAL) { rh_set_error("%s: unknown flags %d", who, flags); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    uint16_t *d_in = nullptr;
    uint32_t *d_r = nullptr, *d_q = nullptr, *d_dist = nullptr;
    int32_t *d_bad = nullptr, *d_idx = nullptr;
    unsigned long long *d_bq = nullptr, *d_br = nullptr;
    RH_TRY(S.alloc(&d_in, std::max(n, m) * RH_DESC_DIM));
    RH_TRY(S.alloc(&d_r, n * MT_ROW_WORDS));
    RH_TRY(S.alloc(&d_q, m * MT_ROW_WORDS));
    RH_TRY(S.alloc(&d_bad, 1));
    SCOPE_HIP(S, hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
    SCOPE_HIP(S, hipMemcpyAsync(d_in, ref_desc, sizeof(uint16_t) * (size_t)n * RH_DESC_DIM, hipMemcpyDefault, st));
    hipLaunchKernelGGL(match_pack_kernel, dim3(blocks_for(n * MT_ROW_WORDS)), dim3(256), 0, st, d_in, n, d_r, d_bad);
    SCOPE_HIP(S, hipMemcpyAsync(d_in, qry_desc, sizeof(uint16_t) * (size_t)m * RH_DESC_DIM, hipMemcpyDefault, st));
    hipLaunchKernelGGL(match_pack_kernel, dim3(blocks_for(m * MT_ROW_WORDS)), dim3(256), 0, st, d_in, m, d_q, d_bad);
    SCOPE_HIP(S, hipGetLastError());
    int32_t bad = 0;
    RH_TRY(S.fetch(&bad, d_bad));
    if (bad) { rh_set_error("%s: a descriptor value is above %d", who, RH_DESC_MAX); return RH_E_INVALID; }
    RH_TRY(S.alloc(&d_bq, m));
    RH_TRY(S.alloc(&d_idx, m));
    if (dist_out_or_null) RH_TRY(S.alloc(&d_dist, m));
    RH_TRY(match_launch(S, d_q, m, d_r, n, d_bq));
    if (flags & RH_MATCH_MUTUAL) {
        RH_TRY(S.alloc(&d_br, n));
        RH_TRY(match_launch(S, d_r, n, d_q, m, d_br));
    }
    hipLaunchKernelGGL(match_finish_kernel, dim3(blocks_for(m)), dim3(256), 0, st, d_bq, m, d_br, n, d_idx, d_dist);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(idx_out, d_idx, sizeof(int32_t) * (size_t)m, hipMemcpyDefault, st));
    if (dist_out_or_null) SCOPE_HIP(S, hipMemcpyAsync(dist_out_or_null, d_dist, sizeof(uint32_t) * (size_t)m, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}
