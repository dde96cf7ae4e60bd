// kdorder.hip -- the internal order of subset 1 on the device: the leaves of a balanced k-d tree, 64 points each, which is
// what gives the culled score kernel its compact groups (cloud.hip builds the same tree on host threads -- std::nth_element
// recursion, 70 ms at 312 500 points, 300 ms at 1.56 M -- and keeps that form behind RH_KD_HOST=1 as the A/B).
//
// The tree's SHAPE depends on the point count alone (a node of cnt > 64 points gives its left child kd_left_count(cnt, aligned)
// of them: rh_internal.h), so the host lays the levels out and the device only orders: per level
//   1. the bounding box of every node that still splits (finite coordinates only; wave-uniform fast path + atomics),
//   2. a 64-bit key per position -- node number << 32 | the point's coordinate along the node's widest axis as an ordered
//      32-bit pattern (binary32 of the coordinate: NaN last, like the host's comparator) -- positions of finished nodes
//      keep their place,
//   3. one stable radix sort of (key, point) pairs over the whole subset (hipCUB): inside a node the points are then
//      ascending along its axis, and the node's children are simply its left and right part.
// log2(s / 64) levels of about 0.1-0.3 ms.  The order differs from the host's in ties and where two coordinates share
// a binary32 value -- any order gives the same counts and masks (they are un-permuted on the way out; every parity test
// holds whatever the order), only the boxes' tightness is at stake, and that is measured.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "rh_internal.h"
#ifdef RH_DIAG
#include "ransac_hip_diag.h"
#endif

namespace {

inline unsigned cdivq(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__device__ __forceinline__ uint32_t ord32(float v)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;   // NaN sorts last
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unord32(uint32_t u)
{
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __builtin_bit_cast(float, b);
}

// subset position j -> its coordinates as three float planes; max |coordinate| and max |normal component| over the finite
// values of the subset (the margins of the binary32 classifier and the slack of the box tests scale with them) as the bit
// patterns of non-negative doubles (they order like the doubles)
__global__ void __launch_bounds__(256)
kd_gather_kernel(const double *__restrict__ xyz, const double *__restrict__ nrm, const int32_t *__restrict__ idx0, int64_t s,
                 float *__restrict__ px, float *__restrict__ py, float *__restrict__ pz, int32_t *__restrict__ ord,
                 unsigned long long *__restrict__ mags)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double cm = 0.0, nm = 0.0;
    if (j < s) {
        const int64_t i = idx0[j];
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        px[j] = (float)x; py[j] = (float)y; pz[j] = (float)z;
        ord[j] = (int32_t)j;
        const double v[6] = { x, y, z, nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2] };
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double a = fabs(v[k]);
            if (a - a == 0) { if (k < 3) cm = a > cm ? a : cm; else nm = a > nm ? a : nm; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oc = __shfl_xor(cm, off), on = __shfl_xor(nm, off);
        cm = oc > cm ? oc : cm;
        nm = on > nm ? on : nm;
    }
    if ((threadIdx.x & 63) == 0) {
        if (cm > 0) atomicMax(&mags[0], __builtin_bit_cast(unsigned long long, cm));
        if (nm > 0) atomicMax(&mags[1], __builtin_bit_cast(unsigned long long, nm));
    }
}

// the segment (node of the current level) of position i: last k with seg_lo[k] <= i
__device__ __forceinline__ int seg_of(const int32_t *__restrict__ seg_lo, int nseg, int32_t i)
{
    int lo = 0, hi = nseg;   // seg_lo[0] = 0 <= i < seg_lo[nseg] = s
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_lo[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// box[seg * 6 + {0,1,2}] = min, {3,4,5} = max of the ordered patterns of the finite coordinates (init: 0xffffffff / 0)
__global__ void __launch_bounds__(256)
kd_box_kernel(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz, const int32_t *__restrict__ ord,
              int64_t s, const int32_t *__restrict__ seg_lo, const uint8_t *__restrict__ seg_active, int nseg, uint32_t *__restrict__ box)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < s;
    const int seg = in ? seg_of(seg_lo, nseg, (int32_t)i) : -1;
    const bool act = in && seg_active[seg] != 0;
    uint32_t mn[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, mx[3] = { 0u, 0u, 0u };
    if (act) {
        const int32_t j = ord[i];
        const float v[3] = { px[j], py[j], pz[j] };
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (v[k] - v[k] == 0.0f) { mn[k] = mx[k] = ord32(v[k]); }
    }
    // (the wave's positions are consecutive: in the upper levels they all belong to one node)
    const int seg0 = __shfl(seg, 0);
    const bool uniform = __builtin_amdgcn_ballot_w64(seg != seg0) == 0;
    if (uniform) {
        if (seg0 < 0 || !__shfl((int)act, 0)) return;
#pragma unroll
        for (int k = 0; k < 3; k++)
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t a = __shfl_xor(mn[k], off), b = __shfl_xor(mx[k], off);
                mn[k] = a < mn[k] ? a : mn[k];
                mx[k] = b > mx[k] ? b : mx[k];
            }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) { atomicMin(&box[seg0 * 6 + k], mn[k]); atomicMax(&box[seg0 * 6 + 3 + k], mx[k]); }
        }
    } else if (act) {
#pragma unroll
        for (int k = 0; k < 3; k++) { atomicMin(&box[seg * 6 + k], mn[k]); atomicMax(&box[seg * 6 + 3 + k], mx[k]); }
    }
}

__global__ void __launch_bounds__(256)
kd_key_kernel(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz, const int32_t *__restrict__ ord,
              int64_t s, const int32_t *__restrict__ seg_lo, const uint8_t *__restrict__ seg_active, int nseg,
              const uint32_t *__restrict__ box, uint64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s) return;
    const int seg = seg_of(seg_lo, nseg, (int32_t)i);
    uint32_t sub = (uint32_t)i;   // a finished node: the position itself (ascending inside the node, like before)
    if (seg_active[seg] != 0) {
        // widest axis of the node's box (the first of equally wide ones, like the host's `e > best`); an axis without a
        // finite coordinate has extent -1
        int ax = 0;
        float best = -2.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t lo = box[seg * 6 + k], hi = box[seg * 6 + 3 + k];
            const float e = lo <= hi ? unord32(hi) - unord32(lo) : -1.0f;
            if (e > best) { best = e; ax = k; }
        }
        const int32_t j = ord[i];
        sub = ord32(ax == 0 ? px[j] : (ax == 1 ? py[j] : pz[j]));
    }
    keys[i] = ((uint64_t)(uint32_t)seg << 32) | sub;
}

__global__ void kd_fill_box_kernel(uint32_t *__restrict__ box, int nseg)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nseg * 6) box[t] = (t % 6) < 3 ? 0xffffffffu : 0u;
}

// sub_perm[i] = subset position of internal position i; sub_idx0[i] = its 0-based index in the cloud
__global__ void kd_finish_kernel(const int32_t *__restrict__ ord, const int32_t *__restrict__ idx0, int64_t s,
                                 int32_t *__restrict__ sub_perm, int32_t *__restrict__ sub_idx0)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s) return;
    const int32_t j = ord[i];
    sub_perm[i] = j;
    sub_idx0[i] = idx0[j];
}

struct KdNode { int32_t lo, hi; };

// The position tree of s points from [0, s) down (kd_left_count, rh_internal.h), depth first, the left child first: node(lo, hi, 0)
// for every node of at most `most` points -- they come in position order and the walk does not descend below them --
// node(lo, hi, mid) for every larger one, split at mid.
template <class F>
void kd_walk(int64_t s, bool aligned, int64_t most, F node)
{
    struct Range { int64_t lo, hi; };
    std::vector<Range> stack(1, Range{ 0, s });
    while (!stack.empty()) {
        const Range nd = stack.back();
        stack.pop_back();
        const int64_t cnt = nd.hi - nd.lo;
        if (cnt <= most) { node(nd.lo, nd.hi, (int64_t)0); continue; }
        const int64_t mid = nd.lo + kd_left_count(cnt, aligned);
        node(nd.lo, nd.hi, mid);
        stack.push_back(Range{ mid, nd.hi });
        stack.push_back(Range{ nd.lo, mid });
    }
}

// ---- the plane order of subset 1 (score4.hip walks it with plane candidates).  The position tree is
// stopped at its nodes of at most PO_ST = 1024 points (whole groups: every split is at a multiple of 64).  With the tree's
// aligned shape (kd_left_count, rh_internal.h: cfg3) those nodes ARE the runs of 1024 consecutive points that the candidate
// lists call super-tiles; with today's shape they are not (576 .. 640 points at cfg3 then, and a run of 1024 straddles two or
// three of them: cutting such a run by normals leaves boxes half as large again, tools/proto/plane_order_proto.py).
// Inside every such node the SAME points, ordered by a k-d tree on their NORMALS: widest axis of the node's finite normals,
// median split, the left child a multiple of 64 like the position tree's, down to 64-point groups (four levels).  A node is
// small enough for one block: the normals in LDS, per level the nodes' boxes by atomics and one bitonic sort of 1024 keys
//     node << 42 | ordered binary32 pattern of the normal along the node's axis << 10 | leaf-order position in the block.
// The keys are distinct, so the order is a function of the normals alone: no ties, no dependence on the schedule.  A NaN
// component sorts last, an axis without a finite value is never the widest; where such a point lands is of no consequence
// (every grouping of the points gives the same counts).  Positions behind the block's end take the last node number and keep
// their place.
constexpr int PO_ST = (int)RH_KD_NODE;
constexpr int PO_THREADS = 512;

__global__ void __launch_bounds__(PO_THREADS)
plane_order_kernel(const double *__restrict__ sub, int64_t stride, const int32_t *__restrict__ blk_lo, int32_t *__restrict__ src)
{
    __shared__ float nv[3][PO_ST];
    __shared__ uint64_t key[PO_ST];
    __shared__ uint16_t ord[PO_ST];     // position in the plane order -> leaf-order position, both inside the block
    __shared__ uint32_t box[16][6];
    __shared__ int nlo[2][18];          // node starts of the level (alternating rows), closed by the point count
    __shared__ int nnode[2];
    const int tid = threadIdx.x;
    const int64_t base = blk_lo[blockIdx.x];
    const int cnt = (int)(blk_lo[blockIdx.x + 1] - base);   // (1 .. PO_ST: rhk_plane_order_build)
    for (int i = tid; i < PO_ST; i += PO_THREADS) {
        const bool in = i < cnt;
#pragma unroll
        for (int k = 0; k < 3; k++) nv[k][i] = in ? (float)sub[(3 + k) * stride + base + i] : 0.0f;
        ord[i] = (uint16_t)i;
    }
    if (tid == 0) { nlo[0][0] = 0; nlo[0][1] = cnt; nnode[0] = 1; }
    __syncthreads();
    for (int level = 0; level < 4; level++) {
        const int *lo = nlo[level & 1];
        const int nn = nnode[level & 1];
        for (int t = tid; t < 16 * 6; t += PO_THREADS) box[t / 6][t % 6] = (t % 6) < 3 ? 0xffffffffu : 0u;
        __syncthreads();
        auto node_of = [&](int i) { int nd = 0; for (int k = 1; k < nn; k++) nd += lo[k] <= i ? 1 : 0; return nd; };
        for (int i = tid; i < cnt; i += PO_THREADS) {
            const int nd = node_of(i);
            if (lo[nd + 1] - lo[nd] <= 64) continue;
            const int j = ord[i];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float v = nv[k][j];
                if (v - v == 0.0f) { atomicMin(&box[nd][k], ord32(v)); atomicMax(&box[nd][3 + k], ord32(v)); }
            }
        }
        __syncthreads();
        for (int i = tid; i < PO_ST; i += PO_THREADS) {
            const int j = ord[i];
            int nd = 31;
            uint32_t sk = (uint32_t)i;   // a finished node, the padding: the position itself
            if (i < cnt) {
                nd = node_of(i);
                if (lo[nd + 1] - lo[nd] > 64) {
                    int ax = 0;
                    float best = -2.0f;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const uint32_t bl = box[nd][k], bh = box[nd][3 + k];
                        const float e = bl <= bh ? unord32(bh) - unord32(bl) : -1.0f;
                        if (e > best) { best = e; ax = k; }
                    }
                    sk = ord32(nv[ax][j]);
                }
            }
            key[i] = ((uint64_t)nd << 42) | ((uint64_t)sk << 10) | (uint64_t)j;
        }
        __syncthreads();
        for (int k = 2; k <= PO_ST; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
                const uint64_t a = key[i], b = key[p];
                if ((a > b) == ((i & k) == 0)) { key[i] = b; key[p] = a; }
                __syncthreads();
            }
        for (int i = tid; i < PO_ST; i += PO_THREADS) ord[i] = (uint16_t)(key[i] & 1023u);
        if (tid == 0) {   // the next level's nodes: the children of those that split
            int *nx = nlo[(level + 1) & 1];
            int m = 0;
            for (int q = 0; q < nn; q++) {
                const int c0 = lo[q + 1] - lo[q];
                nx[m++] = lo[q];
                if (c0 > 64) nx[m++] = lo[q] + ((c0 / 64 + 1) / 2) * 64;   // (kd_left_count's rule for c0 <= 1024)
            }
            nx[m] = cnt;
            nnode[(level + 1) & 1] = m;
        }
        __syncthreads();
    }
    for (int i = tid; i < cnt; i += PO_THREADS) src[base + i] = (int32_t)base + ord[i];
}

// pl_sub = sub read through the table, plane by plane (positions from s on stay zero)
__global__ void __launch_bounds__(256)
plane_gather_kernel(const double *__restrict__ sub, int64_t stride, int64_t s, const int32_t *__restrict__ src, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s) return;
    const int64_t j = src[i];
#pragma unroll
    for (int k = 0; k < 6; k++) out[k * stride + i] = sub[k * stride + j];
}

// the enabled words in plane order: a wave per word, lane = point, the bit of the point's leaf-order position, one ballot
__global__ void __launch_bounds__(256)
plane_enabled_kernel(const uint64_t *__restrict__ sub_enabled, int64_t s, int64_t swords, const int32_t *__restrict__ src,
                     uint64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (i < s) {
        const int64_t j = src[i];
        bit = (sub_enabled[j >> 6] >> (j & 63)) & 1ULL;
    }
    const uint64_t w = __builtin_amdgcn_ballot_w64(bit);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < swords) out[i >> 6] = w;
}

// ---- findAABB (utilities.jl:125-136) of the uploaded cloud: per axis the smallest and the largest value that is not a NaN
// (infinities count, like in the host loop this replaces), and the largest finite magnitude.  Doubles as ordered 64-bit
// patterns; out[0..2] min (init all ones), out[3..5] max (init 0), out[6] the magnitude's bits (init 0).
__device__ __forceinline__ unsigned long long ord64(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__global__ void __launch_bounds__(256)
aabb_kernel(const double *__restrict__ xyz, int64_t n, unsigned long long *__restrict__ out)
{
    unsigned long long mn[3] = { ~0ULL, ~0ULL, ~0ULL }, mx[3] = { 0ULL, 0ULL, 0ULL };
    double mag = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double a = xyz[3 * i + k];
            if (a == a) {
                const unsigned long long o = ord64(a);
                mn[k] = o < mn[k] ? o : mn[k];
                mx[k] = o > mx[k] ? o : mx[k];
                const double m = fabs(a);
                if (m - m == 0 && m > mag) mag = m;
            }
        }
    }
    unsigned long long mb = __builtin_bit_cast(unsigned long long, mag);
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned long long a = __shfl_xor(mn[k], off), b = __shfl_xor(mx[k], off);
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
        const unsigned long long c = __shfl_xor(mb, off);
        mb = c > mb ? c : mb;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { atomicMin(&out[k], mn[k]); atomicMax(&out[3 + k], mx[k]); }
        atomicMax(&out[6], mb);
    }
}

}  // namespace

// lo / hi: per axis the extreme non-NaN values (lo > hi bit patterns: no such value), mag: largest finite |coordinate|
int rhk_cloud_aabb(rh_cloud *c, const double *d_xyz, int64_t n, double lo[3], double hi[3], bool has[3], double *mag)
{
    for (int k = 0; k < 3; k++) { lo[k] = hi[k] = 0; has[k] = false; }
    *mag = 0;
    if (n <= 0) return RH_OK;
    unsigned long long h[7];
    rh_dev<unsigned long long> d;
    RH_TRY(d.alloc(7));
    for (int k = 0; k < 7; k++) h[k] = k < 3 ? ~0ULL : 0ULL;
    RH_HIP(hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(aabb_kernel, dim3((unsigned)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0, c->stream, d_xyz, n, d.get());
    RH_HIP(hipGetLastError());
    RH_HIP(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    auto un = [](unsigned long long u) { const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffULL) : ~u; return __builtin_bit_cast(double, b); };
    for (int k = 0; k < 3; k++) {
        has[k] = h[k] <= h[3 + k];
        if (has[k]) { lo[k] = un(h[k]); hi[k] = un(h[3 + k]); }
    }
    *mag = __builtin_bit_cast(double, h[6]);
    return RH_OK;
}

// d_xyz / d_nrm: the cloud as uploaded (AoS, n x 3); d_idx0: subset position -> 0-based cloud index (s entries).  Fills
// c->sub_perm, c->sub_idx0, c->coord_mag, c->nrm_mag.  Synchronises the stream once (the two magnitudes come back).
int rhk_kd_order(rh_cloud *c, const double *d_xyz, const double *d_nrm, const int32_t *d_idx0)
{
    const int64_t s = c->s;
    if (s <= 0) return RH_OK;
    if (s > (int64_t)0x7fffffff) { rh_set_error("rhk_kd_order: subset of %lld points", (long long)s); return RH_E_INVALID; }
    rh_dev<float> pf;   // (temporaries of the call: gone on every way out)
    rh_dev<int32_t> ord[2], seg_lo;
    rh_dev<uint64_t> keys[2];
    rh_dev<uint32_t> box;
    rh_dev<uint8_t> seg_act;
    rh_dev<unsigned long long> mags;
    rh_dev<char> tmp;
    size_t tmp_bytes = 0;
    // the levels: every node of a level in position order, finished ones (<= 64 points) included
    std::vector<std::vector<KdNode>> levels;
    {
        std::vector<KdNode> cur(1, KdNode{ 0, (int32_t)s });
        for (;;) {
            bool any = false;
            for (const KdNode &nd : cur) any = any || nd.hi - nd.lo > 64;
            if (!any) break;
            levels.push_back(cur);
            std::vector<KdNode> nxt;
            nxt.reserve(cur.size() * 2);
            for (const KdNode &nd : cur) {
                const int32_t cnt = nd.hi - nd.lo;
                if (cnt <= 64) { nxt.push_back(nd); continue; }
                const int32_t nl = (int32_t)kd_left_count(cnt, c->kd_aligned);
                nxt.push_back(KdNode{ nd.lo, nd.lo + nl });
                nxt.push_back(KdNode{ nd.lo + nl, nd.hi });
            }
            cur.swap(nxt);
        }
    }
    size_t max_seg = 1;
    for (const auto &lv : levels) max_seg = std::max(max_seg, lv.size());
    RH_TRY(pf.alloc(3 * s));
    RH_TRY(ord[0].alloc(s));
    RH_TRY(ord[1].alloc(s));
    RH_TRY(keys[0].alloc(s));
    RH_TRY(keys[1].alloc(s));
    RH_TRY(box.alloc(6 * (int64_t)max_seg));
    RH_TRY(mags.alloc(2));
    RH_HIP(hipMemsetAsync(mags, 0, sizeof(unsigned long long) * 2, c->stream));
    float *px = pf, *py = pf + s, *pz = pf + 2 * s;
    const dim3 gs(cdivq(s, 256)), blk(256);
    hipLaunchKernelGGL(kd_gather_kernel, gs, blk, 0, c->stream, d_xyz, d_nrm, d_idx0, s, px, py, pz, ord[0], mags);
    RH_HIP(hipGetLastError());
    RH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys[0].get(), keys[1].get(), ord[0].get(), ord[1].get(), (int)s, 0, 64, c->stream));
    RH_TRY(tmp.alloc((int64_t)tmp_bytes));
    // every level's node starts / flags, uploaded once (pageable source: the arrays live until the final wait)
    std::vector<int32_t> h_lo;
    std::vector<uint8_t> h_act;
    std::vector<size_t> off_lo, off_act;
    for (const auto &lv : levels) {
        off_lo.push_back(h_lo.size());
        off_act.push_back(h_act.size());
        for (const KdNode &nd : lv) { h_lo.push_back(nd.lo); h_act.push_back(nd.hi - nd.lo > 64 ? 1 : 0); }
        h_lo.push_back((int32_t)s);
    }
    RH_TRY(seg_lo.alloc((int64_t)h_lo.size()));
    RH_TRY(seg_act.alloc((int64_t)h_act.size()));
    if (!h_lo.empty()) RH_HIP(hipMemcpyAsync(seg_lo, h_lo.data(), sizeof(int32_t) * h_lo.size(), hipMemcpyHostToDevice, c->stream));
    if (!h_act.empty()) RH_HIP(hipMemcpyAsync(seg_act, h_act.data(), h_act.size(), hipMemcpyHostToDevice, c->stream));
    int cur = 0;
    for (size_t L = 0; L < levels.size(); L++) {
        const int nseg = (int)levels[L].size();
        const int32_t *lo_l = seg_lo + off_lo[L];
        const uint8_t *act_l = seg_act + off_act[L];
        hipLaunchKernelGGL(kd_fill_box_kernel, dim3(cdivq((int64_t)nseg * 6, 256)), blk, 0, c->stream, box, nseg);
        hipLaunchKernelGGL(kd_box_kernel, gs, blk, 0, c->stream, px, py, pz, ord[cur], s, lo_l, act_l, nseg, box);
        hipLaunchKernelGGL(kd_key_kernel, gs, blk, 0, c->stream, px, py, pz, ord[cur], s, lo_l, act_l, nseg, box, keys[0]);
        RH_HIP(hipGetLastError());
        int seg_bits = 1;
        while ((1 << seg_bits) < nseg) seg_bits++;
        RH_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.get(), tmp_bytes, keys[0].get(), keys[1].get(), ord[cur].get(), ord[cur ^ 1].get(), (int)s, 0, 32 + seg_bits, c->stream));
        cur ^= 1;
    }
    hipLaunchKernelGGL(kd_finish_kernel, gs, blk, 0, c->stream, ord[cur], d_idx0, s, c->sub_perm, c->sub_idx0);
    RH_HIP(hipGetLastError());
    unsigned long long h_mags[2] = { 0, 0 };
    RH_HIP(hipMemcpyAsync(h_mags, mags, sizeof h_mags, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    c->coord_mag = __builtin_bit_cast(double, h_mags[0]);
    c->nrm_mag = __builtin_bit_cast(double, h_mags[1]);
    return RH_OK;
}

// The plane order of subset 1, once per cloud, behind the leaf order, the gather of c->sub and the groups' boxes: the table, the
// plane-order copy of the points, then the binary32 boxes and normal-cell masks of its groups and super-tiles (rhk_plane_boxes).
// Only for clouds the culled score kernel runs on; about 52 bytes per subset point.
int rhk_plane_order_build(rh_cloud *c)
{
    if (!c->use_groups || c->s <= 0 || c->nst <= 0) return RH_OK;
    if (c->s > (int64_t)0x7fffffff) { rh_set_error("rhk_plane_order_build: subset of %lld points", (long long)c->s); return RH_E_INVALID; }
    // the blocks: the nodes of the position tree (its shape depends on the point count alone: rhk_kd_order) with <= PO_ST points
    std::vector<int32_t> lo;
    kd_walk(c->s, c->kd_aligned, PO_ST, [&](int64_t a, int64_t, int64_t) { lo.push_back((int32_t)a); });
    lo.push_back((int32_t)c->s);
    const int64_t nblk = (int64_t)lo.size() - 1;
    rh_dev<int32_t> d_lo;   // (lives until rhk_plane_boxes has waited for the stream)
    RH_TRY(d_lo.alloc((int64_t)lo.size()));
    RH_HIP(hipMemcpyAsync(d_lo, lo.data(), sizeof(int32_t) * lo.size(), hipMemcpyHostToDevice, c->stream));
    RH_TRY(c->pl_sub.alloc(6 * c->s_pad));
    RH_TRY(c->pl_src.alloc(c->s_pad));
    RH_TRY(c->pl_st32.alloc(8 * c->nst));
    RH_TRY(c->pl_stm32.alloc(4 * c->nst));
    RH_TRY(c->pl_gb32.alloc(8 * c->ng_pad));
    RH_TRY(c->pl_gm32.alloc(4 * c->ng_pad));
    RH_TRY(c->pl_enabled.alloc(c->swords));
    RH_HIP(hipMemsetAsync(c->pl_sub, 0, sizeof(double) * 6 * (size_t)c->s_pad, c->stream));
    RH_HIP(hipMemsetAsync(c->pl_src, 0, sizeof(int32_t) * (size_t)c->s_pad, c->stream));
    hipLaunchKernelGGL(plane_order_kernel, dim3((unsigned)nblk), dim3(PO_THREADS), 0, c->stream, c->sub, c->s_pad, d_lo.get(), c->pl_src.get());
    hipLaunchKernelGGL(plane_gather_kernel, dim3(cdivq(c->s, 256)), dim3(256), 0, c->stream, c->sub, c->s_pad, c->s, c->pl_src.get(), c->pl_sub.get());
    RH_HIP(hipGetLastError());
    return rhk_plane_boxes(c);
}

int rhk_plane_enabled_sync(rh_cloud *c)
{
    if (c->pl_enabled == nullptr || c->s <= 0) return RH_OK;
    hipLaunchKernelGGL(plane_enabled_kernel, dim3(cdivq(c->swords * 64, 256)), dim3(256), 0, c->stream, c->sub_enabled, c->s, c->swords,
                       c->pl_src.get(), c->pl_enabled.get());
    RH_HIP(hipGetLastError());
    return RH_OK;
}

#ifdef RH_DIAG
// diagnostics (tests): the shape of the position tree of s points as kd_left_count makes it (ransac_hip_diag.h); no GPU
extern "C" int rh_dbg_kd_shape(int64_t s, int aligned, int64_t *info_out, int64_t *nodes_out, int64_t node_cap, int64_t *splits_out,
                               int64_t split_cap, int64_t *leaves_out, int64_t leaf_cap)
{
    if (info_out == nullptr || s < 1 || s > (int64_t)0x7fffffff || aligned < -1 || aligned > 1) { rh_set_error("rh_dbg_kd_shape: bad arguments"); return RH_E_INVALID; }
    const bool al = aligned < 0 ? kd_aligned_for(s, rh_opt_int(nullptr, RH_OPT_KD_ALIGN, 0)) : aligned != 0;
    int64_t nn = 0, ns = 0, nl = 0;
    kd_walk(s, al, RH_KD_NODE, [&](int64_t lo, int64_t hi, int64_t mid) {
        if (mid == 0) {
            if (nodes_out != nullptr && nn < node_cap) { nodes_out[2 * nn] = lo; nodes_out[2 * nn + 1] = hi; }
            nn++;
        } else {
            if (splits_out != nullptr && ns < split_cap) { splits_out[3 * ns] = lo; splits_out[3 * ns + 1] = mid; splits_out[3 * ns + 2] = hi; }
            ns++;
        }
    });
    if (leaves_out != nullptr)
        kd_walk(s, al, 64, [&](int64_t lo, int64_t hi, int64_t mid) {
            if (mid != 0) return;
            if (nl < leaf_cap) { leaves_out[2 * nl] = lo; leaves_out[2 * nl + 1] = hi; }
            nl++;
        });
    // the levels rhk_kd_order would run: the tree's height over its 64-point leaves, by the distinct node sizes of every level
    int64_t depth = 0;
    for (std::vector<int64_t> cur(1, s); ; depth++) {
        std::vector<int64_t> nxt;
        for (int64_t cnt : cur)
            if (cnt > 64) { const int64_t l = kd_left_count(cnt, al); nxt.push_back(l); nxt.push_back(cnt - l); }
        if (nxt.empty()) break;
        std::sort(nxt.begin(), nxt.end());
        nxt.erase(std::unique(nxt.begin(), nxt.end()), nxt.end());
        cur.swap(nxt);
    }
    info_out[0] = nn; info_out[1] = ns; info_out[2] = nl; info_out[3] = depth; info_out[4] = al ? 1 : 0;
    return RH_OK;
}

// the plane order as the cloud holds it, next to the leaf order it was made from (ransac_hip_diag.h)
extern "C" int rh_dbg_plane_order(rh_cloud *c, int64_t *info_out, double *sub_out, double *pl_out, int32_t *src_out, float *gb32_out,
                                  uint32_t *gm32_out, uint64_t *en_out)
{
    if (c == nullptr || info_out == nullptr) { rh_set_error("rh_dbg_plane_order: bad arguments"); return RH_E_INVALID; }
    const bool has = c->pl_sub != nullptr;
    info_out[0] = c->s; info_out[1] = c->ngroups; info_out[2] = c->nst; info_out[3] = has ? 1 : 0;
    if (!has || c->s <= 0) return RH_OK;
    RH_HIP(hipSetDevice(c->device));
    const size_t s = (size_t)c->s;
    for (int k = 0; k < 6; k++) {
        if (sub_out != nullptr) RH_HIP(hipMemcpyAsync(sub_out + k * s, c->sub + k * c->s_pad, sizeof(double) * s, hipMemcpyDeviceToHost, c->stream));
        if (pl_out != nullptr) RH_HIP(hipMemcpyAsync(pl_out + k * s, c->pl_sub + k * c->s_pad, sizeof(double) * s, hipMemcpyDeviceToHost, c->stream));
    }
    if (src_out != nullptr) RH_HIP(hipMemcpyAsync(src_out, c->pl_src, sizeof(int32_t) * s, hipMemcpyDeviceToHost, c->stream));
    if (gb32_out != nullptr) RH_HIP(hipMemcpyAsync(gb32_out, c->pl_gb32, sizeof(float) * 8 * (size_t)c->ngroups, hipMemcpyDeviceToHost, c->stream));
    if (gm32_out != nullptr) RH_HIP(hipMemcpyAsync(gm32_out, c->pl_gm32, sizeof(uint32_t) * 4 * (size_t)c->ngroups, hipMemcpyDeviceToHost, c->stream));
    if (en_out != nullptr) {
        RH_HIP(hipMemcpyAsync(en_out, c->sub_enabled, sizeof(uint64_t) * (size_t)c->swords, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipMemcpyAsync(en_out + c->swords, c->pl_enabled, sizeof(uint64_t) * (size_t)c->swords, hipMemcpyDeviceToHost, c->stream));
    }
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}
#endif
