// orient.hip -- consistent orientation of normals without a viewpoint (rh_orient_normals; include/ransac_hip.h states the
// definition in full): the sign is propagated along the minimum spanning forest of the neighbour graph under the total
// order (descending |ni.nj|, ascending i, ascending j).
//   emit     the shared search (knn_grid.h / knn_device.h, lists of k + 1 entries) with an epilogue of its own: lanes 1 .. k
//            of a wave write the directed pair (min << 32 | max) of every neighbour in V, ~0 otherwise.  A radix sort and
//            hipcub's Unique leave the E undirected edges in (i, j) order; the n x k lists never leave the device
//   rank     a and s per edge, then ONE stable radix sort by ~bits(a): the position of an edge in the result is its rank in
//            the total order (the sort is stable and its input is in (i, j) order).  From here on an edge is its rank, a
//            32-bit integer, and "the smallest edge of a component" is one 32-bit atomicMin
//   rounds   Boruvka on a parity union-find.  link[i] = root << 1 | parity to the root; at the start of a round every tree
//            is a star.
//              select  every live edge whose ends have different roots offers its rank to BOTH roots (atomicMin, one per
//                      distinct root of a wave: the live list is in ascending rank order, so the first lane of a root holds
//                      its smallest rank) and flags itself; hipcub's Flagged compacts the flagged ones into next round's
//                      live list (stable: the order stays)
//              hook    one thread per root c with an offer: the edge (u in c, v in d) links c under d with parity
//                      par(u) ^ s ^ par(v); on a mutual pick the smaller root stays.  Reads link, writes tmp: every hook
//                      sees the state of the round's start
//              jump    pointer doubling tmp -> link -> tmp -> link .. with parity ^= parity of the parent, until every
//                      vertex points at a root
//            The host loops on one small read-back per round; 31 rounds and 31 doublings at most, more is an error.
//   epilogue smallest index, size and (ANCHOR_TOP) topmost point per root, the numbering by a scan over the flags of the
//            smallest indices, the flips, one pass over the edges for n_inconsistent.
// Everything that crosses blocks crosses a kernel boundary; no kernel waits on another block.  No floating-point atomics:
// integer atomics on indices, counts and bit patterns only.
#include "knn_device.h"
#include "wave_keys.h"
#ifdef RH_DIAG
#include "ransac_hip_diag.h"
#endif

namespace {

constexpr uint32_t ORI_NONE = 0xFFFFFFFFu;
constexpr uint64_t ORI_NOPAIR = ~0ULL;
constexpr uint64_t ORI_SBIT = 1ULL << 63;       // s of an edge rides in bit 63 of its pair (i < 2^31)
constexpr int ORI_MAX_ROUNDS = 31, ORI_MAX_JUMPS = 31;

// the call's scalars on the device
struct OriScal {
    unsigned long long n_bad, n_vertices, n_flipped, n_incons, n_tree;
    unsigned long long min_abits;               // bit pattern of the smallest a over the forest (non-negative doubles order as integers)
    int32_t n_unique, n_edges, nlive, largest, m, pad;
    int32_t unfin[ORI_MAX_JUMPS + 1];           // unfin[t] != 0: after doubling t some vertex did not point at a root yet
};

__device__ __forceinline__ uint32_t pair_u(uint64_t key) { return (uint32_t)(key >> 32) & 0x7FFFFFFFu; }
__device__ __forceinline__ uint32_t pair_v(uint64_t key) { return (uint32_t)key; }

// V, and the components that are refused
__global__ void ori_check_kernel(const double *__restrict__ nrm, int64_t n, uint8_t *__restrict__ inv, OriScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, v = false;
    if (i < n) {
        const double x = nrm[3 * i], y = nrm[3 * i + 1], z = nrm[3 * i + 2];
        bad = !(isfinite(x) && isfinite(y) && isfinite(z)) || fabs(x) > 2.0 || fabs(y) > 2.0 || fabs(z) > 2.0;
        v = !bad && !(x == 0.0 && y == 0.0 && z == 0.0);
        inv[i] = v;
    }
    const uint64_t bb = __builtin_amdgcn_ballot_w64(bad), bv = __builtin_amdgcn_ballot_w64(v);
    if ((threadIdx.x & 63) == 0) {
        if (bb) atomicAdd(&sc->n_bad, (unsigned long long)__popcll(bb));
        if (bv) atomicAdd(&sc->n_vertices, (unsigned long long)__popcll(bv));
    }
}

// the search's epilogue: the directed pairs of wave w's point, kk per point
__global__ __launch_bounds__(NRM_BLOCK) void ori_emit_kernel(Grid g, KnnQuery kq, const uint8_t *__restrict__ inv,
                                                             uint64_t *__restrict__ pairs)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= kq.nq) return;                                       // wave-uniform
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, kq, lane, w, p, self, bd, br);
    if (self < 0 || (int64_t)self >= kq.n) return;                // (wave-uniform) nothing is addressed through a bad index
    const int kk = kq.k - 1;                                      // lane 0 is the point itself
    const double r2 = kq.radius * kq.radius;
    if (lane < 1 || lane > kk) return;
    const bool in = br != NRM_NORANK && br >= 1u && (kq.radius <= 0.0 || bd <= r2);
    const uint32_t j = br - 1u;                                   // rank = index + 1
    const bool edge = in && (int64_t)j < kq.n && j != (uint32_t)self && inv[self] != 0 && inv[j] != 0;
    const uint32_t lo = j < (uint32_t)self ? j : (uint32_t)self, hi = j < (uint32_t)self ? (uint32_t)self : j;
    pairs[(int64_t)self * kk + (lane - 1)] = edge ? ((uint64_t)lo << 32) | (uint64_t)hi : ORI_NOPAIR;
}

// E = the unique pairs without the ~0 that sorts last
__global__ void ori_count_kernel(const uint64_t *__restrict__ uniq, OriScal *sc)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t c = sc->n_unique;
    if (c > 0 && uniq[c - 1] == ORI_NOPAIR) c--;
    sc->n_edges = c;
}

// a and s of every edge: s into bit 63 of the pair, ~bits(a) as the key of the rank sort
__global__ void ori_weight_kernel(uint64_t *__restrict__ ekey, int64_t ne, int64_t n, const double *__restrict__ nrm,
                                  uint64_t *__restrict__ akey, uint32_t *__restrict__ eid)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const uint64_t key = ekey[e];
    const uint32_t i = pair_u(key), j = pair_v(key);
    double dot = 0.0;
    if ((int64_t)i < n && (int64_t)j < n) {
        const double *a = nrm + 3 * (int64_t)i, *b = nrm + 3 * (int64_t)j;
        dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    }
    ekey[e] = (key & ~ORI_SBIT) | (dot < 0.0 ? ORI_SBIT : 0ULL);
    akey[e] = ~(uint64_t)__double_as_longlong(fabs(dot));
    eid[e] = (uint32_t)e;
}

// the edges in rank order; every edge is live
__global__ void ori_rank_kernel(const uint64_t *__restrict__ ekey, const uint32_t *__restrict__ order, int64_t ne,
                                uint64_t *__restrict__ redge, uint32_t *__restrict__ live)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne) return;
    const uint32_t e = order[r];
    redge[r] = (int64_t)e < ne ? ekey[e] : 0ULL;
    live[r] = (uint32_t)r;
}

__global__ void ori_init_kernel(uint32_t *__restrict__ link, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) link[i] = (uint32_t)i << 1;
}

// one atomicMin per distinct root among the lanes with `act`: the lanes hold ascending ranks, so the first lane of a root
// holds the root's smallest
__device__ __forceinline__ void offer(bool act, uint32_t root, uint32_t rank, int lane, uint32_t *best)
{
    wave_each_key(act, root, [&](int leader, uint32_t R, uint64_t) {
        if (lane == leader) atomicMin(&best[R], rank);
    });
}

__global__ __launch_bounds__(256) void ori_select_kernel(const uint32_t *__restrict__ live, int64_t nlive, int64_t ne, int64_t n,
                                                         const uint64_t *__restrict__ redge, const uint32_t *__restrict__ link,
                                                         uint32_t *best, uint8_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool act = false;
    uint32_t r = ORI_NONE, ru = 0, rv = 0;
    if (t < nlive) {
        r = live[t];
        if ((int64_t)r < ne) {
            const uint64_t key = redge[r];
            const uint32_t u = pair_u(key), v = pair_v(key);
            if ((int64_t)u < n && (int64_t)v < n) {
                ru = link[u] >> 1; rv = link[v] >> 1;
                act = ru != rv && (int64_t)ru < n && (int64_t)rv < n;
            }
        }
        flag[t] = act;
    }
    offer(act, ru, r, lane, best);
    offer(act, rv, r, lane, best);
}

// link is the state of the round's start and is only read; tmp is the state with this round's hooks
__global__ __launch_bounds__(256) void ori_hook_kernel(const uint32_t *__restrict__ link, const uint32_t *__restrict__ best,
                                                       const uint64_t *__restrict__ redge, const uint64_t *__restrict__ akey_sorted,
                                                       int64_t n, int64_t ne, uint32_t *__restrict__ tmp, OriScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool hooked = false;
    unsigned long long ab = ~0ULL;
    if (i < n) {
        uint32_t out = link[i];
        const uint32_t b = best[i];
        if (b != ORI_NONE && (int64_t)b < ne && out == (uint32_t)i << 1) {
            const uint64_t key = redge[b];
            const uint32_t u = pair_u(key), v = pair_v(key);
            if ((int64_t)u < n && (int64_t)v < n) {
                const uint32_t lu = link[u], lv = link[v];
                const uint32_t d = (lu >> 1) == (uint32_t)i ? (lv >> 1) : (lu >> 1);
                const uint32_t par = (lu ^ lv ^ (uint32_t)(key >> 63)) & 1u;
                // a mutual pick of one edge: the smaller root stays
                const bool stay = (int64_t)d >= n || d == (uint32_t)i || (best[d] == b && (uint32_t)i < d);
                if (!stay) {
                    out = (d << 1) | par;
                    hooked = true;
                    ab = ~akey_sorted[b];
                }
            }
        }
        tmp[i] = out;
    }
    // the round's tree edges and the smallest a among them: one atomic each per wave
    const uint64_t bh = __builtin_amdgcn_ballot_w64(hooked);
    if (bh == 0) return;                                          // wave-uniform
    ab = wave_min_u64(ab);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sc->n_tree, (unsigned long long)__popcll(bh));
        atomicMin(&sc->min_abits, ab);
    }
}

__global__ void ori_jump_kernel(const uint32_t *__restrict__ cur, uint32_t *__restrict__ next, int64_t n, int32_t *unfin)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = cur[i];
    const uint32_t p = l >> 1;
    const uint32_t lp = (int64_t)p < n ? cur[p] : l;
    const uint32_t gp = lp >> 1;
    next[i] = (gp << 1) | ((l ^ lp) & 1u);
    if ((int64_t)gp < n && (cur[gp] >> 1) != gp) *unfin = 1;
}

// t of step 7: ((x*up.x + y*up.y) + z*up.z) + 0.0, a NaN counts as -inf
__device__ __forceinline__ uint64_t top_key(const double *__restrict__ xyz, int64_t i, const double up[3])
{
    double t = ((xyz[3 * i] * up[0] + xyz[3 * i + 1] * up[1]) + xyz[3 * i + 2] * up[2]) + 0.0;
    if (t != t) t = -INFINITY;
    return ord_of(t);
}

struct OriUp { double v[3]; };

// per root: the smallest index, the size and, with top, the largest t of its vertices -- one atomic each per distinct root of a wave
__global__ __launch_bounds__(256) void ori_comp_kernel(const uint32_t *__restrict__ link, const uint8_t *__restrict__ inv, int64_t n,
                                                       const double *__restrict__ xyz, int top, OriUp up, uint32_t *minidx,
                                                       int32_t *size, unsigned long long *pmax)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool act = i < n && inv[i] != 0;
    const uint32_t root = act ? link[i] >> 1 : 0u;
    const uint64_t tk = act && top ? top_key(xyz, i, up.v) : 0ULL;
    wave_each_key(act && (int64_t)root < n, root, [&](int leader, uint32_t R, uint64_t same) {
        unsigned long long m = (act && root == R) ? tk : 0ULL;
        if (top) m = wave_max_u64(m);
        if (lane == leader) {
            atomicMin(&minidx[R], (uint32_t)i);                   // (the lanes hold ascending i: the leader's is the smallest)
            atomicAdd(&size[R], (int32_t)__popcll(same));
            if (top) atomicMax(&pmax[R], m);
        }
    });
}

// ANCHOR_TOP: the smallest index that reaches its root's largest t (one atomicMin per distinct root of a wave)
__global__ __launch_bounds__(256) void ori_top_kernel(const uint32_t *__restrict__ link, const uint8_t *__restrict__ inv, int64_t n,
                                                      const double *__restrict__ xyz, OriUp up, const unsigned long long *__restrict__ pmax,
                                                      uint32_t *anchor)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t root = i < n && inv[i] ? link[i] >> 1 : ORI_NONE;
    const bool act = (int64_t)root < n && top_key(xyz, i, up.v) == pmax[root];
    offer(act, root, (uint32_t)i, threadIdx.x & 63, anchor);
}

// per root: the flag of its component's smallest index, the flip of its vertices of parity 0, the largest size
__global__ __launch_bounds__(256) void ori_root_kernel(const uint32_t *__restrict__ link, const uint8_t *__restrict__ inv, int64_t n,
                                                       const double *__restrict__ nrm, int top, OriUp up,
                                                       const uint32_t *__restrict__ minidx, const uint32_t *__restrict__ anchor,
                                                       const int32_t *__restrict__ size, int32_t *__restrict__ flag,
                                                       uint8_t *__restrict__ rootflip, OriScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool isroot = i < n && inv[i] != 0 && link[i] == (uint32_t)i << 1;
    unsigned long long sz = 0;
    if (isroot) {
        const uint32_t first = minidx[i];
        if ((int64_t)first < n) flag[first] = 1;
        const uint32_t a = top ? anchor[i] : first;
        uint32_t f = 0;
        if ((int64_t)a < n) {
            f = link[a] & 1u;
            if (top) {
                const double t = (nrm[3 * (int64_t)a] * up.v[0] + nrm[3 * (int64_t)a + 1] * up.v[1]) + nrm[3 * (int64_t)a + 2] * up.v[2];
                f ^= t < 0.0 ? 1u : 0u;
            }
        }
        rootflip[i] = (uint8_t)f;
        sz = (unsigned long long)(size[i] > 0 ? size[i] : 0);
    }
    if (__builtin_amdgcn_ballot_w64(isroot) == 0) return;         // wave-uniform
    sz = wave_max_u64(sz);
    if ((threadIdx.x & 63) == 0) atomicMax(&sc->largest, (int32_t)sz);
}

// the flips, on the caller's element type: negation is exact
template <typename T>
__global__ void ori_flip_kernel(const uint32_t *__restrict__ link, const uint8_t *__restrict__ inv, int64_t n,
                                const uint8_t *__restrict__ rootflip, const uint32_t *__restrict__ minidx, const int32_t *__restrict__ num,
                                T *__restrict__ out, int32_t *__restrict__ flip, int32_t *__restrict__ comp, OriScal *sc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool f = false;
    if (i < n) {
        int32_t fo = -1, co = 0;
        if (inv[i]) {
            const uint32_t l = link[i], root = l >> 1;
            if ((int64_t)root < n) {
                f = ((l ^ rootflip[root]) & 1u) != 0;
                const uint32_t first = minidx[root];
                co = (int64_t)first < n ? num[first] + 1 : 0;
            }
            fo = f ? 1 : 0;
            if (f) { out[3 * i] = -out[3 * i]; out[3 * i + 1] = -out[3 * i + 1]; out[3 * i + 2] = -out[3 * i + 2]; }
        }
        flip[i] = fo;
        comp[i] = co;
    }
    const uint64_t bf = __builtin_amdgcn_ballot_w64(f);
    if ((threadIdx.x & 63) == 0 && bf) atomicAdd(&sc->n_flipped, (unsigned long long)__popcll(bf));
}

// the edges whose ends disagree after the orientation: both ends have one root, so flip_u ^ flip_v = par(u) ^ par(v)
__global__ void ori_incons_kernel(const uint64_t *__restrict__ redge, int64_t ne, int64_t n, const uint32_t *__restrict__ link, OriScal *sc)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (r < ne) {
        const uint64_t key = redge[r];
        const uint32_t u = pair_u(key), v = pair_v(key);
        if ((int64_t)u < n && (int64_t)v < n) bad = (((uint32_t)(key >> 63) ^ link[u] ^ link[v]) & 1u) != 0;
    }
    const uint64_t bb = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && bb) atomicAdd(&sc->n_incons, (unsigned long long)__popcll(bb));
}

template <typename T>
int orient(const char *who, const T *xyz_aos, const T *nrm_aos, int64_t n, const rh_orient_params *p, int device, T *nrm_out,
           int32_t *flip_out, int32_t *comp_out, rh_orient_stats *stats)
{
    if (!xyz_aos || !nrm_aos || !p || !nrm_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= (int64_t)0x7FFFFFFF) { rh_set_error("%s: n = %lld outside 1 .. 2^31 - 2", who, (long long)n); return RH_E_INVALID; }
    if (p->k < 1 || p->k > RH_KNN_MAX_K) { rh_set_error("%s: k = %d outside 1 .. %d", who, p->k, RH_KNN_MAX_K); return RH_E_INVALID; }
    if (!(isfinite(p->radius) && p->radius >= 0.0)) { rh_set_error("%s: radius must be finite and >= 0", who); return RH_E_INVALID; }
    if (p->anchor != RH_ORI_ANCHOR_FIRST && p->anchor != RH_ORI_ANCHOR_TOP) { rh_set_error("%s: anchor = %d is not an anchor rule", who, p->anchor); return RH_E_INVALID; }
    const int top = p->anchor == RH_ORI_ANCHOR_TOP;
    if (top) {
        const bool fin = isfinite(p->up[0]) && isfinite(p->up[1]) && isfinite(p->up[2]);
        if (!fin || (p->up[0] == 0.0 && p->up[1] == 0.0 && p->up[2] == 0.0)) { rh_set_error("%s: up must be finite and not zero", who); return RH_E_INVALID; }
    }
    const int k = p->k;
    const int64_t nk = n * k;
    if (nk >= ((int64_t)1 << 31)) { rh_set_error("%s: n * k = %lld directed pairs, the limit is 2^31 - 1", who, (long long)nk); return RH_E_INVALID; }
    OriUp up;
    for (int a = 0; a < 3; a++) up.v[a] = top ? p->up[a] : 0.0;

    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;

    // the cloud, the normals (binary64 for every decision; the caller's element type for the flips), V
    double *d_xyz = nullptr, *d_nrm = nullptr;
    T *d_out = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyDefault));
    if (sizeof(T) == sizeof(double)) {
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        d_out = (T *)d_nrm;
        SCOPE_HIP(S, hipMemcpyAsync(d_nrm, nrm_aos, sizeof(double) * 3 * (size_t)n, hipMemcpyDefault, st));
    } else {
        RH_TRY(S.alloc(&d_out, 3 * n));
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        SCOPE_HIP(S, hipMemcpyAsync(d_out, nrm_aos, sizeof(T) * 3 * (size_t)n, hipMemcpyDefault, st));
        RH_TRY(S.widen(d_out, d_nrm, 3 * n));
    }
    OriScal *d_sc = nullptr, h;
    uint8_t *d_inv = nullptr;
    RH_TRY(S.alloc(&d_sc, 1));
    RH_TRY(S.alloc(&d_inv, n));
    memset(&h, 0, sizeof h);
    h.min_abits = 0x7FF0000000000000ULL;                          // +inf
    SCOPE_HIP(S, hipMemcpyAsync(d_sc, &h, sizeof h, hipMemcpyHostToDevice, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));                       // (h is written again below)
    hipLaunchKernelGGL(ori_check_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_nrm, n, d_inv, d_sc);
    SCOPE_HIP(S, hipGetLastError());

    // the search (it refuses a coordinate that is not finite) and the directed pairs
    KnnIndex ix;
    KnnQuery kq;
    RH_TRY(ix.init(S, d_xyz, n));
    RH_TRY(S.fetch(&h, d_sc));
    if (h.n_bad != 0) { rh_set_error("%s: a normal component is not finite or exceeds 2 in magnitude", who); return RH_E_INVALID; }
    const int64_t nv = (int64_t)h.n_vertices;
    RH_TRY(knn_index_for_k(ix, k + 1, p->radius, kq));
    uint64_t *d_pairs = nullptr, *d_sorted = nullptr;
    RH_TRY(S.alloc(&d_pairs, nk));
    RH_TRY(S.alloc(&d_sorted, nk));
    int32_t *d_flagc = nullptr, *d_num = nullptr;
    RH_TRY(S.alloc(&d_flagc, n));
    RH_TRY(S.alloc(&d_num, n));
    SCOPE_HIP(S, hipMemsetAsync(d_pairs, 0xFF, sizeof(uint64_t) * (size_t)nk, st));
    hipLaunchKernelGGL(ori_emit_kernel, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, d_inv, d_pairs);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortKeys(t, b, d_pairs, d_sorted, (int)nk, 0, 64, st); }));
    uint64_t *d_ekey = d_pairs;                                   // (the unsorted pairs are spent)
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceSelect::Unique(t, b, d_sorted, d_ekey, &d_sc->n_unique, (int)nk, st); }));
    hipLaunchKernelGGL(ori_count_kernel, dim3(1), dim3(64), 0, st, d_ekey, d_sc);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.fetch(&h, d_sc));
    const int64_t ne = h.n_edges;
    if (ne < 0 || ne > nk) { rh_set_error("%s: %lld edges of %lld pairs", who, (long long)ne, (long long)nk); return RH_E_INTERNAL; }

    // ranks
    uint32_t *d_link = nullptr, *d_tmpl = nullptr, *d_best = nullptr;
    RH_TRY(S.alloc(&d_link, n));
    RH_TRY(S.alloc(&d_tmpl, n));
    RH_TRY(S.alloc(&d_best, n));
    hipLaunchKernelGGL(ori_init_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_link, n);
    SCOPE_HIP(S, hipGetLastError());
    uint64_t *d_akey = d_sorted, *d_akey_sorted = nullptr, *d_redge = nullptr;   // (the sorted pairs are spent)
    uint32_t *d_eid = nullptr, *d_order = nullptr, *d_live[2] = { nullptr, nullptr };
    uint8_t *d_flag = nullptr;
    int rounds = 0;
    if (ne > 0) {
        RH_TRY(S.alloc(&d_akey_sorted, ne));
        RH_TRY(S.alloc(&d_redge, ne));
        RH_TRY(S.alloc(&d_eid, ne));
        RH_TRY(S.alloc(&d_order, ne));
        RH_TRY(S.alloc(&d_live[1], ne));
        RH_TRY(S.alloc(&d_flag, ne));
        d_live[0] = d_eid;                                        // (the edge numbers are spent once the ranks stand)
        hipLaunchKernelGGL(ori_weight_kernel, dim3(blocks_for(ne)), dim3(256), 0, st, d_ekey, ne, n, d_nrm, d_akey, d_eid);
        SCOPE_HIP(S, hipGetLastError());
        RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, d_akey, d_akey_sorted, d_eid, d_order, (int)ne, 0, 64, st); }));
        hipLaunchKernelGGL(ori_rank_kernel, dim3(blocks_for(ne)), dim3(256), 0, st, d_ekey, d_order, ne, d_redge, d_live[0]);
        SCOPE_HIP(S, hipGetLastError());

        // rounds
        int64_t nlive = ne;
        int cur = 0;
        while (nlive > 0) {
            SCOPE_HIP(S, hipMemsetAsync(d_best, 0xFF, sizeof(uint32_t) * (size_t)n, st));
            SCOPE_HIP(S, hipMemsetAsync(d_sc->unfin, 0, sizeof h.unfin, st));
            hipLaunchKernelGGL(ori_select_kernel, dim3(blocks_for(nlive)), dim3(256), 0, st, d_live[cur], nlive, ne, n, d_redge, d_link,
                               d_best, d_flag);
            SCOPE_HIP(S, hipGetLastError());
            RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceSelect::Flagged(t, b, d_live[cur], d_flag, d_live[cur ^ 1], &d_sc->nlive, (int)nlive, st); }));
            hipLaunchKernelGGL(ori_hook_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_link, d_best, d_redge, d_akey_sorted, n, ne,
                               d_tmpl, d_sc);
            // doublings tmp -> link -> tmp -> link: three before the first read-back, two before every further one
            int jumps = 0;
            for (;;) {
                const int batch = jumps == 0 ? 3 : 2;
                if (jumps + batch > ORI_MAX_JUMPS) { rh_set_error("%s: a tree deeper than 2^%d", who, ORI_MAX_JUMPS); return RH_E_INTERNAL; }
                for (int b = 0; b < batch; b++, jumps++) {
                    const bool odd = (jumps & 1) == 0;             // doubling 1, 3, 5, ..: tmp -> link
                    hipLaunchKernelGGL(ori_jump_kernel, dim3(blocks_for(n)), dim3(256), 0, st, odd ? d_tmpl : d_link, odd ? d_link : d_tmpl,
                                       n, &d_sc->unfin[jumps]);
                }
                SCOPE_HIP(S, hipGetLastError());
                RH_TRY(S.fetch(&h, d_sc));
                if (!h.unfin[jumps - 1]) break;
            }
            if (h.nlive < 0 || (int64_t)h.nlive > nlive) { rh_set_error("%s: %d live edges of %lld", who, h.nlive, (long long)nlive); return RH_E_INTERNAL; }
            nlive = h.nlive;                                      // the edges that joined two trees at this round's start
            cur ^= 1;
            if (nlive == 0) break;                                // no offer, no hook: the forest stands
            if (++rounds > ORI_MAX_ROUNDS) { rh_set_error("%s: more than %d rounds", who, ORI_MAX_ROUNDS); return RH_E_INTERNAL; }
        }
    }

    // epilogue
    uint32_t *d_minidx = d_best, *d_anchor = nullptr;             // (the offers are spent)
    int32_t *d_size = nullptr, *d_flip = nullptr, *d_comp = nullptr;
    unsigned long long *d_pmax = nullptr;
    uint8_t *d_rootflip = nullptr;
    RH_TRY(S.alloc(&d_size, n));
    RH_TRY(S.alloc(&d_flip, n));
    RH_TRY(S.alloc(&d_comp, n));
    RH_TRY(S.alloc(&d_rootflip, n));
    SCOPE_HIP(S, hipMemsetAsync(d_minidx, 0xFF, sizeof(uint32_t) * (size_t)n, st));
    SCOPE_HIP(S, hipMemsetAsync(d_size, 0, sizeof(int32_t) * (size_t)n, st));
    SCOPE_HIP(S, hipMemsetAsync(d_flagc, 0, sizeof(int32_t) * (size_t)n, st));
    SCOPE_HIP(S, hipMemsetAsync(d_rootflip, 0, (size_t)n, st));
    if (top) {
        RH_TRY(S.alloc(&d_pmax, n));
        RH_TRY(S.alloc(&d_anchor, n));
        SCOPE_HIP(S, hipMemsetAsync(d_pmax, 0, sizeof(unsigned long long) * (size_t)n, st));
        SCOPE_HIP(S, hipMemsetAsync(d_anchor, 0xFF, sizeof(uint32_t) * (size_t)n, st));
    }
    hipLaunchKernelGGL(ori_comp_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_link, d_inv, n, d_xyz, top, up, d_minidx, d_size, d_pmax);
    if (top) hipLaunchKernelGGL(ori_top_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_link, d_inv, n, d_xyz, up, d_pmax, d_anchor);
    hipLaunchKernelGGL(ori_root_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_link, d_inv, n, d_nrm, top, up, d_minidx, d_anchor, d_size,
                       d_flagc, d_rootflip, d_sc);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_flagc, d_num, (int)n, st); }));
    hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(64), 0, st, d_flagc, d_num, n, &d_sc->m);
    hipLaunchKernelGGL(ori_flip_kernel<T>, dim3(blocks_for(n)), dim3(256), 0, st, d_link, d_inv, n, d_rootflip, d_minidx, d_num, d_out,
                       d_flip, d_comp, d_sc);
    if (ne > 0) hipLaunchKernelGGL(ori_incons_kernel, dim3(blocks_for(ne)), dim3(256), 0, st, d_redge, ne, n, d_link, d_sc);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.fetch(&h, d_sc));
    if ((int64_t)h.n_tree != nv - (int64_t)h.m) {
        rh_set_error("%s: %llu tree edges for %lld vertices in %d components", who, h.n_tree, (long long)nv, h.m);
        return RH_E_INTERNAL;
    }
    SCOPE_HIP(S, hipMemcpyAsync(nrm_out, d_out, sizeof(T) * 3 * (size_t)n, hipMemcpyDefault, st));
    if (flip_out) SCOPE_HIP(S, hipMemcpyAsync(flip_out, d_flip, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st));
    if (comp_out) SCOPE_HIP(S, hipMemcpyAsync(comp_out, d_comp, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    if (stats) {
        stats->n_vertices = nv;
        stats->n_edges = ne;
        stats->n_components = h.m;
        stats->n_tree_edges = (int64_t)h.n_tree;
        stats->n_flipped = (int64_t)h.n_flipped;
        stats->n_inconsistent = (int64_t)h.n_incons;
        stats->largest_component = h.largest;
        memcpy(&stats->min_tree_absdot, &h.min_abits, sizeof(double));
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_orient_normals(const double *xyz_aos, const double *nrm_aos, int64_t n, const rh_orient_params *p, int device,
                                 double *nrm_out_aos, int32_t *flip_out_or_null, int32_t *comp_out_or_null, rh_orient_stats *stats_or_null)
{
    return orient<double>("rh_orient_normals", xyz_aos, nrm_aos, n, p, device, nrm_out_aos, flip_out_or_null, comp_out_or_null, stats_or_null);
}

extern "C" int rh_orient_normals_f32(const float *xyz_aos, const float *nrm_aos, int64_t n, const rh_orient_params *p, int device,
                                     float *nrm_out_aos, int32_t *flip_out_or_null, int32_t *comp_out_or_null, rh_orient_stats *stats_or_null)
{
    return orient<float>("rh_orient_normals_f32", xyz_aos, nrm_aos, n, p, device, nrm_out_aos, flip_out_or_null, comp_out_or_null,
                         stats_or_null);
}

#ifdef RH_DIAG
namespace {

// wave_each_key as a kernel of its own (ransac_hip_diag.h: rh_dbg_wave_keys).  A lane without `act` keeps its key: it
// may equal an active lane's and must still be in no ballot.  scal[0]: the leader branch ran; scal[1]: a lane saw
// anything but the whole wave inside f, or a ballot that is not "active and my key is L"
template <typename K>
__global__ void __launch_bounds__(256) dbg_wave_keys_kernel(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ act,
                                                            const int32_t *__restrict__ slot, int32_t n, int32_t *sum,
                                                            int32_t *minlead, int32_t *scal)
{
    const int i = threadIdx.x, lane = i & 63;
    const bool a = i < n && act[i] != 0;
    const K key = i < n ? (K)keys[i] : (K)0;
    const int32_t s = a ? slot[i] : 0;
    wave_each_key(a, key, [&](int leader, K L, uint64_t same) {
        const bool in = a && key == L;
        if (__builtin_amdgcn_ballot_w64(true) != ~0ULL || (((same >> lane) & 1ULL) != 0) != in) atomicAdd(&scal[1], 1);
        if (lane == leader) {
            atomicAdd(&sum[s], (int32_t)__popcll(same));
            atomicMin(&minlead[s], (int32_t)i);
            atomicAdd(&scal[0], 1);
        }
    });
}

}  // namespace

extern "C" int rh_dbg_wave_keys(const uint32_t *keys, const uint8_t *act, const int32_t *slot, int32_t n, int32_t nslots, int u32,
                                int device, int32_t *sum_out, int32_t *minlead_out, int32_t *scal_out)
{
    static const char who[] = "rh_dbg_wave_keys";
    bool ok = keys && act && slot && sum_out && minlead_out && scal_out && n >= 0 && n <= 256 && nslots >= 1;
    for (int32_t i = 0; ok && i < n; i++) ok = slot[i] >= 0 && slot[i] < nslots;   // (a slot is an address on the device)
    if (!ok) { rh_set_error("%s: bad arguments", who); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    uint32_t *d_keys = nullptr;
    uint8_t *d_act = nullptr;
    int32_t *d_slot = nullptr, *d_sum = nullptr, *d_min = nullptr, *d_scal = nullptr;
    RH_TRY(S.alloc(&d_keys, n)); RH_TRY(S.alloc(&d_act, n)); RH_TRY(S.alloc(&d_slot, n));
    RH_TRY(S.alloc(&d_sum, nslots)); RH_TRY(S.alloc(&d_min, nslots)); RH_TRY(S.alloc(&d_scal, 2));
    SCOPE_HIP(S, hipMemcpyAsync(d_keys, keys, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    SCOPE_HIP(S, hipMemcpyAsync(d_act, act, (size_t)n, hipMemcpyHostToDevice, st));
    SCOPE_HIP(S, hipMemcpyAsync(d_slot, slot, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    SCOPE_HIP(S, hipMemsetAsync(d_sum, 0, sizeof(int32_t) * (size_t)nslots, st));
    SCOPE_HIP(S, hipMemsetAsync(d_min, 0x7F, sizeof(int32_t) * (size_t)nslots, st));   // 0x7F7F7F7F: no leader
    SCOPE_HIP(S, hipMemsetAsync(d_scal, 0, sizeof(int32_t) * 2, st));
    if (u32) hipLaunchKernelGGL(dbg_wave_keys_kernel<uint32_t>, dim3(1), dim3(256), 0, st, d_keys, d_act, d_slot, n, d_sum, d_min, d_scal);
    else hipLaunchKernelGGL(dbg_wave_keys_kernel<int32_t>, dim3(1), dim3(256), 0, st, d_keys, d_act, d_slot, n, d_sum, d_min, d_scal);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(sum_out, d_sum, sizeof(int32_t) * (size_t)nslots, hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipMemcpyAsync(minlead_out, d_min, sizeof(int32_t) * (size_t)nslots, hipMemcpyDeviceToHost, st));
    return S.fetch(scal_out, d_scal, 2);
}
#endif   // RH_DIAG
