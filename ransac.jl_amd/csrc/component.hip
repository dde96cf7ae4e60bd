// component.hip -- the largest connected patch of a refit set (Efficient RANSAC, Schnabel et al. 2007, section 4.4), with
// connectivity on a 3-D voxel grid of the inliers instead of a per-shape parameter plane: one definition for all four
// kinds, no seam, no pole, no atan2 (include/ransac_hip.h states it in full).  Input and output are the cloud's
// refit_mask (original order): rhk_component_filter clears the bits of every inlier outside the winning component.
//   1. minimum:    o = componentwise minimum of the inliers (+ maximum for the extent check, + |I|) -- one read-back
//   2. cell table: open addressing (cell_grid.h), 2 |I| slots or more; per slot the cell key, a parent (union-find), the
//                  cell's point count and its smallest point index
//   3. union:      every occupied slot looks up its forward neighbours (13, or 3 without diagonals) and unites lock-free
//                  (union_find.h); flatten; counts and minimum indices summed into the roots
//   4. winner:     one 64-bit maximum over size << 32 | ~min_index
//   5. mask:       an inlier keeps its bit when its cell's root is the winner
// Slot numbers depend on who inserted first; nothing that leaves this file does: components are sets of cells, a
// component is named by its smallest point index, and sizes / minima are sums / minima of integers.
#include <math.h>

#include "call_scope.h"
#include "cell_grid.h"
#include "rh_internal.h"
#include "union_find.h"
#include "wave_keys.h"

namespace {

// scalars of a call (rh_cloud::comp_scal, 8-byte words)
enum { CS_MIN = MM_MIN, CS_MAX = MM_MAX, CS_COUNT = MM_COUNT, CS_BEST = 7, CS_NCOMP = 8, CS_WORDS = 16 };   // (the partial results of the minimum pass lie behind them)

struct comp_table {
    uint64_t *key;       // [cap] cell key, GRID_EMPTY: free
    int32_t *parent;     // [cap] union-find over slots: parent <= self, a root points at itself
    int32_t *count;      // [cap] points in the cell; after the flatten pass a root holds its component's
    int32_t *minidx;     // [cap] smallest 0-based point index, likewise
    uint32_t mask;       // cap - 1 (cap is a power of two)
};

// the cell of a point: floor((x - o) / beta) per axis (binary64 division, no contraction), each + 1 in a 21-bit field,
// so that the -1 / +1 neighbours of cells 0 .. 2^20 - 1 stay inside their fields
__device__ __forceinline__ uint64_t cell_key(double x, double y, double z, double ox, double oy, double oz, double beta)
{
    const long long cx = (long long)floor((x - ox) / beta), cy = (long long)floor((y - oy) / beta), cz = (long long)floor((z - oz) / beta);
    return grid_pack(cx, cy, cz, 1);
}

// ---- 1. minimum, maximum and number of the inliers.  A wave owns whole mask words (lane = bit), so the three planes
// are read 64 points in a row.  Every block (256 threads) leaves its partial result in `part`; the fold of cell_grid.h
// also zeroes the winner and the component count of the call
template <typename T>
__global__ void __launch_bounds__(256)
comp_minmax_kernel(const T *__restrict__ pts, int64_t stride, int64_t nwords, const uint64_t *__restrict__ mask,
                   unsigned long long *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    MinMaxCount acc;
    for (int64_t w = wave; w < nwords; w += nwaves) {
        const uint64_t m = mask[w];
        if (!((m >> lane) & 1ULL)) continue;
        const int64_t i = (w << 6) + lane;
        acc.add((double)pts[i], (double)pts[stride + i], (double)pts[2 * stride + i]);
    }
    acc.store(part);
}

// ---- 2. the cell table
__global__ void __launch_bounds__(256) comp_init_kernel(comp_table T)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > T.mask) return;
    T.key[s] = GRID_EMPTY;
    T.parent[s] = (int32_t)s;
    T.count[s] = 0;
    T.minidx[s] = 0x7FFFFFFF;
}

template <typename T>
__global__ void __launch_bounds__(256)
comp_insert_kernel(const T *__restrict__ pts, int64_t stride, int64_t nwords, const uint64_t *__restrict__ mask,
                   const unsigned long long *__restrict__ scal, double beta, comp_table tab)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = g >> 6;
    if (w >= nwords) return;
    if (!((mask[w] >> (g & 63)) & 1ULL)) return;
    const uint64_t key = cell_key((double)pts[g], (double)pts[stride + g], (double)pts[2 * stride + g], ord_back(scal[CS_MIN]),
                                  ord_back(scal[CS_MIN + 1]), ord_back(scal[CS_MIN + 2]), beta);
    const uint32_t h = table_insert(tab.key, tab.mask, key);
    atomicAdd(&tab.count[h], 1);
    atomicMin(&tab.minidx[h], (int32_t)g);
}

// ---- 3. union-find over the slots (union_find.h)
__global__ void __launch_bounds__(256) comp_union_kernel(comp_table T, int conn26)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > T.mask) return;
    const uint64_t key = T.key[s];
    if (key == GRID_EMPTY) return;
    if (conn26) {
        // the 13 neighbours that follow the cell in (x, y, z) order; the other 13 unite from their side
        for (int dx = 0; dx <= 1; dx++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dz = -1; dz <= 1; dz++) {
                    if (!(dx > 0 || dy > 0 || (dy == 0 && dz > 0))) continue;
                    const int32_t t = (int32_t)table_find(T.key, T.mask, key + (uint64_t)(((long long)dx << 42) + ((long long)dy << 21) + dz));
                    if (t >= 0) uf_unite(T.parent, (int32_t)s, t);
                }
    } else {
        for (int a = 0; a < 3; a++) {
            const int32_t t = (int32_t)table_find(T.key, T.mask, key + (1ULL << (21 * a)));
            if (t >= 0) uf_unite(T.parent, (int32_t)s, t);
        }
    }
}

// flatten + the components' sizes (in points) and smallest indices into their roots.  Only roots are added to and a root
// never reads its own numbers here, so the sums can live in the cells' own fields
__global__ void __launch_bounds__(256) comp_flatten_kernel(comp_table T)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t r = -1, cnt = 0, mi = 0x7FFFFFFF;
    if (s <= T.mask && T.key[s] != GRID_EMPTY) {
        const int32_t root = uf_find(T.parent, (int32_t)s);
        if (root != (int32_t)s) {
            atomicMin(&T.parent[s], root);   // (root is a root, roots never change in this launch, and no ancestor is smaller)
            r = root;
            cnt = T.count[s];
            mi = T.minidx[s];
        }
    }
    // lanes that share a root add up inside the wave first: a plane's one big component would otherwise queue
    // every cell of the table on one address (175 000 cells: 1.8 ms of atomics)
    wave_each_key(r >= 0, r, [&](int leader, int32_t rl, uint64_t) {
        const bool mine = r == rl;
        const int32_t c = wave_sum_i32(mine ? cnt : 0), m = wave_min_i32(mine ? mi : 0x7FFFFFFF);
        if (lane == leader) {
            atomicAdd(&T.count[rl], c);
            atomicMin(&T.minidx[rl], m);
        }
    });
}

// ---- 4. key = size << 32 | ~min_index: the maximum is the largest component, the smallest point index among equals
__global__ void __launch_bounds__(256) comp_best_kernel(comp_table T, unsigned long long *__restrict__ scal)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = s <= T.mask && T.key[s] != GRID_EMPTY && T.parent[s] == (int32_t)s;
    const uint64_t roots = __builtin_amdgcn_ballot_w64(root);
    if (roots == 0) return;
    if ((threadIdx.x & 63) == 0) atomicAdd(&scal[CS_NCOMP], (unsigned long long)__popcll(roots));
    if (root) atomicMax(&scal[CS_BEST], ((unsigned long long)(uint32_t)T.count[s] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)T.minidx[s]));
}

// ---- 5. the mask keeps the winner's points
template <typename T>
__global__ void __launch_bounds__(256)
comp_mask_kernel(const T *__restrict__ pts, int64_t stride, int64_t nwords, uint64_t *__restrict__ mask,
                 const unsigned long long *__restrict__ scal, double beta, comp_table tab)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t w = g >> 6;
    if (w >= nwords) return;
    const uint64_t m = mask[w];
    if (m == 0) return;   // (the whole wave)
    bool keep = false;
    if ((m >> (g & 63)) & 1ULL) {
        const uint64_t key = cell_key((double)pts[g], (double)pts[stride + g], (double)pts[2 * stride + g], ord_back(scal[CS_MIN]),
                                      ord_back(scal[CS_MIN + 1]), ord_back(scal[CS_MIN + 2]), beta);
        const int32_t s = (int32_t)table_find(tab.key, tab.mask, key);
        const int32_t win_min = (int32_t)(0xFFFFFFFFu - (uint32_t)(scal[CS_BEST] & 0xFFFFFFFFu));
        keep = s >= 0 && tab.minidx[tab.parent[s]] == win_min;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(keep);
    if ((g & 63) == 0) mask[w] = b;
}

}  // namespace

int rh_component_check_beta(const char *who, double beta)
{
    if (!(beta > 0.0) || !(beta <= 1.7976931348623157e308)) { rh_set_error("%s: beta must be finite and > 0", who); return RH_E_INVALID; }
    return RH_OK;
}

// refit_mask &= the largest component of its points.  Waits once for the stream (|I|, o and the extent come back: the
// table is sized by |I|); the rest is queued.  n_refit_out: |I|.  The number of components and the winner's size stay on the
// device (comp_scal: rhk_component_stats) for whoever wants them behind the call.
int rhk_component_filter(rh_cloud *c, double beta, int conn26, int64_t *n_refit_out)
{
    if (n_refit_out) *n_refit_out = 0;
    RH_TRY(rh_component_check_beta("component filter", beta));
    if (c->n >= ((int64_t)1 << 31)) { rh_set_error("component filter: clouds of 2^31 points or more are not supported"); return RH_E_INVALID; }
    if (!c->comp_scal) {
        RH_TRY(c->comp_scal.alloc(CS_WORDS + MM_WORDS * GRID_MM_BLOCKS));
        RH_TRY(c->comp_h.alloc(CS_WORDS));
    }
    unsigned long long *scal = (unsigned long long *)c->comp_scal.get();
    if (c->nwords == 0) return RH_OK;
    const int64_t stride = c->n_pad;
    {
        int64_t b = (c->nwords + 3) / 4;
        if (b > GRID_MM_BLOCKS) b = GRID_MM_BLOCKS;
        unsigned long long *part = scal + CS_WORDS;
        if (c->f32) hipLaunchKernelGGL((comp_minmax_kernel<float>), dim3((unsigned)b), dim3(256), 0, c->stream, c->full32, stride, c->nwords, c->refit_mask, part);
        else hipLaunchKernelGGL((comp_minmax_kernel<double>), dim3((unsigned)b), dim3(256), 0, c->stream, c->full, stride, c->nwords, c->refit_mask, part);
        hipLaunchKernelGGL(grid_minmax_fold_kernel, dim3(1), dim3(256), 0, c->stream, part, (int)b, scal, (int)CS_WORDS);
    }
    RH_HIP(hipGetLastError());
    RH_HIP(hipMemcpyAsync(c->comp_h, scal, sizeof(uint64_t) * (CS_COUNT + 1), hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    const int64_t ni = (int64_t)c->comp_h[CS_COUNT];
    if (n_refit_out) *n_refit_out = ni;
    if (ni == 0) return RH_OK;
    for (int a = 0; a < 3; a++) {
        double cells;
        if (!grid_axis_fits(ord_back(c->comp_h[CS_MIN + a]), ord_back(c->comp_h[CS_MAX + a]), beta, &cells)) {
            rh_set_error("component filter: the inliers span more than 2^20 cells of size %g along axis %d", beta, a);
            return RH_E_INVALID;
        }
    }
    int64_t cap = 64;
    while (cap < 2 * ni) cap <<= 1;
    if (cap > c->comp_cap) {
        c->comp_cap = 0;
        RH_TRY(c->comp_tab.grow(c->stream, cap * 20));
        c->comp_cap = cap;
    }
    comp_table T;
    T.key = (uint64_t *)c->comp_tab.get();
    T.parent = (int32_t *)(T.key + cap);
    T.count = T.parent + cap;
    T.minidx = T.count + cap;
    T.mask = (uint32_t)(cap - 1);
    const dim3 blk(256), gs(blocks_for(cap)), gp(blocks_for(c->nwords * 64));
    hipLaunchKernelGGL(comp_init_kernel, gs, blk, 0, c->stream, T);
    if (c->f32) hipLaunchKernelGGL((comp_insert_kernel<float>), gp, blk, 0, c->stream, c->full32, stride, c->nwords, c->refit_mask, scal, beta, T);
    else hipLaunchKernelGGL((comp_insert_kernel<double>), gp, blk, 0, c->stream, c->full, stride, c->nwords, c->refit_mask, scal, beta, T);
    hipLaunchKernelGGL(comp_union_kernel, gs, blk, 0, c->stream, T, conn26 ? 1 : 0);
    hipLaunchKernelGGL(comp_flatten_kernel, gs, blk, 0, c->stream, T);
    hipLaunchKernelGGL(comp_best_kernel, gs, blk, 0, c->stream, T, scal);
    if (c->f32) hipLaunchKernelGGL((comp_mask_kernel<float>), gp, blk, 0, c->stream, c->full32, stride, c->nwords, c->refit_mask, scal, beta, T);
    else hipLaunchKernelGGL((comp_mask_kernel<double>), gp, blk, 0, c->stream, c->full, stride, c->nwords, c->refit_mask, scal, beta, T);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// the last filter's number of components, in stream order (0 behind an empty refit set); the caller waits for the stream
int rhk_component_stats(rh_cloud *c, int64_t *h_ncomp)
{
    *h_ncomp = 0;
    if (!c->comp_scal) return RH_OK;
    RH_HIP(hipMemcpyAsync(h_ncomp, c->comp_scal + CS_NCOMP, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    return RH_OK;
}

extern "C" int rh_refit_component(rh_cloud *c, const rh_shape *shape, const rh_params *p, double beta, int32_t conn26,
                                  int64_t *idx_out, int64_t cap, int64_t *n_out, int64_t *n_refit_out, int32_t *n_components_out)
{
    RH_TRY(rh_cloud_join(c));
    RH_TRY(rh_validate_params(p));
    if (!shape || !n_out || cap < 0 || (cap > 0 && !idx_out)) { rh_set_error("rh_refit_component: bad arguments"); return RH_E_INVALID; }
    if (shape->kind < 0 || shape->kind > 3) { rh_set_error("unknown shape kind %d", shape->kind); return RH_E_INVALID; }
    *n_out = 0;
    if (n_refit_out) *n_refit_out = 0;
    if (n_components_out) *n_components_out = 0;
    RH_TRY(rh_component_check_beta("rh_refit_component", beta));
    rh_prep P;
    rh_prep_host(*shape, &P);
    RH_TRY(rhk_refit_mask(c, P, shape->kind, p->eps[shape->kind], p->cos_alpha[shape->kind]));
    int64_t n_refit = 0, ncomp = 0;
    RH_TRY(rhk_component_filter(c, beta, conn26, &n_refit));
    if (n_refit_out) *n_refit_out = n_refit;
    if (n_refit == 0) return RH_OK;
    RH_TRY(rhk_component_stats(c, &ncomp));   // (queued in front of the compaction, read behind its wait)
    const int rc = rhk_refit_total(c, "rh_refit_component", idx_out, cap, n_out);
    if (n_components_out) *n_components_out = (int32_t)ncomp;
    return rc;
}

extern "C" int rh_cloud_set_component_filter(rh_cloud *c, double beta, int32_t conn26)
{
    if (!c) { rh_set_error("cloud is NULL"); return RH_E_INVALID; }
    if (beta != beta || beta > 1.7976931348623157e308) { rh_set_error("rh_cloud_set_component_filter: beta must be finite"); return RH_E_INVALID; }
    c->comp_beta = beta > 0.0 ? beta : 0.0;
    c->comp_conn26 = conn26 ? 1 : 0;
    return RH_OK;
}

extern "C" int rh_cloud_get_component_filter(const rh_cloud *c, double *beta_out, int32_t *conn26_out)
{
    if (!c) { rh_set_error("cloud is NULL"); return RH_E_INVALID; }
    if (beta_out) *beta_out = c->comp_beta;
    if (conn26_out) *conn26_out = c->comp_conn26;
    return RH_OK;
}
