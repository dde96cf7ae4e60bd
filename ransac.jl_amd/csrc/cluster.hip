// cluster.hip -- density-based clustering of a raw cloud (rh_cluster; include/ransac_hip.h states the definition in full):
// DBSCAN with the border rule made independent of any order, plain Euclidean cluster extraction at min_pts = 1.
//   grid     KnnIndex::build (knn_grid.h) with a cell a little wider than eps, see CL_SLACK
//   items    the work items: (occupied cell, chunk of 64 of its sorted points) = the sorted positions that lie a multiple
//            of 64 behind their cell's first, compacted (hipcub DeviceSelect)
//   walk     one wave per item, one query point per lane.  The wave finds the ranges of the 27 cells around its own --
//            wave-uniform table lookups; the three cells of a row along x are one run of the sorted arrays, so nine runs --
//            and streams their points through in cell order: a tile of 64 candidates is
//            loaded coalesced, one per lane, into the wave's own LDS rows, and every lane tests its query against
//            candidate k, which all 64 lanes read from the same LDS address (a broadcast, no bank conflict).  No lane walks
//            a cell list of its own.  Three passes over this walk (cl_walk_kernel<PASS>):
//              0 core   neighbours counted up to min_pts - 1; the wave leaves once no lane can change any more
//              1 unite  core query, core candidate, d2 <= eps2, query index < candidate index: uf_unite on parents indexed
//                       by ORIGINAL point index, so that a cluster's root is its smallest core index
//              2 root   a point that is no core point keeps its best (d2, index) core candidate and takes that one's root;
//                       a core point looks its own root up.  -> root[], kind[]
//   tail     root_labels.h: sizes, the min_size filter, the numbering, labels, stats and lists
// Nothing waits on another block; uf_unite's retry loop (union_find.h) is the only loop without a static bound.  No
// floating-point atomics: every output is a comparison of binary64 values or an integer.
#include "knn_grid.h"
#include "root_labels.h"
#include "union_find.h"
#include "wave_keys.h"

namespace {

// Why 27 cells suffice.  A pair passes when fl(d2) <= fl(eps*eps).  With u = 2^-53: fl(d2) >= dx*dx * (1 - 3u) for the
// rounded difference dx = fl(q.x - p.x), and fl(eps*eps) <= eps*eps * (1 + u), so |q.x - p.x| <= eps * (1 + 4u), and the
// same along y and z.  cell_of takes floor(t) of t = fl(fl(v - o) / h), at most 2u * t <= 2^-31 away from (v - o) / h
// (t < 2^20 + 1).  The t of the two points therefore differ by less than eps * (1 + 4u) / h + 2^-30, which with
// h >= eps * (1 + 2^-20) is below 1: their floors differ by at most 1 (clamping to the last cell only brings them closer).
// KnnIndex::build may raise h further (L / 2^20), which only widens the cell.
constexpr double CL_SLACK = 1.0 / 1048576.0;
constexpr int CL_BLOCK = 256;
constexpr int CL_WAVES = CL_BLOCK / 64;
constexpr int32_t CL_NONE = 0x7FFFFFFF;

struct ClJob {
    Grid g;
    const uint64_t *skey;    // [n] cell key of every sorted position
    const int32_t *items;    // [nitems] first sorted position of every chunk
    int64_t n, nitems;
    double eps2;
    int32_t need;            // min_pts - 1: the neighbours a core point has at least
    uint8_t *core_s;         // [n] by SORTED position (the tiles load it coalesced)
    int32_t *parent;         // [n] by original index
    int32_t *root;           // [n] by original index: the cluster's smallest core index, -1 = noise
    uint8_t *kind;           // [n] by original index
};

// position i starts a chunk: it lies a multiple of 64 behind the first point of its cell
__global__ void cl_chunk_flag_kernel(Grid g, const uint64_t *__restrict__ skey, int64_t n, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t sl = table_find(g.hkey, (uint32_t)g.mask, skey[i]);
    flag[i] = sl >= 0 && ((i - (int64_t)g.hrange[2 * sl]) & 63) == 0;
}

__global__ void cl_init_parent_kernel(int32_t *__restrict__ parent, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

template <int PASS>
__global__ __launch_bounds__(CL_BLOCK) void cl_walk_kernel(const ClJob J)
{
    __shared__ double tx[CL_WAVES][64], ty[CL_WAVES][64], tz[CL_WAVES][64];
    __shared__ int32_t ti[CL_WAVES][64];     // original index; passes 1 and 2: CL_NONE for a candidate that is no core point
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * CL_WAVES + wv;
    if (w >= J.nitems) return;                                            // (wave-uniform, like every branch on s and key below)
    const Grid &g = J.g;
    const int32_t s = __builtin_amdgcn_readfirstlane(J.items[w]);
    if (s < 0 || (int64_t)s >= J.n) return;
    const uint64_t key = J.skey[s];
    const int64_t own = table_find(g.hkey, (uint32_t)g.mask, key);
    if (own < 0) return;
    int32_t cend = __builtin_amdgcn_readfirstlane(g.hrange[2 * own + 1]);
    if ((int64_t)cend > J.n) cend = (int32_t)J.n;
    const int64_t q = (int64_t)s + lane;                                    // (64-bit: s + 63 and t + 64 may pass 2^31)
    const int64_t qc = q < cend ? q : s;                                   // (a chunk is 64 positions at most: lane < 64)
    const double px = g.sx[qc], py = g.sy[qc], pz = g.sz[qc];
    const int32_t qi = g.sidx[qc];
    const bool live = q < cend && (uint32_t)qi < (uint32_t)J.n;            // nothing is addressed through a bad index
    const int64_t cx = (int64_t)(key % (uint64_t)g.dim[0]);
    const int64_t cyz = (int64_t)(key / (uint64_t)g.dim[0]);
    const int64_t cy = cyz % g.dim[1], cz = cyz / g.dim[1];

    int32_t cnt = 0;                                                       // pass 0
    const bool qcore = PASS != 0 && live && J.core_s[qc] != 0;             // passes 1, 2
    const bool seek = PASS == 2 && live && !qcore;
    double bd = INFINITY;                                                  // pass 2: the best core candidate so far
    int32_t bi = CL_NONE;
    bool walk = true;
    if (PASS == 0) walk = J.need > 0;                                      // min_pts = 1: every point is a core point
    if (PASS == 1) walk = __builtin_amdgcn_ballot_w64(qcore) != 0;
    if (PASS == 2) walk = __builtin_amdgcn_ballot_w64(seek) != 0;

    // the 27 cells as 9 rows along x: the keys of (cx - 1, cx, cx + 1) at one (cy, cz) are consecutive integers, so the
    // points of those of them that are occupied are ONE run of the sorted arrays, streamed through in full tiles
    for (int r = 0; r < 9 && walk; r++) {
        const int64_t ny = cy + r % 3 - 1, nz = cz + r / 3 - 1;
        if (ny < 0 || nz < 0 || ny >= g.dim[1] || nz >= g.dim[2]) continue;
        int32_t a = CL_NONE, b = 0;
        for (int64_t nx = cx - 1; nx <= cx + 1; nx++) {
            if (nx < 0 || nx >= g.dim[0]) continue;
            const int64_t sl = table_find(g.hkey, (uint32_t)g.mask, (uint64_t)(nx + g.dim[0] * (ny + g.dim[1] * nz)));
            if (sl < 0) continue;
            const int32_t ca = __builtin_amdgcn_readfirstlane(g.hrange[2 * sl]), cb = __builtin_amdgcn_readfirstlane(g.hrange[2 * sl + 1]);
            a = ca < a ? ca : a;
            b = cb > b ? cb : b;
        }
        if (a < 0) a = 0;
        if ((int64_t)b > J.n) b = (int32_t)J.n;
        for (int64_t t = a; t < b && walk; t += 64) {
            const int m = b - t < 64 ? (int)(b - t) : 64;
            wave_lds_sync();                                               // the last tile has been read
            if (lane < m) {
                const int64_t j = t + lane;
                tx[wv][lane] = g.sx[j]; ty[wv][lane] = g.sy[j]; tz[wv][lane] = g.sz[j];
                ti[wv][lane] = (PASS == 0 || J.core_s[j] != 0) ? g.sidx[j] : CL_NONE;
            }
            wave_lds_sync();
            for (int k = 0; k < m; k++) {
                const int32_t cj = __builtin_amdgcn_readfirstlane(ti[wv][k]);
                if (PASS != 0 && ((uint32_t)cj >= (uint32_t)J.n)) continue;   // no core point (or no index): wave-uniform
                const double dx = tx[wv][k] - px, dy = ty[wv][k] - py, dz = tz[wv][k] - pz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const bool hit = d2 <= J.eps2 && t + k != q;
                if (PASS == 0) {
                    cnt += (hit && cnt < J.need) ? 1 : 0;
                } else if (PASS == 1) {
                    if (hit && qcore && qi < cj && ld(&J.parent[qi]) != ld(&J.parent[cj])) uf_unite(J.parent, qi, cj);
                } else {
                    if (hit && seek && (d2 < bd || (d2 == bd && cj < bi))) { bd = d2; bi = cj; }
                }
            }
            if (PASS == 0) walk = __builtin_amdgcn_ballot_w64(live && cnt < J.need) != 0;   // no output needs the full degree
        }
    }
    if (!live) return;
    if (PASS == 0) J.core_s[q] = cnt >= J.need;
    if (PASS == 2) {
        const int32_t from = qcore ? qi : bi;
        J.root[qi] = from != CL_NONE ? uf_find(J.parent, from) : -1;
        J.kind[qi] = qcore ? RH_PT_CORE : (from != CL_NONE ? RH_PT_BORDER : RH_PT_NOISE);
    }
}

template <int PASS>
void launch_walk(hipStream_t st, const ClJob &J)
{
    hipLaunchKernelGGL(cl_walk_kernel<PASS>, dim3(blocks_for(J.nitems, CL_WAVES)), dim3(CL_BLOCK), 0, st, J);
}

template <typename T>
int cluster(const char *who, const T *xyz_aos, int64_t n, const rh_cluster_params *p, int device, int32_t *labels_out, uint8_t *kind_out,
            int64_t cap, int64_t *counts_out, int64_t *offsets_out, int64_t *idx_out, int64_t *n_clusters_out, rh_cluster_stats *stats)
{
    if (!xyz_aos || !p || !labels_out || !n_clusters_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= ((int64_t)1 << 31)) { rh_set_error("%s: n = %lld outside 1 .. 2^31 - 1", who, (long long)n); return RH_E_INVALID; }
    if (!(isfinite(p->eps) && p->eps > 0.0)) { rh_set_error("%s: eps must be finite and > 0", who); return RH_E_INVALID; }
    if (p->min_pts < 1 || p->min_size < 1) { rh_set_error("%s: min_pts = %d, min_size = %d: both are >= 1", who, p->min_pts, p->min_size); return RH_E_INVALID; }
    if (p->order != RH_CLUSTER_BY_INDEX && p->order != RH_CLUSTER_BY_SIZE) { rh_set_error("%s: order = %d is not a numbering", who, p->order); return RH_E_INVALID; }
    if (cap < 0) { rh_set_error("%s: cap = %lld", who, (long long)cap); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;

    // grid
    double *d_xyz = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyDefault));   // (the caller's array may be on the device already)
    KnnIndex ix;
    RH_TRY(ix.init(S, d_xyz, n));
    RH_TRY(ix.build(p->eps * (1.0 + CL_SLACK)));

    // items
    RootScal *d_sc = nullptr, h;
    uint8_t *d_flag8 = nullptr;
    int32_t *d_items = nullptr;
    RH_TRY(S.alloc(&d_sc, 1));
    RH_TRY(S.alloc(&d_flag8, n));
    RH_TRY(S.alloc(&d_items, n));
    hipcub::CountingInputIterator<int32_t> zero_based(0);
    SCOPE_HIP(S, hipMemsetAsync(d_sc, 0, sizeof(RootScal), st));
    hipLaunchKernelGGL(cl_chunk_flag_kernel, dim3(blocks_for(n)), dim3(256), 0, st, ix.g, ix.d_key[1], n, d_flag8);
    SCOPE_HIP(S, hipGetLastError());
    RH_TRY(S.cub([&](void *t, size_t &b) { return hipcub::DeviceSelect::Flagged(t, b, zero_based, d_flag8, d_items, &d_sc->aux, (int)n, st); }));
    RH_TRY(S.fetch(&h, d_sc));
    const int64_t nitems = h.aux;
    if (nitems < 1 || nitems > n) { rh_set_error("%s: %lld work items for %lld points", who, (long long)nitems, (long long)n); return RH_E_INTERNAL; }

    // the three passes
    ClJob J;
    J.g = ix.g; J.skey = ix.d_key[1]; J.items = d_items; J.n = n; J.nitems = nitems;
    J.eps2 = p->eps * p->eps;
    J.need = p->min_pts - 1;
    J.core_s = d_flag8;                                          // (the chunk flags are spent: pass 0 writes every position)
    RH_TRY(S.alloc(&J.parent, n)); RH_TRY(S.alloc(&J.root, n)); RH_TRY(S.alloc(&J.kind, n));
    hipLaunchKernelGGL(cl_init_parent_kernel, dim3(blocks_for(n)), dim3(256), 0, st, J.parent, n);
    launch_walk<0>(st, J);
    launch_walk<1>(st, J);
    launch_walk<2>(st, J);
    SCOPE_HIP(S, hipGetLastError());

    // the tail; the grid's unsorted keys are free once it is built, the sorted ones now that the walk is over
    RootTail tl;
    tl.what = "clusters";
    tl.d_root = J.root; tl.d_kind = J.kind; tl.n = n;
    tl.min_size = p->min_size; tl.by_size = p->order == RH_CLUSTER_BY_SIZE; tl.cap = cap;
    tl.d_sc = d_sc; tl.d_mkey = ix.d_key[0]; tl.d_msorted = ix.d_key[1];
    tl.labels_out = labels_out; tl.kind_out = kind_out; tl.counts_out = counts_out; tl.offsets_out = offsets_out; tl.idx_out = idx_out;
    return root_labels(S, tl, [&](const RootScal &r, int64_t m) {
        *n_clusters_out = m;
        if (stats) {
            stats->n_clusters = m;
            stats->n_core = (int64_t)r.n_core; stats->n_border = (int64_t)r.n_border; stats->n_noise = (int64_t)r.n_noise;
            stats->n_small = (int64_t)r.n_small; stats->largest = r.largest;
        }
    });
}

}  // namespace

extern "C" int rh_cluster(const double *xyz_aos, int64_t n, const rh_cluster_params *p, int device, int32_t *labels_out,
                          uint8_t *kind_out_or_null, int64_t cap, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
                          int64_t *idx_out_or_null, int64_t *n_clusters_out, rh_cluster_stats *stats_or_null)
{
    return cluster<double>("rh_cluster", xyz_aos, n, p, device, labels_out, kind_out_or_null, cap, counts_out_or_null, offsets_out_or_null,
                           idx_out_or_null, n_clusters_out, stats_or_null);
}

extern "C" int rh_cluster_f32(const float *xyz_aos, int64_t n, const rh_cluster_params *p, int device, int32_t *labels_out,
                              uint8_t *kind_out_or_null, int64_t cap, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
                              int64_t *idx_out_or_null, int64_t *n_clusters_out, rh_cluster_stats *stats_or_null)
{
    return cluster<float>("rh_cluster_f32", xyz_aos, n, p, device, labels_out, kind_out_or_null, cap, counts_out_or_null,
                          offsets_out_or_null, idx_out_or_null, n_clusters_out, stats_or_null);
}
