// assign.hip -- every point labelled with its nearest compatible shape (include/ransac_hip.h states the definition in full):
// the stage after detection and refit that turns b shapes back into a segmentation of the scan.  Reads the points (raw
// arrays, or a cloud's resident planes) and changes nothing on a cloud.
//   prep     the shapes' rh_prep records: rhk_prep_sorted on the device (cloud entries), rh_prep_host (raw entries)
//   label    one point per lane, ASG_PPT points per lane: the wave walks the shapes in the CALLER'S order -- the record
//            and the kind come through the constant address space, so they are scalar loads and the switch on the kind is
//            a scalar branch -- and keeps the claiming shape of smallest d.  d < best with ascending j IS the tie rule
//            (among equal d the smallest j): no sort by kind, no index to carry.  -> labels, dist
//   count    (counts or lists wanted) a block owns a run of ASG_RUN points, each wave a contiguous quarter; a wave counts
//            its labels into its own LDS row (the leader lane of every distinct label adds the ballot's popcount: no
//            atomics); the block's b + 1 sums are one row of the count matrix [runs][b + 1]
//   colscan  one lane per label walks the rows (coalesced across labels; 16 waves share the rows of 64 labels): the
//            matrix becomes the exclusive prefix down every column, the column sums are the counts
//   offsets  one wave: the exclusive prefix over the b + 1 counts -> offsets, counts
//   scatter  (lists wanted) the run's counts again, per-wave cursors = offsets[L] + matrix[run][L] + the earlier waves'
//            counts, then rank within the wave by ballot + popcount below the lane -> idx
// No floating-point atomics and no atomics at all: nothing depends on which block or wave ran first.
#include <string.h>

#include <vector>

#include "assign_device.h"
#include "call_scope.h"
#include "rh_internal.h"
#include "wave_keys.h"

namespace {

using namespace rhdev;

constexpr int ASG_BLOCK = 256;
constexpr int ASG_WAVES = ASG_BLOCK / 64;
constexpr int ASG_PPT = 4;                           // label kernel: points per lane
constexpr int ASG_TILE = ASG_BLOCK * ASG_PPT;        // ... per block
constexpr int ASG_RUN = 4096;                        // list kernels: points per block,
constexpr int ASG_WRUN = ASG_RUN / ASG_WAVES;        // ... per wave (contiguous)
constexpr int ASG_SCAN_WAVES = 16;                   // colscan: waves that share the rows of 64 labels

struct asg_job {
    const void *xyz, *nrm;        // AoS: n x 3; planes: x y z (nx ny nz) `stride` apart.  nrm null: no normals
    int64_t n, stride;
    const uint64_t *enabled;      // null: every point counts
    const rh_shape *shapes;       // [b] on the device (the kind is read from here)
    const rh_prep *prep;          // [b]
    int32_t b;
    double eps[4], cosa[4];
    int32_t *labels;
    double *dist;                 // optional
    int32_t *mat;                 // [nruns][b + 1]
    int64_t *tot, *off;           // [b + 1], [b + 2] (workspace)
    int64_t *counts, *offsets, *idx;   // the caller's (optional)
    int64_t nruns;
};

template <typename T, bool AOS>
__device__ __forceinline__ void load3(const T *__restrict__ a, int64_t stride, int64_t i, double &x, double &y, double &z)
{
    if (AOS) { x = (double)a[3 * i]; y = (double)a[3 * i + 1]; z = (double)a[3 * i + 2]; }
    else { x = (double)a[i]; y = (double)a[stride + i]; z = (double)a[2 * stride + i]; }
}

// ---- label: labels, dist
template <typename T, bool AOS, bool NRM>
__global__ void __launch_bounds__(ASG_BLOCK) asg_label_kernel(const asg_job J)
{
    const int lane = threadIdx.x & 63;
    const int64_t wbase = (int64_t)blockIdx.x * ASG_TILE + (int64_t)(threadIdx.x >> 6) * (64 * ASG_PPT);
    if (wbase >= J.n) return;   // (wave-uniform)
    double px[ASG_PPT], py[ASG_PPT], pz[ASG_PPT], nx[ASG_PPT], ny[ASG_PPT], nz[ASG_PPT], best[ASG_PPT];
    int32_t lab[ASG_PPT];
#pragma unroll
    for (int r = 0; r < ASG_PPT; r++) {
        const int64_t i = wbase + r * 64 + lane;
        const int64_t ic = i < J.n ? i : J.n - 1;   // lanes past the end stay in the wave (the ballots) and store nothing
        load3<T, AOS>((const T *)J.xyz, J.stride, ic, px[r], py[r], pz[r]);
        if (NRM) load3<T, AOS>((const T *)J.nrm, J.stride, ic, nx[r], ny[r], nz[r]);
        else nx[r] = ny[r] = nz[r] = 0.0;
        best[r] = INFINITY;
        lab[r] = 0;
    }
    for (int32_t j = 0; j < J.b; j++) {   // (wave-uniform)
        const rh_prep P = rh_ld_prep_const(J.prep + j);
        const int kind = ((const RH_CONST_AS rh_shape *)(uintptr_t)(J.shapes + j))->kind;
#define ASG_ROUNDS(CLAIM, K)                                                                                              \
    _Pragma("unroll") for (int r = 0; r < ASG_PPT; r++) {                                                                \
        double d;                                                                                                         \
        if (CLAIM<NRM>(P, px[r], py[r], pz[r], nx[r], ny[r], nz[r], J.eps[K], J.cosa[K], d) && d < best[r]) {             \
            best[r] = d;                                                                                                  \
            lab[r] = j + 1;                                                                                               \
        }                                                                                                                 \
    }
        switch (kind) {
        case RH_PLANE: ASG_ROUNDS(rhasg::claim_plane, RH_PLANE) break;
        case RH_SPHERE: ASG_ROUNDS(rhasg::claim_sphere, RH_SPHERE) break;
        case RH_CYLINDER: ASG_ROUNDS(rhasg::claim_cylinder, RH_CYLINDER) break;
        case RH_CONE: ASG_ROUNDS(rhasg::claim_cone, RH_CONE) break;
        default: break;   // (a device-resident shape of no known kind claims nothing)
        }
#undef ASG_ROUNDS
    }
    const int64_t nwords = (J.n + 63) >> 6;
#pragma unroll
    for (int r = 0; r < ASG_PPT; r++) {
        const int64_t i = wbase + r * 64 + lane;
        if (i >= J.n) continue;
        if (J.enabled != nullptr) {
            const int64_t w = (wbase + r * 64) >> 6;   // one word per wave and round
            const uint64_t word = w < nwords ? J.enabled[w] : 0ULL;
            if (!((word >> lane) & 1ULL)) lab[r] = 0;
        }
        J.labels[i] = lab[r];
        if (J.dist != nullptr) J.dist[i] = lab[r] != 0 ? best[r] : -1.0;
    }
}

// label of point i as a key 0 .. b, -1 for no point (past the end; or a word that is no label: never written by the
// label kernel, but nothing becomes an address unchecked)
__device__ __forceinline__ int32_t key_of(const asg_job &J, int64_t i)
{
    if (i >= J.n) return -1;
    const int32_t l = J.labels[i];
    return (uint32_t)l <= (uint32_t)J.b ? l : -1;
}

// a wave counts the labels of its quarter of run k into its LDS row (zeroed by the caller): per round, the first lane
// of every distinct key adds the number of lanes that hold it
__device__ __forceinline__ void count_quarter(const asg_job &J, int64_t k, int32_t *__restrict__ row)
{
    const int lane = threadIdx.x & 63;
    const int64_t wbase = k * ASG_RUN + (int64_t)(threadIdx.x >> 6) * ASG_WRUN;
    for (int r = 0; r < ASG_WRUN / 64; r++) {
        if (wbase + r * 64 >= J.n) break;   // (wave-uniform)
        const int32_t key = key_of(J, wbase + r * 64 + lane);
        wave_each_key(key >= 0, key, [&](int leader, int32_t L, uint64_t m) {
            if (lane == leader) row[L] += __popcll(m);
        });
    }
}

// ---- count: one row of the matrix per run
__global__ void __launch_bounds__(ASG_BLOCK) asg_count_kernel(const asg_job J)
{
    extern __shared__ int32_t sh[];   // [ASG_WAVES][b + 1]
    const int nl = J.b + 1;
    for (int t = threadIdx.x; t < ASG_WAVES * nl; t += ASG_BLOCK) sh[t] = 0;
    __syncthreads();
    const int64_t k = blockIdx.x;
    count_quarter(J, k, sh + (threadIdx.x >> 6) * nl);
    __syncthreads();
    for (int L = threadIdx.x; L < nl; L += ASG_BLOCK) {
        int32_t v = 0;
#pragma unroll
        for (int w = 0; w < ASG_WAVES; w++) v += sh[w * nl + L];
        J.mat[k * nl + L] = v;
    }
}

// ---- colscan: exclusive prefix down every column of the matrix, the column sums -> tot
__global__ void __launch_bounds__(ASG_SCAN_WAVES * 64) asg_colscan_kernel(const asg_job J)
{
    __shared__ int64_t part[ASG_SCAN_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nl = J.b + 1;
    const int L = blockIdx.x * 64 + lane;
    const int64_t per = (J.nruns + ASG_SCAN_WAVES - 1) / ASG_SCAN_WAVES;
    const int64_t k0 = w * per, k1 = k0 + per < J.nruns ? k0 + per : J.nruns;
    int64_t s = 0;
    if (L < nl)
        for (int64_t k = k0; k < k1; k++) s += J.mat[k * nl + L];
    part[w][lane] = s;
    __syncthreads();
    int64_t run = 0;
    for (int v = 0; v < w; v++) run += part[v][lane];
    if (L >= nl) return;
    if (w == ASG_SCAN_WAVES - 1) J.tot[L] = run + s;
    for (int64_t k = k0; k < k1; k++) {
        const int32_t c = J.mat[k * nl + L];
        J.mat[k * nl + L] = (int32_t)run;   // (< n < 2^31)
        run += c;
    }
}

// ---- offsets: one wave, lane l takes the labels l * per ..; exclusive prefix over the counts
__global__ void __launch_bounds__(64) asg_offsets_kernel(const asg_job J)
{
    const int lane = threadIdx.x;
    const int nl = J.b + 1;
    const int per = (nl + 63) / 64;
    const int L0 = lane * per, L1 = L0 + per < nl ? L0 + per : nl;
    int64_t s = 0;
    for (int L = L0; L < L1; L++) s += J.tot[L];
    int64_t incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    int64_t run = incl - s;
    for (int L = L0; L < L1; L++) {
        const int64_t c = J.tot[L];
        J.off[L] = run;
        if (J.offsets != nullptr) J.offsets[L] = run;
        if (J.counts != nullptr) J.counts[L] = c;
        run += c;
    }
    if (lane == 63) {   // (the last lane's inclusive sum is every point)
        J.off[nl] = incl;
        if (J.offsets != nullptr) J.offsets[nl] = incl;
    }
}

// ---- scatter: the stable partition
__global__ void __launch_bounds__(ASG_BLOCK) asg_scatter_kernel(const asg_job J)
{
    extern __shared__ int32_t sh[];   // [ASG_WAVES][b + 1]: counts, then cursors
    const int nl = J.b + 1;
    const int lane = threadIdx.x & 63;
    for (int t = threadIdx.x; t < ASG_WAVES * nl; t += ASG_BLOCK) sh[t] = 0;
    __syncthreads();
    const int64_t k = blockIdx.x;
    int32_t *row = sh + (threadIdx.x >> 6) * nl;
    count_quarter(J, k, row);
    __syncthreads();
    for (int L = threadIdx.x; L < nl; L += ASG_BLOCK) {
        int64_t at = J.off[L] + J.mat[k * nl + L];
#pragma unroll
        for (int w = 0; w < ASG_WAVES; w++) {
            const int32_t c = sh[w * nl + L];
            sh[w * nl + L] = (int32_t)at;   // (<= n < 2^31)
            at += c;
        }
    }
    __syncthreads();
    const int64_t wbase = k * ASG_RUN + (int64_t)(threadIdx.x >> 6) * ASG_WRUN;
    for (int r = 0; r < ASG_WRUN / 64; r++) {
        if (wbase + r * 64 >= J.n) break;   // (wave-uniform)
        const int64_t i = wbase + r * 64 + lane;
        const int32_t key = key_of(J, i);
        wave_each_key(key >= 0, key, [&](int leader, int32_t L, uint64_t m) {
            int32_t at = 0;
            if (lane == leader) { at = row[L]; row[L] = at + __popcll(m); }   // (the leader alone touches the cursor)
            at = __shfl(at, leader);
            if (key == L) {
                const int64_t pos = (int64_t)at + __popcll(m & ((1ULL << lane) - 1ULL));
                if ((uint64_t)pos < (uint64_t)J.n) J.idx[pos] = i + 1;
            }
        });
    }
}

enum { SRC_AOS64 = 0, SRC_AOS32 = 1, SRC_PLANES64 = 2, SRC_PLANES32 = 3 };

inline int64_t runs_of(int64_t n) { return (n + ASG_RUN - 1) / ASG_RUN; }

// where the workspace's parts lie (prep, mat, tot, off) and how large it is
struct asg_ws_layout { size_t prep, mat, tot, off, bytes; };
asg_ws_layout ws_layout(int64_t n, int32_t b, bool lists_or_counts)
{
    asg_ws_layout W;
    W.prep = 0;
    W.mat = up16(sizeof(rh_prep) * (size_t)(b > 0 ? b : 1));
    W.tot = W.mat + up16(lists_or_counts ? sizeof(int32_t) * (size_t)runs_of(n) * (size_t)(b + 1) : 0);
    W.off = W.tot + up16(sizeof(int64_t) * (size_t)(b + 1));
    W.bytes = W.off + up16(sizeof(int64_t) * (size_t)(b + 2));
    return W;
}
void ws_bind(asg_job &J, void *ws, const asg_ws_layout &W)
{
    char *d = (char *)ws;
    J.prep = (const rh_prep *)(d + W.prep);
    J.mat = (int32_t *)(d + W.mat);
    J.tot = (int64_t *)(d + W.tot);
    J.off = (int64_t *)(d + W.off);
}

template <typename T, bool AOS>
void launch_label(hipStream_t st, const asg_job &J)
{
    const dim3 g((unsigned)((J.n + ASG_TILE - 1) / ASG_TILE)), blk(ASG_BLOCK);
    if (J.nrm != nullptr) hipLaunchKernelGGL((asg_label_kernel<T, AOS, true>), g, blk, 0, st, J);
    else hipLaunchKernelGGL((asg_label_kernel<T, AOS, false>), g, blk, 0, st, J);
}

// the launches (everything in J is on the device, n >= 1, the workspace bound and the records in J.prep made)
int asg_enqueue(hipStream_t st, const asg_job &J, int src)
{
    switch (src) {
    case SRC_AOS64: launch_label<double, true>(st, J); break;
    case SRC_AOS32: launch_label<float, true>(st, J); break;
    case SRC_PLANES64: launch_label<double, false>(st, J); break;
    default: launch_label<float, false>(st, J); break;
    }
    if (J.counts != nullptr || J.idx != nullptr) {
        const size_t lds = sizeof(int32_t) * ASG_WAVES * (size_t)(J.b + 1);   // <= 16 400 bytes
        hipLaunchKernelGGL(asg_count_kernel, dim3((unsigned)J.nruns), dim3(ASG_BLOCK), lds, st, J);
        hipLaunchKernelGGL(asg_colscan_kernel, dim3((unsigned)((J.b + 1 + 63) / 64)), dim3(ASG_SCAN_WAVES * 64), 0, st, J);
        hipLaunchKernelGGL(asg_offsets_kernel, dim3(1), dim3(64), 0, st, J);
        if (J.idx != nullptr) hipLaunchKernelGGL(asg_scatter_kernel, dim3((unsigned)J.nruns), dim3(ASG_BLOCK), lds, st, J);
    }
    RH_HIP(hipGetLastError());
    return RH_OK;
}

// what every entry checks before its first device call; shapes: host shapes or null (device-resident)
int asg_check(const char *who, bool have_points, int64_t n, const rh_shape *host_shapes, bool have_shapes, int32_t b,
              const rh_params *p, int32_t flags, int32_t allowed, const void *labels, const void *offsets, const void *idx)
{
    if (flags & ~allowed) { rh_set_error("%s: flags = %d: unknown or not allowed here", who, flags); return RH_E_INVALID; }
    if (b < 0 || b > RH_ASSIGN_MAX_SHAPES) { rh_set_error("%s: b = %d outside 0 .. %d", who, b, RH_ASSIGN_MAX_SHAPES); return RH_E_INVALID; }
    if (n < 0 || n >= ((int64_t)1 << 31)) { rh_set_error("%s: n = %lld outside 0 .. 2^31 - 1", who, (long long)n); return RH_E_INVALID; }
    if (!p || (b > 0 && !have_shapes) || (n > 0 && (!have_points || !labels))) { rh_set_error("%s: null argument", who); return RH_E_INVALID; }
    if ((offsets != nullptr) != (idx != nullptr)) {
        rh_set_error("%s: lists take offsets and idx, both or neither", who);
        return RH_E_INVALID;
    }
    if (host_shapes)
        for (int32_t j = 0; j < b; j++)
            if (host_shapes[j].kind < 0 || host_shapes[j].kind > 3) { rh_set_error("%s: shape %d has kind %d", who, j, host_shapes[j].kind); return RH_E_INVALID; }
    return RH_OK;
}

void fill_thresholds(asg_job &J, const rh_params *p)
{
    for (int k = 0; k < 4; k++) { J.eps[k] = p->eps[k]; J.cosa[k] = p->cos_alpha[k]; }
}

// b == 0 or n == 0 on host arrays: nothing to compute
void trivial_result(int64_t n, int32_t b, int32_t *labels, double *dist, int64_t *counts, int64_t *offsets, int64_t *idx)
{
    for (int64_t i = 0; i < n; i++) labels[i] = 0;
    if (dist) for (int64_t i = 0; i < n; i++) dist[i] = -1.0;
    if (counts) { counts[0] = n; for (int32_t j = 1; j <= b; j++) counts[j] = 0; }
    if (offsets) { offsets[0] = 0; for (int32_t j = 1; j <= b + 1; j++) offsets[j] = n; }
    if (idx) for (int64_t i = 0; i < n; i++) idx[i] = i + 1;
}

template <typename T>
int assign_raw(const char *who, const T *xyz, const T *nrm, int64_t n, const rh_shape *shapes, int32_t b, const rh_params *p,
               int32_t flags, int device, int32_t *labels, double *dist, int64_t *counts, int64_t *offsets, int64_t *idx)
{
    RH_TRY(asg_check(who, xyz != nullptr, n, shapes, shapes != nullptr, b, p, flags, RH_ASSIGN_NO_NORMALS, labels, offsets, idx));
    if (n == 0 || b == 0) { trivial_result(n, b, labels, dist, counts, offsets, idx); return RH_OK; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const bool use_nrm = nrm != nullptr && !(flags & RH_ASSIGN_NO_NORMALS);
    const bool tally = counts != nullptr || idx != nullptr;
    asg_job J;
    memset(&J, 0, sizeof J);
    J.n = n; J.b = b; J.nruns = runs_of(n);
    fill_thresholds(J, p);
    T *d_xyz = nullptr, *d_nrm = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    SCOPE_HIP(S, hipMemcpyAsync(d_xyz, xyz, sizeof(T) * 3 * (size_t)n, hipMemcpyHostToDevice, S.st));
    if (use_nrm) {
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        SCOPE_HIP(S, hipMemcpyAsync(d_nrm, nrm, sizeof(T) * 3 * (size_t)n, hipMemcpyHostToDevice, S.st));
    }
    J.xyz = d_xyz; J.nrm = d_nrm;
    const asg_ws_layout W = ws_layout(n, b, tally);
    char *d_ws = nullptr;
    RH_TRY(S.alloc(&d_ws, (int64_t)W.bytes));
    ws_bind(J, d_ws, W);
    std::vector<rh_prep> prep((size_t)b);
    for (int32_t j = 0; j < b; j++) rh_prep_host(shapes[j], &prep[(size_t)j]);
    rh_shape *d_shapes = nullptr;
    RH_TRY(S.alloc(&d_shapes, b));
    SCOPE_HIP(S, hipMemcpyAsync(d_shapes, shapes, sizeof(rh_shape) * (size_t)b, hipMemcpyHostToDevice, S.st));
    SCOPE_HIP(S, hipMemcpyAsync((void *)J.prep, prep.data(), sizeof(rh_prep) * (size_t)b, hipMemcpyHostToDevice, S.st));
    J.shapes = d_shapes;
    RH_TRY(S.alloc(&J.labels, n));
    if (dist) RH_TRY(S.alloc(&J.dist, n));
    if (counts) RH_TRY(S.alloc(&J.counts, b + 1));
    if (idx) {
        RH_TRY(S.alloc(&J.offsets, b + 2));
        RH_TRY(S.alloc(&J.idx, n));
    }
    RH_TRY(asg_enqueue(S.st, J, sizeof(T) == sizeof(double) ? SRC_AOS64 : SRC_AOS32));
    SCOPE_HIP(S, hipMemcpyAsync(labels, J.labels, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, S.st));
    if (dist) SCOPE_HIP(S, hipMemcpyAsync(dist, J.dist, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, S.st));
    if (counts) SCOPE_HIP(S, hipMemcpyAsync(counts, J.counts, sizeof(int64_t) * (size_t)(b + 1), hipMemcpyDeviceToHost, S.st));
    if (idx) {
        SCOPE_HIP(S, hipMemcpyAsync(offsets, J.offsets, sizeof(int64_t) * (size_t)(b + 2), hipMemcpyDeviceToHost, S.st));
        SCOPE_HIP(S, hipMemcpyAsync(idx, J.idx, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, S.st));
    }
    SCOPE_HIP(S, hipStreamSynchronize(S.st));
    return RH_OK;
}

// the cloud entries' common part: workspace, records, launches on the cloud's stream (d_shapes and the outputs on the device)
int assign_cloud_enqueue(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p, int32_t flags, int32_t *d_labels,
                         double *d_dist, int64_t *d_counts, int64_t *d_offsets, int64_t *d_idx)
{
    asg_job J;
    memset(&J, 0, sizeof J);
    J.n = c->n; J.b = b; J.nruns = runs_of(c->n); J.stride = c->n_pad;
    fill_thresholds(J, p);
    const asg_ws_layout W = ws_layout(c->n, b, d_counts != nullptr || d_idx != nullptr);
    if ((int64_t)W.bytes > c->asg_ws.count()) RH_TRY(c->asg_ws.grow(c->stream, (int64_t)W.bytes));
    ws_bind(J, c->asg_ws, W);
    if (b > 0) RH_TRY(rhk_prep_records(c, d_shapes, b, const_cast<rh_prep *>(J.prep)));   // made on the device by the score path's own prep kernel
    J.shapes = d_shapes;
    const bool use_nrm = !(flags & RH_ASSIGN_NO_NORMALS);
    if (c->f32) { J.xyz = c->full32; J.nrm = use_nrm ? c->full32 + 3 * c->n_pad : nullptr; }
    else { J.xyz = c->full; J.nrm = use_nrm ? c->full + 3 * c->n_pad : nullptr; }
    J.enabled = (flags & RH_ASSIGN_ENABLED_ONLY) ? c->enabled : nullptr;
    J.labels = d_labels; J.dist = d_dist; J.counts = d_counts; J.offsets = d_offsets; J.idx = d_idx;
    return asg_enqueue(c->stream, J, c->f32 ? SRC_PLANES32 : SRC_PLANES64);
}

}  // namespace

extern "C" int rh_assign_points(const double *xyz_aos, const double *nrm_aos_or_null, int64_t n, const rh_shape *shapes, int32_t b,
                                const rh_params *p, int32_t flags, int device, int32_t *labels_out, double *dist_out_or_null,
                                int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null)
{
    return assign_raw<double>("rh_assign_points", xyz_aos, nrm_aos_or_null, n, shapes, b, p, flags, device, labels_out, dist_out_or_null,
                              counts_out_or_null, offsets_out_or_null, idx_out_or_null);
}

extern "C" int rh_assign_points_f32(const float *xyz_aos, const float *nrm_aos_or_null, int64_t n, const rh_shape *shapes, int32_t b,
                                    const rh_params *p, int32_t flags, int device, int32_t *labels_out, double *dist_out_or_null,
                                    int64_t *counts_out_or_null, int64_t *offsets_out_or_null, int64_t *idx_out_or_null)
{
    return assign_raw<float>("rh_assign_points_f32", xyz_aos, nrm_aos_or_null, n, shapes, b, p, flags, device, labels_out,
                             dist_out_or_null, counts_out_or_null, offsets_out_or_null, idx_out_or_null);
}

extern "C" int rh_cloud_assign_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p, int32_t flags,
                                   int32_t *d_labels, double *d_dist_or_null, int64_t *d_counts_or_null, int64_t *d_offsets_or_null,
                                   int64_t *d_idx_or_null)
{
    const char *who = "rh_cloud_assign_dev";
    if (!c) { rh_set_error("%s: null cloud", who); return RH_E_INVALID; }
    RH_TRY(asg_check(who, true, c->n, nullptr, d_shapes != nullptr, b, p, flags, RH_ASSIGN_NO_NORMALS | RH_ASSIGN_ENABLED_ONLY, d_labels,
                     d_offsets_or_null, d_idx_or_null));
    RH_TRY(rh_cloud_join(c));
    if (c->n == 0) return RH_OK;
    return assign_cloud_enqueue(c, d_shapes, b, p, flags, d_labels, d_dist_or_null, d_counts_or_null, d_offsets_or_null, d_idx_or_null);
}

extern "C" int rh_cloud_assign(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, int32_t flags, int32_t *labels_out,
                               double *dist_out_or_null, int64_t *counts_out_or_null, int64_t *offsets_out_or_null,
                               int64_t *idx_out_or_null)
{
    const char *who = "rh_cloud_assign";
    if (!c) { rh_set_error("%s: null cloud", who); return RH_E_INVALID; }
    RH_TRY(asg_check(who, true, c->n, shapes, shapes != nullptr, b, p, flags, RH_ASSIGN_NO_NORMALS | RH_ASSIGN_ENABLED_ONLY, labels_out,
                     offsets_out_or_null, idx_out_or_null));
    RH_TRY(rh_cloud_join(c));
    const int64_t n = c->n;
    if (n == 0) { trivial_result(0, b, labels_out, dist_out_or_null, counts_out_or_null, offsets_out_or_null, idx_out_or_null); return RH_OK; }
    // the shapes through the pinned block; the outputs in one device block, read back behind the launches: one wait
    const size_t o_shapes = 0, o_lab = up16(sizeof(rh_shape) * (size_t)b), o_dist = o_lab + up16(sizeof(int32_t) * (size_t)n),
                 o_cnt = o_dist + up16(dist_out_or_null ? sizeof(double) * (size_t)n : 0),
                 o_off = o_cnt + up16(sizeof(int64_t) * (size_t)(b + 1)), o_idx = o_off + up16(sizeof(int64_t) * (size_t)(b + 2)),
                 bytes = o_idx + up16(idx_out_or_null ? sizeof(int64_t) * (size_t)n : 0);
    if ((int64_t)bytes > c->asg_io.count()) RH_TRY(c->asg_io.grow(c->stream, (int64_t)bytes));
    char *d = c->asg_io;
    if (b > 0) {
        RH_TRY(rh_ensure_pin(c, (int64_t)o_lab));
        memcpy(c->h_pin, shapes, sizeof(rh_shape) * (size_t)b);
        RH_HIP(hipMemcpyAsync(d + o_shapes, c->h_pin, sizeof(rh_shape) * (size_t)b, hipMemcpyHostToDevice, c->stream));
    }
    RH_TRY(assign_cloud_enqueue(c, (const rh_shape *)(d + o_shapes), b, p, flags, (int32_t *)(d + o_lab),
                                dist_out_or_null ? (double *)(d + o_dist) : nullptr, counts_out_or_null ? (int64_t *)(d + o_cnt) : nullptr,
                                idx_out_or_null ? (int64_t *)(d + o_off) : nullptr, idx_out_or_null ? (int64_t *)(d + o_idx) : nullptr));
    RH_HIP(hipMemcpyAsync(labels_out, d + o_lab, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (dist_out_or_null) RH_HIP(hipMemcpyAsync(dist_out_or_null, d + o_dist, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (counts_out_or_null) RH_HIP(hipMemcpyAsync(counts_out_or_null, d + o_cnt, sizeof(int64_t) * (size_t)(b + 1), hipMemcpyDeviceToHost, c->stream));
    if (idx_out_or_null) {
        RH_HIP(hipMemcpyAsync(offsets_out_or_null, d + o_off, sizeof(int64_t) * (size_t)(b + 2), hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipMemcpyAsync(idx_out_or_null, d + o_idx, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}
