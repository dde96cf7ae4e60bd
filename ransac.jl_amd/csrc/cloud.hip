// cloud.hip -- C-ABI entry points around the device-resident cloud (include/ransac_hip.h).
#include <functional>
#include <system_error>
#include <thread>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "rh_internal.h"
#include "score4_device.h"

// ---------------------------------------------------------------- errors ----
static thread_local char g_err[512] = "";

void rh_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *rh_last_error(void) { return g_err; }
extern "C" int rh_version(void) { return RH_VERSION; }

extern "C" int rh_device_count(int *n_out)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *n_out = 0;
        rh_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return RH_E_NODEVICE;
    }
    *n_out = n;
    return RH_OK;
}

int rh_validate_params(const rh_params *p)
{
    if (!p) { rh_set_error("params is NULL"); return RH_E_INVALID; }
    for (int k = 0; k < 4; k++)
        if (!(p->eps[k] == p->eps[k]) || !(p->cos_alpha[k] == p->cos_alpha[k])) {
            rh_set_error("params: eps/cos_alpha of kind %d is NaN", k);
            return RH_E_INVALID;
        }
    return RH_OK;
}

// ------------------------------------------------------------ allocation ----
int rh_ensure_pin(rh_cloud *c, int64_t bytes)
{
    if (bytes <= c->h_pin.count()) return RH_OK;
    return c->h_pin.alloc(std::max<int64_t>(bytes, 1 << 20));
}

int rh_ensure_batch(rh_cloud *c, rh_batch_ws &w, int64_t b)
{
    if (b <= w.batch_cap) return RH_OK;
    const int64_t cap = std::max<int64_t>(b, std::max<int64_t>(1024, w.batch_cap * 2));
    w.batch_cap = 0;
    RH_TRY(w.d_shapes.grow(c->stream, cap));
    RH_TRY(w.d_prep.grow(c->stream, 4 * cap));
    RH_TRY(w.d_qpre.grow(c->stream, 4 * cap * 64));   // rh4::rh_cls (64 B) per slot
    RH_TRY(w.d_box.grow(c->stream, (int64_t)rh4::RH_BOX_FIELDS * 4 * cap));
    RH_TRY(w.d_orig.grow(c->stream, 4 * cap));
    RH_TRY(w.d_counts.grow(c->stream, cap));
    w.batch_cap = cap;
    return RH_OK;
}

// Where a batch's masks go before they are un-permuted.  The culled kernel (the batch has classifier records) leaves entry
// lists: nothing to zero but, once, the new cursors.  The brute-force kernels OR into dense rows in internal order.
static int rh_masks_begin(rh_cloud *c, rh_batch_ws &w, int32_t b, bool culled)
{
    w.masks4 = false;
    if (culled) {
        w.mstride4 = (c->ngroups + 7) / 8 * 8;
        const int64_t words = 2 * b * w.mstride4;      // (two 64-bit words per entry)
        if (words > w.d_masks_int.count()) RH_TRY(w.d_masks_int.grow(c->stream, words));
        const int64_t cur_bytes = 4 * (int64_t)b;
        if (cur_bytes > w.d_occ.count()) {
            RH_TRY(w.d_occ.grow(c->stream, cur_bytes));
            const hipError_t ez = hipMemsetAsync(w.d_occ, 0, (size_t)cur_bytes, c->stream);
            if (ez != hipSuccess) w.d_occ.reset();   // (cursors that are not zero are no cursors)
            RH_HIP(ez);
        }
        w.masks4 = true;
        return RH_OK;
    }
    const int64_t words = (int64_t)b * c->swords;
    if (words > w.d_masks_int.count()) RH_TRY(w.d_masks_int.grow(c->stream, words));
    RH_HIP(hipMemsetAsync(w.d_masks_int, 0, sizeof(uint64_t) * (size_t)words, c->stream));
    return RH_OK;
}

// ... and from there to d_masks: dense rows in subset order
static int rh_masks_finish(rh_cloud *c, rh_batch_ws &w, int32_t b, uint64_t *d_masks)
{
    const bool lists = w.masks4;
    w.masks4 = false;
    return lists ? rhk_unpermute_masks4(c, w, b, d_masks) : rhk_unpermute_masks(c, w.d_masks_int, b, d_masks);
}

// 63-bit Morton code of a point inside the subset's bounding box (21 bits per axis)
static inline uint64_t spread21(uint64_t v)
{
    v &= 0x1FFFFFULL;
    v = (v | (v << 32)) & 0x1F00000000FFFFULL;
    v = (v | (v << 16)) & 0x1F0000FF0000FFULL;
    v = (v | (v << 8)) & 0x100F00F00F00F00FULL;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ULL;
    v = (v | (v << 2)) & 0x1249249249249249ULL;
    return v;
}

// a batch workspace goes: its stream is waited for and destroyed, the assignment releases its buffers and events
static void batch_ws_free(rh_batch_ws &w)
{
    if (w.stream) (void)hipStreamSynchronize(w.stream);
    if (w.stream) (void)hipStreamDestroy(w.stream);
    w = rh_batch_ws();
}

static void cloud_free(rh_cloud *c)
{
    if (!c) return;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    // a caller's stream (rh_cloud_set_stream) may be gone by now: wait for the device instead of the handle
    if (c->stream != c->own_stream) (void)hipDeviceSynchronize();
    else if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (rh_batch_ws &w : c->ws) batch_ws_free(w);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int k = 0; k < 5; k++)
        if (c->evk[k]) (void)hipEventDestroy(c->evk[k]);
    if (c->ev_cull) (void)hipEventDestroy(c->ev_cull);
    c->stream = c->own_stream;   // (the deleter below waits on c->stream; everything has finished by now)
    if (c->drv_cache != nullptr && c->drv_cache_free != nullptr) c->drv_cache_free(c, c->drv_cache);
    c->drv_cache = nullptr;
    if (c->ev_copied) (void)hipEventDestroy(c->ev_copied);
    if (c->ev_sync) (void)hipEventDestroy(c->ev_sync);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;   // (the buffers go with it: every stream that used them has been waited for above)
}

// bounding cube of the cloud like the reference's octree (findAABB: src/utilities.jl:125-136; the cube's edge is the
// largest extent) and the largest finite |coordinate|
static void cloud_aabb(const double *xyz, int64_t n, double lo[3], double *size_out, double *mag_out)
{
    double hi[3] = { 0, 0, 0 }, mag = 0;
    for (int k = 0; k < 3; k++) lo[k] = 0;
    for (int k = 0; k < 3 && n > 0; k++) { lo[k] = xyz[k]; hi[k] = xyz[k]; }
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const double a = xyz[3 * i + k];
            lo[k] = lo[k] > a ? a : lo[k];
            hi[k] = hi[k] < a ? a : hi[k];
            const double m = fabs(a);
            if (m > mag && m - m == 0) mag = m;
        }
    double size = 0;
    for (int k = 0; k < 3; k++) if (hi[k] - lo[k] > size) size = hi[k] - lo[k];
    size = size * (1 + 1e-9);
    if (!(size > 0)) size = 1;
    *size_out = size;
    *mag_out = mag;
}

// the same box from the uploaded copy (rhk_cloud_aabb, kdorder.hip).  The host loop's lo / hi start at the first point and
// move by plain comparisons, so a NaN in the first point stays (every comparison with it is false) and any other NaN is
// skipped; infinities take part.  Same values, bit for bit: the Morton codes (and the oracle's octree) hang on them.
static int cloud_aabb_device(rh_cloud *c, const double *d_xyz, const double *xyz, int64_t n)
{
    double lo[3], hi[3], mag = 0;
    bool has[3];
    RH_TRY(rhk_cloud_aabb(c, d_xyz, n, lo, hi, has, &mag));
    for (int k = 0; k < 3; k++) {
        const double first = n > 0 ? xyz[k] : 0.0;
        if (n > 0 && !(first == first)) { lo[k] = first; hi[k] = first; }   // a NaN first point: nothing ever replaces it
        else if (!has[k]) { lo[k] = 0; hi[k] = 0; }
        c->k_lo[k] = lo[k];
    }
    double size = 0;
    for (int k = 0; k < 3; k++) if (hi[k] - lo[k] > size) size = hi[k] - lo[k];
    size = size * (1 + 1e-9);
    if (!(size > 0)) size = 1;
    c->k_size = size;
    c->k_mag = mag;
    return RH_OK;
}

// linear (Morton) octree of the full cloud: codes in the bounding CUBE, sorted by (code, index) -- the Morton order the
// cloud was given on the device when it was created (korder.hip); here: the host twins and
// depth = first level whose fullest cell holds <= 8 points (src/octree.jl:163-165), capped.
int rh_octree_ensure(rh_cloud *c, const double *xyz, int max_depth)
{
    (void)xyz;
    if (max_depth < 1) max_depth = 1;
    if (max_depth > 21) max_depth = 21;
    if (c->oct_built && c->oct_max_depth == max_depth) return rhk_oct_sync_enabled(c);
    const int64_t n = c->n;
    if (n > 0 && !c->k_built) { rh_set_error("rh_octree_ensure: the cloud has no Morton order"); return RH_E_INTERNAL; }
    c->h_oct_code.resize((size_t)n);
    c->h_oct_perm.resize((size_t)n);
    c->h_oct_pos.resize((size_t)n);
    if (n > 0) {
        RH_HIP(hipMemcpyAsync(c->h_oct_code.data(), c->oct_code, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipMemcpyAsync(c->h_oct_perm.data(), c->oct_perm, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipMemcpyAsync(c->h_oct_pos.data(), c->oct_pos, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipStreamSynchronize(c->stream));
    }
    int depth = max_depth;
    for (int l = 1; l <= max_depth; l++) {
        const int shift = 3 * (21 - (l - 1));
        int64_t run = 0, best = 0;
        uint64_t prev = 0;
        for (int64_t i = 0; i < n; i++) {
            const uint64_t key = shift >= 63 ? 0 : (c->h_oct_code[(size_t)i] >> shift);
            if (i == 0 || key != prev) { run = 0; prev = key; }
            if (++run > best) best = run;
        }
        if (best <= 8) { depth = l; break; }
    }
    c->oct_depth = depth;
    c->oct_max_depth = max_depth;
    RH_TRY(rhk_oct_build_tab(c));
    c->oct_built = true;
    return rhk_oct_sync_enabled(c);
}

// ------------------------------------------------------------------ cloud ----
extern "C" int rh_cloud_create(const double *xyz, const double *nrm, int64_t n, const int64_t *subset1, int64_t s,
                               int device, rh_cloud **out)
{
    if (!out) { rh_set_error("out is NULL"); return RH_E_INVALID; }
    *out = nullptr;
    if (n < 0 || s < 0 || (n > 0 && (!xyz || !nrm)) || (s > 0 && !subset1)) {
        rh_set_error("rh_cloud_create: bad arguments (n=%lld s=%lld)", (long long)n, (long long)s);
        return RH_E_INVALID;
    }
    if (n > (int64_t)0x7FFFF000) { rh_set_error("clouds above 2^31 points are not supported"); return RH_E_INVALID; }
    for (int64_t j = 0; j < s; j++)
        if (subset1[j] < 1 || subset1[j] > n) {
            rh_set_error("subset index %lld at position %lld outside 1..%lld", (long long)subset1[j], (long long)j,
                         (long long)n);
            return RH_E_INVALID;
        }
    if (n > 2000000000LL) {   // internal indices (subset gather, select list, octree permutation) are int32
        rh_set_error("rh_cloud_create: %lld points exceed the 2e9 limit of one cloud", (long long)n);
        return RH_E_INVALID;
    }
    int ndev = 0;
    RH_TRY(rh_device_count(&ndev));
    if (ndev <= 0) { rh_set_error("no HIP device is visible; libransac_hip has no CPU fallback"); return RH_E_NODEVICE; }
    if (device < 0 || device >= ndev) { rh_set_error("device %d out of range (%d visible)", device, ndev); return RH_E_INVALID; }
    RH_HIP(hipSetDevice(device));
    const auto tc0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    double ms_kd = 0, ms_before_kd = 0;
    // RH_CREATE_PROF=1: wall time of every stage on stderr (each stamp waits for the stream: the stages stop overlapping)
    const bool prof = rh_opt_on(nullptr, RH_OPT_CREATE_PROF);
    double t_prev = 0;

    rh_cloud *c = new (std::nothrow) rh_cloud();
    if (!c) { rh_set_error("out of host memory"); return RH_E_NOMEM; }
    rh_opt_init_cloud(c);
    c->device = device;
    c->n = n;
    c->s = s;
    c->n_pad = ((n + RH_SC_TILE - 1) / RH_SC_TILE) * RH_SC_TILE;
    c->s_pad = ((s + RH_SC_TILE - 1) / RH_SC_TILE) * RH_SC_TILE;
    if (c->n_pad == 0) c->n_pad = RH_SC_TILE;
    if (c->s_pad == 0) c->s_pad = RH_SC_TILE;
    c->nwords = (n + 63) / 64;
    c->swords = (s + 63) / 64;
    c->nblocks = (c->nwords + RH_WORDS_PER_BLOCK - 1) / RH_WORDS_PER_BLOCK;
    c->dis_stride = c->s_pad + RH_SC_TILE;

    int rc = RH_OK;
    rh_dev<double> t_xyz, t_nrm;
    std::unique_ptr<int32_t[]> h_idx_own;
    int32_t *h_idx = nullptr;
    auto stamp = [&](const char *what) {
        if (!prof) return;
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        const double t = ms_since(tc0);
        fprintf(stderr, "[rh_cloud_create] %-28s %8.2f ms\n", what, t - t_prev);
        t_prev = t;
    };
    auto fail = [&](int code) {
        cloud_free(c);
        return code;
    };
#define CK(x) do { rc = (x); if (rc != RH_OK) return fail(rc); } while (0)
#define CKH(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { rh_set_error("%s: %s", #x, hipGetErrorString(e_)); return fail(RH_E_NODEVICE); } } while (0)
    CKH(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CKH(hipEventCreate(&c->ev0));
    CKH(hipEventCreate(&c->ev1));
    for (int k = 0; k < 5; k++) CKH(hipEventCreate(&c->evk[k]));
    CKH(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    CKH(hipEventCreateWithFlags(&c->ev_copied, hipEventDisableTiming));
    CKH(hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming));
    CK(c->full.alloc(6 * c->n_pad));
    CK(c->rec.alloc(8 * std::max<int64_t>(n, 1)));
    CK(c->sel_list.alloc(c->nwords * 64 + 64));
    CK(c->sub.alloc(6 * c->s_pad));
    CK(c->dis.alloc(6 * c->dis_stride));
    CK(c->sub_idx0.alloc(s));
    CK(c->sub_perm.alloc(c->s_pad));   // (whole 64-lane reads of the last group stay inside the allocation: the mask pass, unpermute4.hip)
    CKH(hipMemsetAsync(c->sub_perm, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(c->s_pad, 1), c->stream));
    c->ngroups = (s + 63) / 64;
    c->ng_pad = ((c->ngroups + RH_G2_TG - 1) / RH_G2_TG) * RH_G2_TG + RH_G2_TG;
    CK(c->gb.alloc(7 * c->ng_pad));
    CK(c->gb32.alloc(8 * c->ng_pad));
    c->nst = (c->ngroups + RH_S4_STG - 1) / RH_S4_STG;
    CK(c->st32.alloc(8 * std::max<int64_t>(1, c->nst)));
    c->ntile = (c->ngroups + RH_G2_TG - 1) / RH_G2_TG;
    CK(c->tile32.alloc(8 * std::max<int64_t>(1, c->ntile)));
    CK(c->gm32.alloc(4 * c->ng_pad));
    CK(c->stm32.alloc(4 * std::max<int64_t>(1, c->nst)));
    CK(c->dis_gb.alloc(7 * c->ng_pad));
    CK(c->dis_gb32.alloc(8 * c->ng_pad));
    CKH(hipMemsetAsync(c->dis_gb, 0, sizeof(double) * 7 * (size_t)c->ng_pad, c->stream));
    CKH(hipMemsetAsync(c->gb, 0, sizeof(double) * 7 * (size_t)c->ng_pad, c->stream));
    {
        const int64_t e = rh_opt_int(nullptr, RH_OPT_SCORE_PATH, RH_SCORE_PATH_AUTO);   // rh_set_option(NULL, "score_path", ...): force a path (tests, A/B runs)
        c->use_groups = s >= RH_G2_MIN_POINTS;
        if (e == RH_SCORE_PATH_BRUTE) c->use_groups = false;
        if (e == RH_SCORE_PATH_GROUPS) c->use_groups = s > 0;
        // "kd_align", like the score path: the shape of the position tree of subset 1 is fixed here, for the life of the cloud
        c->kd_aligned = kd_aligned_for(s, rh_opt_int(nullptr, RH_OPT_KD_ALIGN, 0));
    }
    CK(rhk_enabled_alloc(c));
    CK(c->refit_mask.alloc(c->nwords));
    CK(c->idx_out.alloc(n));
    CK(c->d_nk.alloc(4));
    CK(c->ws[0].d_nk2.alloc(8));
    CKH(hipMemsetAsync(c->full, 0, sizeof(double) * 6 * (size_t)c->n_pad, c->stream));
    CKH(hipMemsetAsync(c->sub, 0, sizeof(double) * 6 * (size_t)c->s_pad, c->stream));
    CKH(hipMemsetAsync(c->dis, 0, sizeof(double) * 6 * (size_t)c->dis_stride, c->stream));
    stamp("streams, allocations, memsets");

    if (n > 0) {
        CK(t_xyz.alloc(3 * n));
        CK(t_nrm.alloc(3 * n));
        CKH(hipMemcpyAsync(t_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        CKH(hipMemcpyAsync(t_nrm, nrm, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        stamp("upload (xyz, nrm)");
        CK(rhk_transpose_aos(c, t_xyz, t_nrm, n, nullptr, n, c->full, c->n_pad));
        CK(rhk_pack_records(c, t_xyz, t_nrm, n, c->rec));
        stamp("AoS -> SoA, records");
        if (rh_opt_on(nullptr, RH_OPT_AABB_HOST)) cloud_aabb(xyz, n, c->k_lo, &c->k_size, &c->k_mag);   // (A/B: 25 ms at 10M points, 120 ms at 50M)
        else CK(cloud_aabb_device(c, t_xyz, xyz, n));
        stamp("bounding box");
        CK(rhk_korder_build(c, t_xyz, t_nrm, c->k_lo, c->k_size, c->k_mag));
        stamp("Morton order of the cloud");
        if (s > 0) {
            // internal order of subset 1: 64 consecutive points are spatially compact, which is what the
            // culled score kernel's per-group boxes need (k-d leaves, below)
            h_idx_own.reset(new (std::nothrow) int32_t[2 * (size_t)s]);
            h_idx = h_idx_own.get();
            if (!h_idx) { rh_set_error("out of host memory"); return fail(RH_E_NOMEM); }
            ms_before_kd = ms_since(tc0);
            const auto tkd0 = std::chrono::steady_clock::now();
            // Where the order is made: on the device (kdorder.hip: a radix sort per level of the same balanced k-d tree; the
            // subset's coordinate / normal magnitudes come out of the same pass) unless RH_KD_HOST=1 or RH_SUB_ORDER=morton
            // ask for the host forms below (A/B; the counts do not depend on the order).
            const bool ord_morton = rh_opt_on(nullptr, RH_OPT_SUB_ORDER);
            const bool kd_device = !rh_opt_on(nullptr, RH_OPT_KD_HOST) && !ord_morton;
            if (kd_device) {
                for (int64_t j = 0; j < s; j++) h_idx[j] = (int32_t)(subset1[j] - 1);
                rh_dev<int32_t> d_idx_in;
                CK(d_idx_in.alloc(s));
                CKH(hipMemcpyAsync(d_idx_in, h_idx, sizeof(int32_t) * (size_t)s, hipMemcpyHostToDevice, c->stream));
                CK(rhk_kd_order(c, t_xyz, t_nrm, d_idx_in));
                d_idx_in.reset();
                ms_kd = ms_since(tkd0);
                CK(rhk_transpose_aos(c, t_xyz, t_nrm, n, c->sub_idx0, s, c->sub, c->s_pad));
                CK(rhk_group_bounds(c));
            } else {
            double lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 }, mag = 0;
            bool first = true;
            for (int64_t j = 0; j < s; j++) {
                const double *pp = xyz + 3 * (subset1[j] - 1);
                for (int k = 0; k < 3; k++) {
                    const double v = pp[k];
                    if (!(v == v) || v - v != 0) continue;   // NaN / inf do not shape the box
                    if (first || v < lo[k]) lo[k] = v;
                    if (first || v > hi[k]) hi[k] = v;
                    if (fabs(v) > mag) mag = fabs(v);
                }
                first = false;
            }
            c->coord_mag = mag;
            double nmag = 0;
            for (int64_t j = 0; j < s; j++) {
                const double *nn = nrm + 3 * (subset1[j] - 1);
                for (int k = 0; k < 3; k++) {
                    const double v = fabs(nn[k]);
                    if (v - v == 0 && v > nmag) nmag = v;   // (NaN / inf: score4_device.h, guards)
                }
            }
            c->nrm_mag = nmag;
            // Internal order = leaves of a balanced k-d tree, 64 points each (median split along the widest
            // axis of the node's box, the left child always a multiple of 64 so that only the LAST group
            // is partial).  Against Morton order the groups' boxes are ~30 % smaller in radius and
            // 16-26 % fewer (candidate, group) pairs survive the box tests (cfg3).  RH_SUB_ORDER=morton
            // keeps the Morton order (A/B).
            std::vector<int32_t> order((size_t)s);
            for (int64_t j = 0; j < s; j++) order[(size_t)j] = (int32_t)j;
            if (ord_morton) {
                std::vector<std::pair<uint64_t, int32_t>> keys((size_t)s);
                for (int64_t j = 0; j < s; j++) {
                    const double *pp = xyz + 3 * (subset1[j] - 1);
                    uint64_t code = 0;
                    for (int k = 0; k < 3; k++) {
                        const double ext = hi[k] - lo[k];
                        double t = ext > 0 ? (pp[k] - lo[k]) / ext : 0.0;
                        if (!(t >= 0)) t = 0;
                        if (t > 1) t = 1;
                        code |= spread21((uint64_t)(t * 2097151.0)) << k;
                    }
                    keys[(size_t)j] = std::make_pair(code, (int32_t)j);
                }
                std::sort(keys.begin(), keys.end());
                for (int64_t i = 0; i < s; i++) order[(size_t)i] = keys[(size_t)i].second;
            } else {
                auto key = [&](int32_t j, int ax) {   // NaN sorts last; the order only has to be total
                    const double v = xyz[3 * (subset1[j] - 1) + ax];
                    return v == v ? v : HUGE_VAL;
                };
                // one node: widest axis of the finite points' box, median split at a multiple of 64 (std::nth_element with
                // a TOTAL order, so the result does not depend on who runs it); returns the split position, 0 for a leaf
                auto split = [&](int64_t lo_i, int64_t hi_i) -> int64_t {
                    const int64_t cnt = hi_i - lo_i;
                    if (cnt <= 64) return 0;
                    double blo[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, bhi[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
                    for (int64_t i = lo_i; i < hi_i; i++) {
                        const double *pp = xyz + 3 * (subset1[order[(size_t)i]] - 1);
                        for (int k = 0; k < 3; k++) {
                            const double v = pp[k];
                            if (!(v == v) || v - v != 0) continue;
                            if (v < blo[k]) blo[k] = v;
                            if (v > bhi[k]) bhi[k] = v;
                        }
                    }
                    int ax = 0;
                    double best = -1;
                    for (int k = 0; k < 3; k++) {
                        const double e = bhi[k] - blo[k];
                        if (e > best) { best = e; ax = k; }
                    }
                    const int64_t nl = kd_left_count(cnt, c->kd_aligned);
                    std::nth_element(order.begin() + lo_i, order.begin() + lo_i + nl, order.begin() + hi_i,
                                     [&](int32_t a, int32_t b) {
                                         const double ka = key(a, ax), kb = key(b, ax);
                                         return ka < kb || (ka == kb && a < b);
                                     });
                    return lo_i + nl;
                };
                struct Node { int64_t lo, hi; };
                auto subtree = [&](int64_t lo_i, int64_t hi_i) {   // a whole subtree, depth first, on the calling thread
                    std::vector<Node> stack;
                    stack.push_back({ lo_i, hi_i });
                    while (!stack.empty()) {
                        const Node nd = stack.back();
                        stack.pop_back();
                        const int64_t mid = split(nd.lo, nd.hi);
                        if (mid == 0) continue;
                        stack.push_back({ mid, nd.hi });
                        stack.push_back({ nd.lo, mid });
                    }
                };
                // The subtrees are disjoint ranges of `order`: the top levels hand their right halves to new threads (up
                // to 2^KD_PAR_LEVELS of them, no more than the host has cores), so the O(s) passes of the upper levels run
                // side by side -- 112 ms single-threaded at s = 312 500, a fifth of that on 16 cores.
                constexpr int KD_PAR_LEVELS = 4;
                const unsigned hw = std::thread::hardware_concurrency();
                const int par_levels = (hw >= 16 ? KD_PAR_LEVELS : (hw >= 8 ? 3 : (hw >= 4 ? 2 : (hw >= 2 ? 1 : 0))));
                std::function<void(int64_t, int64_t, int)> build = [&](int64_t lo_i, int64_t hi_i, int depth) {
                    if (depth >= par_levels || hi_i - lo_i < 4096) { subtree(lo_i, hi_i); return; }
                    const int64_t mid = split(lo_i, hi_i);
                    if (mid == 0) return;
                    std::thread right;
                    try {
                        right = std::thread([&, mid, hi_i, depth]() { build(mid, hi_i, depth + 1); });
                    } catch (const std::system_error &) {   // no thread to be had: this one does both halves
                        subtree(mid, hi_i);
                    }
                    build(lo_i, mid, depth + 1);
                    if (right.joinable()) right.join();
                };
                build(0, s, 0);
            }
            int32_t *h_perm = h_idx + s;
            for (int64_t i = 0; i < s; i++) {
                h_perm[i] = order[(size_t)i];
                h_idx[i] = (int32_t)(subset1[h_perm[i]] - 1);
            }
            ms_kd = ms_since(tkd0);
            CKH(hipMemcpyAsync(c->sub_idx0, h_idx, sizeof(int32_t) * (size_t)s, hipMemcpyHostToDevice, c->stream));
            CKH(hipMemcpyAsync(c->sub_perm, h_perm, sizeof(int32_t) * (size_t)s, hipMemcpyHostToDevice, c->stream));
            CK(rhk_transpose_aos(c, t_xyz, t_nrm, n, c->sub_idx0, s, c->sub, c->s_pad));
            CK(rhk_group_bounds(c));
            }   // host forms of the order
        }
    }
    stamp("subset order, gather, boxes");
    // the second internal order of subset 1, for the plane candidates of the culled score kernel (kdorder.hip); the enabled
    // words below are gathered into it too
    if (n > 0 && s > 0) CK(rhk_plane_order_build(c));
    stamp("plane order");
    CK(rhk_enabled_replace(c, nullptr));
    CKH(hipStreamSynchronize(c->stream));
    stamp("enabled bits");
#undef CK
#undef CKH
    t_xyz.reset();   // (inside the time below, as ever)
    t_nrm.reset();
    h_idx_own.reset();
    c->create_ms[0] = ms_since(tc0);
    c->create_ms[1] = ms_kd;
    c->create_ms[2] = ms_before_kd;
    c->create_ms[3] = c->create_ms[0] - ms_kd - ms_before_kd;
    *out = c;
    return RH_OK;
}

// wall time of the rh_cloud_create that made this cloud, in ms: total, the k-d leaf order of subset 1 (device: kdorder.hip;
// RH_KD_HOST=1: host threads) with the subset gather and the group boxes, everything before it (allocations, uploads,
// AoS -> SoA, bounding box, the Morton order of the cloud on the device), everything after it (enabled bits)
extern "C" int rh_cloud_create_ms(const rh_cloud *c, double *out4)
{
    if (!c || !out4) { rh_set_error("rh_cloud_create_ms: NULL argument"); return RH_E_INVALID; }
    for (int i = 0; i < 4; i++) out4[i] = c->create_ms[i];
    return RH_OK;
}

extern "C" int rh_cloud_destroy(rh_cloud *c)
{
    cloud_free(c);
    return RH_OK;
}

// RANSACCloud(vertices, normals, subsets; force_eltype = Float32) (src/octree.jl:102-109): xyz / nrm are Julia's
// Vector{SVector{3,Float32}} memory as is.  Such a cloud makes every operation of the four compatibles* a binary32
// operation -- points, normals and the shapes fitted to them are Float32 -- while eps and cos(alpha) stay what the caller
// made them: the kernels run the tests of score_device.h with T = float and compare with the double thresholds after
// exact promotion.  On the device it has everything a Float64 cloud has, built from the exactly converted values (k-d
// leaf order, boxes, enabled bits, masks, index lists, binary64 candidate records), plus float copies of its point sets:
// full32 / fullk32 (what the refit scans stream, half the bytes) and sub32 (what the brute-force batch score reads;
// subsets of 8192 points and more take the culled kernel of score4.hip, whose margins bracket the binary32 chain).
// The float record of a candidate is derived from its binary64 record where a test needs it (prepf_of, rh_internal.h).
// rh_ransac runs on such a cloud too (binary32 fits: fit_shared.h); rh_refit_lsq stays Float64-only.
extern "C" int rh_cloud_create_f32(const float *xyz, const float *nrm, int64_t n, const int64_t *subset1, int64_t s, int device,
                                   rh_cloud **out)
{
    if (!out) { rh_set_error("out is NULL"); return RH_E_INVALID; }
    *out = nullptr;
    if (n < 0 || (n > 0 && (!xyz || !nrm))) { rh_set_error("rh_cloud_create_f32: bad arguments"); return RH_E_INVALID; }
    std::vector<double> x64((size_t)(3 * n)), n64((size_t)(3 * n));
    for (int64_t i = 0; i < 3 * n; i++) { x64[(size_t)i] = (double)xyz[i]; n64[(size_t)i] = (double)nrm[i]; }
    rh_cloud *c = nullptr;
    RH_TRY(rh_cloud_create(x64.data(), n64.data(), n, subset1, s, device, &c));
    c->f32 = true;
    c->f32_groups = c->use_groups;   // culled kernel with a binary32 exact test where a Float64 cloud would use the culled kernel
    c->use_groups = false;           // (the Float64 dispatch below never runs for this cloud)
    int rc = c->full32.alloc(6 * std::max<int64_t>(c->n_pad, 1));
    if (rc == RH_OK) rc = c->sub32.alloc(6 * std::max<int64_t>(c->s_pad, 1));
    if (rc == RH_OK) rc = rhk_f32_build(c);
    if (rc == RH_OK && hipStreamSynchronize(c->stream) != hipSuccess) { rh_set_error("rh_cloud_create_f32: device error"); rc = RH_E_NODEVICE; }
    if (rc != RH_OK) { cloud_free(c); return rc; }
    *out = c;
    return RH_OK;
}

extern "C" int rh_cloud_info(const rh_cloud *c, int64_t *n, int64_t *s, int *device)
{
    if (!c) { rh_set_error("cloud is NULL"); return RH_E_INVALID; }
    if (n) *n = c->n;
    if (s) *s = c->s;
    if (device) *device = c->device;
    return RH_OK;
}

static int enter_nojoin(rh_cloud *c)
{
    if (!c) { rh_set_error("cloud is NULL"); return RH_E_INVALID; }
    RH_HIP(hipSetDevice(c->device));
    return RH_OK;
}

// every entry point but the pipelined rh_score_batch_dev: the cloud's stream first waits for what the other batch slots
// still have in flight ("batches_in_flight" > 1), so everything else sees one stream's order
int rh_join_batches(rh_cloud *c)
{
    for (rh_batch_ws &w : c->ws) {
        if (w.dirty) RH_HIP(hipStreamWaitEvent(c->stream, w.done, 0));
        w.dirty = false;
        w.started = false;
        w.out_counts = nullptr;
        w.out_masks = nullptr;
    }
    c->pipe_k = 0;
    return RH_OK;
}

static int enter(rh_cloud *c)
{
    RH_TRY(enter_nojoin(c));
    return rh_join_batches(c);
}

int rh_cloud_join(rh_cloud *c) { return enter(c); }

extern "C" int rh_cloud_set_enabled(rh_cloud *c, const uint64_t *chunks, int64_t nchunks)
{
    RH_TRY(enter(c));
    if (nchunks != c->nwords || (nchunks > 0 && !chunks)) {
        rh_set_error("rh_cloud_set_enabled: nchunks=%lld, expected %lld", (long long)nchunks, (long long)c->nwords);
        return RH_E_INVALID;
    }
    return rhk_enabled_replace(c, chunks);   // (null only with an empty cloud, where "all ones" is the same nothing)
}

extern "C" int rh_cloud_get_enabled(rh_cloud *c, uint64_t *chunks, int64_t nchunks)
{
    RH_TRY(enter(c));
    if (nchunks != c->nwords || (nchunks > 0 && !chunks)) {
        rh_set_error("rh_cloud_get_enabled: nchunks=%lld, expected %lld", (long long)nchunks, (long long)c->nwords);
        return RH_E_INVALID;
    }
    if (c->nwords > 0) {
        RH_HIP(hipMemcpyAsync(chunks, c->enabled, sizeof(uint64_t) * (size_t)nchunks, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipStreamSynchronize(c->stream));
    }
    return RH_OK;
}

extern "C" int rh_cloud_enable_all(rh_cloud *c)
{
    RH_TRY(enter(c));
    RH_TRY(rhk_enabled_replace(c, nullptr));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}

extern "C" int rh_cloud_count_enabled(rh_cloud *c, int64_t *out)
{
    RH_TRY(enter(c));
    if (!out) { rh_set_error("out is NULL"); return RH_E_INVALID; }
    return rhk_count_enabled(c, out);
}

// ---------------------------------------------------------------- scoring ----
// all four kind bins of the job against subset 1.
// Culled path (subsets of RH_G2_MIN_POINTS points and more): ONE launch of score4.hip's kernel over all kinds, reading the
// bins' classifier / culling records; masks leave it as entry lists (w.masks4).  ms_kind (the bench's per-kind leg): one
// launch per kind instead, the other kinds' bin sizes read as zero, an event before each.  Small subsets: the brute-force
// kernel, one launch per kind, masks in internal order.  Float32 clouds: the same two paths with the exact tests in binary32.
// launch_info: what the last sized launch of the culled kernel chose (rhk_score4_all).
static int score_bins_subset(rh_cloud *c, rh_batch_ws &w, const rh_score_job &job, const float *ms_kind, int32_t *launch_info = nullptr)
{
    if (rh_score_v4_enabled(c)) {
        if (!ms_kind) return rhk_score4_all(c, w, job, launch_info);
        if (c->d_zero == nullptr) {
            RH_TRY(c->d_zero.alloc(16));
            RH_HIP(hipMemsetAsync(c->d_zero, 0, 64, c->stream));
        }
        for (int k = 0; k < 4; k++) {
            RH_HIP(hipEventRecord(c->evk[k], c->stream));
            if (job.kind_bound[k] == 0) continue;
            rh_score_job one = job;
            for (int q = 0; q < 4; q++) if (q != k) one.nk[q] = c->d_zero;
            one.bound = job.kind_bound[k];
            RH_TRY(rhk_score4_all(c, w, one, launch_info));
        }
        return RH_OK;
    }
    for (int k = 0; k < 4; k++) {
        if (ms_kind) RH_HIP(hipEventRecord(c->evk[k], c->stream));
        if (job.kind_bound[k] == 0) continue;
        auto score = [&](auto *pts) {   // (a Float32 cloud: over the float copy of the subset)
            return rhk_score_kind(c, k, pts, c->s_pad, c->s, job.en[k], job.bins.prep[k], job.bins.orig[k], job.nk[k], job.kind_bound[k],
                                  job.eps[k], job.cosa[k], job.d_counts, job.d_masks_int, c->swords);
        };
        RH_TRY(c->f32 ? score(c->sub32.get()) : score(c->sub.get()));
    }
    return RH_OK;
}

extern "C" int rh_score_batch(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, int32_t *counts_out,
                              uint64_t *masks_out)
{
    RH_TRY(enter(c));
    RH_TRY(rh_validate_params(p));
    if (b < 0 || (b > 0 && (!shapes || !counts_out))) { rh_set_error("rh_score_batch: bad arguments"); return RH_E_INVALID; }
    if (b == 0) return RH_OK;
    int32_t nk[4] = { 0, 0, 0, 0 };
    for (int32_t i = 0; i < b; i++) {
        if (shapes[i].kind < 0 || shapes[i].kind > 3) {
            rh_set_error("candidate %d has unknown kind %d", i, shapes[i].kind);
            return RH_E_INVALID;
        }
        nk[shapes[i].kind]++;
    }
    rh_batch_ws &w = c->ws[0];
    RH_TRY(rh_ensure_batch(c, w, b));
    // Pinned staging: [records | original positions | bin sizes | counts] -- every transfer of the call is
    // asynchronous and the call waits once.  Batches of the size scorecandidates! sees per iteration (a few
    // candidates; here: up to 32) go as ONE small transfer into a device block of the same layout, carrying the
    // prepared records themselves (rh_prep_host is the host twin of the device's prep_one) and the zeroed counts:
    // upload, score launch, read-back.  (Measured: 30 -> 23 us at b = 1, 38 -> 31 us at b = 15; from ~6 KB on the
    // single larger transfer is slower than three small ones, so larger batches upload shapes, positions and
    // bin sizes separately and a kernel prepares the records and zeroes the counts.)
    const bool staged = b <= 32 && !c->f32;   // (the staged form carries prepared Float64 records only)
    const size_t rec_bytes = sizeof(rh_prep) >= sizeof(rh_shape) ? sizeof(rh_prep) : sizeof(rh_shape);
    const size_t o_orig = (size_t)b * rec_bytes, o_nk = (o_orig + (size_t)b * sizeof(int32_t) + 63) / 64 * 64;
    // (staged, culled path: the classifier records -- host twin of the prep kernels' cls_make -- ride along)
    const bool staged_cls = staged && rh_score_v4_enabled(c);
    const size_t o_counts = o_nk + 64, o_cls = (o_counts + (size_t)b * sizeof(int32_t) + 63) / 64 * 64;
    const size_t o_box = o_cls + (size_t)b * 64;   // culling records: RH_BOX_FIELDS arrays of b floats
    const size_t stage_bytes = staged_cls ? o_box + (size_t)rh4::RH_BOX_FIELDS * b * sizeof(float) : o_counts + (size_t)b * sizeof(int32_t);
    RH_TRY(rh_ensure_pin(c, (int64_t)stage_bytes));
    if (staged && c->d_stage == nullptr) RH_TRY(c->d_stage.alloc(32 * (rec_bytes + 8 + 64 + 4 * rh4::RH_BOX_FIELDS) + 512));
    char *hp = (char *)c->h_pin.get(), *dp = (char *)c->d_stage;
    rh_shape *h_sorted = (rh_shape *)hp;
    rh_prep *h_prep = (rh_prep *)hp;
    int32_t *h_orig = (int32_t *)(hp + o_orig);
    int32_t *h_nk = (int32_t *)(hp + o_nk);
    int32_t *h_counts = (int32_t *)(hp + o_counts);
    int32_t off[4], fill[4];
    off[0] = 0;
    for (int k = 1; k < 4; k++) off[k] = off[k - 1] + nk[k - 1];
    for (int k = 0; k < 4; k++) { fill[k] = off[k]; h_nk[k] = nk[k]; }
    // counting sort by kind, walking the batch in the spread order (kernels.hip: neighbours in the batch, often
    // hypotheses of the same primitive, go to different 64-candidate chunks)
    const int64_t spread = rh_opt_on(c, RH_OPT_NO_SPREAD) ? 1 : rh_spread_multiplier(b);
    for (int32_t t = 0; t < b; t++) {
        const int32_t i = (int32_t)(((int64_t)t * spread) % b);
        const int k = shapes[i].kind;
        if (staged) {
            rh_prep_host(shapes[i], &h_prep[fill[k]]);
            if (staged_cls)
                rh4::cls_make(h_prep[fill[k]], k, p->eps[k], p->cos_alpha[k], c->coord_mag, c->nrm_mag, ((rh4::rh_cls *)(hp + o_cls))[fill[k]],
                              (float *)(hp + o_box) + fill[k], b, nullptr, false, c->nrm_len);
        } else h_sorted[fill[k]] = shapes[i];
        h_orig[fill[k]] = i;
        fill[k]++;
    }
    const rh_prep *d_prep_use = w.d_prep;
    const void *d_cls_use = nullptr;
    const float *d_box_use = nullptr;
    int64_t bstride_use = 0;
    const int32_t *d_orig_use = w.d_orig, *d_nk_use = c->d_nk;
    int32_t *d_counts_use = w.d_counts;
    if (staged) {
        memset(h_counts, 0, sizeof(int32_t) * (size_t)b);
        RH_HIP(hipMemcpyAsync(dp, hp, stage_bytes, hipMemcpyHostToDevice, c->stream));
        d_prep_use = (const rh_prep *)dp;
        d_orig_use = (const int32_t *)(dp + o_orig);
        d_nk_use = (const int32_t *)(dp + o_nk);
        d_counts_use = (int32_t *)(dp + o_counts);
        if (staged_cls) { d_cls_use = dp + o_cls; d_box_use = (const float *)(dp + o_box); bstride_use = b; }
    } else {
        RH_HIP(hipMemcpyAsync(w.d_shapes, h_sorted, sizeof(rh_shape) * (size_t)b, hipMemcpyHostToDevice, c->stream));
        RH_HIP(hipMemcpyAsync(w.d_orig, h_orig, sizeof(int32_t) * (size_t)b, hipMemcpyHostToDevice, c->stream));
        RH_HIP(hipMemcpyAsync(c->d_nk, h_nk, 4 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        RH_TRY(rhk_prep_sorted(c, w, b, w.d_counts, p->eps, p->cos_alpha));   // zeroes d_counts as well
        if (w.qpre_v4) { d_cls_use = w.d_qpre; d_box_use = w.d_box; bstride_use = 4 * w.batch_cap; }
    }
    uint64_t *d_masks = nullptr, *d_masks_int = nullptr;
    if (masks_out && c->swords > 0) {
        const int64_t words = (int64_t)b * c->swords;
        if (words > c->d_masks.count()) RH_TRY(c->d_masks.grow(c->stream, words));
        d_masks = c->d_masks;
        RH_TRY(rh_masks_begin(c, w, b, d_cls_use != nullptr));
        d_masks_int = w.d_masks_int;
    }
    const int64_t off64[4] = { off[0], off[1], off[2], off[3] };
    rh_score_job job = rh_subset_job(c, p, rh_bins_at(d_prep_use, d_orig_use, d_cls_use, d_box_use, off64), bstride_use, d_nk_use);
    job.bound = b;
    for (int k = 0; k < 4; k++) job.kind_bound[k] = nk[k];
    job.d_counts = d_counts_use;
    job.d_masks_int = d_masks_int;
    RH_TRY(score_bins_subset(c, w, job, nullptr));
    if (d_masks_int) RH_TRY(rh_masks_finish(c, w, b, d_masks));
    RH_HIP(hipMemcpyAsync(h_counts, d_counts_use, sizeof(int32_t) * (size_t)b, hipMemcpyDeviceToHost, c->stream));
    if (d_masks)
        RH_HIP(hipMemcpyAsync(masks_out, d_masks, sizeof(uint64_t) * (size_t)b * (size_t)c->swords,
                              hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    memcpy(counts_out, h_counts, sizeof(int32_t) * (size_t)b);
    return RH_OK;
}

// A stream that really runs beside the given ones.  The runtime deals its streams to a few hardware queues (the least used
// one at creation), and two streams on one queue run one after the other -- which queue a new stream lands on depends on every
// stream the process has made before (other clouds, torch, copy streams).  So: candidates are created until one of them gets
// a kernel through while all the given streams are held busy by a spinning wave (~0.3 ms, once per slot and cloud).
namespace {
__global__ void spin_kernel(unsigned long long ticks)   // one wave, ~ticks of the 100 MHz clock
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
__global__ void noop_kernel() {}
}  // namespace

static int pick_concurrent_stream(const hipStream_t *busy, int nbusy, hipStream_t *out)
{
    hipStream_t tried[8];
    int ntried = 0, chosen = -1;
    rh_event eb[RH_MAX_IN_FLIGHT], ec;
    for (int i = 0; i < nbusy; i++) RH_TRY(eb[i].create(hipEventDisableTiming));
    RH_TRY(ec.create(hipEventDisableTiming));
    int rc = RH_OK;
    for (; ntried < 8 && chosen < 0 && rc == RH_OK; ntried++) {
        if (hipStreamCreateWithFlags(&tried[ntried], hipStreamNonBlocking) != hipSuccess) { rc = RH_E_NODEVICE; rh_set_error("hipStreamCreateWithFlags failed"); break; }
        for (int i = 0; i < nbusy; i++) {
            hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, busy[i], 30000ULL);   // 0.3 ms
            (void)hipEventRecord(eb[i], busy[i]);
        }
        hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, tried[ntried]);
        (void)hipEventRecord(ec, tried[ntried]);
        (void)hipEventSynchronize(ec);
        bool beside = true;   // the candidate's kernel is through: are all the busy streams still spinning?
        for (int i = 0; i < nbusy; i++) beside = beside && hipEventQuery(eb[i]) == hipErrorNotReady;
        for (int i = 0; i < nbusy; i++) (void)hipEventSynchronize(eb[i]);
        if (beside) chosen = ntried;
    }
    if (rc == RH_OK && chosen < 0) chosen = ntried - 1;   // (none found: the last one -- correct, only not concurrent)
    for (int i = 0; i < ntried; i++)
        if (i != chosen) (void)hipStreamDestroy(tried[i]);
    (void)hipGetLastError();
    if (rc != RH_OK) return rc;
    *out = tried[chosen];
    return RH_OK;
}

// What makes c->ws[slot] (slot >= 1) a slot of the pipeline: a stream beside the cloud's and the other slots', two events and
// the bin-size buffer.  Made into local owners and moved in only when all four exist, so a slot is never half made.
static int batch_slot_create(rh_cloud *c, int slot)
{
    hipStream_t busy[RH_MAX_IN_FLIGHT];
    int nbusy = 0;
    busy[nbusy++] = c->stream;
    for (int q = 1; q < RH_MAX_IN_FLIGHT; q++) if (q != slot && c->ws[q].stream != nullptr) busy[nbusy++] = c->ws[q].stream;
    hipStream_t stream = nullptr;
    rh_event done, start;
    rh_dev<int32_t> d_nk2;
    RH_TRY(pick_concurrent_stream(busy, nbusy, &stream));
    int rc = done.create(hipEventDisableTiming);
    if (rc == RH_OK) rc = start.create(hipEventDisableTiming);
    if (rc == RH_OK) rc = d_nk2.alloc(8);
    if (rc != RH_OK) {
        (void)hipStreamDestroy(stream);
        return rc;
    }
    rh_batch_ws &w = c->ws[slot];
    w.stream = stream; w.done = std::move(done); w.start = std::move(start); w.d_nk2 = std::move(d_nk2);
    return RH_OK;
}

// one batch on workspace c->ws[slot]; c->stream is that workspace's stream (slot > 0: rh_score_batch_dev)
// (zero_extra: the prepare launch also zeroes zero_extra_n ints from there)
static int score_batch_dev_impl(rh_cloud *c, int slot, const rh_shape *d_shapes, int32_t b, const rh_params *p,
                                int32_t *d_counts, uint64_t *d_masks, float *ms_kind, bool joined = true,
                                int32_t *zero_extra = nullptr, int32_t zero_extra_n = 0)
{
    RH_TRY(joined ? enter(c) : enter_nojoin(c));
    RH_TRY(rh_validate_params(p));
    if (b < 0 || (b > 0 && (!d_shapes || !d_counts))) { rh_set_error("rh_score_batch_dev: bad arguments"); return RH_E_INVALID; }
    const bool product_only = ms_kind && ms_kind[0] < 0.f;   // (profiling passes: no per-kind launches beside the product's)
    if (ms_kind) for (int k = 0; k < 5; k++) ms_kind[k] = 0.f;
    if (b == 0) return RH_OK;
    rh_batch_ws &w = c->ws[slot];
    RH_TRY(rh_ensure_batch(c, w, b));
    // bin sizes: two halves of d_nk2 used alternately; the prep kernel zeroes the counts and the other half,
    // so a step is two launches and no memset
    if (!w.nk2_ready) {
        RH_HIP(hipMemsetAsync(w.d_nk2, 0, 8 * sizeof(int32_t), c->stream));
        w.nk2_ready = true;
    }
    int32_t *nk_cur = w.d_nk2 + 4 * w.nk2_flip, *nk_next = w.d_nk2 + 4 * (1 - w.nk2_flip);
    w.nk2_flip = 1 - w.nk2_flip;
    RH_TRY(rhk_prep_binned(c, w, d_shapes, b, nk_cur, d_counts, nk_next, 1, p->eps, p->cos_alpha, zero_extra, zero_extra_n));
    uint64_t *d_masks_int = nullptr;
    if (d_masks && c->swords > 0) {
        RH_TRY(rh_masks_begin(c, w, b, w.qpre_v4));
        d_masks_int = w.d_masks_int;
    }
    const int64_t off[4] = { 0, w.batch_cap, 2 * w.batch_cap, 3 * w.batch_cap };
    // (classifier + culling records: made by rhk_prep_binned above)
    rh_score_job job = rh_subset_job(c, p, rh_bins_at(w.d_prep, w.d_orig, w.qpre_v4 ? w.d_qpre : nullptr, w.qpre_v4 ? w.d_box : nullptr, off), 4 * w.batch_cap, nk_cur);
    job.bound = b;
    for (int k = 0; k < 4; k++) job.kind_bound[k] = b;
    job.d_counts = d_counts;
    job.d_masks_int = d_masks_int;
    int32_t s4[4] = { 0, 0, 0, 0 };   // what the last sized launch below chose
    if (ms_kind) {   // the product launch (all kinds in one kernel) first, then the per-kind launches
        ms_kind[4] = 0.f;
        if (c->ev_cull == nullptr) RH_HIP(hipEventCreate(&c->ev_cull));
        RH_HIP(hipEventRecord(c->evk[0], c->stream));
        rh_score_job timed = job;
        timed.ev_listed = c->ev_cull;
        RH_TRY(score_bins_subset(c, w, timed, nullptr, s4));
        RH_HIP(hipEventRecord(c->evk[1], c->stream));
        RH_HIP(hipEventSynchronize(c->evk[1]));
        c->last_cull_ms = 0.f;
        if (s4[1] != 0) {   // super-tile lists: the list launch and the score launch apart (ms_kind[4] = the score launch alone)
            RH_HIP(hipEventElapsedTime(&c->last_cull_ms, c->evk[0], c->ev_cull));
            RH_HIP(hipEventElapsedTime(&ms_kind[4], c->ev_cull, c->evk[1]));
        } else {
            RH_HIP(hipEventElapsedTime(&ms_kind[4], c->evk[0], c->evk[1]));
        }
        if (!product_only) {
            RH_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)b, c->stream));
            if (d_masks_int && w.masks4) RH_HIP(hipMemsetAsync(w.d_occ, 0, sizeof(int32_t) * (size_t)b, c->stream));   // (the lists' cursors)
            else if (d_masks_int) RH_HIP(hipMemsetAsync(d_masks_int, 0, sizeof(uint64_t) * (size_t)b * (size_t)c->swords, c->stream));
        }
    }
    if (!product_only) RH_TRY(score_bins_subset(c, w, job, ms_kind, s4));
    if (s4[0] != 0) memcpy(c->last_s4, s4, sizeof s4);
    if (d_masks_int) RH_TRY(rh_masks_finish(c, w, b, d_masks));
    if (ms_kind && !product_only) {
        RH_HIP(hipEventRecord(c->evk[4], c->stream));
        RH_HIP(hipEventSynchronize(c->evk[4]));
        for (int k = 0; k < 4; k++) RH_HIP(hipEventElapsedTime(&ms_kind[k], c->evk[k], c->evk[k + 1]));
    }
    return RH_OK;
}

int rh_score_batch_dev_zeroing(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p, int32_t *d_counts, uint64_t *d_masks,
                               int32_t *zero_extra, int32_t zero_extra_n)
{
    // "batches_in_flight" = F > 1 (rh_set_option): batches take turns on the cloud's stream and F - 1 more streams with
    // workspaces of their own, so batch k + 1's prepare and score launches fill the chip while batch k's launch drains (the
    // heaviest tile's block sets a launch's length: cfg2 0.042 -> 0.027 ms a batch, cfg3 0.085 -> 0.071 with F = 2).  The
    // caller gives call k of a run buffer k mod F of F count (and mask) buffers (the stream that wrote a buffer last writes it
    // next; with masks the un-permutation of one batch, HBM-bound, runs under the next batch's score launch, issue-bound); any other call on the cloud (and rh_cloud_sync /
    // rh_timer_stop) first makes the cloud's stream wait for the others.
    const int in_flight = c != nullptr && b > 0 && c->stream == c->own_stream ? rh_opt_int(c, RH_OPT_BATCHES_IN_FLIGHT, 1) : 1;
    if (in_flight <= 1) return score_batch_dev_impl(c, 0, d_shapes, b, p, d_counts, d_masks, nullptr, true, zero_extra, zero_extra_n);
    RH_TRY(enter_nojoin(c));
    int slot = (int)(c->pipe_k % (uint32_t)in_flight);
    // a caller whose buffers are not F apart (the same count buffer call after call, say): never two batches in flight on
    // one buffer -- the streams are joined first and the batch runs alone (correct, only not overlapped)
    for (int t = 0; t < RH_MAX_IN_FLIGHT; t++)
        if (t != slot && ((c->ws[t].out_counts != nullptr && c->ws[t].out_counts == d_counts) || (d_masks != nullptr && c->ws[t].out_masks == d_masks))) {
            RH_TRY(rh_join_batches(c));
            slot = 0;
            break;
        }
    c->pipe_k++;
    rh_batch_ws &w = c->ws[slot];
    w.out_counts = d_counts;
    w.out_masks = d_masks;
    if (slot == 0) return score_batch_dev_impl(c, 0, d_shapes, b, p, d_counts, d_masks, nullptr, false, zero_extra, zero_extra_n);
    if (w.stream == nullptr) RH_TRY(batch_slot_create(c, slot));
    if (!w.started) {   // once per pipelined stretch: the stream starts behind what the cloud's stream holds so far
        RH_HIP(hipEventRecord(w.start, c->stream));
        RH_HIP(hipStreamWaitEvent(w.stream, w.start, 0));
        w.started = true;
    }
    c->stream = w.stream;        // the one redirection: every launcher below enqueues on c->stream and takes its buffers from w
    const int rc = score_batch_dev_impl(c, slot, d_shapes, b, p, d_counts, d_masks, nullptr, false, zero_extra, zero_extra_n);
    c->stream = c->own_stream;   // (in_flight > 1 only on the cloud's own stream)
    // (also behind a failed call: whatever it did enqueue on the slot's stream is waited for at the next join)
    RH_HIP(hipEventRecord(w.done, w.stream));
    w.dirty = true;
    return rc;
}

extern "C" int rh_score_batch_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p,
                                  int32_t *d_counts, uint64_t *d_masks)
{
    return rh_score_batch_dev_zeroing(c, d_shapes, b, p, d_counts, d_masks, nullptr, 0);
}

extern "C" int rh_last_list_launch_ms(rh_cloud *c, float *ms_out)
{
    if (!c || !ms_out) { rh_set_error("rh_last_list_launch_ms: bad arguments"); return RH_E_INVALID; }
    *ms_out = c->last_cull_ms;
    return RH_OK;
}

extern "C" int rh_score_launch_info(rh_cloud *c, int32_t *out4)
{
    if (!c || !out4) { rh_set_error("rh_score_launch_info: bad arguments"); return RH_E_INVALID; }
    for (int i = 0; i < 4; i++) out4[i] = c->last_s4[i];
    return RH_OK;
}

extern "C" int rh_score_batch_dev_timed(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const rh_params *p,
                                        int32_t *d_counts, uint64_t *d_masks, float *ms_kind_out)
{
    if (!ms_kind_out) { rh_set_error("rh_score_batch_dev_timed: ms_kind_out is NULL"); return RH_E_INVALID; }
    return score_batch_dev_impl(c, 0, d_shapes, b, p, d_counts, d_masks, ms_kind_out);
}

// ------------------------------------------------------------------ refit ----
extern "C" int rh_refit(rh_cloud *c, const rh_shape *shape, const rh_params *p, int64_t *idx_out, int64_t cap,
                        int64_t *n_out)
{
    RH_TRY(enter(c));
    RH_TRY(rh_validate_params(p));
    if (!shape || !n_out || cap < 0 || (cap > 0 && !idx_out)) { rh_set_error("rh_refit: bad arguments"); return RH_E_INVALID; }
    if (shape->kind < 0 || shape->kind > 3) { rh_set_error("unknown shape kind %d", shape->kind); return RH_E_INVALID; }
    *n_out = 0;
    rh_prep P;
    rh_prep_host(*shape, &P);
    RH_HIP(hipEventRecord(c->evk[0], c->stream));
    RH_TRY(rhk_refit_mask(c, P, shape->kind, p->eps[shape->kind], p->cos_alpha[shape->kind]));
    RH_HIP(hipEventRecord(c->evk[1], c->stream));
    return rhk_refit_total(c, "rh_refit", idx_out, cap, n_out, c->evk[2]);
}

extern "C" int rh_last_refit_ms(rh_cloud *c, float *ms_scan, float *ms_compact)
{
    RH_TRY(enter(c));
    RH_HIP(hipEventSynchronize(c->evk[2]));
    if (ms_scan) RH_HIP(hipEventElapsedTime(ms_scan, c->evk[0], c->evk[1]));
    if (ms_compact) RH_HIP(hipEventElapsedTime(ms_compact, c->evk[1], c->evk[2]));
    return RH_OK;
}

extern "C" int rh_invalidate(rh_cloud *c, const int64_t *idx, int64_t n)
{
    RH_TRY(enter(c));
    if (n < 0 || (n > 0 && !idx)) { rh_set_error("rh_invalidate: bad arguments"); return RH_E_INVALID; }
    if (n == 0) return RH_OK;
    for (int64_t k = 0; k < n; k++)   // before anything else: an empty cloud has no valid index at all
        if (idx[k] < 1 || idx[k] > c->n) {
            rh_set_error("rh_invalidate: index %lld outside 1..%lld", (long long)idx[k], (long long)c->n);
            return RH_E_INVALID;   // the reference would throw a BoundsError
        }
    if (n > c->n) {   // idx_out is the staging buffer; longer lists (duplicates) go in pieces (c->n >= 1 here)
        for (int64_t o = 0; o < n; o += c->n) RH_TRY(rh_invalidate(c, idx + o, std::min<int64_t>(c->n, n - o)));
        return RH_OK;
    }
    RH_HIP(hipMemcpyAsync(c->idx_out, idx, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return rhk_enabled_clear_list(c, c->idx_out, n);
}

extern "C" int rh_select_enabled(rh_cloud *c, const int64_t *ranks, int32_t k, int64_t *idx_out)
{
    RH_TRY(enter(c));
    if (k < 0 || (k > 0 && (!ranks || !idx_out))) { rh_set_error("rh_select_enabled: bad arguments"); return RH_E_INVALID; }
    if (k == 0) return RH_OK;
    if (c->nwords == 0) { for (int i = 0; i < k; i++) idx_out[i] = 0; return RH_OK; }
    if (2 * (int64_t)k > c->d_ranks.count()) RH_TRY(c->d_ranks.grow(c->stream, 2 * (int64_t)k));   // ranks in the first half, indices in the second
    const int64_t ranks_cap = c->d_ranks.count() / 2;
    RH_TRY(rhk_ensure_select(c));
    if (k <= 1024) {
        // the per-sample call of the reference's loop (a couple of ranks): the kernel reads the ranks from the pinned
        // block and writes the indices back into it -- one launch and one wait, no transfer operation
        RH_TRY(rh_ensure_pin(c, 2 * (int64_t)sizeof(int64_t) * k));
        int64_t *h_ranks = (int64_t *)c->h_pin.get(), *h_out = h_ranks + k;
        memcpy(h_ranks, ranks, sizeof(int64_t) * (size_t)k);
        RH_TRY(rhk_select(c, h_ranks, k, h_out));
        RH_HIP(hipStreamSynchronize(c->stream));
        memcpy(idx_out, h_out, sizeof(int64_t) * (size_t)k);
        return RH_OK;
    }
    RH_HIP(hipMemcpyAsync(c->d_ranks, ranks, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice, c->stream));
    RH_TRY(rhk_select(c, c->d_ranks, k, c->d_ranks + ranks_cap));
    RH_HIP(hipMemcpyAsync(idx_out, c->d_ranks + ranks_cap, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}

// samplepointcloud4! (fitting.jl:383-430) k times in a row on the caller's random stream: see sample_sets_seq_kernel.
extern "C" int rh_sample_sets(rh_cloud *c, int32_t drawN, rh_rng *rng, int32_t k, int64_t *idx_out, int32_t *ok_out, int32_t *level_out)
{
    RH_TRY(enter(c));
    if (!rng || k < 0 || drawN < 2 || drawN > 16 || (k > 0 && (!idx_out || !ok_out))) { rh_set_error("rh_sample_sets: bad arguments (drawN 2..16)"); return RH_E_INVALID; }
    if (k == 0) return RH_OK;
    if (c->n == 0) { rh_set_error("rh_sample_sets: the cloud is empty"); return RH_E_INVALID; }
    int32_t count = 0;
    RH_TRY(rhk_enabled_total(c, &count));
    if (count <= 0) { rh_set_error("rh_sample_sets: no enabled point (the reference would draw for ever, fitting.jl:393)"); return RH_E_INVALID; }
    const int W = drawN + 2;
    constexpr int64_t L_MAX = 1 << 20;
    // draws a call takes: 1 / (enabled share) for the first point + drawN - 1 (+ the rare redraw)
    const double per_call = (double)c->n / (double)count + (double)drawN;
    double grow = 1.5;
    int32_t done = 0;
    while (done < k) {
        int64_t L64 = (int64_t)(grow * per_call * (k - done)) + 8 * drawN + 64;
        if (L64 > L_MAX) L64 = L_MAX;
        const int32_t L = (int32_t)L64;
        // the draws of a COPY of the generator (an injected stream first, like rh_rng_range); the caller's own generator is
        // then advanced by exactly what the calls that completed consumed
        rh_rng tmp = *rng;
        const size_t bytes_raw = sizeof(uint64_t) * (size_t)L, bytes_rec = sizeof(int64_t) * (size_t)L * (size_t)W;
        RH_TRY(rh_ensure_pin(c, (int64_t)(bytes_raw + bytes_rec)));
        uint64_t *h_raw = (uint64_t *)c->h_pin.get();
        int64_t *h_rec = (int64_t *)(h_raw + L);
        for (int32_t i = 0; i < L; i++) h_raw[i] = rh_rng_next_raw(&tmp);
        const int64_t need = (int64_t)L * (1 + W);
        if (need > c->d_ranks.count()) RH_TRY(c->d_ranks.grow(c->stream, 2 * ((need + 1) / 2)));   // (an even count: rh_select_enabled halves it)
        uint64_t *d_raw = (uint64_t *)c->d_ranks.get();
        int64_t *d_rec = c->d_ranks + L;
        RH_HIP(hipMemcpyAsync(d_raw, h_raw, bytes_raw, hipMemcpyHostToDevice, c->stream));
        RH_TRY(rhk_sample_sets_seq(c, d_raw, L, drawN, d_rec));
        RH_HIP(hipMemcpyAsync(h_rec, d_rec, bytes_rec, hipMemcpyDeviceToHost, c->stream));
        RH_HIP(hipStreamSynchronize(c->stream));
        int64_t p = 0;
        const int32_t done_before = done;
        while (done < k && p < L) {
            const int64_t *r = h_rec + p * W;
            if (r[drawN] <= 0) break;   // the draws ran out inside this call: it is played again from here in the next round
            for (int q = 0; q < drawN; q++) idx_out[(int64_t)done * drawN + q] = r[q];
            ok_out[done] = (int32_t)r[drawN + 1];
            if (level_out) level_out[done] = r[drawN + 1] ? 1 : 0;   // argmax(levelweight[1:depth]) = 1 always: SURVEY.md 0.5
            p += r[drawN];
            done++;
        }
        for (int64_t i = 0; i < p; i++) (void)rh_rng_next_raw(rng);
        if (done == done_before) {   // not one call finished inside the window: a longer one, or give up
            if (L64 >= L_MAX) { rh_set_error("rh_sample_sets: a call did not finish within %d draws (%d of %lld points enabled)", L, count, (long long)c->n); return RH_E_INTERNAL; }
            grow *= 4.0;
        }
    }
    return RH_OK;
}

// ------------------------------------------------------------ measurement ----
extern "C" int rh_timer_start(rh_cloud *c)
{
    RH_TRY(enter(c));
    RH_HIP(hipEventRecord(c->ev0, c->stream));
    return RH_OK;
}

extern "C" int rh_timer_stop(rh_cloud *c, float *ms_out)
{
    RH_TRY(enter(c));
    RH_HIP(hipEventRecord(c->ev1, c->stream));
    RH_HIP(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    RH_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (ms_out) *ms_out = ms;
    return RH_OK;
}

extern "C" int rh_cloud_set_stream(rh_cloud *c, void *hip_stream, int use_external)
{
    RH_TRY(enter(c));
    RH_HIP(hipStreamSynchronize(c->stream));   // nothing of this cloud may still be in flight on the old stream
    c->stream = use_external ? (hipStream_t)hip_stream : c->own_stream;
    return RH_OK;
}

extern "C" int rh_cloud_sync(rh_cloud *c)
{
    RH_TRY(enter(c));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}

extern "C" int rh_dev_alloc(rh_cloud *c, int64_t bytes, void **d_out)
{
    RH_TRY(enter(c));
    if (!d_out || bytes < 0) { rh_set_error("rh_dev_alloc: bad arguments"); return RH_E_INVALID; }
    rh_dev<char> buf;
    RH_TRY(buf.alloc(bytes));
    *d_out = buf.release();   // the caller's from here on: back through rh_dev_free
    return RH_OK;
}

extern "C" int rh_dev_free(rh_cloud *c, void *d)
{
    RH_TRY(enter(c));
    RH_HIP(hipStreamSynchronize(c->stream));
    RH_HIP(rh_free_callers_block(d));
    return RH_OK;
}

extern "C" int rh_dev_upload(rh_cloud *c, void *d_dst, const void *h_src, int64_t bytes)
{
    RH_TRY(enter(c));
    if (bytes <= 0) return RH_OK;
    RH_HIP(hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}

extern "C" int rh_dev_download(rh_cloud *c, void *h_dst, const void *d_src, int64_t bytes)
{
    RH_TRY(enter(c));
    if (bytes <= 0) return RH_OK;
    RH_HIP(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    return RH_OK;
}
