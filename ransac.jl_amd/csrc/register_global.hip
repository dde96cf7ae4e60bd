// register_global.hip -- a rigid motion from correspondences without a start: RANSAC over triples of correspondences
// (rh_register_global; include/ransac_hip.h states the definition in full, operation by operation).
//   1. both clouds go to the device (widened exactly), their finiteness is found there (cloud_box), and glob_gather_kernel
//      leaves the c corresponding pairs (q_i, r_i) as 6 doubles each; one copy brings them to the host;
//   2. the host draws the triples (rh_rng_range, three per trial) or takes the caller's, tests them and builds the
//      hypotheses (global_hyp.h): 12 doubles per trial in the stated order -- a few hundred operations per trial, and
//      the definition fixes the bits wherever they are formed;
//   3. glob_score_kernel: one hypothesis per lane, its 12 doubles in registers; the pairs stream through LDS in tiles
//      and are read as wave-wide broadcasts.  grid.y cuts the pairs when the trials alone do not fill the device; the
//      partial counts meet in an integer atomicAdd.  An invalid trial keeps the -1 it was given;
//   4. the counts come back; the largest, ties to the smaller trial, names the transform.
// No floating-point sums, so nothing depends on an order: the same bytes on every run.
#include "global_hyp.h"
#include "knn_grid.h"

namespace {

constexpr int GL_BLOCK = 256;            // hypotheses per block
constexpr int GL_TILE = 256;             // pairs per LDS tile: 12 KiB
constexpr int GL_MIN_BLOCKS = 1024;

__global__ __launch_bounds__(256) void glob_gather_kernel(const double *__restrict__ qxyz, int64_t m, const double *__restrict__ rxyz,
                                                          int64_t n, const int32_t *__restrict__ cq, const int32_t *__restrict__ cr,
                                                          int64_t c, double *__restrict__ pairs, int32_t *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const int64_t a = (int64_t)cq[i] - 1, b = (int64_t)cr[i] - 1;
    if (a < 0 || a >= m || b < 0 || b >= n) {
        atomicOr(bad, 1);
        for (int k = 0; k < 6; k++) pairs[6 * i + k] = 0.0;
        return;
    }
    for (int k = 0; k < 3; k++) {
        pairs[6 * i + k] = qxyz[3 * a + k];
        pairs[6 * i + 3 + k] = rxyz[3 * b + k];
    }
}

__global__ __launch_bounds__(GL_BLOCK) void glob_score_kernel(const GlobHyp *__restrict__ hyp, int32_t trials, const double *__restrict__ pairs,
                                                              int64_t c, int64_t chunk, double tau2, int32_t *__restrict__ counts)
{
    __shared__ double tile[GL_TILE * 6];
    const int32_t t = (int32_t)(blockIdx.x * GL_BLOCK + threadIdx.x);
    const bool live = t < trials && counts[t] >= 0;               // (-1: not valid; a live count only grows)
    double R[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, tr[3] = { 0, 0, 0 };
    if (live) {
        for (int k = 0; k < 9; k++) R[k] = hyp[t].R[k];
        for (int k = 0; k < 3; k++) tr[k] = hyp[t].t[k];
    }
    const int64_t c0 = (int64_t)blockIdx.y * chunk, c1 = c0 + chunk < c ? c0 + chunk : c;
    int cnt = 0;
    for (int64_t base = c0; base < c1; base += GL_TILE) {
        const int len = (int)(c1 - base < GL_TILE ? c1 - base : GL_TILE);
        __syncthreads();
        for (int u = threadIdx.x; u < len * 6; u += GL_BLOCK) tile[u] = pairs[base * 6 + u];
        __syncthreads();
        for (int i = 0; i < len; i++) {
            const double x = tile[6 * i], y = tile[6 * i + 1], z = tile[6 * i + 2];
            const double z0 = (((R[0] * x + R[1] * y) + R[2] * z) + tr[0]) - tile[6 * i + 3];
            const double z1 = (((R[3] * x + R[4] * y) + R[5] * z) + tr[1]) - tile[6 * i + 4];
            const double z2 = (((R[6] * x + R[7] * y) + R[8] * z) + tr[2]) - tile[6 * i + 5];
            cnt += ((z0 * z0 + z1 * z1) + z2 * z2) <= tau2 ? 1 : 0;
        }
    }
    if (live && cnt) atomicAdd(&counts[t], cnt);
}

template <typename T>
int register_global(const T *ref_aos, int64_t n, const T *qry_aos, int64_t m, const int32_t *corr_qry, const int32_t *corr_ref,
                    int64_t c, const rh_global_params *p, const int32_t *triples, int device, double *transform_out,
                    rh_global_result *result, int32_t *counts_out)
{
    static const char who[] = "rh_register_global";
    if (!ref_aos || !qry_aos || !corr_qry || !corr_ref || !p || !transform_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n >= (int64_t)0x7FFFFFFF || m < 1 || m >= (int64_t)0x7FFFFFFF) {
        rh_set_error("%s: n = %lld, m = %lld outside 1 .. 2^31 - 2", who, (long long)n, (long long)m);
        return RH_E_INVALID;
    }
    if (c < 3 || c > (int64_t)0x7FFFFFFF / 6) { rh_set_error("%s: %lld correspondences outside 3 .. (2^31 - 1) / 6", who, (long long)c); return RH_E_INVALID; }
    if (p->trials < 1 || p->trials > RH_GLOBAL_MAX_TRIALS) {
        rh_set_error("%s: trials = %d outside 1 .. %d", who, p->trials, RH_GLOBAL_MAX_TRIALS);
        return RH_E_INVALID;
    }
    if (!(p->tau > 0.0) || !isfinite(p->tau)) { rh_set_error("%s: tau must be finite and > 0", who); return RH_E_INVALID; }
    if (!(p->edge_ratio > 0.0 && p->edge_ratio <= 1.0)) { rh_set_error("%s: edge_ratio outside (0, 1]", who); return RH_E_INVALID; }
    if (!(p->min_edge >= 0.0) || !isfinite(p->min_edge)) { rh_set_error("%s: min_edge must be finite and >= 0", who); return RH_E_INVALID; }
    const int32_t trials = p->trials;

    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    // the triples: the caller's (wherever they live) or the draws
    std::vector<int32_t> tri((size_t)trials * 3);
    if (triples) {
        SCOPE_HIP(S, hipMemcpyAsync(tri.data(), triples, sizeof(int32_t) * tri.size(), hipMemcpyDefault, st));
        SCOPE_HIP(S, hipStreamSynchronize(st));
        for (int32_t v : tri)
            if (v < 0 || (int64_t)v >= c) { rh_set_error("%s: a triple names correspondence %d of %lld", who, v, (long long)c); return RH_E_INVALID; }
    } else {
        rh_rng rng;
        rh_rng_seed(&rng, p->seed);
        for (size_t u = 0; u < tri.size(); u++) tri[u] = (int32_t)(rh_rng_range(&rng, c) - 1);
    }
    // 1. the pairs
    double *d_ref = nullptr, *d_qry = nullptr, *d_pairs = nullptr;
    int32_t *d_cq = nullptr, *d_cr = nullptr, *d_bad = nullptr, *d_counts = nullptr;
    GlobHyp *d_hyp = nullptr;
    RH_TRY(S.alloc(&d_ref, 3 * n));
    RH_TRY(S.upload(ref_aos, d_ref, 3 * n, hipMemcpyDefault));
    RH_TRY(S.alloc(&d_qry, 3 * m));
    RH_TRY(S.upload(qry_aos, d_qry, 3 * m, hipMemcpyDefault));
    {
        double lo[3], hi[3];
        RH_TRY(cloud_box(S, d_ref, n, lo, hi));
        RH_TRY(cloud_box(S, d_qry, m, lo, hi));
    }
    RH_TRY(S.alloc(&d_cq, c));
    RH_TRY(S.alloc(&d_cr, c));
    RH_TRY(S.alloc(&d_bad, 1));
    RH_TRY(S.alloc(&d_pairs, 6 * c));
    RH_TRY(S.alloc(&d_counts, trials));
    RH_TRY(S.alloc(&d_hyp, trials));
    SCOPE_HIP(S, hipMemcpyAsync(d_cq, corr_qry, sizeof(int32_t) * (size_t)c, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipMemcpyAsync(d_cr, corr_ref, sizeof(int32_t) * (size_t)c, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(glob_gather_kernel, dim3(blocks_for(c)), dim3(256), 0, st, d_qry, m, d_ref, n, d_cq, d_cr, c, d_pairs, d_bad);
    SCOPE_HIP(S, hipGetLastError());
    int32_t bad = 0;
    RH_TRY(S.fetch(&bad, d_bad));
    if (bad) { rh_set_error("%s: a correspondence names a point outside its cloud", who); return RH_E_INVALID; }
    std::vector<double> pairs((size_t)c * 6);
    RH_TRY(S.fetch(pairs.data(), d_pairs, pairs.size()));
    // 2. the hypotheses
    std::vector<GlobHyp> hyp((size_t)trials);
    std::vector<int32_t> counts((size_t)trials);
    int32_t nvalid = 0;
    for (int32_t t = 0; t < trials; t++) {
        memset(&hyp[(size_t)t], 0, sizeof(GlobHyp));
        const bool ok = gl_hypothesis(pairs.data(), tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2], *p, hyp[(size_t)t]);
        counts[(size_t)t] = ok ? 0 : -1;
        nvalid += ok;
    }
    // 3. the counts
    if (nvalid) {
        SCOPE_HIP(S, hipMemcpyAsync(d_hyp, hyp.data(), sizeof(GlobHyp) * hyp.size(), hipMemcpyHostToDevice, st));
        SCOPE_HIP(S, hipMemcpyAsync(d_counts, counts.data(), sizeof(int32_t) * counts.size(), hipMemcpyHostToDevice, st));
        const int64_t bx = ((int64_t)trials + GL_BLOCK - 1) / GL_BLOCK, tiles = (c + GL_TILE - 1) / GL_TILE;
        int64_t by = std::min<int64_t>(std::min<int64_t>(tiles, (GL_MIN_BLOCKS + bx - 1) / bx), 65535);
        const int64_t chunk = ((tiles + by - 1) / by) * GL_TILE;
        by = (c + chunk - 1) / chunk;
        hipLaunchKernelGGL(glob_score_kernel, dim3((unsigned)bx, (unsigned)by), dim3(GL_BLOCK), 0, st, d_hyp, trials, d_pairs, c, chunk,
                           p->tau * p->tau, d_counts);
        SCOPE_HIP(S, hipGetLastError());
        RH_TRY(S.fetch(counts.data(), d_counts, counts.size()));
    }
    // 4. the best
    int32_t best = -1, best_count = -1;
    for (int32_t t = 0; t < trials; t++)
        if (counts[(size_t)t] > best_count) { best_count = counts[(size_t)t]; best = t; }
    static const double ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    if (best < 0) memcpy(transform_out, ident, sizeof ident);
    else
        for (int k = 0; k < 3; k++) {
            for (int l = 0; l < 3; l++) transform_out[4 * k + l] = hyp[(size_t)best].R[3 * k + l];
            transform_out[4 * k + 3] = hyp[(size_t)best].t[k];
        }
    if (result) {
        result->status = best < 0 ? RH_GLOB_NO_TRIAL : RH_GLOB_OK;
        result->best_trial = best;
        result->best_count = best_count;
        result->n_valid_trials = nvalid;
    }
    if (counts_out) {
        SCOPE_HIP(S, hipMemcpyAsync(counts_out, counts.data(), sizeof(int32_t) * counts.size(), hipMemcpyDefault, st));
        SCOPE_HIP(S, hipStreamSynchronize(st));
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_register_global(const double *ref_xyz_aos, int64_t n, const double *qry_xyz_aos, int64_t m, const int32_t *corr_qry,
                                  const int32_t *corr_ref, int64_t c, const rh_global_params *p, const int32_t *triples_or_null,
                                  int device, double *transform_out_3x4, rh_global_result *result_or_null, int32_t *counts_out_or_null)
{
    return register_global<double>(ref_xyz_aos, n, qry_xyz_aos, m, corr_qry, corr_ref, c, p, triples_or_null, device, transform_out_3x4,
                                   result_or_null, counts_out_or_null);
}

extern "C" int rh_register_global_f32(const float *ref_xyz_aos, int64_t n, const float *qry_xyz_aos, int64_t m, const int32_t *corr_qry,
                                      const int32_t *corr_ref, int64_t c, const rh_global_params *p, const int32_t *triples_or_null,
                                      int device, double *transform_out_3x4, rh_global_result *result_or_null,
                                      int32_t *counts_out_or_null)
{
    return register_global<float>(ref_xyz_aos, n, qry_xyz_aos, m, corr_qry, corr_ref, c, p, triples_or_null, device, transform_out_3x4,
                                  result_or_null, counts_out_or_null);
}
