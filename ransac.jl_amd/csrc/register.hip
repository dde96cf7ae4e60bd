// register.hip -- rigid registration of a query cloud onto a reference cloud by iterative closest point (rh_register;
// include/ransac_hip.h states the definition in full, operation by operation).  Per iteration:
//   1. reg_transform_kernel writes p_j = (R y_j + t) + c, 24 bytes per query;
//   2. QuerySearch (knn_query_search.h) binds them to the reference's grid -- box, margin, keys, sort -- and finds nn_j;
//   3. reg_accumulate_kernel gathers r_nn (and its normal), forms the 28 (plane) or 16 (point) leaves of the normal
//      equations and folds them in the tree T() of tree_sum.h: a lane's four adjacent queries as (l0 + l1) + (l2 + l3), the
//      xor butterfly over the wave, adjacent pairs of the four wave sums through LDS, one vector of partials per block of
//      RH_OUT_BLOCK_POINTS queries; reg_fold_kernel is the same tree over the block partials, one grid row per component;
//   4. one copy of the roots and the count of valid queries to the host, where the 6 x 6 system is solved by Cholesky and
//      the state updated by the Cayley map.
// No floating-point atomics; every buffer is allocated before the loop (call_scope.h) and freed on every way out.
#include "knn_query_search.h"
#include "tree_sum.h"

namespace {

constexpr int REG_NC_PLANE = 28, REG_NC_POINT = 16;

// the state of an iteration: y' = R (q - c) + t
struct RegState {
    double c[3], R[9], t[3];
};

__device__ __forceinline__ void reg_moved(const RegState &s, const double *__restrict__ q, double yp[3])
{
    const double y0 = q[0] - s.c[0], y1 = q[1] - s.c[1], y2 = q[2] - s.c[2];
    for (int k = 0; k < 3; k++) yp[k] = ((s.R[3 * k] * y0 + s.R[3 * k + 1] * y1) + s.R[3 * k + 2] * y2) + s.t[k];
}

__global__ __launch_bounds__(256) void reg_transform_kernel(RegState s, const double *__restrict__ qxyz, int64_t m,
                                                            double *__restrict__ pxyz)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    double yp[3];
    reg_moved(s, qxyz + 3 * j, yp);
    for (int k = 0; k < 3; k++) pxyz[3 * j + k] = yp[k] + s.c[k];
}

struct RegAccArgs {
    RegState s;
    const double *qxyz;      // the caller's queries
    const int32_t *nn;       // 1-based nearest reference point of p_j, 0: query j is not valid
    const double *rxyz;      // the reference, AoS
    const double *rnrm;      // its normals (plane metric)
    int64_t m, n;
};

// the leaves of query j (ransac_hip.h, step 4); false and +0.0 everywhere when j is past the end or not valid
template <int METRIC>
__device__ __forceinline__ bool reg_leaves(const RegAccArgs &a, int64_t j, double *l)
{
    constexpr int NC = METRIC == RH_DIST_PLANE ? REG_NC_PLANE : REG_NC_POINT;
    for (int c = 0; c < NC; c++) l[c] = 0.0;
    if (j >= a.m) return false;
    const int64_t ri = (int64_t)a.nn[j] - 1;
    if (ri < 0 || ri >= a.n) return false;
    double y[3], e[3];
    reg_moved(a.s, a.qxyz + 3 * j, y);
    for (int k = 0; k < 3; k++) e[k] = (a.rxyz[3 * ri + k] - a.s.c[k]) - y[k];
    if (METRIC == RH_DIST_PLANE) {
        const double n0 = a.rnrm[3 * ri], n1 = a.rnrm[3 * ri + 1], n2 = a.rnrm[3 * ri + 2];
        const double r[6] = { y[1] * n2 - y[2] * n1, y[2] * n0 - y[0] * n2, y[0] * n1 - y[1] * n0, n0, n1, n2 };
        const double b = (e[0] * n0 + e[1] * n1) + e[2] * n2;
        int at = 0;
        for (int u = 0; u < 6; u++)
            for (int v = u; v < 6; v++) l[at++] = r[u] * r[v];
        for (int u = 0; u < 6; u++) l[at++] = r[u] * b;
        l[at] = b * b;
    } else {
        l[0] = y[0] * y[0]; l[1] = y[1] * y[1]; l[2] = y[2] * y[2];
        l[3] = y[0] * y[1]; l[4] = y[0] * y[2]; l[5] = y[1] * y[2];
        l[6] = y[0]; l[7] = y[1]; l[8] = y[2];
        l[9] = y[1] * e[2] - y[2] * e[1]; l[10] = y[2] * e[0] - y[0] * e[2]; l[11] = y[0] * e[1] - y[1] * e[0];
        l[12] = e[0]; l[13] = e[1]; l[14] = e[2];
        l[15] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    return true;
}

// Block b leaves T() of the leaves of its OUT_BLOCK_POINTS queries, component c at part[c * gridDim.x + b], and adds its
// valid queries to *nvalid (an integer count).  A grid of one block has the roots: it writes the count behind them, as
// bits, at part[NC].
template <int METRIC>
__global__ __launch_bounds__(OUT_THREADS) void reg_accumulate_kernel(RegAccArgs a, double *__restrict__ part, unsigned long long *nvalid)
{
    constexpr int NC = METRIC == RH_DIST_PLANE ? REG_NC_PLANE : REG_NC_POINT;
    const int64_t base = ((int64_t)blockIdx.x * OUT_THREADS + threadIdx.x) * OUT_PER_THREAD;
    double acc[NC], l[NC];
    int nv = 0;
    // (l0 + l1) + (l2 + l3), a pair at a time: never four sets of leaves at once
    nv += reg_leaves<METRIC>(a, base, acc);
    nv += reg_leaves<METRIC>(a, base + 1, l);
    for (int c = 0; c < NC; c++) acc[c] = acc[c] + l[c];
    {
        double h[NC];
        nv += reg_leaves<METRIC>(a, base + 2, h);
        nv += reg_leaves<METRIC>(a, base + 3, l);
        for (int c = 0; c < NC; c++) acc[c] = acc[c] + (h[c] + l[c]);
    }
    __shared__ double ws[OUT_THREADS / 64][NC];
    __shared__ int wn[OUT_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < NC; c++) {
        const double s = tree64(acc[c]);
        if (lane == 0) ws[wave][c] = s;
    }
    for (int j = 1; j < 64; j <<= 1) nv += __shfl_xor(nv, j);
    if (lane == 0) wn[wave] = nv;
    __syncthreads();
    if (threadIdx.x < NC) {
        const int c = threadIdx.x;
        part[(size_t)c * gridDim.x + blockIdx.x] = (ws[0][c] + ws[1][c]) + (ws[2][c] + ws[3][c]);
    }
    if (threadIdx.x == 0) {
        const unsigned long long cnt = (unsigned long long)((wn[0] + wn[1]) + (wn[2] + wn[3]));
        if (gridDim.x == 1) ((unsigned long long *)part)[NC] = cnt;
        else if (cnt) atomicAdd(nvalid, cnt);
    }
}

// One more level of the tree for every component: out_tree_kernel<2> of tree_sum.h with the component in blockIdx.y.
// Component c has its len values at in[c * len ..] and leaves gridDim.x of them at out[c * gridDim.x ..].  The launch that
// leaves the roots (gridDim.x == 1) copies the count behind them.
__global__ __launch_bounds__(OUT_THREADS) void reg_fold_kernel(const double *__restrict__ in, int64_t len, double *__restrict__ out,
                                                              const unsigned long long *nvalid)
{
    const double *v = in + (size_t)blockIdx.y * (size_t)len;
    const int64_t base = ((int64_t)blockIdx.x * OUT_THREADS + threadIdx.x) * OUT_PER_THREAD;
    double a[OUT_PER_THREAD];
    for (int j = 0; j < OUT_PER_THREAD; j++) a[j] = base + j < len ? v[base + j] : 0.0;
    const double s = tree64((a[0] + a[1]) + (a[2] + a[3]));
    __shared__ double ws[OUT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    if (gridDim.x == 1 && blockIdx.y == 0) ((unsigned long long *)out)[gridDim.y] = *nvalid;
}

// ------------------------------------------------------------------------------ host side ----
// H x = g by Cholesky in the stated order (ransac_hip.h, step 6); false: a pivot was not accepted
bool reg_solve(const double H[6][6], const double g[6], double x[6])
{
    double L[6][6], z[6];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double v = H[j][i];
            for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
            if (j < i) { L[i][j] = v / L[j][j]; continue; }
            if (!(v > 1e-10 * H[i][i])) return false;
            L[i][i] = sqrt(v);
        }
    for (int i = 0; i < 6; i++) {
        double v = g[i];
        for (int k = 0; k < i; k++) v = v - L[i][k] * z[k];
        z[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double v = z[i];
        for (int k = i + 1; k < 6; k++) v = v - L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    return true;
}

// the upper triangle of H (mirrored), g and E from the roots S(..) = T(..) + 0.0 (step 4)
void reg_system(int metric, const double *root, int64_t nvalid, double H[6][6], double g[6], double *E)
{
    double S[REG_NC_PLANE];
    const int nc = metric == RH_DIST_PLANE ? REG_NC_PLANE : REG_NC_POINT;
    for (int c = 0; c < nc; c++) S[c] = root[c] + 0.0;
    if (metric == RH_DIST_PLANE) {
        int at = 0;
        for (int u = 0; u < 6; u++)
            for (int v = u; v < 6; v++) H[u][v] = H[v][u] = S[at++];
        for (int u = 0; u < 6; u++) g[u] = S[at++];
        *E = S[at];
        return;
    }
    for (int u = 0; u < 6; u++)
        for (int v = 0; v < 6; v++) H[u][v] = 0.0;
    H[0][0] = S[1] + S[2]; H[1][1] = S[0] + S[2]; H[2][2] = S[0] + S[1];
    H[0][1] = H[1][0] = -S[3]; H[0][2] = H[2][0] = -S[4]; H[1][2] = H[2][1] = -S[5];
    H[0][4] = H[4][0] = -S[8]; H[0][5] = H[5][0] = S[7];
    H[1][3] = H[3][1] = S[8];  H[1][5] = H[5][1] = -S[6];
    H[2][3] = H[3][2] = -S[7]; H[2][4] = H[4][2] = S[6];
    H[3][3] = H[4][4] = H[5][5] = (double)nvalid;
    for (int u = 0; u < 6; u++) g[u] = S[9 + u];
    *E = S[15];
}

// step 7: the Cayley step of x on (R, t)
void reg_update(const double x[6], RegState &s)
{
    const double a0 = 0.5 * x[0], a1 = 0.5 * x[1], a2 = 0.5 * x[2];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2, d = 1.0 + aa, f = 1.0 - aa;
    double C[9];
    C[0] = (f + 2.0 * (a0 * a0)) / d; C[4] = (f + 2.0 * (a1 * a1)) / d; C[8] = (f + 2.0 * (a2 * a2)) / d;
    C[1] = (2.0 * (a0 * a1) - 2.0 * a2) / d; C[3] = (2.0 * (a0 * a1) + 2.0 * a2) / d;
    C[2] = (2.0 * (a0 * a2) + 2.0 * a1) / d; C[6] = (2.0 * (a0 * a2) - 2.0 * a1) / d;
    C[5] = (2.0 * (a1 * a2) - 2.0 * a0) / d; C[7] = (2.0 * (a1 * a2) + 2.0 * a0) / d;
    double Rn[9], tn[3];
    for (int k = 0; k < 3; k++) {
        for (int l = 0; l < 3; l++) Rn[3 * k + l] = (C[3 * k] * s.R[l] + C[3 * k + 1] * s.R[3 + l]) + C[3 * k + 2] * s.R[6 + l];
        tn[k] = ((C[3 * k] * s.t[0] + C[3 * k + 1] * s.t[1]) + C[3 * k + 2] * s.t[2]) + x[3 + k];
    }
    memcpy(s.R, Rn, sizeof Rn);
    memcpy(s.t, tn, sizeof tn);
}

template <typename T>
int reg_register(const T *ref_aos, const T *nrm_aos, int64_t n, const T *qry_aos, int64_t m, const rh_register_params *p,
                 const double *init, int device, double *transform_out, rh_register_result *result, int32_t *n_valid_it,
                 double *rms_it)
{
    static const char who[] = "rh_register";
    if (!p || !transform_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    RH_TRY(check_query(who, ref_aos, n, qry_aos, m, 1, p->radius));
    if (p->metric != RH_DIST_POINT && p->metric != RH_DIST_PLANE) {
        rh_set_error("%s: metric = %d is not a distance metric", who, p->metric);
        return RH_E_INVALID;
    }
    if (p->metric == RH_DIST_PLANE && !nrm_aos) { rh_set_error("%s: the plane metric needs the reference's normals", who); return RH_E_INVALID; }
    if (!(p->rot_tol >= 0.0) || !(p->trans_tol >= 0.0)) { rh_set_error("%s: rot_tol and trans_tol must be >= 0", who); return RH_E_INVALID; }
    if (p->max_iter < 1 || p->max_iter > RH_REG_MAX_ITERATIONS) {
        rh_set_error("%s: max_iter = %d outside 1 .. %d", who, p->max_iter, RH_REG_MAX_ITERATIONS);
        return RH_E_INVALID;
    }
    if (init)
        for (int i = 0; i < 12; i++)
            if (!isfinite(init[i])) { rh_set_error("%s: init is not finite", who); return RH_E_INVALID; }
    const int metric = p->metric, nc = metric == RH_DIST_PLANE ? REG_NC_PLANE : REG_NC_POINT;

    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    QuerySearch q;
    RH_TRY(q.open_reference(S, ref_aos, n, 1, p->radius));
    double *d_qry = nullptr, *d_moved = nullptr, *d_nrm = nullptr;
    RH_TRY(S.alloc(&d_qry, 3 * m));
    RH_TRY(S.upload(qry_aos, d_qry, 3 * m, hipMemcpyDefault));
    {   // the queries' finiteness, once: the moved ones are checked by every bind()
        double lo[3], hi[3];
        RH_TRY(cloud_box(S, d_qry, m, lo, hi));
    }
    RH_TRY(S.alloc(&d_moved, 3 * m));
    if (metric == RH_DIST_PLANE) {
        RH_TRY(S.alloc(&d_nrm, 3 * n));
        RH_TRY(S.upload(nrm_aos, d_nrm, 3 * n, hipMemcpyDefault));
    }
    RH_TRY(q.reserve(S, m));
    RH_TRY(S.alloc(&q.a.dist, m));
    RH_TRY(S.alloc(&q.a.nn, m));
    q.a.metric = RH_DIST_POINT;
    // the tree's levels: len[0] blocks of partials, then folds down to one; every level has room for the count behind it
    double *d_part[2] = { nullptr, nullptr };
    unsigned long long *d_cnt = nullptr;
    const int64_t len1 = (m + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS, len2 = (len1 + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS;
    RH_TRY(S.alloc(&d_part[0], nc * len1 + 1));
    RH_TRY(S.alloc(&d_part[1], nc * len2 + 1));
    RH_TRY(S.alloc(&d_cnt, 1));

    RegAccArgs acc;
    RegState &s = acc.s;
    for (int k = 0; k < 3; k++) s.c[k] = 0.5 * (q.ix.lo[k] + q.ix.hi[k]);
    static const double ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    const double *A = init ? init : ident;
    for (int k = 0; k < 3; k++) {
        for (int l = 0; l < 3; l++) s.R[3 * k + l] = A[4 * k + l];
        s.t[k] = (((A[4 * k] * s.c[0] + A[4 * k + 1] * s.c[1]) + A[4 * k + 2] * s.c[2]) + A[4 * k + 3]) - s.c[k];
    }
    acc.qxyz = d_qry; acc.nn = q.a.nn; acc.rxyz = q.ix.d_xyz; acc.rnrm = d_nrm; acc.m = m; acc.n = n;

    std::vector<int32_t> h_nv((size_t)p->max_iter, 0);
    std::vector<double> h_rms((size_t)p->max_iter, 0.0);
    int status = RH_REG_MAX_ITER, iters = 0;
    int64_t nvalid = 0;
    double rms = 0.0;
    for (int it = 0; it < p->max_iter; it++) {
        hipLaunchKernelGGL(reg_transform_kernel, dim3(blocks_for(m)), dim3(256), 0, st, s, d_qry, m, d_moved);
        SCOPE_HIP(S, hipGetLastError());
        RH_TRY(q.bind(S, d_moved));
        RH_TRY(q.run(S));
        SCOPE_HIP(S, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), st));
        if (metric == RH_DIST_PLANE)
            hipLaunchKernelGGL(reg_accumulate_kernel<RH_DIST_PLANE>, dim3((unsigned)len1), dim3(OUT_THREADS), 0, st, acc, d_part[0], d_cnt);
        else
            hipLaunchKernelGGL(reg_accumulate_kernel<RH_DIST_POINT>, dim3((unsigned)len1), dim3(OUT_THREADS), 0, st, acc, d_part[0], d_cnt);
        SCOPE_HIP(S, hipGetLastError());
        int cur = 0;
        for (int64_t len = len1; len > 1;) {
            const int64_t nb = (len + OUT_BLOCK_POINTS - 1) / OUT_BLOCK_POINTS;
            hipLaunchKernelGGL(reg_fold_kernel, dim3((unsigned)nb, (unsigned)nc), dim3(OUT_THREADS), 0, st, d_part[cur], len, d_part[cur ^ 1], d_cnt);
            SCOPE_HIP(S, hipGetLastError());
            cur ^= 1;
            len = nb;
        }
        double root[REG_NC_PLANE + 1];
        RH_TRY(S.fetch(root, d_part[cur], (size_t)(nc + 1)));
        unsigned long long cnt;
        memcpy(&cnt, &root[nc], sizeof cnt);
        if (cnt > (unsigned long long)m) { rh_set_error("%s: the count of valid queries is out of range", who); return RH_E_INTERNAL; }
        double H[6][6], g[6], x[6], E;
        nvalid = (int64_t)cnt;
        reg_system(metric, root, nvalid, H, g, &E);
        rms = nvalid ? sqrt(E / (double)nvalid) : 0.0;
        h_nv[(size_t)it] = (int32_t)nvalid;
        h_rms[(size_t)it] = rms;
        iters = it + 1;
        if (nvalid < 6) { status = RH_REG_TOO_FEW; break; }
        if (!reg_solve(H, g, x)) { status = RH_REG_DEGENERATE; break; }
        reg_update(x, s);
        if (sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) <= p->rot_tol && sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) <= p->trans_tol) {
            status = RH_REG_CONVERGED;
            break;
        }
    }
    for (int k = 0; k < 3; k++) {
        for (int l = 0; l < 3; l++) transform_out[4 * k + l] = s.R[3 * k + l];
        transform_out[4 * k + 3] = (s.t[k] + s.c[k]) - ((s.R[3 * k] * s.c[0] + s.R[3 * k + 1] * s.c[1]) + s.R[3 * k + 2] * s.c[2]);
    }
    if (result) { result->status = status; result->iterations = iters; result->n_valid = nvalid; result->rms = rms; }
    if (n_valid_it) memcpy(n_valid_it, h_nv.data(), sizeof(int32_t) * h_nv.size());
    if (rms_it) memcpy(rms_it, h_rms.data(), sizeof(double) * h_rms.size());
    return RH_OK;
}

}  // namespace

extern "C" int rh_register(const double *ref_xyz_aos, const double *ref_nrm_aos_or_null, int64_t n, const double *qry_xyz_aos,
                           int64_t m, const rh_register_params *p, const double *init_3x4_or_null, int device,
                           double *transform_out_3x4, rh_register_result *result_or_null, int32_t *n_valid_it_out_or_null,
                           double *rms_it_out_or_null)
{
    return reg_register<double>(ref_xyz_aos, ref_nrm_aos_or_null, n, qry_xyz_aos, m, p, init_3x4_or_null, device, transform_out_3x4,
                                result_or_null, n_valid_it_out_or_null, rms_it_out_or_null);
}

extern "C" int rh_register_f32(const float *ref_xyz_aos, const float *ref_nrm_aos_or_null, int64_t n, const float *qry_xyz_aos,
                               int64_t m, const rh_register_params *p, const double *init_3x4_or_null, int device,
                               double *transform_out_3x4, rh_register_result *result_or_null, int32_t *n_valid_it_out_or_null,
                               double *rms_it_out_or_null)
{
    return reg_register<float>(ref_xyz_aos, ref_nrm_aos_or_null, n, qry_xyz_aos, m, p, init_3x4_or_null, device, transform_out_3x4,
                               result_or_null, n_valid_it_out_or_null, rms_it_out_or_null);
}
