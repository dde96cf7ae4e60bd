// normals.hip -- oriented point normals for a cloud that has none (rh_estimate_normals, include/ransac_hip.h).
// The reference starts from clouds with normals and names the missing step: "If normal information is not available,
// there are algorithms to approximate it (PCA for example)" (docs/src/ransac.md:13).  This is that PCA, exact in its
// neighbours:
//   1. a uniform grid: cell width from the k-th neighbour distance of a sample of points (found exactly on a first,
//      coarse grid whose width comes from the bounding box), points radix-sorted by cell key, an open-addressing hash
//      table key -> [start, end) of the occupied cells only (empty space costs nothing);
//   2. one wave per query point, k <= 64 = the wave width: lane j holds the j-th best (d^2, rank) pair, rank 0 = the
//      point itself, rank i + 1 = point i (so ties go to the smaller index).  The cells of shell s (Chebyshev distance s
//      from the query's cell) stream their points in 64 at a time; a batch with a candidate below the k-th best is
//      sorted (bitonic, __shfl_xor) and merged with the best list.  The search stops when the k-th best d^2 is below
//      the squared distance to the faces of the cube searched so far (or beyond the radius), so the result is exact.
//      A point whose next shell would enumerate more cells than the hash table has slots scans the table instead
//      (every occupied cell not yet visited, pruned by its box distance): isolated points end, and end exact;
//   3. two-pass mean and covariance in binary64 (fixed butterfly order: the same bits on every run), cyclic Jacobi on
//      the 3x3 matrix (accurate when lambda0 ~ lambda1), degenerate rule, canonical sign, orientation.
// Steps 1 and 2 are the shared search of knn_grid.h / knn_device.h (rh_knn and rh_remove_outliers run on it too); this
// file holds step 3 and the entry points.
#include "jacobi3.h"
#include "knn_device.h"

namespace {

__device__ inline double wsum(double v)
{
    for (int j = 32; j > 0; j >>= 1) v += __shfl_xor(v, j);   // butterfly: every lane ends with the same bits
    return v;
}

struct NrmArgs {
    int orient;              // 0 canonical, 1 viewpoint, 2 hints
    double view[3];
    const double *hints;     // AoS, original order
};

template <typename OutT>
__global__ __launch_bounds__(NRM_BLOCK) void nrm_query_kernel(Grid g, KnnQuery kq, NrmArgs a, OutT *__restrict__ nrm,
                                                              OutT *__restrict__ curv, int32_t *__restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + (threadIdx.x >> 6);
    if (w >= kq.nq) return;                                       // wave-uniform
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, kq, lane, w, p, self, bd, br);
    const int k = kq.k;
    const double radius = kq.radius;

    // the neighbourhood: the first k of the order, those beyond the radius dropped (a prefix of the list)
    const double r2 = radius * radius;
    const bool in = lane < k && br != NRM_NORANK && (radius <= 0.0 || bd <= r2);
    const int m = __popcll(__builtin_amdgcn_ballot_w64(in));
    double q[3] = { 0.0, 0.0, 0.0 };
    if (in) {
        const int64_t qi = br == 0 ? (int64_t)self : (int64_t)br - 1;
        for (int ax = 0; ax < 3; ax++) q[ax] = g.xyz[3 * qi + ax];
    }
    double mean[3], e[3];
    for (int ax = 0; ax < 3; ax++) mean[ax] = wsum(q[ax]) / (double)m;
    for (int ax = 0; ax < 3; ax++) e[ax] = in ? q[ax] - mean[ax] : 0.0;
    double A[3][3];
    A[0][0] = wsum(e[0] * e[0]) / m; A[0][1] = wsum(e[0] * e[1]) / m; A[0][2] = wsum(e[0] * e[2]) / m;
    A[1][1] = wsum(e[1] * e[1]) / m; A[1][2] = wsum(e[1] * e[2]) / m; A[2][2] = wsum(e[2] * e[2]) / m;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    if (lane != 0) return;

    double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    rh_jacobi3(A, V);
    int i0 = 0, i1 = 1, i2 = 2;                                    // ascending eigenvalues
    if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
    if (A[i2][i2] < A[i1][i1]) { const int t = i1; i1 = i2; i2 = t; }
    if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
    const double l0 = A[i0][i0], l1 = A[i1][i1], l2 = A[i2][i2];
    double nv[3] = { V[0][i0], V[1][i0], V[2][i0] };
    const double nn = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    for (int ax = 0; ax < 3; ax++) nv[ax] /= nn;
    double cv = l0 / ((l0 + l1) + l2);
    bool degenerate = m < 3 || l2 == 0.0 || l1 <= 1e-12 * l2 || !(isfinite(nv[0]) && isfinite(nv[1]) && isfinite(nv[2]))
                      || !isfinite(cv);
    if (degenerate) {
        nv[0] = nv[1] = nv[2] = 0.0;
        cv = 0.0;
    } else {
        int im = 0;                                                // canonical sign: the largest component positive
        if (fabs(nv[1]) > fabs(nv[im])) im = 1;
        if (fabs(nv[2]) > fabs(nv[im])) im = 2;
        double sg = nv[im] < 0.0 ? -1.0 : 1.0;
        double dot = 0.0;
        if (a.orient == 1)
            dot = (sg * nv[0] * (a.view[0] - p[0]) + sg * nv[1] * (a.view[1] - p[1])) + sg * nv[2] * (a.view[2] - p[2]);
        else if (a.orient == 2) {
            const double *hv = a.hints + 3 * (int64_t)self;
            dot = (sg * nv[0] * hv[0] + sg * nv[1] * hv[1]) + sg * nv[2] * hv[2];
        }
        if (dot < 0.0) sg = -sg;
        for (int ax = 0; ax < 3; ax++) nv[ax] = sg * nv[ax] + 0.0;   // (+ 0.0: no negative zero)
    }
    for (int ax = 0; ax < 3; ax++) nrm[3 * (int64_t)self + ax] = (OutT)nv[ax];
    if (curv) curv[self] = (OutT)cv;
    if (flags) flags[self] = degenerate ? 1 : 0;
}

template <typename T>
int estimate(const T *xyz_aos, int64_t n, const rh_normals_params *p, const T *hints, int device, T *nrm_out,
             T *curv_out, int32_t *flags_out)
{
    static const char who[] = "rh_estimate_normals";
    if (!xyz_aos || !p || !nrm_out) { rh_set_error("rh_estimate_normals: NULL argument"); return RH_E_INVALID; }
    if (n < 1 || n > (int64_t)0x7FFFF000) { rh_set_error("rh_estimate_normals: n = %lld outside 1 .. 2^31 - 4096", (long long)n); return RH_E_INVALID; }
    if (p->k < 3 || p->k > 64) { rh_set_error("rh_estimate_normals: k = %d outside 3 .. 64", p->k); return RH_E_INVALID; }
    if (p->orient < 0 || p->orient > 2) { rh_set_error("rh_estimate_normals: orient = %d outside 0 .. 2", p->orient); return RH_E_INVALID; }
    if (p->orient == 2 && !hints) { rh_set_error("rh_estimate_normals: orient = 2 needs hints"); return RH_E_INVALID; }
    if (!(isfinite(p->radius) && p->radius >= 0.0)) { rh_set_error("rh_estimate_normals: radius must be finite and >= 0"); return RH_E_INVALID; }
    if (p->orient == 1 && !(isfinite(p->viewpoint[0]) && isfinite(p->viewpoint[1]) && isfinite(p->viewpoint[2]))) {
        rh_set_error("rh_estimate_normals: the viewpoint is not finite");
        return RH_E_INVALID;
    }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;

    double *d_xyz = nullptr, *d_hints = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyHostToDevice));
    if (p->orient == 2) {
        RH_TRY(S.alloc(&d_hints, 3 * n));
        RH_TRY(S.upload(hints, d_hints, 3 * n, hipMemcpyHostToDevice));
    }
    KnnIndex ix;
    RH_TRY(ix.init(S, d_xyz, n));
    KnnQuery kq;
    RH_TRY(knn_index_for_k(ix, p->k, p->radius, kq));

    NrmArgs na;
    memset(&na, 0, sizeof na);
    na.orient = p->orient;
    for (int ax = 0; ax < 3; ax++) na.view[ax] = p->viewpoint[ax];
    na.hints = d_hints;
    // every point's neighbours and normal
    T *d_nrm = nullptr, *d_curv = nullptr;
    int32_t *d_flags = nullptr;
    RH_TRY(S.alloc(&d_nrm, 3 * n));
    if (curv_out) RH_TRY(S.alloc(&d_curv, n));
    if (flags_out) RH_TRY(S.alloc(&d_flags, n));
    hipLaunchKernelGGL(nrm_query_kernel<T>, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, na, d_nrm, d_curv, d_flags);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(nrm_out, d_nrm, sizeof(T) * 3 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (curv_out) SCOPE_HIP(S, hipMemcpyAsync(curv_out, d_curv, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (flags_out) SCOPE_HIP(S, hipMemcpyAsync(flags_out, d_flags, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}

}  // namespace

extern "C" int rh_estimate_normals(const double *xyz_aos, int64_t n, const rh_normals_params *p, const double *hints_aos_or_null,
                                   int device, double *nrm_out_aos, double *curv_out_or_null, int32_t *flags_out_or_null)
{
    return estimate<double>(xyz_aos, n, p, hints_aos_or_null, device, nrm_out_aos, curv_out_or_null, flags_out_or_null);
}

extern "C" int rh_estimate_normals_f32(const float *xyz_aos, int64_t n, const rh_normals_params *p, const float *hints_aos_or_null,
                                       int device, float *nrm_out_aos, float *curv_out_or_null, int32_t *flags_out_or_null)
{
    return estimate<float>(xyz_aos, n, p, hints_aos_or_null, device, nrm_out_aos, curv_out_or_null, flags_out_or_null);
}
