// describe.hip -- an integer point-feature histogram per point of a raw cloud with normals (rh_describe;
// include/ransac_hip.h states the definition in full, operation by operation).  The search is the shared one of
// knn_grid.h / knn_device.h, the one rh_knn runs: a list of k + 1 entries whose first is the point itself.
//   1. desc_pair_kernel, one wave per point i: lane j = neighbour j of rh_knn's list.  The lane forms the three pair
//      features of (i, j) in binary64 and their bins; the wave's 33 counts S_i are integer adds in its own LDS row.  S_i
//      (uint16, <= 63), the neighbour list and count_i go to global memory: 66 + 4k + 4 bytes per point;
//   2. desc_gather_kernel, one thread per (i, c): D_i[c] = count_i * S_i[c] + sum over the list of S_j[c].  Integers
//      only, so the order of the sum does not show.
// No floating-point sums at all, no atomics on global memory: the same bytes on every run.
#include "knn_device.h"

namespace {

constexpr int DESC_DIM = RH_DESC_DIM;

__device__ __forceinline__ double desc_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void desc_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// clamp(floor(x), 0, 10), decided in binary64 (x may be beyond any integer type)
__device__ __forceinline__ int desc_bin(double x)
{
    const double t = floor(x);
    return t < 0.0 ? 0 : (t > 10.0 ? 10 : (int)t);
}

// the wave's LDS row: what its lanes wrote before is seen by all of them after
__device__ __forceinline__ void desc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the bins of the pair (p_i, u = n_i) -> (p_j, s = n_j); false: the pair is degenerate (ransac_hip.h, step 2)
__device__ inline bool desc_pair(const double pi[3], const double u[3], const double pj[3], const double s[3], int bin[3])
{
    const double d[3] = { pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2] };
    const double d2 = desc_dot(d, d);
    double v[3], w[3];
    desc_cross(u, d, v);
    const double v2 = desc_dot(v, v);
    desc_cross(u, v, w);
    const double len = sqrt(d2), vl = sqrt(v2);
    const double f1 = desc_dot(u, d) / len;
    const double f2 = desc_dot(v, s) / vl;
    const double a = desc_dot(w, s) / vl;
    const double b = desc_dot(u, s);
    const double g = fabs(a) + fabs(b);
    const double r = b / g;
    const double psi = a >= 0.0 ? 1.0 - r : 3.0 + r;
    if (d2 == 0.0 || v2 == 0.0 || g == 0.0 || f1 != f1 || f2 != f2 || psi != psi) return false;
    bin[0] = desc_bin((f1 + 1.0) * 5.5);
    bin[1] = desc_bin((f2 + 1.0) * 5.5);
    bin[2] = desc_bin(psi * 2.75);
    return true;
}

__global__ __launch_bounds__(NRM_BLOCK) void desc_pair_kernel(Grid g, KnnQuery kq, const double *__restrict__ nrm,
                                                             uint16_t *__restrict__ spfh, int32_t *__restrict__ nb,
                                                             int32_t *__restrict__ count)
{
    __shared__ int hist[NRM_BLOCK / 64][DESC_DIM + 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * (NRM_BLOCK / 64) + wave;
    if (w >= kq.nq) return;                                       // wave-uniform; no block-wide barrier below
    double p[3], bd;
    int32_t self;
    uint32_t br;
    knn_search(g, kq, lane, w, p, self, bd, br);
    if (self < 0 || (int64_t)self >= kq.n) return;                // (wave-uniform) nothing is addressed through a bad index
    const int kk = kq.k - 1;
    const double r2 = kq.radius * kq.radius;
    const bool in = lane >= 1 && lane <= kk && br != NRM_NORANK && br != 0u && (int64_t)br <= kq.n && (kq.radius <= 0.0 || bd <= r2);
    const int cnt = __popcll(__builtin_amdgcn_ballot_w64(in));
    int *h = hist[wave];
    if (lane < DESC_DIM) h[lane] = 0;
    desc_wave_sync();
    if (in) {
        const int64_t j = (int64_t)br - 1;
        const double pj[3] = { g.xyz[3 * j], g.xyz[3 * j + 1], g.xyz[3 * j + 2] };
        const double u[3] = { nrm[3 * (int64_t)self], nrm[3 * (int64_t)self + 1], nrm[3 * (int64_t)self + 2] };
        const double s[3] = { nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2] };
        int bin[3];
        if (desc_pair(p, u, pj, s, bin)) {
            atomicAdd(&h[bin[0]], 1);
            atomicAdd(&h[11 + bin[1]], 1);
            atomicAdd(&h[22 + bin[2]], 1);
        }
    }
    desc_wave_sync();
    if (lane < DESC_DIM) spfh[(int64_t)self * DESC_DIM + lane] = (uint16_t)h[lane];
    if (lane >= 1 && lane <= kk) nb[(int64_t)self * kk + (lane - 1)] = in ? (int32_t)br : 0;
    if (lane == 0) count[self] = cnt;
}

__global__ __launch_bounds__(256) void desc_gather_kernel(const uint16_t *__restrict__ spfh, const int32_t *__restrict__ nb,
                                                          const int32_t *__restrict__ count, int64_t n, int kk,
                                                          uint16_t *__restrict__ desc)
{
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n * DESC_DIM) return;
    const int64_t i = at / DESC_DIM;
    const int c = (int)(at - i * DESC_DIM);
    const int cnt = count[i];
    int acc = cnt * (int)spfh[at];
    for (int l = 0; l < kk; l++) {                                // the list is a prefix: 0 behind count_i
        const int64_t j = (int64_t)nb[i * kk + l] - 1;
        if (j >= 0 && j < n) acc += (int)spfh[j * DESC_DIM + c];
    }
    desc[at] = (uint16_t)acc;
}

template <typename T>
int describe(const T *xyz_aos, const T *nrm_aos, int64_t n, int32_t k, double radius, int device, uint16_t *desc_out,
             int32_t *count_out)
{
    static const char who[] = "rh_describe";
    if (!xyz_aos || !nrm_aos || !desc_out) { rh_set_error("%s: NULL argument", who); return RH_E_INVALID; }
    if (n < 1 || n > (int64_t)0x7FFFFFFF / DESC_DIM) { rh_set_error("%s: n = %lld outside 1 .. (2^31 - 1) / 33", who, (long long)n); return RH_E_INVALID; }
    if (k < 1 || k > RH_KNN_MAX_K) { rh_set_error("%s: k = %d outside 1 .. %d", who, k, RH_KNN_MAX_K); return RH_E_INVALID; }
    if (!(isfinite(radius) && radius >= 0.0)) { rh_set_error("%s: radius must be finite and >= 0", who); return RH_E_INVALID; }
    CallScope S;
    RH_TRY(S.open(who, device));
    const hipStream_t st = S.st;
    double *d_xyz = nullptr, *d_nrm = nullptr;
    RH_TRY(S.alloc(&d_xyz, 3 * n));
    RH_TRY(S.upload(xyz_aos, d_xyz, 3 * n, hipMemcpyDefault));
    RH_TRY(S.alloc(&d_nrm, 3 * n));
    RH_TRY(S.upload(nrm_aos, d_nrm, 3 * n, hipMemcpyDefault));
    {   // the normals' finiteness: the bounding-box pass counts the rows that are finite
        double lo[3], hi[3];
        if (cloud_box(S, d_nrm, n, lo, hi) != RH_OK) { rh_set_error("%s: a normal is not finite", who); return RH_E_INVALID; }
    }
    KnnIndex ix;
    KnnQuery kq;
    RH_TRY(ix.init(S, d_xyz, n));                                  // (a coordinate that is not finite ends the call here)
    RH_TRY(knn_index_for_k(ix, k + 1, radius, kq));
    uint16_t *d_spfh = nullptr, *d_desc = nullptr;
    int32_t *d_nb = nullptr, *d_count = nullptr;
    RH_TRY(S.alloc(&d_spfh, n * DESC_DIM));
    RH_TRY(S.alloc(&d_desc, n * DESC_DIM));
    RH_TRY(S.alloc(&d_nb, n * k));
    RH_TRY(S.alloc(&d_count, n));
    hipLaunchKernelGGL(desc_pair_kernel, dim3(blocks_for(n, NRM_BLOCK / 64)), dim3(NRM_BLOCK), 0, st, ix.g, kq, d_nrm, d_spfh, d_nb, d_count);
    SCOPE_HIP(S, hipGetLastError());
    hipLaunchKernelGGL(desc_gather_kernel, dim3(blocks_for(n * DESC_DIM)), dim3(256), 0, st, d_spfh, d_nb, d_count, n, (int)k, d_desc);
    SCOPE_HIP(S, hipGetLastError());
    SCOPE_HIP(S, hipMemcpyAsync(desc_out, d_desc, sizeof(uint16_t) * (size_t)n * DESC_DIM, hipMemcpyDefault, st));
    if (count_out) SCOPE_HIP(S, hipMemcpyAsync(count_out, d_count, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st));
    SCOPE_HIP(S, hipStreamSynchronize(st));
    return RH_OK;
}

}  // namespace

extern "C" int rh_describe(const double *xyz_aos, const double *nrm_aos, int64_t n, int32_t k, double radius, int device,
                           uint16_t *desc_out, int32_t *count_out_or_null)
{
    return describe<double>(xyz_aos, nrm_aos, n, k, radius, device, desc_out, count_out_or_null);
}

extern "C" int rh_describe_f32(const float *xyz_aos, const float *nrm_aos, int64_t n, int32_t k, double radius, int device,
                               uint16_t *desc_out, int32_t *count_out_or_null)
{
    return describe<float>(xyz_aos, nrm_aos, n, k, radius, device, desc_out, count_out_or_null);
}
