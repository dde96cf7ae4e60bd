// extent.hip -- oriented extents and fit residuals of extracted shapes: for b shapes with their index lists, the frame the
// points suggest, their box in that frame and their distances to the shape (include/ransac_hip.h states the definition in
// full).  The stage after the loop: it reads the cloud's resident coordinate planes and changes nothing on the cloud.
//
// Work item = a chunk of EXT_CHUNK list entries that never crosses a segment (= shape) boundary, so a 170 000-point plane
// next to a 300-point cone is 167 blocks next to one, not one long wave next to a short one.  The chunk table is a formula:
// segment j owns the chunk numbers  offsets[j] / EXT_CHUNK + j  ..  offsets[j + 1] / EXT_CHUNK + j  (one more than it can
// need: a segment of q whole chunks + t entries starting r entries into a chunk takes q + (t > 0) <= q + (r + t) / CHUNK + 1),
// chunk c of it covers the entries offsets[j] + c * EXT_CHUNK ..., and a block finds its segment by bisection on that
// strictly increasing first-chunk number.  offsets[b] / EXT_CHUNK + b chunks in all; the few a segment leaves unused
// write an empty row.  Chunks are cut from the segment's own start, so a shape's sums are the same bits alone or in a batch.
//   pass 1   one block per chunk: bounds-check the indices, gather x / y / z, n, sum q, sum q q^T (q = p - first listed point)
//            -> butterfly across the wave, LDS across the waves in wave order, one partial row per chunk
//   fold 1   one wave per shape: lanes add the rows k0 + lane, k0 + lane + 64, ... and meet in a butterfly; S, the 2 x 2 or
//            3 x 3 eigenproblem, the frame, centroid, lambda, n, flags -> the shape's record
//   pass 2   the same chunks against the record's frame: (tu, tv, tw), e; six minima / maxima, max |e|, sum e^2 per chunk
//   fold 2   lo, hi, dist_maxabs, dist_rms
// Every sum has a fixed order (no floating-point atomics); the only atomic is the OR into the call's error word.
#include <math.h>
#include <string.h>

#include <vector>

#include "call_scope.h"
#include "jacobi3.h"
#include "rh_internal.h"

namespace {

constexpr int EXT_BLOCK = 256;
constexpr int EXT_PER_LANE = 4;
constexpr int EXT_CHUNK = EXT_BLOCK * EXT_PER_LANE;
constexpr int EXT_ROW = 10;   // doubles per partial row: pass 1 fills all ten (n, 3 sums, 6 products), pass 2 eight
// the error word
enum { EXT_BAD_OFFSETS = 1, EXT_BAD_INDEX = 2, EXT_BAD_COORD = 4, EXT_BAD_AXIS = 8, EXT_BAD_KIND = 16 };

struct ext_job {
    const rh_shape *shapes;
    const int64_t *off;      // [b + 1]
    const int64_t *idx;      // [total], 1-based
    rh_extent *out;          // [b]
    double *part;            // [nchunks][EXT_ROW]
    int32_t *flag;
    int64_t total, nchunks, n, stride;
    int32_t b;
};

// offsets are only trusted as far as they are used: clamped into the list, so that no entry outside it is ever addressed
__device__ __forceinline__ int64_t seg_off(const ext_job &J, int32_t j)
{
    const int64_t o = J.off[j];
    return o < 0 ? 0 : (o > J.total ? J.total : o);
}
__device__ __forceinline__ int64_t seg_first_chunk(const ext_job &J, int32_t j) { return seg_off(J, j) / EXT_CHUNK + j; }

// chunk k -> its segment and its entries [s, e) (s >= e: one of the spare chunks)
__device__ __forceinline__ int32_t chunk_range(const ext_job &J, int64_t k, int64_t &s, int64_t &e)
{
    int32_t lo = 0, hi = J.b - 1;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi + 1) >> 1);
        if (seg_first_chunk(J, mid) <= k) lo = mid;
        else hi = mid - 1;
    }
    const int64_t o0 = seg_off(J, lo), o1 = seg_off(J, lo + 1), c = k - (o0 / EXT_CHUNK + lo);
    s = c < 0 ? o1 : o0 + c * EXT_CHUNK;
    e = s + EXT_CHUNK < o1 ? s + EXT_CHUNK : o1;
    return lo;
}

// 1-based list entry -> 0-based point, -1 unless it lies in 1 .. n
__device__ __forceinline__ int64_t point_of(int64_t entry, int64_t n)
{
    const uint64_t i = (uint64_t)entry - 1ULL;
    return i < (uint64_t)n ? (int64_t)i : -1;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // butterfly: every lane ends with the same bits
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// the first listed point of a segment (the shift of the moments) -> 0, or the EXT_BAD_* bit of what is wrong with it
template <typename T>
__device__ __forceinline__ int first_point(const ext_job &J, const T *__restrict__ pts, int64_t o0, double p0[3])
{
    p0[0] = p0[1] = p0[2] = 0.0;
    if (o0 >= J.total) return EXT_BAD_OFFSETS;
    const int64_t i0 = point_of(J.idx[o0], J.n);
    if (i0 < 0) return EXT_BAD_INDEX;
    p0[0] = (double)pts[i0]; p0[1] = (double)pts[J.stride + i0]; p0[2] = (double)pts[2 * J.stride + i0];
    return finite3(p0[0], p0[1], p0[2]) ? 0 : EXT_BAD_COORD;
}

// ---- pass 1: n, sum q, sum q q^T per chunk
template <typename T>
__global__ void __launch_bounds__(EXT_BLOCK) ext_moments_kernel(ext_job J, const T *__restrict__ pts)
{
    __shared__ double sh[EXT_BLOCK / 64][EXT_ROW];
    const int64_t k = blockIdx.x;
    int64_t s, e;
    const int32_t j = chunk_range(J, k, s, e);
    double a[EXT_ROW];
#pragma unroll
    for (int t = 0; t < EXT_ROW; t++) a[t] = 0.0;
    if (s < e) {   // (block-uniform)
        double p0[3];
        int bad = first_point(J, pts, seg_off(J, j), p0);
        if (!bad) {
#pragma unroll
            for (int r = 0; r < EXT_PER_LANE; r++) {
                const int64_t pos = s + r * EXT_BLOCK + threadIdx.x;
                if (pos >= e) continue;
                const int64_t i = point_of(J.idx[pos], J.n);
                if (i < 0) { bad |= EXT_BAD_INDEX; continue; }
                const double x = (double)pts[i], y = (double)pts[J.stride + i], z = (double)pts[2 * J.stride + i];
                if (!finite3(x, y, z)) { bad |= EXT_BAD_COORD; continue; }
                const double qx = x - p0[0], qy = y - p0[1], qz = z - p0[2];
                a[0] += 1.0;
                a[1] += qx; a[2] += qy; a[3] += qz;
                a[4] += qx * qx; a[5] += qx * qy; a[6] += qx * qz;
                a[7] += qy * qy; a[8] += qy * qz; a[9] += qz * qz;
            }
        }
        if (bad) atomicOr(J.flag, bad);
    }
#pragma unroll
    for (int t = 0; t < EXT_ROW; t++) a[t] = wave_sum(a[t]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int t = 0; t < EXT_ROW; t++) sh[threadIdx.x >> 6][t] = a[t];
    }
    __syncthreads();
    if (threadIdx.x < EXT_ROW) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < EXT_BLOCK / 64; w++) v += sh[w][threadIdx.x];
        J.part[k * EXT_ROW + threadIdx.x] = v;
    }
}

__device__ __forceinline__ double norm3(const double a[3]) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// unit length, the component of largest magnitude positive (the first one on a tie)
__device__ __forceinline__ void unit_signed(double u[3])
{
    const double nn = norm3(u);
    for (int t = 0; t < 3; t++) u[t] /= nn;
    int big = 0;
    if (fabs(u[1]) > fabs(u[big])) big = 1;
    if (fabs(u[2]) > fabs(u[big])) big = 2;
    if (u[big] < 0.0)
        for (int t = 0; t < 3; t++) u[t] = -u[t];
}

// ---- fold 1: one wave per shape -> frame, centroid, lambda, n, flags (and the checks on offsets, kind and axis)
template <typename T>
__global__ void __launch_bounds__(64) ext_frame_kernel(ext_job J, const T *__restrict__ pts)
{
    const int32_t j = blockIdx.x;
    const int lane = threadIdx.x;
    const rh_shape sh = J.shapes[j];
    int bad = 0;
    if (J.off[j + 1] < J.off[j] || (j == 0 && J.off[0] != 0) || (j == J.b - 1 && J.off[J.b] != J.total)) bad |= EXT_BAD_OFFSETS;
    int64_t k0 = seg_first_chunk(J, j), k1 = seg_first_chunk(J, j + 1);
    if (k1 > J.nchunks) k1 = J.nchunks;
    double a[EXT_ROW];
#pragma unroll
    for (int t = 0; t < EXT_ROW; t++) a[t] = 0.0;
    for (int64_t k = k0 + lane; k < k1; k += 64) {
#pragma unroll
        for (int t = 0; t < EXT_ROW; t++) a[t] += J.part[k * EXT_ROW + t];
    }
#pragma unroll
    for (int t = 0; t < EXT_ROW; t++) a[t] = wave_sum(a[t]);

    rh_extent E;
    E.n = (int64_t)a[0];
    E.kind = sh.kind;
    E.flags = 0;
    for (int t = 0; t < 9; t++) E.frame[t] = 0.0;
    for (int t = 0; t < 3; t++) E.origin[t] = E.lo[t] = E.hi[t] = E.centroid[t] = E.lambda[t] = 0.0;
    E.dist_rms = E.dist_maxabs = 0.0;
    const int kind = sh.kind;
    double axis[3] = { 0.0, 0.0, 0.0 };
    if (kind == RH_PLANE) { for (int t = 0; t < 3; t++) { E.origin[t] = sh.v[t]; axis[t] = sh.v[3 + t]; } }
    else if (kind == RH_SPHERE) { for (int t = 0; t < 3; t++) E.origin[t] = sh.v[t]; }
    else if (kind == RH_CYLINDER) { for (int t = 0; t < 3; t++) { E.origin[t] = sh.v[3 + t]; axis[t] = sh.v[t]; } }
    else if (kind == RH_CONE) { for (int t = 0; t < 3; t++) { E.origin[t] = sh.v[t]; axis[t] = sh.v[3 + t]; } }
    else bad |= EXT_BAD_KIND;
    double w[3] = { 0.0, 0.0, 1.0 };
    if (kind != RH_SPHERE && !(bad & EXT_BAD_KIND)) {
        const double nn = norm3(axis);
        if (!(nn > 0.0) || !isfinite(nn)) bad |= EXT_BAD_AXIS;
        else for (int t = 0; t < 3; t++) w[t] = axis[t] / nn;
    }
    double p0[3] = { 0.0, 0.0, 0.0 };
    if (E.n > 0) bad |= first_point(J, pts, seg_off(J, j), p0);   // (pass 1 has said so already)
    if (bad) {
        if (lane == 0) { atomicOr(J.flag, bad); J.out[j] = E; }
        return;
    }
    if (E.n == 0) {
        E.flags = RH_EXT_EMPTY;
        if (lane == 0) J.out[j] = E;
        return;
    }
    const double n = (double)E.n;
    const double m[3] = { a[1] / n, a[2] / n, a[3] / n };
    double S[3][3];
    S[0][0] = a[4] / n - m[0] * m[0]; S[0][1] = a[5] / n - m[0] * m[1]; S[0][2] = a[6] / n - m[0] * m[2];
    S[1][1] = a[7] / n - m[1] * m[1]; S[1][2] = a[8] / n - m[1] * m[2]; S[2][2] = a[9] / n - m[2] * m[2];
    S[1][0] = S[0][1]; S[2][0] = S[0][2]; S[2][1] = S[1][2];
    for (int t = 0; t < 3; t++) E.centroid[t] = p0[t] + m[t];
    double u[3], v[3];
    double V[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    if (kind == RH_SPHERE) {
        rh_jacobi3(S, V);
        int i0 = 0, i1 = 1, i2 = 2;                                    // descending eigenvalues
        if (S[i1][i1] > S[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
        if (S[i2][i2] > S[i1][i1]) { const int t = i1; i1 = i2; i2 = t; }
        if (S[i1][i1] > S[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
        E.lambda[0] = S[i0][i0]; E.lambda[1] = S[i1][i1]; E.lambda[2] = S[i2][i2];
        if (E.lambda[0] > 0.0) {
            for (int t = 0; t < 3; t++) { u[t] = V[t][i0]; v[t] = V[t][i1]; }
            unit_signed(u);
            unit_signed(v);
            cross3(u, v, w);
        } else {
            E.flags |= RH_EXT_NO_DIRECTION;
            u[0] = 1.0; u[1] = 0.0; u[2] = 0.0;
            v[0] = 0.0; v[1] = 1.0; v[2] = 0.0;
            w[0] = 0.0; w[1] = 0.0; w[2] = 1.0;
        }
    } else {
        // an orthonormal basis (b1, b2) of the plane across w -- b1 is the fallback's u --, S restricted to it, one rotation
        int kk = 0;
        if (fabs(w[1]) < fabs(w[kk])) kk = 1;
        if (fabs(w[2]) < fabs(w[kk])) kk = 2;
        double b1[3], b2[3];
        for (int t = 0; t < 3; t++) b1[t] = (t == kk ? 1.0 : 0.0) - w[t] * w[kk];
        const double nb = norm3(b1);
        for (int t = 0; t < 3; t++) b1[t] /= nb;
        cross3(w, b1, b2);
        double s1[3], s2[3];
        for (int t = 0; t < 3; t++) { s1[t] = dot3(S[t], b1); s2[t] = dot3(S[t], b2); }
        double A[3][3] = { { dot3(b1, s1), dot3(b1, s2), 0.0 }, { 0.0, dot3(b2, s2), 0.0 }, { 0.0, 0.0, 0.0 } };
        A[1][0] = A[0][1];
        rh_jrot(A, V, 0, 1);
        const int i0 = A[1][1] > A[0][0] ? 1 : 0;
        E.lambda[0] = A[i0][i0];
        E.lambda[1] = A[1 - i0][1 - i0];
        if (E.lambda[0] > 0.0) {
            for (int t = 0; t < 3; t++) u[t] = V[0][i0] * b1[t] + V[1][i0] * b2[t];
            const double uw = dot3(u, w);
            for (int t = 0; t < 3; t++) u[t] = u[t] - w[t] * uw;
            unit_signed(u);
        } else {
            E.flags |= RH_EXT_NO_DIRECTION;
            for (int t = 0; t < 3; t++) u[t] = b1[t];
        }
        cross3(w, u, v);
    }
    for (int t = 0; t < 3; t++) { E.frame[t] = u[t]; E.frame[3 + t] = v[t]; E.frame[6 + t] = w[t]; }
    if (lane == 0) J.out[j] = E;
}

// ---- pass 2: coordinates in the frame and distances per chunk
template <typename T>
__global__ void __launch_bounds__(EXT_BLOCK) ext_box_kernel(ext_job J, const T *__restrict__ pts)
{
    __shared__ double sh[EXT_BLOCK / 64][8];
    const int64_t k = blockIdx.x;
    int64_t s, e;
    const int32_t j = chunk_range(J, k, s, e);
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY }, amax = 0.0, ssq = 0.0;
    if (s < e) {   // (block-uniform, and so are the shape and its record)
        const rh_extent *__restrict__ R = J.out + j;
        const rh_shape *__restrict__ sp = J.shapes + j;
        const int kind = R->kind;
        double o[3], f[9];
        for (int t = 0; t < 3; t++) o[t] = R->origin[t];
        for (int t = 0; t < 9; t++) f[t] = R->frame[t];
        const double r = kind == RH_SPHERE ? sp->v[3] : sp->v[6], c7 = sp->v[7], c8 = sp->v[8];
#pragma unroll
        for (int q = 0; q < EXT_PER_LANE; q++) {
            const int64_t pos = s + q * EXT_BLOCK + threadIdx.x;
            if (pos >= e) continue;
            const int64_t i = point_of(J.idx[pos], J.n);
            if (i < 0) continue;   // (pass 1 raised the flag)
            const double x = (double)pts[i], y = (double)pts[J.stride + i], z = (double)pts[2 * J.stride + i];
            const double dx = x - o[0], dy = y - o[1], dz = z - o[2];
            double t[3];
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                t[ax] = (dx * f[3 * ax] + dy * f[3 * ax + 1]) + dz * f[3 * ax + 2];
                lo[ax] = t[ax] < lo[ax] ? t[ax] : lo[ax];
                hi[ax] = t[ax] > hi[ax] ? t[ax] : hi[ax];
            }
            double d;
            if (kind == RH_PLANE) d = t[2];
            else if (kind == RH_SPHERE) d = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) - r;
            else if (kind == RH_CYLINDER) d = sqrt(t[0] * t[0] + t[1] * t[1]) - r;
            else d = sqrt(t[0] * t[0] + t[1] * t[1]) * c7 + t[2] * c8;
            const double ad = fabs(d);
            amax = ad > amax ? ad : amax;
            ssq += d * d;
        }
    }
    double v[8];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) { v[ax] = wave_min(lo[ax]); v[3 + ax] = wave_max(hi[ax]); }
    v[6] = wave_max(amax);
    v[7] = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int t = 0; t < 8; t++) sh[threadIdx.x >> 6][t] = v[t];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int t = threadIdx.x;
        double x = sh[0][t];
        for (int w = 1; w < EXT_BLOCK / 64; w++) {
            const double y = sh[w][t];
            x = t < 3 ? (y < x ? y : x) : t < 7 ? (y > x ? y : x) : x + y;
        }
        J.part[k * EXT_ROW + t] = x;
    }
}

// ---- fold 2: lo, hi, dist_maxabs, dist_rms; a call with bad input marks every record
__global__ void __launch_bounds__(64) ext_finish_kernel(ext_job J)
{
    const int32_t j = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t k0 = seg_first_chunk(J, j), k1 = seg_first_chunk(J, j + 1);
    if (k1 > J.nchunks) k1 = J.nchunks;
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY }, amax = 0.0, ssq = 0.0;
    for (int64_t k = k0 + lane; k < k1; k += 64) {
        const double *row = J.part + k * EXT_ROW;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            lo[ax] = row[ax] < lo[ax] ? row[ax] : lo[ax];
            hi[ax] = row[3 + ax] > hi[ax] ? row[3 + ax] : hi[ax];
        }
        amax = row[6] > amax ? row[6] : amax;
        ssq += row[7];
    }
#pragma unroll
    for (int ax = 0; ax < 3; ax++) { lo[ax] = wave_min(lo[ax]); hi[ax] = wave_max(hi[ax]); }
    amax = wave_max(amax);
    ssq = wave_sum(ssq);
    if (lane != 0) return;
    rh_extent *R = J.out + j;
    if (*J.flag != 0) { R->flags |= RH_EXT_INVALID; return; }
    if (R->n == 0) return;
    for (int ax = 0; ax < 3; ax++) { R->lo[ax] = lo[ax]; R->hi[ax] = hi[ax]; }
    R->dist_maxabs = amax;
    R->dist_rms = sqrt(ssq / (double)R->n);
}

template <typename T>
void launch_all(rh_cloud *c, const ext_job &J, const T *pts)
{
    const dim3 gc((unsigned)J.nchunks), gs((unsigned)J.b);
    hipLaunchKernelGGL((ext_moments_kernel<T>), gc, dim3(EXT_BLOCK), 0, c->stream, J, pts);
    hipLaunchKernelGGL((ext_frame_kernel<T>), gs, dim3(64), 0, c->stream, J, pts);
    hipLaunchKernelGGL((ext_box_kernel<T>), gc, dim3(EXT_BLOCK), 0, c->stream, J, pts);
    hipLaunchKernelGGL(ext_finish_kernel, gs, dim3(64), 0, c->stream, J);
}

// the four launches on the cloud's stream (the caller has joined the batches and checked the arguments)
int extents_enqueue(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const int64_t *d_off, const int64_t *d_idx, int64_t total,
                    rh_extent *d_out)
{
    const int64_t nchunks = total / EXT_CHUNK + b;
    if (nchunks > 0x7FFFFFFF) { rh_set_error("rh_shape_extents: %lld list entries are more than one call takes", (long long)total); return RH_E_INVALID; }
    if (!c->ext_flag) RH_TRY(c->ext_flag.alloc(16));
    if (nchunks > c->ext_part_rows) {
        c->ext_part_rows = 0;
        RH_TRY(c->ext_part.grow(c->stream, (int64_t)EXT_ROW * nchunks));
        c->ext_part_rows = nchunks;
    }
    RH_HIP(hipMemsetAsync(c->ext_flag, 0, sizeof(int32_t), c->stream));
    ext_job J;
    J.shapes = d_shapes; J.off = d_off; J.idx = d_idx; J.out = d_out;
    J.part = c->ext_part; J.flag = c->ext_flag;
    J.total = total; J.nchunks = nchunks; J.n = c->n; J.stride = c->n_pad; J.b = b;
    if (c->f32) launch_all<float>(c, J, c->full32);
    else launch_all<double>(c, J, c->full);
    RH_HIP(hipGetLastError());
    return RH_OK;
}

struct ext_run { const int64_t *src; int64_t at, count; };   // a stretch of list entries that is contiguous on the host

// the host entries: shapes + offsets through the pinned block, the lists straight from where they are, one wait
int extents_host(rh_cloud *c, const char *who, const rh_shape *shapes, size_t shape_stride, int32_t b, const int64_t *offsets,
                 const std::vector<ext_run> &runs, rh_extent *out)
{
    if (offsets[0] != 0) { rh_set_error("%s: offsets[0] = %lld, expected 0", who, (long long)offsets[0]); return RH_E_INVALID; }
    for (int32_t j = 0; j < b; j++)
        if (offsets[j + 1] < offsets[j]) { rh_set_error("%s: offsets decrease at shape %d", who, j); return RH_E_INVALID; }
    const int64_t total = offsets[b];
    const size_t o_shapes = 0, o_off = up16(sizeof(rh_shape) * (size_t)b), o_out = o_off + up16(sizeof(int64_t) * (size_t)(b + 1)),
                 o_idx = o_out + up16(sizeof(rh_extent) * (size_t)b), bytes = o_idx + sizeof(int64_t) * (size_t)total;
    if ((int64_t)bytes > c->ext_in.count()) RH_TRY(c->ext_in.grow(c->stream, (int64_t)bytes));
    RH_TRY(rh_ensure_pin(c, (int64_t)(o_idx + 16)));
    char *h = c->h_pin, *d = c->ext_in;
    for (int32_t j = 0; j < b; j++)
        memcpy(h + o_shapes + sizeof(rh_shape) * (size_t)j, (const char *)shapes + shape_stride * (size_t)j, sizeof(rh_shape));
    memcpy(h + o_off, offsets, sizeof(int64_t) * (size_t)(b + 1));
    RH_HIP(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, c->stream));
    for (const ext_run &r : runs)
        if (r.count > 0)
            RH_HIP(hipMemcpyAsync(d + o_idx + sizeof(int64_t) * (size_t)r.at, r.src, sizeof(int64_t) * (size_t)r.count, hipMemcpyHostToDevice, c->stream));
    RH_TRY(extents_enqueue(c, (const rh_shape *)(d + o_shapes), b, (const int64_t *)(d + o_off), (const int64_t *)(d + o_idx), total,
                           (rh_extent *)(d + o_out)));
    // records and error word come back behind the uploads' staging area (the stream has consumed it by then)
    RH_HIP(hipMemcpyAsync(h + o_out, d + o_out, sizeof(rh_extent) * (size_t)b, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipMemcpyAsync(h + o_idx, c->ext_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    int32_t flag;
    memcpy(&flag, h + o_idx, sizeof flag);
    if (flag != 0) {
        rh_set_error("%s: invalid input:%s%s%s%s%s", who, flag & EXT_BAD_OFFSETS ? " offsets" : "",
                     flag & EXT_BAD_INDEX ? " an index outside 1..N" : "", flag & EXT_BAD_COORD ? " a listed point with a non-finite coordinate" : "",
                     flag & EXT_BAD_AXIS ? " a shape whose axis has no finite, positive norm" : "", flag & EXT_BAD_KIND ? " an unknown shape kind" : "");
        return RH_E_INVALID;
    }
    memcpy(out, h + o_out, sizeof(rh_extent) * (size_t)b);
    return RH_OK;
}

}  // namespace

extern "C" int rh_shape_extents_dev(rh_cloud *c, const rh_shape *d_shapes, int32_t b, const int64_t *d_offsets,
                                    const int64_t *d_idx_1based, int64_t total, rh_extent *d_out)
{
    RH_TRY(rh_cloud_join(c));
    if (b < 0 || total < 0) { rh_set_error("rh_shape_extents_dev: b = %d, total = %lld", b, (long long)total); return RH_E_INVALID; }
    if (b == 0) return RH_OK;
    if (!d_shapes || !d_offsets || !d_out || (total > 0 && !d_idx_1based)) { rh_set_error("rh_shape_extents_dev: null argument"); return RH_E_INVALID; }
    return extents_enqueue(c, d_shapes, b, d_offsets, d_idx_1based, total, d_out);
}

extern "C" int rh_shape_extents(rh_cloud *c, const rh_shape *shapes, int32_t b, const int64_t *offsets, const int64_t *idx_1based,
                                rh_extent *out)
{
    RH_TRY(rh_cloud_join(c));
    if (b < 0) { rh_set_error("rh_shape_extents: b = %d", b); return RH_E_INVALID; }
    if (b == 0) return RH_OK;
    if (!shapes || !offsets || !out || (offsets[b] > 0 && !idx_1based)) { rh_set_error("rh_shape_extents: null argument"); return RH_E_INVALID; }
    const std::vector<ext_run> runs = { { idx_1based, 0, offsets[b] } };
    return extents_host(c, "rh_shape_extents", shapes, sizeof(rh_shape), b, offsets, runs, out);
}

extern "C" int rh_result_extents(rh_cloud *c, const rh_result *r, rh_extent *out)
{
    RH_TRY(rh_cloud_join(c));
    if (!r || r->n_shapes < 0 || r->n_shapes > 0x7FFFFFFF) { rh_set_error("rh_result_extents: bad result"); return RH_E_INVALID; }
    const int32_t b = (int32_t)r->n_shapes;
    if (b == 0) return RH_OK;
    if (!r->shapes || !out) { rh_set_error("rh_result_extents: null argument"); return RH_E_INVALID; }
    std::vector<int64_t> off((size_t)b + 1, 0);
    std::vector<ext_run> runs;   // the lists follow one another in the result's block: usually one run
    for (int32_t j = 0; j < b; j++) {
        const rh_extracted &x = r->shapes[j];
        if (x.n_inpoints < 0 || (x.n_inpoints > 0 && !x.inpoints)) { rh_set_error("rh_result_extents: bad list of shape %d", j); return RH_E_INVALID; }
        off[(size_t)j + 1] = off[(size_t)j] + x.n_inpoints;
        if (x.n_inpoints == 0) continue;
        if (!runs.empty() && runs.back().src + runs.back().count == x.inpoints) runs.back().count += x.n_inpoints;
        else runs.push_back({ x.inpoints, off[(size_t)j], x.n_inpoints });
    }
    return extents_host(c, "rh_result_extents", &r->shapes[0].shape, sizeof(rh_extracted), b, off.data(), runs, out);
}
