// score4_diag.hip -- the diag build's view of the v4 score path (score4.hip): the audits of the classifier's margins and
// decisions, the census of what the boxes and masks rule out, the host probes of single functions and the launch's event
// counters.  Everything here exists with -DRH_DIAG only (include/ransac_hip_diag.h); the product build compiles it to nothing.
#ifdef RH_DIAG
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "rh_internal.h"
#include "ransac_hip_diag.h"
#include "score_device.h"
#include "score4_device.h"
#include "score4_shared.h"
#include "wave_keys.h"

namespace {

using namespace rhdev;
using namespace rh4;

// ---- audit of the classifier's margins (tests): every (candidate, point) of a batch against subset 1.
// a32 / b32 are what the score kernel computes (the very same functions: ua, ub of score4_device.h); a64 / b64 the same scaled
// quantities from the reference's binary64 arithmetic.  |x32 - x64| has to stay below 1/2 for the classification to be sound; by
// construction (RH_CLS_SAFETY) it should stay below ~1/8.  out[kind * 2 + {0, 1}] = max over the batch of |a32 - a64|,
// |b32 - b64| (sphere / cylinder: only where the distance half is not far outside, ua64 < 2 -- the norm's error is relative
// to the norm); out[8 + kind] = pairs looked at.
struct S4AuditCand { rh_prep P; rh_cls C; double cNhi, wN, eDlo, wD, cosa, eps; int kind, usable; };   // (cNhi .. wD: cls_make's dbg4)

__global__ void __launch_bounds__(256)
cls_audit_kernel(const double *__restrict__ pts, int64_t stride, int64_t s, const S4AuditCand *__restrict__ cands, int ncand,
                 unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (c >= ncand) return;
    const S4AuditCand &Q = cands[c];
    double ea = 0.0, eb = 0.0;
    bool counted = false;
    if (i < s && Q.usable) {
        const double x = pts[i], y = pts[stride + i], z = pts[2 * stride + i];
        const double nx = pts[3 * stride + i], ny = pts[4 * stride + i], nz = pts[5 * stride + i];
        const rh_prep &P = Q.P;
        float a32, b32;
        double a64, b64;
        if (Q.kind == RH_PLANE) {
            cls_plane_ab(Q.C, (float)x, (float)y, (float)z, (float)nx, (float)ny, (float)nz, a32, b32);
            const double dn = (P.f[3] * nx + P.f[4] * ny) + P.f[5] * nz;
            const double d = (P.f[6] * (x - P.f[0]) + P.f[7] * (y - P.f[1])) + P.f[8] * (z - P.f[2]);
            a64 = (Q.cNhi - dn) / Q.wN;
            b64 = (fabs(d) - Q.eDlo) / Q.wD;
            ea = fabs((double)a32 - a64);
            eb = fabs((double)b32 - b64);
            counted = true;
        } else if (Q.kind == RH_SPHERE || Q.kind == RH_CYLINDER) {
            double qx, qy, qz, R, sgn;
            if (Q.kind == RH_SPHERE) {
                cls_round_ab<RH_SPHERE>(Q.C, (float)x, (float)y, (float)z, (float)nx, (float)ny, (float)nz, a32, b32);
                qx = x - P.f[0]; qy = y - P.f[1]; qz = z - P.f[2]; R = P.f[3]; sgn = P.f[4];
            } else {
                cls_round_ab<RH_CYLINDER>(Q.C, (float)x, (float)y, (float)z, (float)nx, (float)ny, (float)nz, a32, b32);
                const double tx = x - P.f[3], ty = y - P.f[4], tz = z - P.f[5];
                const double sd = (P.f[0] * tx + P.f[1] * ty) + P.f[2] * tz;
                qx = (x - P.f[0] * sd) - P.f[3]; qy = (y - P.f[1] * sd) - P.f[4]; qz = (z - P.f[2] * sd) - P.f[5];
                R = P.f[6]; sgn = P.f[7];
            }
            // the squared form (score4_device.h, "Round kinds without a square root"): dbg4 = m2, W2, mv, Wv
            const double m2 = Q.cNhi, W2 = Q.wN, mv = Q.eDlo, Wv = Q.wD;
            const double n2 = (qx * qx + qy * qy) + qz * qz;
            const double qn = (qx * nx + qy * ny) + qz * nz;
            a64 = (fabs(n2 - (R * R + Q.eps * Q.eps)) - (2.0 * R * Q.eps - m2)) / W2;
            b64 = (mv + (Q.cosa * Q.cosa * n2 - sgn * qn * fabs(qn))) / Wv;
            // the error of n2 is relative (3 u n2): far outside the band it exceeds any fixed margin and cannot matter
            // (ua is a few thousand widths above 1 there); what has to hold is the bound NEAR the band
            if (a64 < 2.0) { ea = fabs((double)a32 - a64); eb = fabs((double)b32 - b64); }
            counted = true;
        } else if (Q.kind == RH_CONE) {
            // a64 / b64 from the reference's own frame (cone_frame: its dist and its normal cosine), the closed form only
            // supplies rho for the multiplied-through angle test; points the classifier hands to the exact test because
            // they lie next to the axis are not looked at
            bool near_axis;
            cls_cone_ab(Q.C, (float)x, (float)y, (float)z, (float)nx, (float)ny, (float)nz, a32, b32, near_axis);
            if (!near_axis) {
                double dist, dt;
                cone_frame(P, x, y, z, nx, ny, nz, dist, dt);
                const double an = sqrt((P.f[3] * P.f[3] + P.f[4] * P.f[4]) + P.f[5] * P.f[5]);
                const double wx = x - P.f[0], wy = y - P.f[1], wz = z - P.f[2];
                const double h = ((P.f[3] * wx + P.f[4] * wy) + P.f[5] * wz) / an;
                const double qx = wx - h * (P.f[3] / an), qy = wy - h * (P.f[4] / an), qz = wz - h * (P.f[5] / an);
                const double rho = sqrt((qx * qx + qy * qy) + qz * qz);
                a64 = (fabs(dist) - Q.eDlo) / Q.wD;
                b64 = 0.5 - rho * (P.f[8] * dt - Q.cosa) / Q.wN;
                ea = fabs((double)a32 - a64);
                eb = fabs((double)b32 - b64);
                counted = true;
            }
        }
        if (!(ea == ea)) ea = 1e30;   // a NaN on one side only is a failure
        if (!(eb == eb)) eb = 1e30;
    }
    // block maximum, then one atomic per block (non-negative doubles order like their bit patterns)
    __shared__ unsigned long long sa[4], sb[4];
    __shared__ int sc[4];
    unsigned long long ua = __builtin_bit_cast(unsigned long long, ea), ub = __builtin_bit_cast(unsigned long long, eb);
    int cnt = counted ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long va = __shfl_down(ua, off), vb = __shfl_down(ub, off);
        ua = va > ua ? va : ua;
        ub = vb > ub ? vb : ub;
        cnt += __shfl_down(cnt, off);
    }
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = ua; sb[threadIdx.x >> 6] = ub; sc[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0 && Q.kind >= 0 && Q.kind < 4) {
        unsigned long long ma = 0, mb = 0;
        int n = 0;
        for (int w = 0; w < 4; w++) { ma = sa[w] > ma ? sa[w] : ma; mb = sb[w] > mb ? sb[w] : mb; n += sc[w]; }
        atomicMax(&out[Q.kind * 2], ma);
        atomicMax(&out[Q.kind * 2 + 1], mb);
        atomicAdd(&out[8 + Q.kind], (unsigned long long)n);
    }
}

// ---- audit of the DECISIONS (tests, tools/fuzz_score.py): what the margin audit above argues, counted.  One wave per
// (candidate, 64-point group of subset 1), lane = point, with the very records (cls_make) and functions (box_skip32,
// cls_*_t) the score kernel uses, against the exact test of the cloud's element type:
//   out[kind * 10 + 0] pairs, 1 pairs the box test skips, 2 VIOLATION: skipped pairs with an exact inlier,
//   3 points, 4 classified surely-in, 5 surely-out, 6 VIOLATION: surely-in but the exact test rejects,
//   7 VIOLATION: surely-out but the exact test accepts, 8 exact inliers, 9 VIOLATION: the all-zero point a disabled point
//   is staged as comes out surely-in (plane / sphere / cylinder count what the classifier says without looking at the
//   enabled bits; the cone masks them).
struct S4SoundCand { rh_prep P; rh_prepf Pf; rh_cls C; float box[RH_BOX_FIELDS]; int kind; int pad; };
struct S4SoundArgs { double eps[4], cosa[4]; int f32; };

template <int KIND>
static __device__ __forceinline__ void sound_one(const S4SoundCand &Q, const S4SoundArgs &A, double x, double y, double z, double nx, double ny,
                                                 double nz, const uint64_t valid, const rh_box32 &G, const rh_box32 &GS, const rh_box32 &GT, const rh_u32x4 gm, const rh_u32x4 sm, const int lane, unsigned long long *__restrict__ out)
{
    const double eps = A.eps[KIND], cosa = A.cosa[KIND];
    uint64_t ex;
    if (A.f32) ex = test_point<KIND>(Q.Pf, (float)x, (float)y, (float)z, (float)nx, (float)ny, (float)nz, eps, cosa);
    else ex = test_point<KIND>(Q.P, x, y, z, nx, ny, nz, eps, cosa);
    ex &= valid;
    const bool skip = box_skip32<KIND>(Q.box, G);
    const bool stskip = box_skip32<KIND>(Q.box, GS);   // the super-tile's box (st_cull_kernel): out[48 + k] such pairs, out[52 + k] VIOLATION: with an exact inlier
    const bool tlskip = box_skip32<KIND>(Q.box, GT);   // the tile's box (the lists the score launch walks): out[56 + k] such pairs, out[60 + k] VIOLATION: with an exact inlier
    const bool exact_only = is_nan_bits(Q.C.f[RH_CLS_FLAG]);
    const float fx = (float)x, fy = (float)y, fz = (float)z, fnx = (float)nx, fny = (float)ny, fnz = (float)nz;
    float t, t0;   // (the u of score4_device.h: sign bit = surely in, 0 <= u <= 1 undecided)
    if (KIND == RH_PLANE) { t = cls_plane_u(Q.C, fx, fy, fz, fnx, fny, fnz); t0 = cls_plane_u(Q.C, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f); }
    else if (KIND == RH_CONE) { t = cls_cone_u(Q.C, fx, fy, fz, fnx, fny, fnz); t0 = 0.5f; }
    else { t = cls_round_u<KIND == RH_SPHERE ? RH_SPHERE : RH_CYLINDER>(Q.C, fx, fy, fz, fnx, fny, fnz);
           t0 = cls_round_u<KIND == RH_SPHERE ? RH_SPHERE : RH_CYLINDER>(Q.C, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f); }
    const float sum = (fabsf(fx) + fabsf(fy)) + (fabsf(fz) + fabsf(fnx)) + (fabsf(fny) + fabsf(fnz));
    const bool weird = WB(!(sum < __builtin_inff()) && ((valid >> lane) & 1ULL)) != 0;   // the kernel: every candidate exact-only on this tile
    const bool decided = !exact_only && !weird;
    // (the cone's per-point undecided bit is the sign of u - 1, not-surely-in: u = 1 exactly counts as surely out there)
    const uint64_t sin_ = WB(decided && cls_sure(t)) & valid;
    const uint64_t amb = (WB(!decided || (KIND == RH_CONE ? (!cls_sure(t) && cls_sure(t - 1.0f)) : cls_undecided(t)))) & valid;
    const uint64_t sout = valid & ~sin_ & ~amb;
    // a "band point": its DISTANCE half alone is not surely failed (the normal half aside) -- a pair whose group holds one
    // cannot be decided by any test on the group's position box: the floor of the necessary (candidate, group) work
    float du, dn;
    bool near_axis = false;
    if (KIND == RH_PLANE) cls_plane_ab(Q.C, fx, fy, fz, fnx, fny, fnz, dn, du);
    else if (KIND == RH_CONE) cls_cone_ab(Q.C, fx, fy, fz, fnx, fny, fnz, du, dn, near_axis);
    else cls_round_ab<KIND == RH_SPHERE ? RH_SPHERE : RH_CYLINDER>(Q.C, fx, fy, fz, fnx, fny, fnz, du, dn);
    const uint64_t band = WB(!decided || near_axis || !(du > 1.0f)) & valid;
    if (lane == 0) {
        if (band != 0) atomicAdd(&out[40 + KIND], 1ULL);
        if (ex != 0) atomicAdd(&out[44 + KIND], 1ULL);
        if (stskip) atomicAdd(&out[48 + KIND], 1ULL);
        if (stskip && ex != 0) atomicAdd(&out[52 + KIND], 1ULL);
        if (tlskip) atomicAdd(&out[56 + KIND], 1ULL);
        if (tlskip && ex != 0) atomicAdd(&out[60 + KIND], 1ULL);
        if (KIND == RH_PLANE) {
            // the normal-cell masks (planes): out[64] pairs the GROUP's mask rules out, out[65] VIOLATION: such a pair with an exact
            // inlier, out[66] / out[67] the same for the SUPER-TILE's mask (the list launch)
            const bool gskip = !nsig_meet(Q.box, gm), sskip = !nsig_meet(Q.box, sm);
            if (gskip) atomicAdd(&out[64], 1ULL);
            if (gskip && ex != 0) atomicAdd(&out[65], 1ULL);
            if (sskip) atomicAdd(&out[66], 1ULL);
            if (sskip && ex != 0) atomicAdd(&out[67], 1ULL);
        }
        unsigned long long *o = out + KIND * 10;
        atomicAdd(&o[0], 1ULL);
        if (skip) atomicAdd(&o[1], 1ULL);
        if (skip && ex != 0) atomicAdd(&o[2], 1ULL);
        atomicAdd(&o[3], (unsigned long long)__popcll(valid));
        if (sin_) atomicAdd(&o[4], (unsigned long long)__popcll(sin_));
        if (sout) atomicAdd(&o[5], (unsigned long long)__popcll(sout));
        if (sin_ & ~ex) atomicAdd(&o[6], (unsigned long long)__popcll(sin_ & ~ex));
        if (sout & ex) atomicAdd(&o[7], (unsigned long long)__popcll(sout & ex));
        if (ex) atomicAdd(&o[8], (unsigned long long)__popcll(ex));
        if (blockIdx.x == 0 && !exact_only && cls_sure(t0)) atomicAdd(&o[9], 1ULL);
    }
}

__global__ void __launch_bounds__(64)
cls_sound_kernel(const double *__restrict__ pts, int64_t stride, int64_t s, const float *__restrict__ gb32, const float *__restrict__ st32, const float *__restrict__ tile32, const uint32_t *__restrict__ gm32, const uint32_t *__restrict__ stm32, const S4SoundCand *__restrict__ cands,
                 int ncand, const S4SoundArgs A, const int kinds, unsigned long long *__restrict__ out)   // kinds: bit k = candidates of kind k count
{
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t i = g * 64 + lane;
    const uint64_t valid = valid_mask(g * 64, s);
    const bool on = (valid >> lane) & 1ULL;
    const double x = on ? pts[i] : 0.0, y = on ? pts[stride + i] : 0.0, z = on ? pts[2 * stride + i] : 0.0;
    const double nx = on ? pts[3 * stride + i] : 0.0, ny = on ? pts[4 * stride + i] : 0.0, nz = on ? pts[5 * stride + i] : 0.0;
    rh_box32 G;
    G.cx = gb32[g * 8 + 0]; G.cy = gb32[g * 8 + 1]; G.cz = gb32[g * 8 + 2]; G.hx = gb32[g * 8 + 3];
    G.hy = gb32[g * 8 + 4]; G.hz = gb32[g * 8 + 5]; G.hr = gb32[g * 8 + 6];
    rh_box32 GS;
    {
        const float *b = st32 + (g / S4_STG) * 8;
        GS.cx = b[0]; GS.cy = b[1]; GS.cz = b[2]; GS.hx = b[3]; GS.hy = b[4]; GS.hz = b[5]; GS.hr = b[6];
    }
    rh_box32 GT;
    {
        const float *b = tile32 + (g / S4_TG) * 8;
        GT.cx = b[0]; GT.cy = b[1]; GT.cz = b[2]; GT.hx = b[3]; GT.hy = b[4]; GT.hz = b[5]; GT.hr = b[6];
    }
    const rh_u32x4 gm = ((const rh_u32x4 *)gm32)[g], sm = ((const rh_u32x4 *)stm32)[g / S4_STG];
    for (int c = blockIdx.y; c < ncand; c += gridDim.y) {
        const S4SoundCand &Q = cands[c];
        if (Q.kind < 0 || Q.kind > 3 || !((kinds >> Q.kind) & 1)) continue;
        switch (Q.kind) {
        case RH_PLANE: sound_one<RH_PLANE>(Q, A, x, y, z, nx, ny, nz, valid, G, GS, GT, gm, sm, lane, out); break;
        case RH_SPHERE: sound_one<RH_SPHERE>(Q, A, x, y, z, nx, ny, nz, valid, G, GS, GT, gm, sm, lane, out); break;
        case RH_CYLINDER: sound_one<RH_CYLINDER>(Q, A, x, y, z, nx, ny, nz, valid, G, GS, GT, gm, sm, lane, out); break;
        case RH_CONE: sound_one<RH_CONE>(Q, A, x, y, z, nx, ny, nz, valid, G, GS, GT, gm, sm, lane, out); break;
        default: break;
        }
    }
}

// ---- the cone's classifier on points of the caller's choice (rh_dbg_cls_cone): cls_cone_ab is device code -- its rho goes
// through the hardware's reciprocal root --, so what it says of a point can only be asked here.  pts: 6 rows of n binary32
// values (x y z nx ny nz), converted on the host the way the staging converts them.
__global__ void __launch_bounds__(256)
cls_cone_dbg_kernel(const rh_cls C, const float *__restrict__ pts, int64_t n, float *__restrict__ ua, float *__restrict__ ub,
                    uint8_t *__restrict__ near_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a, b;
    bool near_axis;
    cls_cone_ab(C, pts[i], pts[n + i], pts[2 * n + i], pts[3 * n + i], pts[4 * n + i], pts[5 * n + i], a, b, near_axis);
    ua[i] = a;
    ub[i] = b;
    near_out[i] = near_axis ? 1 : 0;
}

// ---- the shared steps of the per-shape host probes (rh_dbg_nsig, _cylbox, _cls_round, _cls_u2, _conebox, _cls_cone)
// the candidate as the host builds it -- cls_make on rh_prep_host's record: what the staged path uploads
struct Probe {
    rh_prep P;
    rh_cls C;
    float box[RH_BOX_FIELDS];
    double d4[4];
};

// Q for a shape of one of `kinds` (bit k = kind k; any other: "<who>: <only> only"); rec_out[16], fields_out[RH_BOX_FIELDS] and
// dbg4_out[4] take the classifier record, the culling record and cls_make's dbg4 where they are not null
int probe_make(const char *who, const char *only, int kinds, const rh_shape *shape, const rh_params *p, double M, double Nm, double Ln, int f32,
               Probe &Q, float *rec_out = nullptr, float *fields_out = nullptr, double *dbg4_out = nullptr)
{
    const int kind = shape->kind;
    if (kind < 0 || kind > 3 || !((kinds >> kind) & 1)) { rh_set_error("%s: %s only", who, only); return RH_E_INVALID; }
    rh_prep_host(*shape, &Q.P);
    for (int k = 0; k < 4; k++) Q.d4[k] = 0;
    cls_make(Q.P, kind, p->eps[kind], p->cos_alpha[kind], M, Nm, Q.C, Q.box, 1, Q.d4, f32 != 0, Ln);
    if (rec_out != nullptr)
        for (int k = 0; k < 16; k++) rec_out[k] = Q.C.f[k];
    if (fields_out != nullptr)
        for (int k = 0; k < RH_BOX_FIELDS; k++) fields_out[k] = Q.box[k];
    if (dbg4_out != nullptr)
        for (int k = 0; k < 4; k++) dbg4_out[k] = Q.d4[k];
    return RH_OK;
}

// a binary64 box (centre, half extents: b[0 .. 5]) converted by box_to_f32 like a group's
rh_box32 probe_box(const double *b)
{
    float o[8];
    box_to_f32(b, b + 3, o);
    rh_box32 G;
    G.cx = o[0]; G.cy = o[1]; G.cz = o[2]; G.hx = o[3]; G.hy = o[4]; G.hz = o[5]; G.hr = o[6];
    return G;
}

// point i and its normal as the staging converts them: q = x y z nx ny nz
void probe_point(const double *xyz, const double *nrm, int64_t i, float q[6])
{
    for (int k = 0; k < 3; k++) { q[k] = (float)xyz[3 * i + k]; q[3 + k] = (float)nrm[3 * i + k]; }
}

}  // namespace

// diagnostics (tests): the classifier's worst binary32 error on a batch, in units of its margin widths (see
// cls_audit_kernel); out[12]: per kind (plane, sphere, cylinder, -) the two maxima, then the numbers of pairs
extern "C" int rh_dbg_cls_audit(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, double *out)
{
    if (c == nullptr || out == nullptr || p == nullptr || b < 0 || (b > 0 && shapes == nullptr)) { rh_set_error("rh_dbg_cls_audit: bad arguments"); return RH_E_INVALID; }
    for (int i = 0; i < 12; i++) out[i] = 0.0;
    if (b == 0 || c->s == 0) return RH_OK;
    RH_HIP(hipSetDevice(c->device));
    std::vector<S4AuditCand> h((size_t)b);
    for (int32_t i = 0; i < b; i++) {
        S4AuditCand &Q = h[(size_t)i];
        Q.kind = shapes[i].kind;
        Q.usable = 0;
        if (Q.kind < 0 || Q.kind > 3) continue;
        rh_prep_host(shapes[i], &Q.P);
        double d4[4] = { 0, 0, 0, 0 };
        cls_make(Q.P, Q.kind, p->eps[Q.kind], p->cos_alpha[Q.kind], c->coord_mag, c->nrm_mag, Q.C, nullptr, 0, d4, c->f32);
        Q.cNhi = d4[0]; Q.wN = d4[1]; Q.eDlo = d4[2]; Q.wD = d4[3]; Q.cosa = p->cos_alpha[Q.kind]; Q.eps = p->eps[Q.kind];
        Q.usable = !(Q.C.f[RH_CLS_FLAG] != Q.C.f[RH_CLS_FLAG]) && Q.wN > 0 && Q.wD > 0;
    }
    rh_dev<S4AuditCand> d_c;
    rh_dev<unsigned long long> d_o;
    RH_TRY(d_c.alloc(b));
    RH_TRY(d_o.alloc(12));
    RH_HIP(hipMemcpyAsync(d_c, h.data(), sizeof(S4AuditCand) * (size_t)b, hipMemcpyHostToDevice, c->stream));
    RH_HIP(hipMemsetAsync(d_o, 0, sizeof(unsigned long long) * 12, c->stream));
    for (int32_t c0 = 0; c0 < b; c0 += 32768) {
        const int32_t nb = std::min<int32_t>(32768, b - c0);
        hipLaunchKernelGGL(cls_audit_kernel, dim3((unsigned)cdiv4(c->s, 256), (unsigned)nb), dim3(256), 0, c->stream, c->sub, c->s_pad,
                           c->s, d_c + c0, nb, d_o);
    }
    unsigned long long ho[12];
    RH_HIP(hipMemcpyAsync(ho, d_o, sizeof ho, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; i++) out[i] = __builtin_bit_cast(double, ho[i]);
    for (int i = 8; i < 12; i++) out[i] = (double)ho[i];
    return RH_OK;
}

// diagnostics (tests, tools/fuzz_score.py): the decisions of the box test and of the classifier against the exact test
// on every (candidate, point) of a batch x subset 1 (all points taken as enabled): 72 counters, layout at sound_one.
// rh_dbg_cls_soundness hands out the first 56 (its callers' buffers hold that many), rh_dbg_cls_soundness_tiles the 8 of the
// tile level, rh_dbg_cls_soundness_nsig the 4 of the normal-cell masks.
static int cls_soundness_run(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out, const int first, const int nout)
{
    if (c == nullptr || out == nullptr || p == nullptr || b < 0 || (b > 0 && shapes == nullptr)) { rh_set_error("rh_dbg_cls_soundness: bad arguments"); return RH_E_INVALID; }
    for (int i = 0; i < nout; i++) out[i] = 0;
    if (b == 0 || c->s == 0 || c->ngroups == 0 || c->gb32 == nullptr || c->st32 == nullptr || c->tile32 == nullptr || c->gm32 == nullptr || c->stm32 == nullptr) return RH_OK;
    RH_HIP(hipSetDevice(c->device));
    std::vector<S4SoundCand> h((size_t)b);
    for (int32_t i = 0; i < b; i++) {
        S4SoundCand &Q = h[(size_t)i];
        Q.kind = shapes[i].kind;
        Q.pad = 0;
        if (Q.kind < 0 || Q.kind > 3) { Q.kind = -1; continue; }
        rh_prep_host(shapes[i], &Q.P);
        Q.Pf = prepf_of_kind(Q.P, Q.kind);
        cls_make(Q.P, Q.kind, p->eps[Q.kind], p->cos_alpha[Q.kind], c->coord_mag, c->nrm_mag, Q.C, Q.box, 1, nullptr, c->f32, c->nrm_len);
    }
    S4SoundArgs A;
    for (int k = 0; k < 4; k++) { A.eps[k] = p->eps[k]; A.cosa[k] = p->cos_alpha[k]; }
    A.f32 = c->f32 ? 1 : 0;
    rh_dev<S4SoundCand> d_c;
    rh_dev<unsigned long long> d_o;
    RH_TRY(d_c.alloc(b));
    RH_TRY(d_o.alloc(72));
    RH_HIP(hipMemcpyAsync(d_c, h.data(), sizeof(S4SoundCand) * (size_t)b, hipMemcpyHostToDevice, c->stream));
    RH_HIP(hipMemsetAsync(d_o, 0, sizeof(unsigned long long) * 72, c->stream));
    // The census describes what the score kernel walks: with the plane order in use ("plane_order"), the plane candidates meet
    // the plane-order groups -- their points, boxes and masks, those of the plane order's super-tiles, and the boxes of runs of
    // S4_TG of them, made here -- and the other kinds the leaf order's.
    const bool pl = rhk_plane_order_wanted(c);
    const dim3 grid((unsigned)c->ngroups, (unsigned)std::min<int32_t>(b, 64));
    hipLaunchKernelGGL(cls_sound_kernel, grid, dim3(64), 0, c->stream, c->sub, c->s_pad, c->s, c->gb32, c->st32, c->tile32, c->gm32, c->stm32, d_c, b, A,
                       pl ? 0xe : 0xf, d_o);
    rh_dev<double> pl_gb;
    rh_dev<float> pl_tile32;
    if (pl) {
        RH_TRY(pl_gb.alloc(7 * c->ng_pad));
        RH_TRY(pl_tile32.alloc(8 * std::max<int64_t>(1, c->ntile)));
        RH_HIP(hipMemsetAsync(pl_gb, 0, sizeof(double) * 7 * (size_t)c->ng_pad, c->stream));
        RH_TRY(rhk_group_bounds_of(c, c->pl_sub, c->s_pad, c->s, c->ngroups, pl_gb, c->ng_pad));
        rhk_runs32_of(c, pl_gb, S4_TG, c->ntile, pl_tile32);
        hipLaunchKernelGGL(cls_sound_kernel, grid, dim3(64), 0, c->stream, c->pl_sub, c->s_pad, c->s, c->pl_gb32, c->pl_st32, pl_tile32, c->pl_gm32, c->pl_stm32, d_c,
                           b, A, 0x1, d_o);
    }
    RH_HIP(hipGetLastError());
    unsigned long long ho[72];
    RH_HIP(hipMemcpyAsync(ho, d_o, sizeof ho, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < nout; i++) out[i] = (uint64_t)ho[first + i];
    return RH_OK;
}

extern "C" int rh_dbg_cls_soundness(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out)
{
    return cls_soundness_run(c, shapes, b, p, out, 0, 56);
}

// the tile level of the same census: out[k] = pairs (candidate, group) whose TILE's box rules the candidate out -- the pairs the
// tile lists keep from the score launch --, out[4 + k] = VIOLATION: such a pair with an exact inlier
extern "C" int rh_dbg_cls_soundness_tiles(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out)
{
    return cls_soundness_run(c, shapes, b, p, out, 56, 8);
}

// the normal-cell masks in the same census (planes): out[0] = pairs (candidate, group) the group's mask rules out, out[1] =
// VIOLATION: such a pair with an exact inlier, out[2] / out[3] = the same for the super-tile's mask
extern "C" int rh_dbg_cls_soundness_nsig(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out)
{
    return cls_soundness_run(c, shapes, b, p, out, 64, 4);
}

// the candidate mask as the host builds it (probe_make), and the cell function on `ndirs` directions (-1: a zero or NaN vector,
// -2: an infinite component).  Host only: needs no GPU.
extern "C" int rh_dbg_nsig(const rh_shape *shape, const rh_params *p, double M, double Nm, double Ln, int f32, uint32_t *mask_out,
                           const double *dirs, int64_t ndirs, int32_t *cells_out)
{
    if (p == nullptr || ndirs < 0 || (ndirs > 0 && (dirs == nullptr || cells_out == nullptr)) || (shape != nullptr && mask_out == nullptr)) {
        rh_set_error("rh_dbg_nsig: bad arguments");
        return RH_E_INVALID;
    }
    if (shape != nullptr) {
        Probe Q;
        RH_TRY(probe_make("rh_dbg_nsig", "planes", 1 << RH_PLANE, shape, p, M, Nm, Ln, f32, Q));
        for (int k = 0; k < 3; k++) mask_out[k] = __builtin_bit_cast(uint32_t, Q.box[5 + k]);
    }
    for (int64_t i = 0; i < ndirs; i++) {
        uint32_t w[3];
        nsig_point_bits(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], w);
        if ((w[0] & w[1] & w[2]) == 0xffffffffu) cells_out[i] = -2;
        else if ((w[0] | w[1] | w[2]) == 0u) cells_out[i] = -1;
        else cells_out[i] = nsig_cell(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    }
    return RH_OK;
}

// the binary64 boxes of the 64-point groups of subset 1, in group order: out[6 g ..] = centre, half extents; *ngroups_out: how
// many there are (out = null or cap too small: only the number)
extern "C" int rh_dbg_group_boxes(rh_cloud *c, double *out, int64_t cap, int64_t *ngroups_out)
{
    if (c == nullptr || ngroups_out == nullptr || cap < 0) { rh_set_error("rh_dbg_group_boxes: bad arguments"); return RH_E_INVALID; }
    *ngroups_out = c->gb == nullptr ? 0 : c->ngroups;
    if (out == nullptr || cap < *ngroups_out || *ngroups_out == 0) return RH_OK;
    RH_HIP(hipSetDevice(c->device));
    std::vector<double> h((size_t)c->ngroups * 6);
    const double *gb = c->gb;
    for (int k = 0; k < 6; k++)
        RH_HIP(hipMemcpyAsync(h.data() + (size_t)k * c->ngroups, gb + (int64_t)k * c->ng_pad, sizeof(double) * (size_t)c->ngroups, hipMemcpyDeviceToHost, c->stream));
    RH_HIP(hipStreamSynchronize(c->stream));
    for (int64_t g = 0; g < c->ngroups; g++)
        for (int k = 0; k < 6; k++) out[6 * g + k] = h[(size_t)k * c->ngroups + g];
    return RH_OK;
}

// the cylinder's box test as the host runs it: the culling record cls_make builds for the shape (fields_out[RH_BOX_FIELDS]), and
// for each of the n binary64 boxes (centre, half extents: boxes[6 i ..]), converted by box_to_f32 like a group's, the decision
// of the kernel's own function (skip_out) and of its two ball clauses alone (ball_out).  Host only: needs no GPU.
extern "C" int rh_dbg_cylbox(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, const double *boxes, int64_t n,
                             uint8_t *skip_out, uint8_t *ball_out, float *fields_out)
{
    if (shape == nullptr || p == nullptr || n < 0 || (n > 0 && (boxes == nullptr || skip_out == nullptr || ball_out == nullptr))) {
        rh_set_error("rh_dbg_cylbox: bad arguments");
        return RH_E_INVALID;
    }
    Probe Q;
    RH_TRY(probe_make("rh_dbg_cylbox", "cylinders", 1 << RH_CYLINDER, shape, p, M, Nm, 0.0, f32, Q, nullptr, fields_out));
    for (int64_t i = 0; i < n; i++) {
        const rh_box32 G = probe_box(boxes + 6 * i);
        skip_out[i] = cyl_box_skip32<true>(Q.box, G) ? 1 : 0;
        ball_out[i] = cyl_box_skip32<false>(Q.box, G) ? 1 : 0;
    }
    return RH_OK;
}

// the classifier of a round candidate as the host runs it: the record cls_make builds for the shape, its margins (dbg4: m2, W2,
// mv, Wv) and the kernel's own cls_round_ab on n points.  Host only: needs no GPU.
extern "C" int rh_dbg_cls_round(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                                const double *nrm, float *ua_out, float *ub_out, float *rec_out, double *dbg4_out)
{
    if (shape == nullptr || p == nullptr || n < 0 || (n > 0 && (xyz == nullptr || nrm == nullptr || ua_out == nullptr || ub_out == nullptr))) {
        rh_set_error("rh_dbg_cls_round: bad arguments");
        return RH_E_INVALID;
    }
    Probe Q;
    RH_TRY(probe_make("rh_dbg_cls_round", "spheres and cylinders", (1 << RH_SPHERE) | (1 << RH_CYLINDER), shape, p, M, Nm, 0.0, f32, Q, rec_out, nullptr, dbg4_out));
    for (int64_t i = 0; i < n; i++) {
        float q[6];
        probe_point(xyz, nrm, i, q);
        if (shape->kind == RH_SPHERE) cls_round_ab<RH_SPHERE>(Q.C, q[0], q[1], q[2], q[3], q[4], q[5], ua_out[i], ub_out[i]);
        else cls_round_ab<RH_CYLINDER>(Q.C, q[0], q[1], q[2], q[3], q[4], q[5], ua_out[i], ub_out[i]);
    }
    return RH_OK;
}

// the two-bit books of the score kernel's point loops as the host runs them (score4_device.h, "Two-bit books": books2_push and
// the four read-outs, the very statements of score4_batch): nseq sequences of 64 values u' each, pushed in point order.  Host
// only: needs no GPU.
extern "C" int rh_dbg_books2(const float *u2, int64_t nseq, int32_t *sure_count_out, uint64_t *sure_word_out, uint64_t *und_word_out,
                             uint8_t *any_und_out)
{
    if (nseq < 0 || (nseq > 0 && (u2 == nullptr || sure_count_out == nullptr || sure_word_out == nullptr || und_word_out == nullptr || any_und_out == nullptr))) {
        rh_set_error("rh_dbg_books2: bad arguments");
        return RH_E_INVALID;
    }
    for (int64_t s = 0; s < nseq; s++) {
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
        for (int q = 0; q < 4; q++)
            for (int j = 0; j < 16; j++) w[q] = books2_push(w[q], u2[64 * s + 16 * q + j]);
        sure_count_out[s] = books2_sure_count(w);
        sure_word_out[s] = books2_sure64(w);
        und_word_out[s] = books2_und64(w);
        any_und_out[s] = books2_any_undecided(w) ? 1 : 0;
    }
    return RH_OK;
}

// the undecided word of the counts-only launches as the host runs it (score4_device.h, "Books in place"): per sequence of 64
// values u' the packed word in the books' own bit order; pi_out[L] = the point that bit L stands for; and, for point-ordered
// words (may be null), what books2_deposit64 makes of them -- the form the pairs that ignore their books queue.  Host only.
extern "C" int rh_dbg_books2_inplace(const float *u2, int64_t nseq, uint64_t *packed_out, int32_t *pi_out, const uint64_t *point_words,
                                     uint64_t *deposit_out)
{
    if (nseq < 0 || pi_out == nullptr || (nseq > 0 && (u2 == nullptr || packed_out == nullptr)) || ((point_words == nullptr) != (deposit_out == nullptr))) {
        rh_set_error("rh_dbg_books2_inplace: bad arguments");
        return RH_E_INVALID;
    }
    for (int L = 0; L < 64; L++) pi_out[L] = books2_point_of_bit(L);
    for (int64_t s = 0; s < nseq; s++) {
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
        for (int q = 0; q < 4; q++)
            for (int j = 0; j < 16; j++) w[q] = books2_push(w[q], u2[64 * s + 16 * q + j]);
        packed_out[s] = books2_und64_inplace(w);
        if (point_words != nullptr) deposit_out[s] = books2_deposit64(point_words[s]);
    }
    return RH_OK;
}

// u and u' of a plane, sphere or cylinder candidate on n points, on the host: u = max(ua, ub) by the functions every other caller
// uses on the record cls_make builds, u' by the point loops' own path -- that record doubled by cls_double, then cls_u2.  Host
// only: needs no GPU.
extern "C" int rh_dbg_cls_u2(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                             const double *nrm, float *u_out, float *u2_out, float *rec_out)
{
    if (shape == nullptr || p == nullptr || n < 0 || (n > 0 && (xyz == nullptr || nrm == nullptr || u_out == nullptr || u2_out == nullptr))) {
        rh_set_error("rh_dbg_cls_u2: bad arguments");
        return RH_E_INVALID;
    }
    Probe Q;
    RH_TRY(probe_make("rh_dbg_cls_u2", "planes, spheres and cylinders", (1 << RH_PLANE) | (1 << RH_SPHERE) | (1 << RH_CYLINDER), shape, p, M, Nm, 0.0, f32, Q, rec_out));
    const int kind = shape->kind;
    const rh_cls &C = Q.C;
    rh_cls D = C;
    if (kind == RH_PLANE) cls_double<RH_PLANE>(D);
    else if (kind == RH_SPHERE) cls_double<RH_SPHERE>(D);
    else cls_double<RH_CYLINDER>(D);
    for (int64_t i = 0; i < n; i++) {
        float q[6];
        probe_point(xyz, nrm, i, q);
        const float x = q[0], y = q[1], z = q[2], nx = q[3], ny = q[4], nz = q[5];
        if (kind == RH_PLANE) { u_out[i] = cls_plane_u(C, x, y, z, nx, ny, nz); u2_out[i] = cls_u2<RH_PLANE>(D, x, y, z, nx, ny, nz); }
        else if (kind == RH_SPHERE) { u_out[i] = cls_round_u<RH_SPHERE>(C, x, y, z, nx, ny, nz); u2_out[i] = cls_u2<RH_SPHERE>(D, x, y, z, nx, ny, nz); }
        else { u_out[i] = cls_round_u<RH_CYLINDER>(C, x, y, z, nx, ny, nz); u2_out[i] = cls_u2<RH_CYLINDER>(D, x, y, z, nx, ny, nz); }
    }
    return RH_OK;
}

// the cone's box test as the host runs it: the culling record cls_make builds for the shape (fields_out[RH_BOX_FIELDS]), and for
// each of the n binary64 boxes (centre, half extents: boxes[6 i ..]), converted by box_to_f32 like a group's, the decision of
// the kernel's own function.  Host only: needs no GPU.
extern "C" int rh_dbg_conebox(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, const double *boxes, int64_t n,
                              uint8_t *skip_out, float *fields_out)
{
    if (shape == nullptr || p == nullptr || n < 0 || (n > 0 && (boxes == nullptr || skip_out == nullptr))) {
        rh_set_error("rh_dbg_conebox: bad arguments");
        return RH_E_INVALID;
    }
    Probe Q;
    RH_TRY(probe_make("rh_dbg_conebox", "cones", 1 << RH_CONE, shape, p, M, Nm, 0.0, f32, Q, nullptr, fields_out));
    for (int64_t i = 0; i < n; i++) skip_out[i] = cone_box_skip32(Q.box, probe_box(boxes + 6 * i)) ? 1 : 0;
    return RH_OK;
}

// the classifier of a cone candidate: the record cls_make builds for the shape on the host, its thresholds and widths (dbg4:
// 0, wL, eD_lo, wD) and the kernel's own cls_cone_ab on n points, on the device (cls_cone_dbg_kernel).  Synchronous.
extern "C" int rh_dbg_cls_cone(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                               const double *nrm, int device, float *ua_out, float *ub_out, uint8_t *near_out, float *rec_out, double *dbg4_out)
{
    if (shape == nullptr || p == nullptr || n < 0 || n > (int64_t)1 << 24 ||
        (n > 0 && (xyz == nullptr || nrm == nullptr || ua_out == nullptr || ub_out == nullptr || near_out == nullptr))) {
        rh_set_error("rh_dbg_cls_cone: bad arguments");
        return RH_E_INVALID;
    }
    Probe Q;
    RH_TRY(probe_make("rh_dbg_cls_cone", "cones", 1 << RH_CONE, shape, p, M, Nm, 0.0, f32, Q, rec_out, nullptr, dbg4_out));
    if (n == 0) return RH_OK;
    std::vector<float> h((size_t)n * 6);
    for (int64_t i = 0; i < n; i++) {
        float q[6];
        probe_point(xyz, nrm, i, q);
        for (int k = 0; k < 6; k++) h[(size_t)(k * n + i)] = q[k];
    }
    RH_HIP(hipSetDevice(device));
    rh_dev<float> d_p, d_a, d_b;
    rh_dev<uint8_t> d_n;
    RH_TRY(d_p.alloc(n * 6));
    RH_TRY(d_a.alloc(n));
    RH_TRY(d_b.alloc(n));
    RH_TRY(d_n.alloc(n));
    RH_HIP(hipMemcpy(d_p, h.data(), sizeof(float) * (size_t)n * 6, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(cls_cone_dbg_kernel, dim3((unsigned)cdiv4(n, 256)), dim3(256), 0, 0, Q.C, (const float *)d_p, n, (float *)d_a, (float *)d_b, (uint8_t *)d_n);
    RH_HIP(hipGetLastError());
    RH_HIP(hipMemcpy(ua_out, d_a, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    RH_HIP(hipMemcpy(ub_out, d_b, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    RH_HIP(hipMemcpy(near_out, d_n, (size_t)n, hipMemcpyDeviceToHost));
    return RH_OK;
}

// diagnostics: the event counters of the score launches on this cloud (layout: S4_STAT, score4.hip).  mode 0: read (out[128],
// null: nothing), 1: switch the counting on and zero the counters, 2: switch it off.  Synchronises the cloud's stream.
extern "C" int rh_dbg_s4_stats(rh_cloud *c, int mode, uint64_t *out)
{
    if (c == nullptr || mode < 0 || mode > 2) { rh_set_error("rh_dbg_s4_stats: bad arguments"); return RH_E_INVALID; }
    RH_HIP(hipSetDevice(c->device));
    RH_HIP(hipStreamSynchronize(c->stream));
    if (mode == 1) {
        if (c->s4_stats == nullptr) RH_TRY(c->s4_stats.alloc(128));
        RH_HIP(hipMemset(c->s4_stats, 0, sizeof(unsigned long long) * 128));
    } else if (mode == 2) {
        c->s4_stats.reset();
    } else if (out != nullptr) {
        for (int i = 0; i < 128; i++) out[i] = 0;
        if (c->s4_stats != nullptr) RH_HIP(hipMemcpy(out, c->s4_stats, sizeof(unsigned long long) * 128, hipMemcpyDeviceToHost));
    }
    return RH_OK;
}

#endif   // RH_DIAG
