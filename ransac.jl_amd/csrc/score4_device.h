// score4_device.h -- the two-sided binary32 CLASSIFIER of the v4 score kernel (score4.hip), its per-candidate records and
// the binary32 box tests of its culling stage.
//
// Idea.  The reference's per-point tests (compatibles{Plane,Sphere,Cylinder,Cone}, /root/reference/src/shapes/*.jl) are
// binary64 and the score must reproduce their bits.  Almost every (candidate, point) pair, however, is nowhere near a
// threshold: a binary32 evaluation of the same quantities (fused multiply-adds allowed; ~2.3 SIMD cycles per wave64
// instruction against ~4.4 for binary64, 8 against 16+ for sqrt / rcp: tools/ubench/valu_rates.hip) already DECIDES it.
// The classifier evaluates each compared quantity q (distance, normal deviation) in binary32 as q32 and compares it with
// TWO thresholds, t - m and t + m, where m bounds |q32 - q64| rigorously (below).  Then
//     q32 inside by more than m   ->  the binary64 test passes:  "sure"
//     q32 outside by more than m  ->  the binary64 test fails
//     otherwise                   ->  "ambiguous": the pair goes to the exact binary64 test (score_device.h), unchanged.
// A point is an inlier iff every comparison passes, so  sure = AND of the sure bits,  maybe = AND of the "not surely
// outside" bits,  ambiguous = maybe & ~sure.  Counts are therefore bit-identical to the exact test whatever the margins'
// tightness; tightness only decides how many pairs take the slow path.
//
// Margins.  u = 2^-24.  Inputs are converted to binary32 (relative error u each), every binary32 operation adds (1 + d),
// |d| <= u.  With M = max |coordinate| of the point set, Nm = max |normal component|, T = M + max |centre coordinate|:
//   plane     dn = n . np - c             |.32 - .|   <= u (5.05 |n|_1 Nm + 4.1 |c|)      (c = cos alpha, added first)
//             d  = oz . p - oz . P0       |d32 - d|   <= 6.1 u (|oz|_1 M + |oz . P0|)
//   sphere    q = p - o (per component e = 2.01 u T), tested in the squared quantities n2 = |q|^2 and s |s|, s = sgn q . np:
//             "Round kinds without a square root" below
//   cylinder  q = t - a (a . t), t = p - c0: per component e_q = u T (3.01 + 8.04 |a|_inf |a|_1);  then as the sphere
//             with e_q for e
//   cone      the reference's frame in closed form (cone.jl:68-85 reduces to it, derivation at cls_cone_u): with w = p - apex,
//             h = w . a^, q = w - h a^, rho = |q| (e_q as the cylinder's with the unit axis a^), c', s' = cos / sin of
//             -opang/2 normalised:  D = c' rho + s' h  (the test is |D| < eps)
//                                         |D32 - D|   <= |c'| (sqrt(3) e_q + 5.5 u rho) + |s'| (6 u |a^|_1 T + 2 u |h|) + 4 u eps
//             L = sgn (c' q . np + s' rho a^ . np) - cos(alpha) rho  (the test is L > 0; no division by rho):
//                                         |L32 - L|   <= e_q (3 Nm |c'| + sqrt(3) G) + u rho (8.7 Nm |c'| + 6.5 G + 7 |s'| |a^|_1 Nm + 2 |c|)
//             with G = sqrt(3) Nm (|c'| + |s'|) + |c| + 1/4 and rho, |h| <= sqrt(3) T.  Points next to the axis
//             (rho^2 <= alpha |w|^2 + beta), where the reference's own frame is ill-conditioned, are always undecided.
// Every margin is the first-order bound x RH_CLS_SAFETY (2) plus the conversion error of the threshold itself; the
// binary64 side's own rounding (~1e-15 relative) disappears in that factor.  rh_dbg_cls_audit (score4_diag.hip) evaluates
// max |q32 - q64| / (width of the ambiguity band = 2 m) over real batches with these very functions: sound below 1/2,
// by construction below 1/4 (measured worst 0.21 = 0.84 of the first-order bound); tests/test_parity_gpu.py and
// tools/cls_audit.py hold it below 0.3.  (Round 3 started with a safety factor of 4 and widths rounded up to powers of
// two: 8.6 % of the cylinder pairs of the cfg3 batch were redone in binary64 then.)
//
// The records are SCALED: with wN, wD = 2 x margin, the kernel computes ua = (cN_hi - dn) / wN and ub = (|d| - eD_lo) / wD
// directly (the scaling is folded into the coefficients before they are rounded to binary32), so that with u = max(ua, ub)
//     sure <=> u < 0,   maybe <=> u <= 1                        (read off the bit pattern of u: cls_plane_u below; the score
//                                                                kernel's point loops read both off the top two bits of 2 u and
//                                                                take u = 1 for "out": "Two-bit books" below).
//
// Guards.  Non-finite or huge inputs would make binary32 overflow where binary64 does not, so a candidate is marked
// EXACT-ONLY (field RH_CLS_FLAG = NaN) unless all its parameters are finite and below 2^20 (cylinder axis components
// below 16) and M, Nm <= 2^20; a tile with an infinite or NaN value in an enabled point treats every candidate as
// exact-only.  Exact-only means: every enabled point is ambiguous.  Disabled points are staged as zeros and masked out
// (plane: their zero normal fails the angle test by itself, which needs cos(alpha) - margin > 0, else exact-only).
#pragma once

#include "rh_internal.h"

namespace rh4 {

constexpr double RH_CLS_U = 5.9604644775390625e-08;   // 2^-24
constexpr double RH_CLS_SAFETY = 2.0;
constexpr double RH_CLS_BIG = 1048576.0;               // 2^20

// 64-byte record, gathered per lane (lane = (candidate, group) pair or (candidate, point) pair)
struct rh_cls {
    float f[16];
};
constexpr int RH_CLS_FLAG = 15;   // NaN = exact-only
// plane:    0-2 -n / wN | 3 cN_hi / wN | 4-6 oz / wD | 7 -(oz . P0) / wD | 8 eD_lo / wD
// sphere:   0-2 o | 3 K | 4 1 / W2 | 5 -(H - m2) / W2 | 6 -sgn / Wv | 7 cos^2(alpha) / Wv      (K = R^2 + eps^2, H = 2 R eps; the
// cylinder: 0-2 a | 3-5 c0 | 6 K | 7 1 / W2 | 8 -(H - m2) / W2 | 9 -sgn / Wv | 10 cos^2(alpha) / Wv   sixth constant mv / Wv is 1/2)
// cone:     0-2 apex | 3-5 a^ | 6 c' / wD | 7 s' / wD | 8 eD_lo / wD | 9 -sgn c' / wL | 10 -sgn s' / wL | 11 cos(alpha) / wL | 12 beta

// culling record of a candidate, structure-of-arrays over the batch (field f of slot i at box[f * stride + i]): what
// the box tests of stage 1 read, coalesced, with lane = candidate
constexpr int RH_BOX_FIELDS = 11;
// plane:    0-2 oz | 3 -(oz . P0) | 4 eps + slack | 5-7 the 96 bits of the normal-cell mask, bit-cast (all ones: never skip)
// sphere:   0-2 o | 3 A2 | 4 B2
// cylinder: 0-2 a | 3-5 c0 | 6 (R + eps) + slack | 7 (R - eps) - slack | 8 max(1, |1 - |a|^2|) | 9 A2 of the support clause
// cone:     0-2 apex | 3-5 a^ | 6 kk | 7 1 / cn | 8 (eps + slack) / cn | 9 beta | 10 alpha
constexpr float RH_CONE_ALPHA = (float)((RH_CLS_SAFETY * 49.0 + 64.0) * RH_CLS_U);

__host__ __device__ inline bool cls_fin(double v) { return v - v == 0.0; }

// round a threshold to binary32 towards the SAFE side (lo thresholds down, hi thresholds up) by widening with its own ulp
__host__ __device__ inline float cls_dn(double v) { return (float)(v - fabs(v) * (2.0 * RH_CLS_U) - 1e-37); }
__host__ __device__ inline float cls_up(double v) { return (float)(v + fabs(v) * (2.0 * RH_CLS_U) + 1e-37); }

// the old kernel's slack of the conservative stages: covers the exact test's own binary64 rounding (score_device.h)
__host__ __device__ inline double cls_slack64(const rh_prep &P, double M) { return 1e-9 * ((1.0 + M) + P.f[11]); }

// ---- Normal cells (planes).  The boxes of stage 1 know where a group's points lie, not where their normals point: three
// quarters of the plane pairs that survive the boxes fail on the normal half of the test in every point.  The unit sphere
// of directions is cut into RH_NSIG_CELLS = 96 cells (a cube map: 6 faces x 4 x 4); a group of subset 1 carries the set of
// cells its points' normals fall in (96 bits, made once per cloud: nsig_kernel, boxes32.hip -- ALL points, enabled or not, so
// that the set stays a superset through every extraction), a plane candidate the set of cells that can hold the normal of a
// point it accepts (cls_make, fields 5-7 of the culling record).  A pair whose two sets do not meet is not walked.
// Soundness -- a skipped pair holds no inlier:
//   1. a point the exact test accepts has n . np > cos(alpha) as the exact test evaluates it; the true value of n . np
//      then exceeds cos(alpha) - mN, mN being the margin cls_make derives for the classifier's normal half: it bounds a
//      binary32 evaluation of this very dot product (tripled on a Float32 cloud, whose exact test IS such a chain), and the
//      binary64 chain's rounding is 2^-29 of that;
//   2. with |np| <= L (the largest finite normal length of the subset, nsig_kernel; without it sqrt(3) Nm) the direction
//      d = np / |np| has n^ . d > (cos(alpha) - mN) / (L |n|) =: T, so d lies in the cone of half-angle theta = acos(T)
//      about n^ -- normals of other lengths than 1 widen the cone, they never break it.  T <= 0 (a cone of 90 degrees or
//      more), an exact-only candidate, cos(alpha) - mN <= 0 or anything non-finite: all 96 bits, never skip;
//   3. nsig_cell(np) is the ONE definition of a cell, evaluated on the point side only (exact comparisons of the
//      components, no division: a direction on a border belongs to the cell the comparisons say).  Every direction that
//      nsig_cell maps to cell k lies within the angular radius r_k of the cell's centre c_k (closed cell: its borders and
//      corners included; the radius is the angle to the farthest corner -- c . d along a great-circle arc shorter than pi
//      takes its minimum at an end);
//   4. hence angle(n^, c_k) <= theta + r_k, and the candidate's mask holds every cell with
//      n^ . c_k >= cos(theta + r_k + slack) = T cos(r_k + slack) - sqrt(1 - T^2) sin(r_k + slack)  (theta + r_k < pi).
// Slack: 2e-6 rad inside the table's cos / sin (the table's 17 digits and the candidate side's binary64 arithmetic -- the
// normalisation of n, T, the square root where T is within 1e-16 of 1: together below 1e-7) and 1e-9 on T itself.
constexpr int RH_NSIG_CELLS = 96;

// ---- The cylinder's box by its support (cyl_box_skip32 below, field 9 of the culling record).  The two older clauses of the
// cylinder's box test take the box for a ball: the distance from the axis at the centre, +- the Lipschitz constant x the half
// diagonal hr.  A k-d leaf on a surface patch is flat, not round.  With t = c - c0, q = M t (M = I - a a', symmetric for any
// axis a), rho_c = |q| and ANY unit vector v, every point p = c + d of the box (|d_k| <= h_k) has
//     rho(p) = |M (t + d)| >= v . M (t + d) = v . q + (M v) . d >= v . q - sum_k |(M v)_k| h_k,
// the tangent plane of the convex function rho; at v = q / rho_c it reads rho_c - s / rho_c with g = M q = q - a (a . q) and
// s = sum |g_k| h_k.  The third clause skips when that lower bound clears the band: with w = rho_c^2 - s,
//     w > 0  and  w^2 > A^2 rho_c^2                     (no square root; A = R + eps + slack > 0; A <= 0: stored as A^2 = 0).
// It is ORed to the older two, so the pairs walked are a subset of what they were, and it says nothing about the inner
// cylinder.  g is computed in the kernel (6 instructions) and not replaced by q: for a unit axis they agree, but q's direction
// carries the error e_q / rho_c, which the box's LONG sides would multiply (a term h e_q / rho_c that no stored slack bounds);
// M q^ costs that error a second-order effect only -- and the clause stays sound for an axis of any length, which is legal
// input (cylinder.jl uses it as stored), with nothing to disable.
// Soundness in binary32 -- a skipped pair holds no point of the band.  Hats are the kernel's values, rho' = |q^| and
// s' = sum |g^_k| h_k the exact functions of them, v = q^ / rho':
//   1. the binary32 box holds the binary64 one (box_to_f32), so c, h are the binary32 numbers; |q^_k - q_k| <= e_q
//      (Margins above: the conversion of a and c0 included), hence v . q >= rho' - sqrt(3) e_q;
//   2. g^ = fma(-a32, fl(a32 . q^), q^) against rho' M v, per component: the dot product is off by 4.1 u |a|_1 rho' (its 3
//      roundings and the conversion of a), the fma by u (1 + 2 |a|_inf |a|_1) rho' more (a_k's conversion, its rounding):
//      together u (1 + 6.1 |a|_inf |a|_1) rho' <= u c_g rho' with
//      c_g = 2 + 8 |a|_inf |a|_1, and sum_k h_k <= 3.01 M (a box of the point set: h_k <= M, widened by box_to_f32 and the
//      unions of st32_kernel by parts in 10^6 at most).  So  rho(p) >= rho' - s' / rho' - sqrt(3) e_q - 3.01 u c_g M;
//   3. rho2^ = fl(sum q^_k^2) and s^ = fl(sum |g^_k| h_k) are sums of non-negative terms, three roundings each:
//      rho2^ <= rho'^2 (1 + 3.01 u), s^ >= s' (1 - 3.01 u).  w^ = fma(rho2^, 0.999999f, -s^) takes 16.9 u of rho2^ off before
//      the difference is formed: w^ > 0 implies rho'^2 - s' >= w^ (1 - u) -- the cancellation costs no absolute term;
//   4. fl(w^ w^) <= w^2 (1 + u) and fl(A2 rho2^) >= A2 rho'^2 (1 - u)^4: the stored A2 = A^2 (1 + 16 u), rounded up, covers
//      both.  Overflow: w^ <= rho2^ <= 3.1 T^2 (1 + |a|_inf |a|_1)^2, kept below 1e18 (else the field is NaN), its square
//      below 3.4e38.  Underflow only lowers fl(w^ w^) or, where A2 rho2^ underflows, rho2^ < A2 (A >= 1e-9) and monotone
//      rounding keeps fl(w^ w^) <= fl(rho2^ rho2^) <= fl(A2 rho2^): no skip;
//   5. A = (R + eps) + sB + S 3.01 u c_g M, sB the slack of the older clauses: it holds S sqrt(3) e_q (item 1), the rounding of
//      R and eps, the exact test's own slack (cls_slack64) and, on a Float32 cloud, the tripled part for the exact chain.
// NaN anywhere (a record that is not usable, a NaN box) fails every comparison: no skip.  A centre on the axis has
// w^ <= 0.  A ZERO axis is no cylinder: its record keeps NaN box fields, for the older clauses too.

// cell of a direction with finite components, not all zero: face = the component of largest magnitude with its sign,
// the other two components against +-1/2 of that magnitude and 0 (their quotients cut at -1/2, 0, 1/2)
__host__ __device__ inline int nsig_cell(double x, double y, double z)
{
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    double m, a, b;
    int axis;
    if (ax >= ay && ax >= az) { axis = 0; m = x; a = y; b = z; }
    else if (ay >= az) { axis = 1; m = y; a = z; b = x; }
    else { axis = 2; m = z; a = x; b = y; }
    const double h = 0.5 * fabs(m);
    const int i = (a >= -h ? 1 : 0) + (a >= 0.0 ? 1 : 0) + (a >= h ? 1 : 0);
    const int j = (b >= -h ? 1 : 0) + (b >= 0.0 ? 1 : 0) + (b >= h ? 1 : 0);
    return (axis * 2 + (m < 0.0 ? 1 : 0)) * 16 + i * 4 + j;
}

// the bits a point's normal sets in its group's mask: an infinite component -- the exact test's dot product may be +inf --
// sets all 96; a NaN or the zero vector nothing (n . np > cos(alpha) is false for them whenever cos(alpha) > 0, and a
// candidate with cos(alpha) - mN <= 0 skips nothing)
__host__ __device__ inline void nsig_point_bits(double nx, double ny, double nz, uint32_t w[3])
{
    w[0] = w[1] = w[2] = 0u;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    if (ax == __builtin_inf() || ay == __builtin_inf() || az == __builtin_inf()) { w[0] = w[1] = w[2] = 0xffffffffu; return; }
    if (!(nx == nx) || !(ny == ny) || !(nz == nz) || (ax == 0.0 && ay == 0.0 && az == 0.0)) return;
    const int k = nsig_cell(nx, ny, nz);
    w[k >> 5] = 1u << (k & 31);
}

// the cells that can hold a direction d with n . d >= thr / L: the candidate's mask (all ones: never skip)
__host__ __device__ inline void nsig_cand_mask(double nx, double ny, double nz, double thr, double L, uint32_t m[3])
{
    // centre (major, a, b) of the 16 cells of a face at quotients (-3/4, -1/4, 1/4, 3/4)^2, and cos / sin of the cell's angular
    // radius (the angle to its farthest corner) + 2e-6: rows i * 4 + j as nsig_cell numbers them; the six faces permute them
    static constexpr double tab[16][5] = {
        { 0.68599434057003528, -0.51449575542752646, -0.51449575542752646, 0.97182484440108552, 0.23570420404567663 },
        { 0.78446454055273618, -0.58834840541455213, -0.19611613513818404, 0.96076836812840516, 0.27735201964990502 },
        { 0.78446454055273618, -0.58834840541455213, 0.19611613513818404, 0.96076836812840516, 0.27735201964990502 },
        { 0.68599434057003528, -0.51449575542752646, 0.51449575542752646, 0.97182484440108552, 0.23570420404567663 },
        { 0.78446454055273618, -0.19611613513818404, -0.58834840541455213, 0.96076836812840516, 0.27735201964990502 },
        { 0.94280904158206347, -0.23570226039551587, -0.23570226039551587, 0.94280837491351122, 0.33333521895074958 },
        { 0.94280904158206347, -0.23570226039551587, 0.23570226039551587, 0.94280837491351122, 0.33333521895074958 },
        { 0.78446454055273618, -0.19611613513818404, 0.58834840541455213, 0.96076836812840516, 0.27735201964990502 },
        { 0.78446454055273618, 0.19611613513818404, -0.58834840541455213, 0.96076836812840516, 0.27735201964990502 },
        { 0.94280904158206347, 0.23570226039551587, -0.23570226039551587, 0.94280837491351122, 0.33333521895074958 },
        { 0.94280904158206347, 0.23570226039551587, 0.23570226039551587, 0.94280837491351122, 0.33333521895074958 },
        { 0.78446454055273618, 0.19611613513818404, 0.58834840541455213, 0.96076836812840516, 0.27735201964990502 },
        { 0.68599434057003528, 0.51449575542752646, -0.51449575542752646, 0.97182484440108552, 0.23570420404567663 },
        { 0.78446454055273618, 0.58834840541455213, -0.19611613513818404, 0.96076836812840516, 0.27735201964990502 },
        { 0.78446454055273618, 0.58834840541455213, 0.19611613513818404, 0.96076836812840516, 0.27735201964990502 },
        { 0.68599434057003528, 0.51449575542752646, 0.51449575542752646, 0.97182484440108552, 0.23570420404567663 },
    };
    m[0] = m[1] = m[2] = 0xffffffffu;
    const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(thr > 0.0) || !(L > 0.0) || !(nn > 0.0) || !cls_fin(thr) || !cls_fin(L) || !cls_fin(nn)) return;
    double T = thr / (L * nn) * (1.0 - 1e-9);   // cos(theta), rounded towards the wider cone
    if (!(T > 0.0)) return;
    if (T > 1.0) T = 1.0;
    const double Sn = sqrt(fmax(0.0, 1.0 - T * T));
    const double ux = nx / nn, uy = ny / nn, uz = nz / nn;
    // per face: (major, a, b) of the unit normal in the face's frame, nsig_cell's permutation
    const double fm[3] = { ux, uy, uz }, fa[3] = { uy, uz, ux }, fb[3] = { uz, ux, uy };
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
#pragma unroll
    for (int axis = 0; axis < 3; axis++)
#pragma unroll
        for (int neg = 0; neg < 2; neg++) {
            uint32_t bits = 0u;
            for (int r = 0; r < 16; r++) {
                const double c = ((neg ? -tab[r][0] : tab[r][0]) * fm[axis] + tab[r][1] * fa[axis]) + tab[r][2] * fb[axis];
                bits |= c >= T * tab[r][3] - Sn * tab[r][4] ? (1u << r) : 0u;
            }
            const int f = axis * 2 + neg;   // 16 bits per face, two faces per word
            if (f < 2) w0 |= bits << (16 * (f & 1));
            else if (f < 4) w1 |= bits << (16 * (f & 1));
            else w2 |= bits << (16 * (f & 1));
        }
    m[0] = w0; m[1] = w1; m[2] = w2;
}

// ---- Round kinds without a square root (cls_round_ab below; the records of the sphere and the cylinder).  The exact test is
// |nr - R| < eps and s / nr > c with nr = |q|, s = sgn (q . np), c = cos(alpha).  Until round 10 the classifier formed
// nr = n2 rsq(n2) and s / nr: a reciprocal root (8.1 issue cycles against 2.3 of a plain operation, ubench_valu_rates) and two
// multiplies per point that the decision does not need.  With n2 = nr^2, K = R^2 + eps^2, H = 2 R eps:
//     |nr - R| < eps  <=>  (R - eps)^2 < n2 < (R + eps)^2  <=>  |n2 - K| < H                       (needs R - eps > 0)
//     s / nr > c      <=>  s > 0 and s^2 > c^2 n2           <=>  v := s |s| - c^2 n2 > 0          (needs c > 0, nr > 0)
// and the kernel computes, both scaled like the plane's (widths W2 = 2 m2, Wv = 2 mv),
//     ua = (|n2 - K| - (H - m2)) / W2,      ub = (mv - v) / Wv = 1/2 + (c^2 n2 - sgn qn |qn|) / Wv,       u = max(ua, ub).
// Margins, first order x S (RH_CLS_SAFETY; tripled on a Float32 cloud).  mD, the margin of the older form on nr itself
// (S (sqrt(3) e + 7 u (R + eps))), only places two radii: nrmax = R + eps + 3 mD, nrmin = R - eps - 3 mD.
//   Which points count.  A point with nr > nrmax has ua > 1: |q^| >= nr - sqrt(3) e >= (R + eps) + 2.5 mD (sqrt(3) e <= mD / S),
//   so |q^|^2 >= (K + H) + 5 mD (R + eps) + 6.25 mD^2, while m2 (below) <= S (2 (R + eps) sqrt(3) e + 20 u (R + eps)^2) + 6.5 mD^2:
//   what is left, S (3 sqrt(3) e (R + eps) + 15 u (R + eps)^2) - mD^2 / 4 >= 2 mD (R + eps) >= 28 u (R + eps)^2 (R + eps > 3 mD),
//   holds the roundings of n2^, of the subtraction and of the fma (~7 u (R + eps)^2) four times, and |q^|^2 (1 - 3.01 u) grows
//   with nr.  Such a point is truly outside, so u > 1 is right whatever ub is.  Every bound below is therefore needed for
//   nr <= nrmax only, where |q^| <= nq = nrmax + sqrt(3) e.
//   n2:  |q^|^2 - n2 = 2 q . dq + |dq|^2 with |dq| <= sqrt(3) e; the three roundings of the sum of squares (non-negative terms)
//        3.01 u nq^2; K's conversion, the subtraction, the scaled constants and the fma, near the band where |n2 - K| ~ H <= K:
//        below 6 u K.       dn2 = 2 nrmax sqrt(3) e + 3 e^2 + 4 u nq^2 + 6 u K,        m2 = S dn2.
//   qn:  the conversion of np and of q (3 Nm e + u Nm |q^|_1) and three roundings of partial sums below Nm |q^|_1 <= Nm sqrt(3) nq:
//                           ds = 3 Nm e + 5 u Nm sqrt(3) nq.
//   v:   |s^ |s^| - s |s|| <= 2 |s| ds + ds^2 (x |x| has slope 2 |x|); c^2 dn2 for n2; the product, the two scaled constants and
//        the two fma: 2 u s^2 + 3 u c^2 n2.  Only |s| <= c nr + ds has to be covered:
//          - "surely in" (v^ > mv) of a point the test rejects (s <= c nr): for s^ <= 0 both addends of ub are >= 0 whatever the
//            roundings (they are relative, signs are exact) and ub >= 1/2; else -ds <= s <= c nr;
//          - "surely out" (v^ < -mv) of a point the test accepts (s > c nr): the shortfall error(s) - v(s) has the derivative
//            2 ds + 4 u s - 2 s < 0 for s > 1.01 ds, so its largest value over s >= c nr is taken at s = c nr (or below c nr + ds),
//            where v = 0.
//                           mv = S (2 (c nrmax + ds) ds + ds^2 + c^2 dn2 + 8 u c^2 nq^2).
//        With sqrt(3) Nm nrmax (all a normal can give) in place of c nrmax + ds the undecided points rise by a third (tools/proto/root_free.py).
//   Float32 cloud: the exact chain's error in nr and in s / nr reaches n2 and v through the factors 2 nr and 2 c nr^2, the very
//   factors that carry the classifier's own e and u terms into dn2 and ds above: two more parts of the same bounds, as everywhere.
// Guards (any failure: exact-only).  eps >= 0, c > 0, nrmin > 0.  A point whose ua can be <= 1 has n2^ >= n2min =
// (R - eps)^2 - 2 m2; n2min > 0 makes the point ON the centre / axis (n2 = 0) surely out.  A disabled point is staged as zeros:
// qn = 0 and ub = 1/2 + c^2 n2^ / Wv, which exceeds 1 -- surely out, not merely undecided -- iff c^2 n2^ > mv: c^2 n2min >
// 1.001 mv.  No product may overflow (inf - inf = NaN, and the books read the sign bit of u): every scaled constant x the
// largest value of its operand on this point set (n2 <= 3.1 T^2 (1 + |a|_inf |a|_1)^2, qn^2 <= 3 Nm^2 n2) stays below 2^120.

// P: the binary64 record of the candidate (rh_prep, kernels.hip prep_one, with prep_derived); eps, cosa: the kind's
// thresholds; M, Nm: max |coordinate| / max |normal component| of the point set.  o: classifier record; box: the culling
// record's fields go to box[f * bstride] (f < RH_BOX_FIELDS).
// dbg4 (audit): the unscaled thresholds and widths behind a scaled record: cN_hi, wN, eD_lo, wD (plane, cone); the margins and
// widths of the squared form m2, W2, mv, Wv (sphere, cylinder)
__host__ __device__ inline void cls_make(const rh_prep &P, int kind, double eps, double cosa, double M, double Nm, rh_cls &o,
                                         float *box, int64_t bstride, double *dbg4 = nullptr, bool f32cloud = false, double Ln = 0.0)
{
    // Ln: the largest finite normal LENGTH of the point set (0: not known -- sqrt(3) Nm bounds it), for the plane's normal-cell mask
    // f32cloud: the EXACT test of this cloud is itself a binary32 chain without fused operations (Float32 cloud,
    // score_device.h with T = float: 1.3 - 2 x the rounding steps of the classifier's chain on the same magnitudes).  Every margin
    // is tripled: one part for the classifier's own error, two for the exact chain's.
    const double u = RH_CLS_U, S = f32cloud ? 3.0 * RH_CLS_SAFETY : RH_CLS_SAFETY;
    const float fnan = __builtin_nanf("");
    for (int i = 0; i < 16; i++) o.f[i] = 0.0f;
    float bx[RH_BOX_FIELDS];
    for (int i = 0; i < RH_BOX_FIELDS; i++) bx[i] = fnan;   // NaN fields: the box test never skips
    bool ok = cls_fin(eps) && cls_fin(cosa) && cls_fin(M) && cls_fin(Nm) && M <= RH_CLS_BIG && Nm <= RH_CLS_BIG && fabs(eps) <= RH_CLS_BIG;
    const double slack64 = cls_slack64(P, M);
    if (kind == RH_PLANE) {
        bool fin = true;
        for (int i = 0; i < 9; i++) fin = fin && cls_fin(P.f[i]) && fabs(P.f[i]) <= RH_CLS_BIG;
        ok = ok && fin;
        const double n1 = (fabs(P.f[3]) + fabs(P.f[4])) + fabs(P.f[5]);
        const double z1 = (fabs(P.f[6]) + fabs(P.f[7])) + fabs(P.f[8]);
        const double zp = (P.f[6] * P.f[0] + P.f[7] * P.f[1]) + P.f[8] * P.f[2];
        // (the threshold is the first addend of the fused chain: every partial sum is as large as it is, hence the
        // 4.1 |cos alpha| and 4 |eps| beside the products' own 5.05 / 6.1)
        const double mN = S * u * (5.05 * (n1 * Nm) + 4.1 * (fabs(cosa) + 1e-3)) + 1e-30;
        // Float32 cloud: the test to be bracketed is the reference's OWN binary32 chain oz32 . (p - p0), whose error does not
        // shrink when oz . p0 cancels: p - p0 is rounded per component (u |p_i - p0_i|), oz32 = normalize in binary32 is
        // off by u per component, then three products and two sums -- u (6.2) sum_i |oz_i| (M + |p0_i|) to first order.  A
        // plane through the cloud given by a point 1e6 away is a legal candidate (test_f32_gpu.py).
        const double zabs = (fabs(P.f[6] * P.f[0]) + fabs(P.f[7] * P.f[1])) + fabs(P.f[8] * P.f[2]);
        const double mRef = f32cloud ? RH_CLS_SAFETY * u * 6.2 * (z1 * M + zabs) : 0.0;
        const double mD = S * u * (6.1 * (z1 * M + fabs(zp)) + 4.0 * fabs(eps)) + mRef + 1e-30;
        ok = ok && cls_fin(mN) && cls_fin(mD) && cls_fin(zp) && mN < 1e30 && mD < 1e30;
        if (ok) {
            const double wN = 2.0 * mN, wD = 2.0 * mD;
            const double iN = 1.0 / wN, iD = 1.0 / wD;
            const double cNhi = cosa + 0.5 * wN, eDlo = eps - 0.5 * wD;
            ok = cosa - 0.5 * wN > 0.0;   // a zero normal (a disabled point) must fail the angle test surely
            o.f[0] = (float)(-P.f[3] * iN); o.f[1] = (float)(-P.f[4] * iN); o.f[2] = (float)(-P.f[5] * iN);
            o.f[3] = (float)(cNhi * iN);
            o.f[4] = (float)(P.f[6] * iD); o.f[5] = (float)(P.f[7] * iD); o.f[6] = (float)(P.f[8] * iD);
            o.f[7] = (float)(-zp * iD);
            o.f[8] = (float)(eDlo * iD);
            if (dbg4 != nullptr) { dbg4[0] = cNhi; dbg4[1] = wN; dbg4[2] = eDlo; dbg4[3] = wD; }
            for (int i = 0; i < 9; i++) ok = ok && fabs((double)o.f[i]) < 1e30;
        }
        // the normal-cell mask (nsig_cand_mask above): whatever the box fields are, all ones unless the record decides points
        uint32_t cm[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu };
        if (ok) {
            const double Lb = 1.7320508075688774 * Nm * (1.0 + 1e-12);
            nsig_cand_mask(P.f[3], P.f[4], P.f[5], cosa - mN, (Ln > 0.0 && Ln < Lb ? Ln * (1.0 + 1e-12) : Lb), cm);
        }
        bx[5] = __builtin_bit_cast(float, cm[0]); bx[6] = __builtin_bit_cast(float, cm[1]); bx[7] = __builtin_bit_cast(float, cm[2]);
        if (fin && cls_fin(zp) && cls_fin(eps) && cls_fin(M)) {
            // box: d(centre) against eps + sum |oz_i| h_i; binary32 error of both sides + the binary64 test's own slack
            const double sB = S * 10.1 * u * (z1 * M + fabs(zp)) + mRef + slack64;
            bx[0] = (float)P.f[6]; bx[1] = (float)P.f[7]; bx[2] = (float)P.f[8];
            bx[3] = (float)(-zp);
            bx[4] = cls_up(eps + sB);
        }
    } else if (kind == RH_SPHERE || kind == RH_CYLINDER) {
        const bool sph = kind == RH_SPHERE;
        bool fin = true;
        for (int i = 0; i < 7; i++) fin = fin && ((sph && i >= 4) || (cls_fin(P.f[i]) && fabs(P.f[i]) <= RH_CLS_BIG));   // (no run-time indices)
        ok = ok && fin;
        const double R = sph ? P.f[3] : P.f[6], sgn = sph ? P.f[4] : P.f[7];
        const double c0 = sph ? P.f[0] : P.f[3], c1 = sph ? P.f[1] : P.f[4], c2 = sph ? P.f[2] : P.f[5];
        const double T = M + fmax(fabs(c0), fmax(fabs(c1), fabs(c2)));
        double e, lipk = 1.0;   // e: error bound per component of the vector whose norm is taken
        double a1 = 0.0, ai = 0.0;
        bool axis_ok = true;
        if (sph) {
            e = 2.01 * u * T;
        } else {
            a1 = (fabs(P.f[0]) + fabs(P.f[1])) + fabs(P.f[2]);
            ai = fmax(fabs(P.f[0]), fmax(fabs(P.f[1]), fabs(P.f[2])));
            axis_ok = ai <= 16.0;
            ok = ok && axis_ok;
            e = u * T * (3.01 + 8.04 * ai * a1);
            lipk = fmax(1.0, fabs(P.f[9] - 1.0));   // |1 - |a|^2| = |k - 1| (prep_derived)
        }
        const double s3 = 1.7320508075688774;
        // the root-free form ("Round kinds without a square root" above).  mD, the margin of the older form on nr itself, only
        // places the two radii between which a point's ua can be <= 1
        const double mD = S * (s3 * e + 7.0 * u * (fabs(R) + fabs(eps))) + 1e-30;
        const double nrmax = R + eps + 3.0 * mD, nrmin = R - eps - 3.0 * mD;
        const double nq = nrmax + s3 * e;                        // |q^| where nr <= nrmax
        const double K = R * R + eps * eps, H = 2.0 * R * eps, ca2 = cosa * cosa;
        const double dn2 = 2.0 * nrmax * s3 * e + 3.0 * e * e + 4.0 * u * nq * nq + 6.0 * u * K;
        const double m2 = S * dn2 + 1e-30;
        const double ds = 3.0 * Nm * e + 5.0 * u * Nm * s3 * nq;
        const double mv = S * (2.0 * (fabs(cosa) * nrmax + ds) * ds + ds * ds + ca2 * dn2 + 8.0 * u * ca2 * nq * nq) + 1e-30;
        // a point whose ua can be <= 1 has n2 (true and computed) above this
        const double n2min = (R - eps) * (R - eps) - 2.0 * m2;
        ok = ok && cls_fin(m2) && cls_fin(mv) && (sgn == 1.0 || sgn == -1.0) && m2 < 1e30 && mv < 1e30;
        // the equivalences need R - eps > 0 and cos(alpha) > 0; a disabled point (staged as zeros: qn = 0, ub = (cos^2 n2 + mv) / Wv)
        // must come out SURELY out wherever its ua does not say so already
        ok = ok && eps >= 0.0 && cosa > 0.0 && nrmin > 0.0 && n2min > 0.0 && ca2 * n2min > 1.001 * mv;
        // (constant indices only: a run-time index would move the record to scratch memory)
        if (sph) { o.f[0] = (float)P.f[0]; o.f[1] = (float)P.f[1]; o.f[2] = (float)P.f[2]; }
        else { o.f[0] = (float)P.f[0]; o.f[1] = (float)P.f[1]; o.f[2] = (float)P.f[2]; o.f[3] = (float)P.f[3]; o.f[4] = (float)P.f[4]; o.f[5] = (float)P.f[5]; }
        if (ok) {
            const double W2 = 2.0 * m2, Wv = 2.0 * mv;
            const double i2 = 1.0 / W2, iv = 1.0 / Wv;
            const float s0 = (float)K, s1 = (float)i2, s2 = (float)(-(H - m2) * i2), s3f = (float)(-sgn * iv), s4 = (float)(ca2 * iv);
            if (dbg4 != nullptr) { dbg4[0] = m2; dbg4[1] = W2; dbg4[2] = mv; dbg4[3] = Wv; }
            if (sph) { o.f[3] = s0; o.f[4] = s1; o.f[5] = s2; o.f[6] = s3f; o.f[7] = s4; }
            else { o.f[6] = s0; o.f[7] = s1; o.f[8] = s2; o.f[9] = s3f; o.f[10] = s4; }
            // no product of the chain may overflow (inf - inf = NaN, and the books read the sign bit of u): every scaled constant x
            // the largest value its operand takes on this point set stays below 2^120
            const double big = 1.329227995784916e36;
            const double n2max = 3.1 * T * T * ((1.0 + ai * a1) * (1.0 + ai * a1)), qn2max = 3.0 * Nm * Nm * n2max;
            ok = ok && fabs((double)s0) < 1e30 && fabs((double)s1) < 1e30 && fabs((double)s2) < 1e30 && fabs((double)s3f) < 1e30 && fabs((double)s4) < 1e30;
            ok = ok && (n2max + K) * i2 < big && qn2max * iv < big && n2max * ca2 * iv < big;
        }
        if (fin && axis_ok && (sph || a1 > 0.0) && cls_fin(eps) && cls_fin(M)) {
            // box: |p - o| (sphere) or the distance from the axis (cylinder, at the centre of the box +- Lipschitz) against
            // R +- eps; binary32 error of the norm at the centre + of the squares + the binary64 test's own slack
            const double sB = S * (s3 * e + 4.0 * u * (fabs(R) + fabs(eps)) + 4.0 * u * lipk * s3 * M) + slack64;
            const double A = (R + eps) + sB, B = (R - eps) - sB;
            if (cls_fin(A) && cls_fin(B)) {
                if (sph) {
                    bx[0] = (float)P.f[0]; bx[1] = (float)P.f[1]; bx[2] = (float)P.f[2];
                    bx[3] = A > 0.0 ? cls_up(A * A * (1.0 + 16.0 * u)) : 0.0f;   // A <= 0: any positive distance is outside
                    bx[4] = B > 0.0 ? cls_dn(B * B * (1.0 - 16.0 * u)) : -1.0f;  // B <= 0: never "inside the inner ball"
                } else {
                    for (int i = 0; i < 6; i++) bx[i] = (float)P.f[i];
                    bx[6] = cls_up(A);
                    bx[7] = cls_dn(B);
                    bx[8] = cls_up(lipk);
                    // the support clause ("The cylinder's box by its support" above): A^2, NaN where its squares could overflow
                    const double As = A + S * 3.01 * u * (2.0 + 8.0 * ai * a1) * M;
                    const double r2max = 3.1 * T * T * ((1.0 + ai * a1) * (1.0 + ai * a1));
                    if (cls_fin(As) && r2max < 1e18) bx[9] = As > 0.0 ? cls_up(As * As * (1.0 + 16.0 * u)) : 0.0f;
                }
            }
        }
    } else {
        // cone: the two-sided classifier works on the closed form of the reference's frame (cls_cone_u below); the culling
        // record keeps the band form: with t = p - apex, h = t . a^, rho^2 = |t|^2 - h^2 the reference's distance is
        // -(c rho + s h) / sqrt(c^2 + s^2) (c, s = cos / sin of -opang/2): |dist| < eps <=> rho in (k h - e, k h + e),
        // k = -s / c, e = eps sqrt(c^2 + s^2) / c   (c > 0)
        for (int i = 0; i < 8; i++) ok = ok && cls_fin(P.f[i]) && fabs(P.f[i]) <= RH_CLS_BIG;
        const double ax = P.f[3], ay = P.f[4], az = P.f[5], c = P.f[6], sn = P.f[7], sgn = P.f[8];
        const double an = sqrt((ax * ax + ay * ay) + az * az), cs = sqrt(c * c + sn * sn);
        ok = ok && (an > 1e-300) && cls_fin(an) && (cs > 1e-300) && cls_fin(cs) && (sgn == 1.0 || sgn == -1.0);
        const bool band_ok = ok && (c > 1e-6 * cs);     // the band form (culling record; Float32 clouds: the point record too)
        const double ia = ok ? 1.0 / an : 0.0;
        const double T = M + fmax(fabs(P.f[0]), fmax(fabs(P.f[1]), fabs(P.f[2])));
        const double kk = band_ok ? -sn / c : 0.0;
        const double cn = band_ok ? c / cs : 1.0;
        // band half width: exact form + the f64 prefilter's slack + binary32 error of k h (|t| <= sqrt(3) T)
        // (Float32 cloud: the exact test's frame is a long binary32 chain, ~1e-5 relative near its band: score_device.h F32 margins)
        const double ek = S * 19.1 * fabs(kk) * u * T + 1e-8 * (1.0 + T) * (1.0 + fabs(kk)) + (f32cloud ? 2e-5 * (1.0 + T) * (1.0 + fabs(kk)) : 0.0);
        const double beta = S * 1.75 * u * T * T + 1e-30;
        // ---- the point record
        const double a0 = ax * ia, a1v = ay * ia, a2v = az * ia;          // a^
        const double cp = ok ? c / cs : 0.0, sp = ok ? sn / cs : 0.0;     // c', s'
        const double a1 = (fabs(a0) + fabs(a1v)) + fabs(a2v), ai = fmax(fabs(a0), fmax(fabs(a1v), fabs(a2v)));
        const double s3 = 1.7320508075688774;
        const double eq = u * T * (3.01 + 8.04 * ai * a1);
        const double rmax = s3 * T;
        // (classifier's own binary32 error, first order x RH_CLS_SAFETY -- never the tripled S: a Float32 cloud's exact
        // chain is bracketed by its own term below)
        const double mDc = RH_CLS_SAFETY * (fabs(cp) * (s3 * eq + 5.5 * u * rmax) + fabs(sp) * (6.0 * u * a1 * T + 2.0 * u * rmax) + 4.0 * u * fabs(eps));
        const double G = s3 * Nm * (fabs(cp) + fabs(sp)) + fabs(cosa) + 0.25;
        const double mLc = RH_CLS_SAFETY * (eq * (3.0 * Nm * fabs(cp) + s3 * G) +
                                            u * rmax * (8.7 * Nm * fabs(cp) + 6.5 * G + 7.0 * fabs(sp) * a1 * Nm + 2.0 * fabs(cosa)));
        double mD, mL;
        if (!f32cloud) {
            // the binary64 chain of the reference differs from the closed form by ~1e-15 |t| / sin(angle to the axis); the
            // axis guard (alpha, beta) keeps that sine above ~3e-3: 1e-11 (1 + T) covers it 30 times over
            mD = mDc + 1e-11 * (1.0 + T) + 1e-30;
            mL = mLc + 1e-11 * (1.0 + T) * (1.0 + Nm) + 1e-30;
        } else {
            // Float32 cloud: the exact test is a ~60-operation binary32 chain.  Its distance is bracketed like round 3's
            // prefilter did (band form, needs c > 0; 2e-5 relative: in ek); its normal half is never decided here -- every
            // point inside the widened band goes to the exact test.
            ok = ok && band_ok;
            mD = mDc + ek * cn + 1e-9 * fabs(eps) + 1e-30;
            mL = __builtin_inf();
        }
        o.f[0] = (float)P.f[0]; o.f[1] = (float)P.f[1]; o.f[2] = (float)P.f[2];
        o.f[3] = (float)a0; o.f[4] = (float)a1v; o.f[5] = (float)a2v;
        ok = ok && cls_fin(mD) && mD < 1e30 && (f32cloud || (cls_fin(mL) && mL < 1e30)) && cls_fin(beta);
        if (ok) {
            const double wD = 2.0 * mD, iD = 1.0 / wD, eDlo = eps - 0.5 * wD;
            const double wL = 2.0 * mL, iL = f32cloud ? 0.0 : 1.0 / wL;
            o.f[6] = (float)(cp * iD); o.f[7] = (float)(sp * iD);
            o.f[8] = (float)(eDlo * iD);
            o.f[9] = (float)(-sgn * cp * iL); o.f[10] = (float)(-sgn * sp * iL); o.f[11] = (float)(cosa * iL);
            if (dbg4 != nullptr) { dbg4[0] = 0.0; dbg4[1] = wL; dbg4[2] = eDlo; dbg4[3] = wD; }
            for (int i = 6; i < 12; i++) ok = ok && fabs((double)o.f[i]) < 1e30;
        }
        o.f[12] = cls_up(beta);     // next to the axis: rho^2 <= alpha |w|^2 + beta -> undecided (alpha = RH_CONE_ALPHA)
        const double e = band_ok ? (eps / cn) * (1.0 + 1e-9) + ek : 0.0;
        const bool box_ok = band_ok && cls_fin(e) && cls_fin(kk) && fabs(kk) <= 1e6 && cls_fin(beta);
        if (box_ok) {
            // box: the same closed form at the centre of the box, the band widened by the radius of the box (the
            // distance is 1-Lipschitz in p): half width (hr + eps + slack) / cn
            bx[0] = o.f[0]; bx[1] = o.f[1]; bx[2] = o.f[2];
            bx[3] = o.f[3]; bx[4] = o.f[4]; bx[5] = o.f[5];
            bx[6] = (float)kk;
            bx[7] = cls_up(1.0 / cn);
            bx[8] = cls_up((eps + slack64) / cn * (1.0 + 1e-9) + ek);
            bx[9] = cls_up(beta);
            // Float32 cloud: the exact test's frame degrades as 2^-24 / sin(angle to the axis) -- never skip a box whose
            // centre lies within ~0.03 rad of the axis (rho^2 <= alpha |t|^2)
            bx[10] = f32cloud ? 1e-3f : RH_CONE_ALPHA;
        }
    }
    if (!ok) o.f[RH_CLS_FLAG] = fnan;
    if (box != nullptr)
        for (int i = 0; i < RH_BOX_FIELDS; i++) box[(int64_t)i * bstride] = bx[i];
}

// binary32 box of a 64-point group from its binary64 box (centre c, half extents h): the half extents absorb the
// conversion of the centre and are rounded up; o = cx cy cz hx hy hz hr 0
__host__ __device__ inline void box_to_f32(const double c[3], const double h[3], float o[8])
{
    double h2 = 0;
    for (int k = 0; k < 3; k++) {
        const float cf = (float)c[k];
        const double hh = (h[k] + fabs(c[k] - (double)cf)) * (1.0 + 4.0 * RH_CLS_U) + 1e-37;
        const float hf = cls_up(hh);
        o[k] = cf;
        o[3 + k] = hf;
        h2 += (double)hf * (double)hf;
    }
    o[6] = cls_up(sqrt(h2));
    o[7] = 0.0f;
}

#ifdef __HIPCC__
#define WB4(cond) __builtin_amdgcn_ballot_w64(cond)

// ---- stage 1: may the group's box be skipped for this candidate?  lane = candidate (B = its culling record),
// the box is wave-uniform.  Every comparison is written so that NaN means "do not skip".
struct rh_box32 { float cx, cy, cz, hx, hy, hz, hr; };

// the cylinder's decision, host and device (rh_dbg_cylbox runs this very code).  SUPPORT = false: the two clauses that take the
// box for a ball, alone -- what the test was before the support clause, kept for the census of what the clause adds.
template <bool SUPPORT>
static __host__ __device__ __forceinline__ bool cyl_box_skip32(const float (&B)[RH_BOX_FIELDS], const rh_box32 &G)
{
    const float tx = G.cx - B[3], ty = G.cy - B[4], tz = G.cz - B[5];
    const float sd = __builtin_fmaf(B[2], tz, __builtin_fmaf(B[1], ty, B[0] * tx));
    const float qx = __builtin_fmaf(-B[0], sd, tx), qy = __builtin_fmaf(-B[1], sd, ty), qz = __builtin_fmaf(-B[2], sd, tz);
    const float rho2 = __builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, qx * qx));
    const float lip = B[8] * G.hr * 1.000001f;
    const float X = B[6] + lip, Y = B[7] - lip;
    const float X2 = X > 0.0f ? X * X * 1.000001f : (X <= 0.0f ? 0.0f : X);   // NaN stays NaN
    bool skip = (rho2 * 0.999999f > X2) | ((Y > 0.0f) & (rho2 * 1.000001f < Y * Y));
    if (SUPPORT) {
        // rho >= rho_c - sum |g_k| h_k / rho_c over the box, g = q - a (a . q): "The cylinder's box by its support" above
        const float aq = __builtin_fmaf(B[2], qz, __builtin_fmaf(B[1], qy, B[0] * qx));
        const float gx = __builtin_fmaf(-B[0], aq, qx), gy = __builtin_fmaf(-B[1], aq, qy), gz = __builtin_fmaf(-B[2], aq, qz);
        const float s = __builtin_fmaf(__builtin_fabsf(gz), G.hz, __builtin_fmaf(__builtin_fabsf(gy), G.hy, __builtin_fabsf(gx) * G.hx));
        const float w = __builtin_fmaf(rho2, 0.999999f, -s);
        skip |= (w > 0.0f) & (w * w > B[9] * rho2);
    }
    return skip;
}

// the cone's decision, host and device (rh_dbg_conebox runs this very code): "surely outside the widened band", positive
// comparisons only.  The closed form at the centre of the box (h, rho2 against the band k h +- e, e widened by the half
// diagonal); a centre inside the axis guard (rho2 <= alpha |t|^2 + beta) is never skipped; on the far nappe the whole band lies
// below rho = 0 (hi <= 0), and the inner clause needs a band that starts above the axis (lo > 0).
static __host__ __device__ __forceinline__ bool cone_box_skip32(const float (&B)[RH_BOX_FIELDS], const rh_box32 &G)
{
    const float tx = G.cx - B[0], ty = G.cy - B[1], tz = G.cz - B[2];
    const float tt = __builtin_fmaf(tz, tz, __builtin_fmaf(ty, ty, tx * tx));
    const float h = __builtin_fmaf(tz, B[5], __builtin_fmaf(ty, B[4], tx * B[3]));
    const float rho2 = __builtin_fmaf(-h, h, tt);
    const float s2 = __builtin_fmaf(B[10], tt, B[9]);
    const float e = __builtin_fmaf(G.hr, B[7], B[8]) * 1.000001f;
    const float uu = B[6] * h;
    const float lo = uu - e, hi = uu + e;
    const float hi2 = __builtin_fmaf(hi, hi, s2), lo2 = __builtin_fmaf(lo, lo, -s2);
    return (rho2 > s2) & ((hi <= 0.0f) | (rho2 > hi2) | ((lo > 0.0f) & (rho2 < lo2)));
}

template <int KIND>
static __device__ __forceinline__ bool box_skip32(const float (&B)[RH_BOX_FIELDS], const rh_box32 &G)
{
    if (KIND == RH_PLANE) {
        const float d = __builtin_fmaf(B[2], G.cz, __builtin_fmaf(B[1], G.cy, __builtin_fmaf(B[0], G.cx, B[3])));
        const float ext = __builtin_fmaf(__builtin_fabsf(B[2]), G.hz, __builtin_fmaf(__builtin_fabsf(B[1]), G.hy, __builtin_fmaf(__builtin_fabsf(B[0]), G.hx, B[4])));
        return __builtin_fabsf(d) > ext;
    }
    if (KIND == RH_SPHERE) {
        const float ax = __builtin_fabsf(G.cx - B[0]), ay = __builtin_fabsf(G.cy - B[1]), az = __builtin_fabsf(G.cz - B[2]);
        const float nx = fmaxf(ax - G.hx, 0.0f), ny = fmaxf(ay - G.hy, 0.0f), nz = fmaxf(az - G.hz, 0.0f);
        const float fx = ax + G.hx, fy = ay + G.hy, fz = az + G.hz;
        const float dmin2 = __builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx));
        const float dmax2 = __builtin_fmaf(fz, fz, __builtin_fmaf(fy, fy, fx * fx)) * 1.000001f;
        return (dmin2 * 0.999999f > B[3]) | (dmax2 < B[4]);
    }
    if (KIND == RH_CYLINDER) return cyl_box_skip32<true>(B, G);
    return cone_box_skip32(B, G);
}

// ---- The classifier's value of a (candidate, point) pair: u = max(ua, ub), the scaled "outsideness" of the two tests --
// ua = (threshold_lo - quantity) / width for the test that wants its quantity large (the normal's cosine), (quantity -
// threshold_lo) / width for the one that wants it small (the distance), widths = 2 x margin:
//     u < 0  (sign bit set)   both tests pass by more than their margins: SURELY an inlier
//     0 <= u <= 1             some test is within its margin and none fails surely: UNDECIDED -> the exact test
//     u > 1                   some test fails by more than its margin: surely not
// so that the 64-point loops of the score kernel (score4.hip) keep the books with ONE instruction per point and no compare:
// they evaluate u' = 2 u, whose top two bits hold the verdict, and shift both into the pair's books with a v_alignbit_b32
// ("Two-bit books" at the end of this file).  Rounds 4 to 11 shifted the sign bit of u alone and kept a running UNSIGNED
// minimum over the bit patterns of the u beside it (v_min3_u32, two points per instruction), which ended <= bits(1.0f) iff
// SOME point was undecided -- and a second evaluation of the classifier, lane = point, then had to find out which.
// (Measured on this GPU, tools/ubench/count_seq.hip: v_cmp / v_cndmask / v_addc / v_min_f32 hold the issue port 4.2 cycles
// each, fma / add / mul 2.3-2.9; round 3's t = min(a, b) with `count += t > 1/2` and a running minimum of |t| cost 14.6
// cycles per point beside the arithmetic, the form with the minimum 10.5.)  u = -0 counts as surely-in: it stands for a test
// passed by exactly its margin, and the margins carry a factor RH_CLS_SAFETY over the first-order bound.
static __host__ __device__ __forceinline__ void cls_plane_ab(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz, float &ua, float &ub)
{
    ua = __builtin_fmaf(C.f[2], nz, __builtin_fmaf(C.f[1], ny, __builtin_fmaf(C.f[0], nx, C.f[3])));
    const float d = __builtin_fmaf(C.f[6], z, __builtin_fmaf(C.f[5], y, __builtin_fmaf(C.f[4], x, C.f[7])));
    ub = __builtin_fabsf(d) - C.f[8];
}
static __host__ __device__ __forceinline__ float cls_plane_u(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz)
{
    float a, b;
    cls_plane_ab(C, x, y, z, nx, ny, nz, a, b);
    return fmaxf(a, b);
}

// ---- sphere / cylinder: the same u = max(ua, ub) from the scaled record, in the squared quantities n2 = |q|^2 and qn |qn|
// ("Round kinds without a square root" above).  Host and device: the kernel's point loops (with a doubled record and
// half = 1: cls_u2), the audits, rh_dbg_cls_round and rh_dbg_cls_u2 run this one statement.
template <int KIND>
static __host__ __device__ __forceinline__ void cls_round_ab(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz, float &ua, float &ub,
                                                            const float half = 0.5f)
{
    float qx, qy, qz;
    constexpr int b = KIND == RH_SPHERE ? 3 : 6;
    if (KIND == RH_SPHERE) {
        qx = x - C.f[0]; qy = y - C.f[1]; qz = z - C.f[2];
    } else {
        const float tx = x - C.f[3], ty = y - C.f[4], tz = z - C.f[5];
        const float sd = __builtin_fmaf(C.f[2], tz, __builtin_fmaf(C.f[1], ty, C.f[0] * tx));
        qx = __builtin_fmaf(-C.f[0], sd, tx); qy = __builtin_fmaf(-C.f[1], sd, ty); qz = __builtin_fmaf(-C.f[2], sd, tz);
    }
    // (nothing is divided: a point ON the centre / axis has n2 = 0, and ua > 1 says surely out as the exact test's NaN does)
    const float n2 = __builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, qx * qx));
    const float qn = __builtin_fmaf(qz, nz, __builtin_fmaf(qy, ny, qx * nx));
    ua = __builtin_fmaf(__builtin_fabsf(n2 - C.f[b]), C.f[b + 1], C.f[b + 2]);
    ub = __builtin_fmaf(qn * __builtin_fabsf(qn), C.f[b + 3], __builtin_fmaf(n2, C.f[b + 4], half));   // (mv / Wv = 1/2: no field; 1 with a doubled record, cls_double)
}
template <int KIND>
static __host__ __device__ __forceinline__ float cls_round_u(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz, const float half = 0.5f)
{
    float a, b;
    cls_round_ab<KIND>(C, x, y, z, nx, ny, nz, a, b, half);
    return fmaxf(a, b);
}

// ---- cone: the same u = max(ua, ub).  The reference builds a frame per point (project2cone, cone.jl:68-85): with
// w = p - apex = h a^ + rho e_rho (a^ the unit axis, e_rho the unit radial direction, phi^ = a^ x e_rho)
//     rot_ax = normalize(axis x normalize(-w)) = -phi^,   comp_n = normalize(axis x rot_ax) = e_rho,
//     current_normal = normalize(R(rot_ax, -opang/2) comp_n) = (c e_rho + s (rot_ax x comp_n)) / |(c, s)| = c' e_rho + s' a^
// so dist = dot(-current_normal, apex - p) = -(c' rho + s' h) and the normal's cosine is c' (q . n) / rho + s' (a^ . n).
// ua = (|D| - eD_lo) / wD with D = c' rho + s' h;  ub = 1/2 - L / wL with L = sgn (c' q . n + s' rho a^ . n) - cos(alpha) rho
// (the angle test multiplied through by rho > 0: its margin is absolute, nothing is divided by a small rho).  Next to the
// axis the reference's frame is ill-conditioned (and NaN on it): u = 1/2, undecided, the exact test answers.
static __device__ __forceinline__ void cls_cone_ab(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz, float &ua, float &ub,
                                                   bool &near_axis)
{
    const float wx = x - C.f[0], wy = y - C.f[1], wz = z - C.f[2];
    const float h = __builtin_fmaf(wz, C.f[5], __builtin_fmaf(wy, C.f[4], wx * C.f[3]));
    const float qx = __builtin_fmaf(-C.f[3], h, wx), qy = __builtin_fmaf(-C.f[4], h, wy), qz = __builtin_fmaf(-C.f[5], h, wz);
    const float n2 = __builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, qx * qx));
    const float rho = n2 * __builtin_amdgcn_rsqf(n2);
    const float D = __builtin_fmaf(C.f[6], rho, C.f[7] * h);
    ua = __builtin_fabsf(D) - C.f[8];
    const float qn = __builtin_fmaf(qz, nz, __builtin_fmaf(qy, ny, qx * nx));
    const float an = __builtin_fmaf(C.f[5], nz, __builtin_fmaf(C.f[4], ny, C.f[3] * nx));
    ub = __builtin_fmaf(qn, C.f[9], __builtin_fmaf(rho, __builtin_fmaf(an, C.f[10], C.f[11]), 0.5f));
    const float tt = __builtin_fmaf(h, h, n2);
    near_axis = !(n2 > __builtin_fmaf(RH_CONE_ALPHA, tt, C.f[12]));   // (NaN -> near; alpha is the same for every cone)
}
static __device__ __forceinline__ float cls_cone_u(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz)
{
    float a, b;
    bool near_axis;
    cls_cone_ab(C, x, y, z, nx, ny, nz, a, b, near_axis);
    return near_axis ? 0.5f : fmaxf(a, b);
}
// what the books say of a u (score kernel, audits)
static __device__ __forceinline__ bool cls_sure(float u) { return (__builtin_bit_cast(uint32_t, u) >> 31) != 0; }
static __device__ __forceinline__ bool cls_undecided(float u) { return __builtin_bit_cast(uint32_t, u) <= 0x3f800000u; }   // 0 <= u <= 1

// ---- Two-bit books (plane, sphere, cylinder: the point loops of score4_batch).  The kernel evaluates u' = 2 u: the record
// fields that enter u linearly are doubled in registers once per batch (cls_double; the records in memory, the audits and
// every other caller keep u) and the inline 1/2 of cls_round_ab becomes 1.  Doubling commutes with every rounding of the
// chain (powers of two; below the normal range a partial result may differ in its last place, 2^-149 of a quantity whose
// margin is of order 1, and a subnormal u' keeps its sign, which is all the books read of it; overflow: cls_make keeps every
// product below 2^120).  The verdict is then in the TOP TWO BITS of u':
//     sign set                    u' < 0 (or -0)          surely an inlier
//     sign clear, bit 30 clear    0 <= u' < 2             undecided -> the exact test
//     sign clear, bit 30 set      u' >= 2                 surely out (u = 1 exactly too: the margins say so; a NaN with a
//                                                         clear sign as well -- none arrives: exact-only pairs ignore the books)
// One v_alignbit_b32(w, bits(u'), 30) per point shifts both bits into a word from the right: 16 points per word, four words
// per pair, and no running minimum beside them.  Layout: word q holds the points 16 q .. 16 q + 15 in push order; after its
// 16 pushes point 16 q + j has its sign bit at bit 31 - 2 j and its bit 30 at bit 30 - 2 j (the first point on top).
// Host and device run these very statements (rh_dbg_books2).
template <int KIND>
static __host__ __device__ __forceinline__ void cls_double(rh_cls &C)
{
    constexpr int lo = KIND == RH_PLANE ? 0 : (KIND == RH_SPHERE ? 4 : 7), hi = KIND == RH_PLANE ? 9 : (KIND == RH_SPHERE ? 8 : 11);
#pragma unroll
    for (int f = lo; f < hi; f++) C.f[f] = C.f[f] + C.f[f];
}
// u' of a point by the doubled record (C: after cls_double<KIND>)
template <int KIND>
static __host__ __device__ __forceinline__ float cls_u2(const rh_cls &C, float x, float y, float z, float nx, float ny, float nz)
{
    if (KIND == RH_PLANE) return cls_plane_u(C, x, y, z, nx, ny, nz);
    return cls_round_u<KIND == RH_PLANE ? RH_SPHERE : KIND>(C, x, y, z, nx, ny, nz, 1.0f);
}
static __host__ __device__ __forceinline__ uint32_t books2_push(uint32_t w, float u2)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, u2);
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbit(w, b, 30);
#else
    return (w << 2) | (b >> 30);
#endif
}
constexpr uint32_t RH_BOOKS2_SIGN = 0xAAAAAAAAu;   // the sign bits of a word's 16 points
// points surely in, over the pair's four words
static __host__ __device__ __forceinline__ int books2_sure_count(const uint32_t (&w)[4])
{
    return (__builtin_popcount(w[0] & RH_BOOKS2_SIGN) + __builtin_popcount(w[1] & RH_BOOKS2_SIGN)) +
           (__builtin_popcount(w[2] & RH_BOOKS2_SIGN) + __builtin_popcount(w[3] & RH_BOOKS2_SIGN));
}
// a word's undecided points, at their sign bits' places: both bits clear
static __host__ __device__ __forceinline__ uint32_t books2_und_bits(uint32_t w) { return ~(w | (w << 1)) & RH_BOOKS2_SIGN; }
static __host__ __device__ __forceinline__ bool books2_any_undecided(const uint32_t (&w)[4])
{
    return (((books2_und_bits(w[0]) | books2_und_bits(w[1])) | books2_und_bits(w[2])) | books2_und_bits(w[3])) != 0u;
}
// the 16 sign-place bits of a word (x & RH_BOOKS2_SIGN == x) in point order: point j of the word at bit j
static __host__ __device__ __forceinline__ uint32_t books2_compress(uint32_t x)
{
    x = __builtin_bitreverse32(x);                 // point j at bit 2 j
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    return (x | (x >> 8)) & 0x0000ffffu;
}
// the pair's undecided / surely-in points as 64-bit words in point order (bit p = point p of the group)
static __host__ __device__ __forceinline__ uint64_t books2_und64(const uint32_t (&w)[4])
{
    const uint32_t lo = books2_compress(books2_und_bits(w[0])) | (books2_compress(books2_und_bits(w[1])) << 16);
    const uint32_t hi = books2_compress(books2_und_bits(w[2])) | (books2_compress(books2_und_bits(w[3])) << 16);
    return ((uint64_t)hi << 32) | lo;
}
static __host__ __device__ __forceinline__ uint64_t books2_sure64(const uint32_t (&w)[4])
{
    const uint32_t lo = books2_compress(w[0] & RH_BOOKS2_SIGN) | (books2_compress(w[1] & RH_BOOKS2_SIGN) << 16);
    const uint32_t hi = books2_compress(w[2] & RH_BOOKS2_SIGN) | (books2_compress(w[3] & RH_BOOKS2_SIGN) << 16);
    return ((uint64_t)hi << 32) | lo;
}

// ---- Books in place (counts-only launches).  Nothing behind the point loops needs the undecided bits of a pair in point order:
// the ring entry names its point itself.  The words' undecided bits sit at the sign places (odd bits), so two words interleave
// into one without a compression: lo = U0 | (U1 >> 1), hi = U2 | (U3 >> 1) with Uq = books2_und_bits(w[q]) -- bit 31 - 2 j of
// a half holds point j of its first word, bit 30 - 2 j point 16 + j of its second.  Bit L of the 64-bit word therefore stands
// for point books2_point_of_bit(L), a fixed permutation of 0 .. 63 (a lane constant in the kernel), and popcounts, ranks and
// "any" read the same off either form.  Host and device run these very statements (rh_dbg_books2_inplace).
static __host__ __device__ __forceinline__ uint64_t books2_und64_inplace(const uint32_t (&w)[4])
{
    const uint32_t lo = books2_und_bits(w[0]) | (books2_und_bits(w[1]) >> 1);
    const uint32_t hi = books2_und_bits(w[2]) | (books2_und_bits(w[3]) >> 1);
    return ((uint64_t)hi << 32) | lo;
}
static __host__ __device__ __forceinline__ int books2_point_of_bit(int L)
{
    return (L & 32) + ((~L & 1) << 4) + ((31 - (L & 31)) >> 1);
}
// a point-ordered word (bit p = point p: the group's enabled word) in the books' order -- the inverse of books2_compress per
// 16 points; for the rare pairs that ignore their books (exact-only records, tiles with a non-finite value)
static __host__ __device__ __forceinline__ uint32_t books2_expand(uint32_t x)
{
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;              // point j at bit 2 j
    return __builtin_bitreverse32(x);              // point j at bit 31 - 2 j
}
static __host__ __device__ __forceinline__ uint64_t books2_deposit64(uint64_t v)
{
    const uint32_t a = (uint32_t)v, b = (uint32_t)(v >> 32);
    const uint32_t lo = books2_expand(a & 0xffffu) | (books2_expand(a >> 16) >> 1);
    const uint32_t hi = books2_expand(b & 0xffffu) | (books2_expand(b >> 16) >> 1);
    return ((uint64_t)hi << 32) | lo;
}
#endif   // __HIPCC__

}  // namespace rh4
