// global_hyp.h -- the host side of rh_register_global's hypotheses (include/ransac_hip.h, steps 2 to 4): is a triple of
// correspondences valid, the frames of its two triangles, and the transform between them.  Plain C++ without the HIP
// runtime, so tests/native/global_hyp_check.cpp runs it under the sanitizers; it must be compiled with -ffp-contract=off
// like everything else, since the definition fixes every operation.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ransac_hip.h"

namespace {

struct GlobHyp {
    double R[9], t[3];
};

inline double gl_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

inline void gl_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// the frame of (x0, x1, x2), columns e1, e2, e3 in F[k][0 .. 2]; false: it does not exist (step 3)
inline bool gl_frame(const double *x0, const double *x1, const double *x2, double F[3][3])
{
    const double h[3] = { x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2] };
    const double hh = gl_dot(h, h);
    if (!(hh > 0.0)) return false;
    const double hl = sqrt(hh);
    const double e1[3] = { h[0] / hl, h[1] / hl, h[2] / hl };
    const double w[3] = { x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2] };
    double gv[3], e2[3];
    gl_cross(e1, w, gv);
    const double g2 = gl_dot(gv, gv);
    if (!(g2 > 0.0)) return false;
    const double gl = sqrt(g2);
    const double e3[3] = { gv[0] / gl, gv[1] / gl, gv[2] / gl };
    gl_cross(e3, e1, e2);
    for (int k = 0; k < 3; k++) { F[k][0] = e1[k]; F[k][1] = e2[k]; F[k][2] = e3[k]; }
    return true;
}

// the hypothesis of the triple (a, b, d) of pairs; false: the trial is not valid (steps 2 to 4)
inline bool gl_hypothesis(const double *pairs, int64_t a, int64_t b, int64_t d, const rh_global_params &p, GlobHyp &out)
{
    if (a == b || a == d || b == d) return false;
    const double *q[3] = { pairs + 6 * a, pairs + 6 * b, pairs + 6 * d };
    const double *r[3] = { pairs + 6 * a + 3, pairs + 6 * b + 3, pairs + 6 * d + 3 };
    const double ee = p.edge_ratio * p.edge_ratio, mm = p.min_edge * p.min_edge;
    static const int ex[3] = { 0, 0, 1 }, ey[3] = { 1, 2, 2 };
    for (int s = 0; s < 3; s++) {
        const double *qx = q[ex[s]], *qy = q[ey[s]], *rx = r[ex[s]], *ry = r[ey[s]];
        const double dq[3] = { qx[0] - qy[0], qx[1] - qy[1], qx[2] - qy[2] };
        const double dr[3] = { rx[0] - ry[0], rx[1] - ry[1], rx[2] - ry[2] };
        const double lq = gl_dot(dq, dq), lr = gl_dot(dr, dr);
        if (!(lq >= ee * lr) || !(lr >= ee * lq) || !(lq >= mm)) return false;
    }
    double Fq[3][3], Fr[3][3];
    if (!gl_frame(q[0], q[1], q[2], Fq) || !gl_frame(r[0], r[1], r[2], Fr)) return false;
    double cq[3], cr[3];
    for (int k = 0; k < 3; k++) {
        cq[k] = ((q[0][k] + q[1][k]) + q[2][k]) / 3.0;
        cr[k] = ((r[0][k] + r[1][k]) + r[2][k]) / 3.0;
    }
    for (int k = 0; k < 3; k++)
        for (int l = 0; l < 3; l++) out.R[3 * k + l] = (Fr[k][0] * Fq[l][0] + Fr[k][1] * Fq[l][1]) + Fr[k][2] * Fq[l][2];
    for (int k = 0; k < 3; k++) out.t[k] = cr[k] - ((out.R[3 * k] * cq[0] + out.R[3 * k + 1] * cq[1]) + out.R[3 * k + 2] * cq[2]);
    return true;
}

}  // namespace
