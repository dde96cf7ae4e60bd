// assign_device.h -- the per-point VALUE functions of the label kernel (assign.hip): where score_device.h's tests return
// the wave's mask of compatible lanes, these return the lane's claim and leave d, the distance side of the test, for the
// lanes that claim.  Same numerics contract and the same operation order, line for line, as test_plane / test_sphere /
// test_cylinder / cone_frame there (IEEE binary64, no contraction, 1 / sqrt and multiply for normalize), and the same
// wave-level early-outs: the cheap half first, a ballot, and the other half skipped when no lane of the wave passes --
// the same bits as evaluating both.  Every lane of the wave must be in the call (the ballots say so).
// NRM = false: no normals, the distance half alone decides.
#pragma once

#include "score_device.h"

namespace rhasg {

using rhdev::cone_frame;

// plane: compatiblesPlane shapes/plane.jl:114-130; d = |dot(o_z, p - point)|, t = dot(normal, n)
template <bool NRM>
static __device__ __forceinline__ bool claim_plane(const rh_prep &P, double px, double py, double pz, double nx, double ny,
                                                   double nz, double eps, double cosa, double &d)
{
    bool tn = true;
    if (NRM) {
        const double t = (P.f[3] * nx + P.f[4] * ny) + P.f[5] * nz;
        tn = t > cosa;
        if (WB(tn) == 0) return false;
    }
    const double vx = px - P.f[0], vy = py - P.f[1], vz = pz - P.f[2];
    d = fabs((P.f[6] * vx + P.f[7] * vy) + P.f[8] * vz);
    return tn && d < eps;
}

// sphere: compatiblesSphere shapes/sphere.jl:144-172; d = |norm(p - o) - R|, t = sgn * dot(normalize(p - o), n)
template <bool NRM>
static __device__ __forceinline__ bool claim_sphere(const rh_prep &P, double px, double py, double pz, double nx, double ny,
                                                    double nz, double eps, double cosa, double &d)
{
    const double dx = px - P.f[0], dy = py - P.f[1], dz = pz - P.f[2];
    const double nr = sqrt((dx * dx + dy * dy) + dz * dz);
    d = fabs(nr - P.f[3]);
    const bool td = d < eps;
    if (!NRM) return td;
    if (WB(td) == 0) return false;
    const double inv = 1.0 / nr;
    const double ux = inv * dx, uy = inv * dy, uz = inv * dz;
    const double dt = (ux * nx + uy * ny) + uz * nz;
    return td && P.f[4] * dt > cosa;
}

// cylinder: compatiblesCylinder shapes/cylinder.jl:194-221; d = |norm(curr_norm) - R|, t = sgn * dot(normalize(curr_norm), n)
template <bool NRM>
static __device__ __forceinline__ bool claim_cylinder(const rh_prep &P, double px, double py, double pz, double nx, double ny,
                                                      double nz, double eps, double cosa, double &d)
{
    const double ax = P.f[0], ay = P.f[1], az = P.f[2];
    const double cx = P.f[3], cy = P.f[4], cz = P.f[5];
    const double tx = px - cx, ty = py - cy, tz = pz - cz;
    const double sd = (ax * tx + ay * ty) + az * tz;
    const double qx = (px - ax * sd) - cx, qy = (py - ay * sd) - cy, qz = (pz - az * sd) - cz;
    const double nr = sqrt((qx * qx + qy * qy) + qz * qz);
    d = fabs(nr - P.f[6]);
    const bool td = d < eps;
    if (!NRM) return td;
    if (WB(td) == 0) return false;
    const double inv = 1.0 / nr;
    const double ux = inv * qx, uy = inv * qy, uz = inv * qz;
    const double dt = (ux * nx + uy * ny) + uz * nz;
    return td && P.f[7] * dt > cosa;
}

// cone: compatiblesCone shapes/cone.jl:132-153 over project2cone :68-85; d = |dist|, t = sgn * dot(current_normal, n)
// (one frame gives both sides: nothing to skip)
template <bool NRM>
static __device__ __forceinline__ bool claim_cone(const rh_prep &P, double px, double py, double pz, double nx, double ny,
                                                  double nz, double eps, double cosa, double &d)
{
    double dist, dt;
    cone_frame(P, px, py, pz, nx, ny, nz, dist, dt);
    d = fabs(dist);
    return d < eps && (!NRM || P.f[8] * dt > cosa);
}

}  // namespace rhasg
