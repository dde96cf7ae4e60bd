// jacobi3.h -- the cyclic Jacobi eigen-solver of a symmetric 3 x 3 matrix, shared by normals.hip (the covariance of a
// neighbourhood) and extent.hip (the scatter of a shape's points).  Plain binary64, no contraction: the same bits on every run.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

// one Jacobi rotation annihilating A[p][q] (Numerical Recipes' jacobi, written out for 3 x 3)
__device__ __forceinline__ void rh_jrot(double A[3][3], double V[3][3], int p, int q)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double app = A[p][p], aqq = A[q][q], g = 100.0 * fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { A[p][q] = A[q][p] = 0.0; return; }
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta
                                         : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p][p] = app - t * apq;
    A[q][q] = aqq + t * apq;
    A[p][q] = A[q][p] = 0.0;
    const int r = 3 - p - q;
    const double arp = A[r][p], arq = A[r][q];
    A[r][p] = A[p][r] = c * arp - s * arq;
    A[r][q] = A[q][r] = s * arp + c * arq;
    for (int i = 0; i < 3; i++) {
        const double vip = V[i][p], viq = V[i][q];
        V[i][p] = c * vip - s * viq;
        V[i][q] = s * vip + c * viq;
    }
}

// A -> diag(eigenvalues) (on A's diagonal), V's columns -> the eigenvectors; V must come in as the identity
__device__ __forceinline__ void rh_jacobi3(double A[3][3], double V[3][3])
{
    for (int sweep = 0; sweep < 32; sweep++) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
        rh_jrot(A, V, 0, 1);
        rh_jrot(A, V, 0, 2);
        rh_jrot(A, V, 1, 2);
    }
}
