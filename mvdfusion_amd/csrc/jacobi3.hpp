// The cyclic Jacobi eigen-decomposition of a symmetric 3 x 3 in fp64 that normals.hip (a point's covariance) and meshsimplify.hip (a
// cluster's quadric) share: one copy, so both restate the same sweep order (include/mvd_hip.h: mvd_point_normals has the rule).
#pragma once
#include "fusion_common.hpp"

namespace {

#define PN_HD __host__ __device__ __forceinline__

constexpr double kPnThetaBig = 1e150;                 // above it theta^2 + 1 == theta^2 in fp64 (csrc/align.hip: kAlThetaBig)

// Cyclic Jacobi on a symmetric 3 x 3: A -> diagonal, the eigenvectors in the columns of V.  Compile-time subscripts throughout.
PN_HD void pn_jacobi3(double A[3][3], double V[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < MVD_NORMALS_SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p][q];
        if (apq != 0.0) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq), at = fabs(theta);
          double t = at > kPnThetaBig ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
          if (theta < 0.0) t = -t;
          const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - sn * akq, A[k][q] = sn * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - sn * aqk, A[q][k] = sn * apk + c * aqk;
          }
          A[p][q] = A[q][p] = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - sn * vkq, V[k][q] = sn * vkp + c * vkq;
          }
        }
      }
  }
}

}  // namespace
