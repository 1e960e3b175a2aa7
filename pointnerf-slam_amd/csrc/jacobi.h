// jacobi.h -- the one-sided (Hestenes) Jacobi SVD shared by the relative pose (relpose.hip: the essential
// matrix's decomposition, the DLT's null vector) and the ICP's Kabsch rotation (recon.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pnr {

// One-sided Jacobi: rotates the columns of A until they are orthogonal; A <- U S, V accumulates.
template <int N>
__device__ __forceinline__ void jacobi(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 20; ++sweep) {
    bool any = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        double al = 0.0, be = 0.0, g = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          al += A[i][p] * A[i][p];
          be += A[i][q] * A[i][q];
          g += A[i][p] * A[i][q];
        }
        if (fabs(g) > 2.3e-16 * sqrt(al * be)) {
          any = true;
          const double zeta = (be - al) / (2.0 * g);
          const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
            A[i][p] = c * ap - s * aq;
            A[i][q] = s * ap + c * aq;
            V[i][p] = c * vp - s * vq;
            V[i][q] = s * vp + c * vq;
          }
        }
      }
    if (!any) break;
  }
}

}  // namespace pnr
