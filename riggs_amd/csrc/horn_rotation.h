// Horn's closed-form absolute orientation (Horn 1987) as a rotation fit: shared by the ARAP regulariser (node_reg.hip) and the ARAP
// handle editor (arap.hip), which must fit the same rotation to the same covariance.
#pragma once
#include "common.h"

namespace riggs {

// The rotation that maximises tr(R S), S = sum_n src_n tgt_n^T: the unit quaternion of the largest eigenvalue of Horn's 4x4
// matrix (cyclic Jacobi, fp64).  For a proper optimum this is estimate_rotation's V U^T with the Kabsch flip; S = 0 gives I.
__device__ inline void nr_horn_rotation(const double S[9], double R[9]) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, dia = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (p != q) off += A[p][q] * A[p][q];
        else dia += A[p][q] * A[p][q];
      }
    if (off <= 1e-30 * dia || off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq != 0.0) {
          const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double kp = A[k][p], kq = A[k][q];
            A[k][p] = c * kp - s * kq; A[k][q] = s * kp + c * kq;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double pk = A[p][k], qk = A[q][k];
            A[p][k] = c * pk - s * qk; A[q][k] = s * pk + c * qk;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double kp = V[k][p], kq = V[k][q];
            V[k][p] = c * kp - s * kq; V[k][q] = s * kp + c * kq;
          }
        }
      }
  }
  // the largest eigenvalue's vector, the lowest index on ties
  double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > best) { best = A[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
  const double n = sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
}

}  // namespace riggs
