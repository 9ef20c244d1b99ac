// rgc_cov.h -- what a neighbourhood's second moment becomes: the symmetric 3x3 device helpers (one Jacobi rotation, the eigen-decomposition,
// the inverse) and the RegularizationMethod applied to a covariance, shared by the translation units that estimate covariances:
// rgc_kernels.hip (cov6_of behind the exact kNN, the PLANE normal, the solve) and rgc_rbf.hip (k_rbf_cov6); inv_sym3 is also the one inverse of
// the Mahalanobis terms of rgc_ndt.hip, rgc_gicp.hip and rgc_gicp_mp.hip (their other shared pieces: rgc_terms.h).  Everything here is
// __forceinline__, as in rgc_nn.h: each kernel inlines its own copy.  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace rgck {

// One Jacobi rotation in the (P,Q) plane, R = the third index.  Same rotation as the textbook two-sided product
// A <- G^T A G (t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq)) written in its closed
// form: only the five entries that change are touched, and t comes from ONE division and ONE square root
// (t = 2 |a_pq| sgn(theta) / (|d| + sqrt(d^2 + 4 a_pq^2)), d = a_qq - a_pp) -- fp64 divisions and roots are ~15 VALU ops each
// and this routine runs once per point of the map.
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&V)[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double d = A[Q][Q] - A[P][P];
  const bool pos = (d == 0.0) || ((d > 0.0) == (apq > 0.0));  // sign of theta, with theta = 0 counted positive
  const double t = (pos ? 2.0 : -2.0) * fabs(apq) / (fabs(d) + sqrt(d * d + 4.0 * apq * apq));
  const double c = rsqrt(t * t + 1.0), s = t * c;
  const double tap = t * apq;
  A[P][P] -= tap;
  A[Q][Q] += tap;
  A[P][Q] = 0.0;
  A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
  A[R][P] = nrp; A[P][R] = nrp;
  A[R][Q] = nrq; A[Q][R] = nrq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

__device__ __forceinline__ bool inv_sym3(const double S[6], double M[6]) {
  const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  if (det == 0.0) return false;
  const double id = 1.0 / det;
  M[0] = c00 * id; M[1] = c01 * id; M[2] = c02 * id;
  M[3] = (a * f - c * c) * id; M[4] = (b * c - a * e) * id; M[5] = (a * d - b * b) * id;
  return true;
}

// all three eigenpairs of a symmetric 3x3 (same cyclic Jacobi as min_eigenvector); ord[] = indices by DESCENDING eigenvalue
__device__ __forceinline__ void eig3_sym(const double S[6], double ev[3], double (&V)[3][3], int ord[3]) {
  double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) V[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-40 * diag || off == 0.0) break;
    jacobi_rot<0, 1, 2>(A, V);
    jacobi_rot<0, 2, 1>(A, V);
    jacobi_rot<1, 2, 0>(A, V);
  }
  ev[0] = A[0][0]; ev[1] = A[1][1]; ev[2] = A[2][2];
  ord[0] = 0; ord[1] = 1; ord[2] = 2;
  for (int i = 0; i < 2; i++)
    for (int j = i + 1; j < 3; j++)
      if (ev[ord[j]] > ev[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
}

// fast_gicp_impl.hpp:264-293 (fast_vgicp_cuda.cu:210,218 for the RBF moment): the selected regularisation of the covariance S -> C, both
// {xx, xy, xz, yy, yz, zz}.  JacobiSVD of a symmetric positive semi-definite matrix is its eigen-decomposition (U = V), which is what is
// computed here; method = rgc_regularization_method (0 NONE, 1 MIN_EIG, 2 NORMALIZED_MIN_EIG, 3 PLANE, 4 FROBENIUS).
__device__ __forceinline__ void regularize6(const double (&S)[6], int method, double (&C)[6]) {
  if (method == 0) {                                                       // NONE, :264-265
    for (int a = 0; a < 6; a++) C[a] = S[a];
  } else if (method == 4) {                                                // FROBENIUS, :266-271: (C_inv / |C_inv|_F)^-1 = |C_inv|_F (S + lambda I)
    const double R[6] = {S[0] + 1e-3, S[1], S[2], S[3] + 1e-3, S[4], S[5] + 1e-3};
    double Ci[6];
    if (!inv_sym3(R, Ci)) { for (int a = 0; a < 6; a++) Ci[a] = 0.0; }
    const double nrm = sqrt(Ci[0] * Ci[0] + Ci[3] * Ci[3] + Ci[5] * Ci[5] + 2.0 * (Ci[1] * Ci[1] + Ci[2] * Ci[2] + Ci[4] * Ci[4]));
    for (int a = 0; a < 6; a++) C[a] = nrm * R[a];
  } else {
    double ev[3], V[3][3];
    int ord[3];
    eig3_sym(S, ev, V, ord);                                                  // :273, singular values in descending order
    double val[3];
    const double smax = ev[ord[0]];
    for (int r = 0; r < 3; r++) {
      const double sv = ev[ord[r]];
      if (method == 3) val[r] = r < 2 ? 1.0 : 1e-3;                        // PLANE, :280-282
      else if (method == 1) val[r] = sv > 1e-3 ? sv : 1e-3;                // MIN_EIG, :283-285
      else { const double t = sv / smax; val[r] = t > 1e-3 ? t : 1e-3; }      // NORMALIZED_MIN_EIG, :286-289
    }
    for (int a = 0; a < 6; a++) C[a] = 0.0;
    for (int r = 0; r < 3; r++) {                                             // U diag(values) V^T, :293
      const int c = ord[r];
      const double v0 = V[0][c], v1 = V[1][c], v2 = V[2][c], w = val[r];
      C[0] += w * v0 * v0; C[1] += w * v0 * v1; C[2] += w * v0 * v2; C[3] += w * v1 * v1; C[4] += w * v1 * v2; C[5] += w * v2 * v2;
    }
  }
}

}  // namespace rgck
