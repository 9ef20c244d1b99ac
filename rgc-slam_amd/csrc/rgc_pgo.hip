// rgc_pgo.hip -- gfx950 kernels of the 4-DoF pose graph over the keyframe store's key poses: the mapping node's PoseGraphOptimize4DoF
// (src/RGC_mapping.cpp:2303-2466) with FourDOFError / AngleLocalParameterization (src/lidarFactor.hpp:490-595); citations are relative to
// rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).  Everything is fp64, nothing is contracted (-ffp-contract=off), no floating-point
// atomics: every sum runs in an order fixed by the graph alone, so H, g, the cost and the step are bit-identical from run to run.
//
//   Unknowns: 4 per position n of the selection, {yaw in DEGREES, tx, ty, tz}.  Edges: odometry edge e = n (n -> n + 1), e < N - 1, then the
// used loops in the caller's order.  The constant node keeps its four rows and columns, all zero (its Jacobians are zeroed in k_pgo_edges);
// the solve gives it the identity on the diagonal, so its step is exactly zero.
//
//   The damped system (H + clamp(diag H, 1e-6, 1e32) / radius) d = -g is solved directly, by nested dissection with a data-independent
// operation count: SEPARATORS (position 0, the constant node, every loop endpoint, every S-th position) cut the chain into block-tridiagonal
// segments that touch nothing but their two separators.  k_pgo_segments eliminates each segment's interior, one lane per segment (a block
// Cholesky, a 4x4 block per step, registers only), and leaves the Schur complement's contributions in slots of its own; k_pgo_dense adds them up in a fixed order
// into the separators' dense system, factors it (Cholesky, one workgroup) and solves it; k_pgo_backsub walks each segment back.  The launch
// boundary is the only synchronisation between workgroups.
#include "rgc_kernels.h"

namespace rgck {

namespace {

__device__ inline double pgo_normalize(double a) {  // NormalizeAngle, src/lidarFactor.hpp:490-499: one wrap at +-180
  if (a > 180.0) return a - 360.0;
  if (a < -180.0) return a + 360.0;
  return a;
}

// the diagonal block of node n as the solve sees it: damped, the identity on the constant node.  (k_pgo_segments never meets the constant node:
// it is a loop endpoint, so a separator, never a segment's interior -- the branch is a guard there; k_pgo_dense has the live copy of it.)
__device__ inline void pgo_load_damped(const double* __restrict__ D, int n, int fixed, double inv_radius, double A[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) A[k] = D[(size_t)n * 16 + k];
  if (n == fixed) {
#pragma unroll
    for (int k = 0; k < 16; k++) A[k] = (k % 5 == 0) ? 1.0 : 0.0;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) A[k * 5] += fmin(fmax(A[k * 5], 1e-6), 1e32) * inv_radius;
  }
}

// Cholesky factor L (row-major, lower) of a symmetric positive definite 4x4; false where a pivot is not positive
__device__ inline bool pgo_chol4(const double A[16], double L[16]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (j <= i) {
        double s = A[i * 4 + j];
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (k < j) s -= L[i * 4 + k] * L[j * 4 + k];
        if (i == j) {
          if (!(s > 0.0)) { ok = false; s = 1.0; }
          L[i * 4 + i] = sqrt(s);
        } else {
          L[i * 4 + j] = s / L[j * 4 + j];
        }
      } else {
        L[i * 4 + j] = 0.0;
      }
    }
  }
  return ok;
}
// Y = L^-1 B (transposed: L^-1 B^T), column by column; y = L^-1 v; x = L^-T v
__device__ inline void pgo_lsolve(const double L[16], const double B[16], bool transposed, double Y[16]) {
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      double s = transposed ? B[c * 4 + i] : B[i * 4 + c];
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k < i) s -= L[i * 4 + k] * Y[k * 4 + c];
      Y[i * 4 + c] = s / L[i * 4 + i];
    }
}
__device__ inline void pgo_lsolve_v(const double L[16], const double v[4], double y[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double s = v[i];
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < i) s -= L[i * 4 + k] * y[k];
    y[i] = s / L[i * 4 + i];
  }
}
__device__ inline void pgo_ltsolve_v(const double L[16], const double v[4], double x[4]) {
#pragma unroll
  for (int i = 3; i >= 0; i--) {
    double s = v[i];
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k > i) s -= L[k * 4 + i] * x[k];
    x[i] = s / L[i * 4 + i];
  }
}

// C = A B, C = A^T B, C = A B^T of 4x4 row-major blocks
__device__ inline void pgo_mm(const double A[16], const double B[16], double C[16]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double s = A[i * 4] * B[j];
#pragma unroll
      for (int k = 1; k < 4; k++) s += A[i * 4 + k] * B[k * 4 + j];
      C[i * 4 + j] = s;
    }
}
__device__ inline void pgo_mtm(const double A[16], const double B[16], double C[16]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double s = A[i] * B[j];
#pragma unroll
      for (int k = 1; k < 4; k++) s += A[k * 4 + i] * B[k * 4 + j];
      C[i * 4 + j] = s;
    }
}
__device__ inline void pgo_mmt(const double A[16], const double B[16], double C[16]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double s = A[i * 4] * B[j * 4];
#pragma unroll
      for (int k = 1; k < 4; k++) s += A[i * 4 + k] * B[j * 4 + k];
      C[i * 4 + j] = s;
    }
}
__device__ inline void pgo_mv(const double A[16], const double v[4], double o[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = ((A[i * 4] * v[0] + A[i * 4 + 1] * v[1]) + A[i * 4 + 2] * v[2]) + A[i * 4 + 3] * v[3];
}
__device__ inline void pgo_mtv(const double A[16], const double v[4], double o[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = ((A[i] * v[0] + A[4 + i] * v[1]) + A[8 + i] * v[2]) + A[12 + i] * v[3];
}

}  // namespace

// ---- edge terms: one lane per edge (FourDOFError, src/lidarFactor.hpp:557-595, analytic Jacobians) --------------------------------
// record of kPgoTerm doubles: r[4], g_i[4] = J_i^T r, g_j[4] = J_j^T r, A_ii[16] = J_i^T J_i, A_jj[16], A_ij[16] = J_i^T J_j (rows: the
// unknowns of i, columns: of j), 1/2 |r|^2, three unused
__global__ void __launch_bounds__(kPgoBlock) k_pgo_edges(const int* __restrict__ ij, const double* __restrict__ meas, int n_edges, const double* __restrict__ x,
                                                          int fixed, double* __restrict__ terms) {
  const int e = blockIdx.x * kPgoBlock + (int)threadIdx.x;
  if (e >= n_edges) return;
  const int i = ij[2 * e], j = ij[2 * e + 1];
  const double* m = meas + (size_t)e * 6;
  const double yaw_i = x[4 * i], yaw_j = x[4 * j];
  const double dt[3] = {x[4 * j + 1] - x[4 * i + 1], x[4 * j + 2] - x[4 * i + 2], x[4 * j + 3] - x[4 * i + 3]};
  // YawPitchRollToRotationMatrix (:517-533), degrees in
  const double y = yaw_i / 180.0 * M_PI, p = m[4] / 180.0 * M_PI, r = m[5] / 180.0 * M_PI;
  const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(r), sr = sin(r);
  double R[9];
  R[0] = cy * cp; R[1] = -sy * cr + cy * sp * sr; R[2] = sy * sr + cy * sp * cr;
  R[3] = sy * cp; R[4] = cy * cr + sy * sp * sr;  R[5] = -cy * sr + sy * sp * cr;
  R[6] = -sp;     R[7] = cp * sr;                 R[8] = cp * cr;
  double res[4], Ji[16], Jj[16];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    res[a] = ((R[a] * dt[0] + R[3 + a] * dt[1]) + R[6 + a] * dt[2]) - m[a];          // R^T (t_j - t_i) - m
    Ji[a * 4] = (M_PI / 180.0) * (-R[3 + a] * dt[0] + R[a] * dt[1]);                 // (pi/180) (dR/dyaw)^T (t_j - t_i)
    Jj[a * 4] = 0.0;
#pragma unroll
    for (int b = 0; b < 3; b++) { Ji[a * 4 + 1 + b] = -R[b * 3 + a]; Jj[a * 4 + 1 + b] = R[b * 3 + a]; }
  }
  res[3] = pgo_normalize(yaw_j - yaw_i - m[3]);
  Ji[12] = -1.0; Ji[13] = Ji[14] = Ji[15] = 0.0;
  Jj[12] = 1.0;  Jj[13] = Jj[14] = Jj[15] = 0.0;
  if (i == fixed) {
#pragma unroll
    for (int k = 0; k < 16; k++) Ji[k] = 0.0;
  }
  if (j == fixed) {
#pragma unroll
    for (int k = 0; k < 16; k++) Jj[k] = 0.0;
  }
  double* T = terms + (size_t)e * kPgoTerm;
#pragma unroll
  for (int k = 0; k < 4; k++) T[k] = res[k];
  pgo_mtv(Ji, res, T + 4);
  pgo_mtv(Jj, res, T + 8);
  double B[16];
  pgo_mtm(Ji, Ji, B);
#pragma unroll
  for (int k = 0; k < 16; k++) T[12 + k] = B[k];
  pgo_mtm(Jj, Jj, B);
#pragma unroll
  for (int k = 0; k < 16; k++) T[28 + k] = B[k];
  pgo_mtm(Ji, Jj, B);
#pragma unroll
  for (int k = 0; k < 16; k++) T[44 + k] = B[k];
  T[60] = 0.5 * (((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]) + res[3] * res[3]);
  T[61] = T[62] = T[63] = 0.0;
}

// ---- assembly: one lane per node gathers its diagonal block and gradient over its incident edges, in the order chain in (n - 1 -> n),
// chain out (n -> n + 1), then its loops in ascending loop order (inc: loop index * 2 + side, side 1 = the node is the edge's j) ----------
__global__ void __launch_bounds__(kPgoBlock) k_pgo_gather(const double* __restrict__ terms, int n_nodes, const int* __restrict__ inc_start,
                                                           const int* __restrict__ inc, double* __restrict__ D, double* __restrict__ g) {
  const int n = blockIdx.x * kPgoBlock + (int)threadIdx.x;
  if (n >= n_nodes) return;
  double a[20];
#pragma unroll
  for (int k = 0; k < 20; k++) a[k] = 0.0;
  auto add = [&](int e, int side) {
    const double* T = terms + (size_t)e * kPgoTerm;
#pragma unroll
    for (int k = 0; k < 16; k++) a[k] += T[(side ? 28 : 12) + k];
#pragma unroll
    for (int k = 0; k < 4; k++) a[16 + k] += T[(side ? 8 : 4) + k];
  };
  if (n > 0) add(n - 1, 1);
  if (n < n_nodes - 1) add(n, 0);
  for (int q = inc_start[n]; q < inc_start[n + 1]; q++) add(n_nodes - 1 + (inc[q] >> 1), inc[q] & 1);
#pragma unroll
  for (int k = 0; k < 16; k++) D[(size_t)n * 16 + k] = a[k];
#pragma unroll
  for (int k = 0; k < 4; k++) g[(size_t)n * 4 + k] = a[16 + k];
}

// ---- fixed-order folds, one workgroup: out[c] = sum over i of v[i * stride + off + c] (c < ncomp <= 4), or its largest magnitude.  Lane t
// adds i = t, t + kPgoBlock, ... in ascending order, then a binary tree over the lanes ------------------------------------------------
__global__ void __launch_bounds__(kPgoBlock) k_pgo_fold(const double* __restrict__ v, int stride, int off, int n, int ncomp, int absmax, double* __restrict__ out) {
  __shared__ double sh[4][kPgoBlock];
  const int t = (int)threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < n; i += kPgoBlock)
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < ncomp) {
        const double w = v[(size_t)i * stride + off + c];
        a[c] = absmax ? fmax(a[c], fabs(w)) : a[c] + w;
      }
#pragma unroll
  for (int c = 0; c < 4; c++) sh[c][t] = a[c];
  __syncthreads();
  for (int h = kPgoBlock / 2; h > 0; h >>= 1) {
    if (t < h)
#pragma unroll
      for (int c = 0; c < 4; c++) sh[c][t] = absmax ? fmax(sh[c][t], sh[c][t + h]) : sh[c][t] + sh[c][t + h];
    __syncthreads();
  }
  if (t < ncomp) out[t] = sh[t][0];
}

// ---- the segments' interiors, one lane per segment ------------------------------------------------------------------------------------
// Segment s: the positions strictly between sep[s] = a and sep[s + 1] = b (the last one: between sep[P - 1] and N, no right separator).
// A block Cholesky along the chain: walking k = a + 1 .. b - 1 with the block F = H[a, k] the elimination has filled in so far (F = the
// chain block of a at k = a + 1) and D_k = L L^T:
//   Y = L^-1 F^T;  Z = L^-1 E_k  (E_k = H[k, k + 1], the chain block);  y = L^-1 r_k
//   S_aa -= Y^T Y, r_a -= Y^T y;   H[a, k + 1] = -Y^T Z;   D_{k+1} -= Z^T Z, r_{k+1} -= Z^T y
// (no inverse is formed: every update is a symmetric product of triangular solves) and L, Y, Z, y are kept for the way back (ws: kPgoWs
// doubles per position).  At k = b - 1 the three updates are the segment's contributions to the separators' system: slot s = {S_aa[16],
// r_a[4], S_bb[16], r_b[4], S_ab[16]} (kPgoSlot doubles), all zero for an empty segment.  flag[0] is raised where a diagonal block is not
// positive definite.
__global__ void __launch_bounds__(64) k_pgo_segments(const double* __restrict__ terms, const double* __restrict__ D, const double* __restrict__ g, int n_nodes,
                                                     const int* __restrict__ sep, int n_sep, int fixed, double inv_radius, double* __restrict__ ws,
                                                     double* __restrict__ slots, int* __restrict__ flag) {
  const int s = blockIdx.x * 64 + (int)threadIdx.x;
  if (s >= n_sep) return;
  const int a = sep[s];
  const bool has_right = s + 1 < n_sep;
  const int b = has_right ? sep[s + 1] : n_nodes;
  double Saa[16], ra[4], F[16], Dk[16], rk[4];
#pragma unroll
  for (int k = 0; k < 16; k++) { Saa[k] = 0.0; F[k] = 0.0; Dk[k] = 0.0; }
#pragma unroll
  for (int k = 0; k < 4; k++) { ra[k] = 0.0; rk[k] = 0.0; }
  double* slot = slots + (size_t)s * kPgoSlot;
  bool bad = false;
  if (b - a > 1) {
#pragma unroll
    for (int k = 0; k < 16; k++) F[k] = terms[(size_t)a * kPgoTerm + 44 + k];
    pgo_load_damped(D, a + 1, fixed, inv_radius, Dk);
#pragma unroll
    for (int k = 0; k < 4; k++) rk[k] = -g[(size_t)(a + 1) * 4 + k];
  }
  for (int k = a + 1; k < b; k++) {
    double L[16], Y[16], Z[16], tmp[16], y[4], v[4];
    bad = !pgo_chol4(Dk, L) || bad;
    pgo_lsolve(L, F, true, Y);
    pgo_lsolve_v(L, rk, y);
    const bool has_next = k + 1 < n_nodes;   // false only at the last position of the last segment
#pragma unroll
    for (int q = 0; q < 16; q++) tmp[q] = has_next ? terms[(size_t)k * kPgoTerm + 44 + q] : 0.0;
    pgo_lsolve(L, tmp, false, Z);
    double* W = ws + (size_t)k * kPgoWs;
#pragma unroll
    for (int q = 0; q < 16; q++) { W[q] = L[q]; W[16 + q] = Y[q]; W[32 + q] = Z[q]; }
#pragma unroll
    for (int q = 0; q < 4; q++) W[48 + q] = y[q];
    pgo_mtm(Y, Y, tmp);
#pragma unroll
    for (int q = 0; q < 16; q++) Saa[q] -= tmp[q];
    pgo_mtv(Y, y, v);
#pragma unroll
    for (int q = 0; q < 4; q++) ra[q] -= v[q];
    pgo_mtm(Y, Z, tmp);
#pragma unroll
    for (int q = 0; q < 16; q++) F[q] = -tmp[q];                 // H[a, k + 1]
    pgo_mtv(Z, y, v);
    pgo_mtm(Z, Z, tmp);
    if (k + 1 < b) {
      pgo_load_damped(D, k + 1, fixed, inv_radius, Dk);
#pragma unroll
      for (int q = 0; q < 16; q++) Dk[q] -= tmp[q];
#pragma unroll
      for (int q = 0; q < 4; q++) rk[q] = -g[(size_t)(k + 1) * 4 + q] - v[q];
    } else {
#pragma unroll
      for (int q = 0; q < 16; q++) Dk[q] = -tmp[q];              // the contribution to S_bb
#pragma unroll
      for (int q = 0; q < 4; q++) rk[q] = -v[q];
    }
  }
#pragma unroll
  for (int q = 0; q < 16; q++) { slot[q] = Saa[q]; slot[20 + q] = Dk[q]; slot[40 + q] = F[q]; }
#pragma unroll
  for (int q = 0; q < 4; q++) { slot[16 + q] = ra[q]; slot[36 + q] = rk[q]; }
  if (bad) flag[0] = 1;
}

// ---- the separators' system, one workgroup: assembled in a fixed order, factored (Cholesky, column by column: the scaled column goes
// through LDS, the trailing update runs with consecutive lanes on consecutive columns of a row), solved; d at the separators' positions ---
__global__ void __launch_bounds__(kPgoDenseBlock) k_pgo_dense(const double* __restrict__ terms, const double* __restrict__ D, const double* __restrict__ g, int n_nodes,
                                                               const int* __restrict__ sep, const int* __restrict__ sep_of, int n_sep, const int* __restrict__ ij,
                                                               int n_loops, int fixed, double inv_radius, const double* __restrict__ slots, double* __restrict__ M,
                                                               double* __restrict__ d, int* __restrict__ flag) {
  __shared__ double col[4 * kPgoMaxSep], rhs[4 * kPgoMaxSep];
  __shared__ int s_bad;
  const int t = (int)threadIdx.x, nt = kPgoDenseBlock;
  const int n = 4 * n_sep;
  if (t == 0) s_bad = 0;
  for (int i = t >> 6; i < n; i += nt >> 6)   // the lower triangle alone is ever read: a wave per row, lanes along it
    for (int k = t & 63; k <= i; k += 64) M[(size_t)i * n + k] = 0.0;
  __syncthreads();
  // diagonal blocks, chain blocks (below the diagonal: the transpose of H[s, s + 1]) and the right-hand side: 16 lanes per separator
  for (int w = t; w < n_sep * 16; w += nt) {
    const int s = w >> 4, q = w & 15, r = q >> 2, c = q & 3;
    const int node = sep[s];
    const bool left_seg = s > 0 && sep[s] - sep[s - 1] > 1;
    const bool right_seg = (s + 1 < n_sep ? sep[s + 1] : n_nodes) - sep[s] > 1;
    double v = D[(size_t)node * 16 + q];
    if (node == fixed) v = (r == c) ? 1.0 : 0.0;
    else if (r == c) v += fmin(fmax(v, 1e-6), 1e32) * inv_radius;
    if (left_seg) v += slots[(size_t)(s - 1) * kPgoSlot + 20 + q];
    if (right_seg) v += slots[(size_t)s * kPgoSlot + q];
    if (c <= r) M[(size_t)(4 * s + r) * n + 4 * s + c] = v;
    if (s + 1 < n_sep) {
      const double o = right_seg ? slots[(size_t)s * kPgoSlot + 40 + q] : terms[(size_t)node * kPgoTerm + 44 + q];
      M[(size_t)(4 * (s + 1) + c) * n + 4 * s + r] = o;
    }
    if (c == 0) {
      double b = -g[(size_t)node * 4 + r];
      if (left_seg) b += slots[(size_t)(s - 1) * kPgoSlot + 36 + r];
      if (right_seg) b += slots[(size_t)s * kPgoSlot + 16 + r];
      rhs[4 * s + r] = b;
    }
  }
  __syncthreads();
  // the loops, in ascending loop order: lane q owns entry q of every block, so no two lanes meet
  if (t < 16) {
    const int r = t >> 2, c = t & 3;
    for (int l = 0; l < n_loops; l++) {
      const int e = n_nodes - 1 + l;
      const int si = sep_of[ij[2 * e]], sj = sep_of[ij[2 * e + 1]];
      const double v = terms[(size_t)e * kPgoTerm + 44 + t];                       // A_ij[r][c]
      if (si > sj) M[(size_t)(4 * si + r) * n + 4 * sj + c] += v;
      else M[(size_t)(4 * sj + c) * n + 4 * si + r] += v;
    }
  }
  __syncthreads();
  for (int j = 0; j < n; j++) {
    const double pivot = M[(size_t)j * n + j];
    if (!(pivot > 0.0)) { if (t == 0) s_bad = 1; }
    const double dj = sqrt(pivot > 0.0 ? pivot : 1.0);
    for (int i = j + 1 + t; i < n; i += nt) {
      const double v = M[(size_t)i * n + j] / dj;
      M[(size_t)i * n + j] = v;
      col[i] = v;
    }
    __syncthreads();
    if (t == 0) M[(size_t)j * n + j] = dj;
    for (int i = j + 1 + (t >> 6); i < n; i += nt >> 6) {
      const double li = col[i];
      for (int k = j + 1 + (t & 63); k <= i; k += 64) M[(size_t)i * n + k] -= li * col[k];
    }
    __syncthreads();
  }
  // L y = rhs, L^T x = y
  for (int j = 0; j < n; j++) {
    const double yj = rhs[j] / M[(size_t)j * n + j];
    __syncthreads();
    if (t == 0) rhs[j] = yj;
    for (int i = j + 1 + t; i < n; i += nt) rhs[i] -= M[(size_t)i * n + j] * yj;
    __syncthreads();
  }
  for (int j = n - 1; j >= 0; j--) {
    const double xj = rhs[j] / M[(size_t)j * n + j];
    __syncthreads();
    if (t == 0) rhs[j] = xj;
    for (int i = t; i < j; i += nt) rhs[i] -= M[(size_t)j * n + i] * xj;
    __syncthreads();
  }
  for (int w = t; w < n; w += nt) d[(size_t)sep[w >> 2] * 4 + (w & 3)] = rhs[w];
  if (t == 0 && s_bad) flag[0] = 1;
}

// ---- the way back, one lane per segment: d_k = L^-T (y - Y d_a - Z d_{k+1}), k = b - 1 .. a + 1 -----------------------------------------
__global__ void __launch_bounds__(64) k_pgo_backsub(int n_nodes, const int* __restrict__ sep, int n_sep, const double* __restrict__ ws, double* __restrict__ d) {
  const int s = blockIdx.x * 64 + (int)threadIdx.x;
  if (s >= n_sep) return;
  const int a = sep[s];
  const int b = s + 1 < n_sep ? sep[s + 1] : n_nodes;
  double xa[4], xn[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { xa[q] = d[(size_t)a * 4 + q]; xn[q] = b < n_nodes ? d[(size_t)b * 4 + q] : 0.0; }
  for (int k = b - 1; k > a; k--) {
    const double* W = ws + (size_t)k * kPgoWs;
    double A[16], v[4], u[4];
#pragma unroll
    for (int q = 0; q < 16; q++) A[q] = W[16 + q];
    pgo_mv(A, xa, v);
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = W[48 + q] - v[q];
#pragma unroll
    for (int q = 0; q < 16; q++) A[q] = W[32 + q];
    pgo_mv(A, xn, v);                                           // Z is zero at the last position of the last segment
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] -= v[q];
#pragma unroll
    for (int q = 0; q < 16; q++) A[q] = W[q];
    pgo_ltsolve_v(A, u, xn);
#pragma unroll
    for (int q = 0; q < 4; q++) d[(size_t)k * 4 + q] = xn[q];
  }
}

// ---- what the LM decision needs, one lane per node: (H d)_n over the node's incident edges in k_pgo_gather's order, the node's share of the
// model decrease -d^T (g + H d / 2), |d_n|^2, the candidate x+ = Plus(x, d) (AngleLocalParameterization on the yaw, :501-515) and |x+_n|^2
// over the free parameters; part: 4 doubles per node {model, |d|^2, |x+|^2, 0} for k_pgo_fold ------------------------------------------------
__global__ void __launch_bounds__(kPgoBlock) k_pgo_step(const double* __restrict__ terms, const double* __restrict__ D, const double* __restrict__ g, int n_nodes,
                                                         const int* __restrict__ inc_start, const int* __restrict__ inc, const int* __restrict__ ij, int fixed,
                                                         const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ x_new, double* __restrict__ part) {
  const int n = blockIdx.x * kPgoBlock + (int)threadIdx.x;
  if (n >= n_nodes) return;
  double dn[4], Hd[4], A[16], o[4], v[4];
#pragma unroll
  for (int q = 0; q < 4; q++) dn[q] = d[(size_t)n * 4 + q];
#pragma unroll
  for (int q = 0; q < 16; q++) A[q] = D[(size_t)n * 16 + q];
  pgo_mv(A, dn, Hd);
  auto add = [&](int e, int side) {   // side 1: n is the edge's j, the block applies transposed to d_i
    const int other = side ? ij[2 * e] : ij[2 * e + 1];
#pragma unroll
    for (int q = 0; q < 16; q++) A[q] = terms[(size_t)e * kPgoTerm + 44 + q];
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = d[(size_t)other * 4 + q];
    if (side) pgo_mtv(A, o, v); else pgo_mv(A, o, v);
#pragma unroll
    for (int q = 0; q < 4; q++) Hd[q] += v[q];
  };
  if (n > 0) add(n - 1, 1);
  if (n < n_nodes - 1) add(n, 0);
  for (int q = inc_start[n]; q < inc_start[n + 1]; q++) add(n_nodes - 1 + (inc[q] >> 1), inc[q] & 1);
  double model = 0.0, d2 = 0.0, x2 = 0.0, xp[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    model -= dn[q] * (g[(size_t)n * 4 + q] + 0.5 * Hd[q]);
    d2 += dn[q] * dn[q];
  }
  xp[0] = pgo_normalize(x[(size_t)n * 4] + dn[0]);
#pragma unroll
  for (int q = 1; q < 4; q++) xp[q] = x[(size_t)n * 4 + q] + dn[q];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if (n == fixed) xp[q] = x[(size_t)n * 4 + q];
    else x2 += xp[q] * xp[q];
    x_new[(size_t)n * 4 + q] = xp[q];
  }
  part[(size_t)n * 4] = model; part[(size_t)n * 4 + 1] = d2; part[(size_t)n * 4 + 2] = x2; part[(size_t)n * 4 + 3] = 0.0;
}

void pgo_evaluate(hipStream_t s, const PgoGraph& G, const double* x, double* terms, double* D, double* g, double* out2) {
  if (G.n_edges > 0) hipLaunchKernelGGL(k_pgo_edges, dim3((G.n_edges + kPgoBlock - 1) / kPgoBlock), dim3(kPgoBlock), 0, s, G.ij, G.meas, G.n_edges, x, G.fixed, terms);
  hipLaunchKernelGGL(k_pgo_gather, dim3((G.n_nodes + kPgoBlock - 1) / kPgoBlock), dim3(kPgoBlock), 0, s, terms, G.n_nodes, G.inc_start, G.inc, D, g);
  hipLaunchKernelGGL(k_pgo_fold, dim3(1), dim3(kPgoBlock), 0, s, terms, kPgoTerm, 60, G.n_edges, 1, 0, out2);
  hipLaunchKernelGGL(k_pgo_fold, dim3(1), dim3(kPgoBlock), 0, s, g, 1, 0, 4 * G.n_nodes, 1, 1, out2 + 1);
}

void pgo_solve(hipStream_t s, const PgoGraph& G, const double* terms, const double* D, const double* g, double radius, double* ws, double* slots, double* M, double* d,
               int* flag) {
  const double inv_radius = 1.0 / radius;
  const int nb = (G.n_sep + 63) / 64;
  hipLaunchKernelGGL(k_pgo_segments, dim3(nb), dim3(64), 0, s, terms, D, g, G.n_nodes, G.sep, G.n_sep, G.fixed, inv_radius, ws, slots, flag);
  hipLaunchKernelGGL(k_pgo_dense, dim3(1), dim3(kPgoDenseBlock), 0, s, terms, D, g, G.n_nodes, G.sep, G.sep_of, G.n_sep, G.ij, G.n_edges - (G.n_nodes - 1), G.fixed,
                     inv_radius, slots, M, d, flag);
  hipLaunchKernelGGL(k_pgo_backsub, dim3(nb), dim3(64), 0, s, G.n_nodes, G.sep, G.n_sep, ws, d);
}

void pgo_step(hipStream_t s, const PgoGraph& G, const double* terms, const double* D, const double* g, const double* x, const double* d, double* x_new, double* part,
              double* out3) {
  hipLaunchKernelGGL(k_pgo_step, dim3((G.n_nodes + kPgoBlock - 1) / kPgoBlock), dim3(kPgoBlock), 0, s, terms, D, g, G.n_nodes, G.inc_start, G.inc, G.ij, G.fixed, x, d,
                     x_new, part);
  hipLaunchKernelGGL(k_pgo_fold, dim3(1), dim3(kPgoBlock), 0, s, part, 4, 0, G.n_nodes, 3, 0, out3);
}

}  // namespace rgck
