// rgc_terms.h -- the device code the solvers share: the Gauss-Newton term of one Mahalanobis correspondence, R C R^T of a six-entry covariance,
// the covariance of a sorted point, and the fixed-order sums (a wave's shuffle tree, the shuffle-tree block store, the column fold).  Included by
// rgc_kernels.hip (VGICP, the mapping registration's fold), rgc_vgicp_radius.hip, rgc_ndt.hip, rgc_gicp.hip, rgc_gicp_mp.hip and rgc_frontend.hip; the symmetric 3x3
// inverse they use is rgc_cov.h's inv_sym3, the fp32 query transform rgc_nn.h's transform_f32.  Everything here is __forceinline__, as in those
// two headers: each kernel inlines its own copy, no __global__ lives here.  The project's arithmetic holds for every caller alike -- fp64 after
// the fp32 key, every sum in a fixed order, no contraction (compile with -ffp-contract=off) -- so one definition serves them all bit for bit.
// The term and R C R^T are __host__ __device__: tests/cpp/terms_table.cpp holds the host compile to a longdouble reference, no GPU.
//
// Different ON PURPOSE, and therefore not here:
//   ndt_jacobi_rot / ndt_min_eig (rgc_ndt.hip)   another threshold and another closed form than rgc_cov.h's jacobi_rot;
//   k_ndt_fold (rgc_ndt.hip)                     ONE lane adds the rows sequentially: another order than fold_column's;
//   block_reduce_store (rgc_kernels.hip)         the quad-DPP tree of the tuned solve: another order than block_sum_store's, and measured;
//   k_pgo_fold (rgc_pgo.hip)                     has an abs-max mode.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace rgck {

// One correspondence's share of the normal equations: with J = [skew(q) | -I] (3 x 6, columns [rotation, translation]) and the symmetric M
// (xx xy xz yy yz zz), acc[0..21) the upper triangle of J^T M J by rows, acc[21..27) J^T M e, acc[27] e^T M e.  kWeightedSum: acc[u] += w * (..)
// (VGICP, NDT: several terms per lane); else acc[u] = (..) and w is not read (FastGICP; FastGICPMultiPoints, which passes W = M M for M).
// want_H == 0: the cost alone.
template <bool kWeightedSum, int N>
__host__ __device__ __forceinline__ void gn_term(const double (&M)[6], double q0, double q1, double q2, double e0, double e1, double e2, double w,
                                                 int want_H, double (&acc)[N]) {
  static_assert(N >= 28, "21 + 6 + 1 sums");
  const double Me0 = M[0] * e0 + M[1] * e1 + M[2] * e2;
  const double Me1 = M[1] * e0 + M[3] * e1 + M[4] * e2;
  const double Me2 = M[2] * e0 + M[4] * e1 + M[5] * e2;
  if (kWeightedSum) acc[27] += w * (e0 * Me0 + e1 * Me1 + e2 * Me2);
  else acc[27] = e0 * Me0 + e1 * Me1 + e2 * Me2;
  if (!want_H) return;
  const double J[3][6] = {{0.0, -q2, q1, -1.0, 0.0, 0.0}, {q2, 0.0, -q0, 0.0, -1.0, 0.0}, {-q1, q0, 0.0, 0.0, 0.0, -1.0}};
  double MJ[3][6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    MJ[0][c] = M[0] * J[0][c] + M[1] * J[1][c] + M[2] * J[2][c];
    MJ[1][c] = M[1] * J[0][c] + M[3] * J[1][c] + M[4] * J[2][c];
    MJ[2][c] = M[2] * J[0][c] + M[4] * J[1][c] + M[5] * J[2][c];
  }
  int u = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int c = a; c < 6; c++) {
      if (kWeightedSum) acc[u] += w * (J[0][a] * MJ[0][c] + J[1][a] * MJ[1][c] + J[2][a] * MJ[2][c]);
      else acc[u] = J[0][a] * MJ[0][c] + J[1][a] * MJ[1][c] + J[2][a] * MJ[2][c];
      u++;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; a++) {
    if (kWeightedSum) acc[21 + a] += w * (J[0][a] * Me0 + J[1][a] * Me1 + J[2][a] * Me2);
    else acc[21 + a] = J[0][a] * Me0 + J[1][a] * Me1 + J[2][a] * Me2;
  }
}

// the upper triangle of R C R^T (R row-major 3x3, C and out xx xy xz yy yz zz): (R C) first, each entry ((r0 c0 + r1 c1) + r2 c2), then times R^T.
// NDT's D2D term and VGICP's general route call it.  k_gicp_terms and k_gicp_mp_terms keep the same expressions written in place: behind any
// function boundary (this one, a local lambda, tried in five spellings) those two kernels came out with 4 to 8 more SGPRs -- same VGPRs, LDS, no
// scratch -- and the refactor's rule was an unchanged resource table for every kernel.
__host__ __device__ __forceinline__ void rcrt6(const double (&R)[9], const double (&C)[6], double (&out)[6]) {
  const double Cs[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double RC[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) RC[a][b] = R[3 * a] * Cs[0][b] + R[3 * a + 1] * Cs[1][b] + R[3 * a + 2] * Cs[2][b];
  int u = 0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++) out[u++] = RC[a][0] * R[3 * b] + RC[a][1] * R[3 * b + 1] + RC[a][2] * R[3 * b + 2];
}

#ifdef __HIPCC__

constexpr int kWaveLanes = 64;

// the six shuffle steps of a wave: lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// the covariance of sorted point s as its upper triangle (xx xy xz yy yz zz): the general route's six doubles (c6[a * n + s]), or the tuned
// route's unit normal expanded as the getters expand it, C = I - 0.999 n n^T (fast_gicp_impl.hpp:280-293)
template <bool kGeneral>
__device__ __forceinline__ void point_cov6(const double* __restrict__ c6, const double* __restrict__ nx, const double* __restrict__ ny,
                                           const double* __restrict__ nz, int n, int s, double C[6]) {
  if (kGeneral) {
#pragma unroll
    for (int a = 0; a < 6; a++) C[a] = c6[(size_t)a * n + s];
  } else {
    const double v0 = nx[s], v1 = ny[s], v2 = nz[s];
    C[0] = 1.0 - 0.999 * v0 * v0; C[1] = 0.0 - 0.999 * v0 * v1; C[2] = 0.0 - 0.999 * v0 * v2;
    C[3] = 1.0 - 0.999 * v1 * v1; C[4] = 0.0 - 0.999 * v1 * v2;
    C[5] = 1.0 - 0.999 * v2 * v2;
  }
}

// Sum of the workgroup's NACC accumulators (T threads) in a FIXED order: the six shuffle steps of a wave, the waves' sums parked in LDS, then
// thread a adds accumulator a's waves ascending, starting FROM WAVE 0's value.  row: NACC doubles.  kCount: the same for one int per lane
// (exact), thread NACC writes *cnt.  (A partial row of negative zeros alone keeps its sign here; every fold of such rows starts from +0.0.)
template <int T, int NACC, bool kCount>
__device__ __forceinline__ void block_sum_store_impl(double (&acc)[NACC], double* __restrict__ row, int nterm, int* __restrict__ cnt) {
  static_assert(T % kWaveLanes == 0 && NACC + (kCount ? 1 : 0) <= T, "whole waves, a thread per sum");
  __shared__ double red[T / kWaveLanes][NACC];
  const int lane = threadIdx.x & (kWaveLanes - 1), w = threadIdx.x / kWaveLanes;
#pragma unroll
  for (int a = 0; a < NACC; a++) {
    double v = acc[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) red[w][a] = v;
  }
  if constexpr (kCount) {
    __shared__ int cred[T / kWaveLanes];
    int c = nterm;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (lane == 0) cred[w] = c;
    __syncthreads();
    if (threadIdx.x == NACC) {
      int t = 0;
#pragma unroll
      for (int j = 0; j < T / kWaveLanes; j++) t += cred[j];
      *cnt = t;
    }
  } else {
    __syncthreads();
  }
  if (threadIdx.x < NACC) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < T / kWaveLanes; j++) t += red[j][threadIdx.x];
    row[threadIdx.x] = t;
  }
}
template <int T, int NACC>
__device__ __forceinline__ void block_sum_store(double (&acc)[NACC], double* __restrict__ row) {
  block_sum_store_impl<T, NACC, false>(acc, row, 0, nullptr);
}
template <int T, int NACC>
__device__ __forceinline__ void block_sum_count_store(double (&acc)[NACC], int nterm, double* __restrict__ row, int* __restrict__ cnt) {
  block_sum_store_impl<T, NACC, true>(acc, row, nterm, cnt);
}

// Column col of nrows rows of ncol doubles folded by ONE wave in a fixed order: lane l adds rows l, l + 64, ... ascending from +0.0, then the
// wave's shuffle tree.  Lane 0 holds the sum.  The fold kernels are per-file __global__ wrappers over this body.
__device__ __forceinline__ double fold_column(const double* partials, int nrows, int ncol, int col, int lane) {
  double s = 0;
  for (int r = lane; r < nrows; r += kWaveLanes) s += partials[(size_t)r * ncol + col];
  return wave_sum(s);
}

#endif  // __HIPCC__

}  // namespace rgck
