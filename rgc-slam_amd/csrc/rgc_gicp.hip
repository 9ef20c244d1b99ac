// rgc_gicp.hip -- gfx950 kernels of FastGICP: GICP on an exact nearest neighbour per source point, under the kNN covariances of both clouds.
// Reference: fast_gicp::FastGICP (include/fast_gicp/gicp/fast_gicp.hpp, include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237); written from its
// formulas, in the project's arithmetic: the query and the search key in fp32 (never FMA-contracted: -ffp-contract=off), everything after
// them fp64, every sum in a fixed order, no floating-point atomics.  Citations are relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own, over the pieces every solver shares: the term, the covariance of a sorted point, the shuffle-tree block store
// and the column fold are rgc_terms.h's, the inverse rgc_cov.h's, the fp32 query and the search rgc_nn.h's.  Two kernels per linearisation
// rather than one: the fp32 search (its cube walk holds two dozen live registers and a loop) and the fp64 term (28 accumulators) each keep
// their registers to themselves -- no spill, no private segment, no accumulator registers.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_cov.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int GICP_T = 256;   // threads per workgroup
constexpr int GICP_WAVE = 64;

int gicp_blocks(int n) { return (n + GICP_T - 1) / GICP_T; }

// fast_gicp_impl.hpp:115-141 (update_correspondences): q = T.cast<float>() * p_s in fp32, ((m0 x + m1 y) + m2 z) + m3 as k_fitness and
// k_transform_f32 compute it; the exact nearest target point of q (nn_search: smallest ((dx dx + dy dy) + dz dz), ties to the smaller original
// index), kept iff (double)key < d_max^2 (:136, strict).  One lane per source point in SORTED order s: corr[s] = the neighbour's position in
// the target's sorted array or -1, key[s] = the squared distance whether kept or not (:135).
__global__ void __launch_bounds__(GICP_T) k_gicp_correspond(const float4* __restrict__ SP, int ns, PoseF T, const float4* __restrict__ TP,
                                                             const int* __restrict__ tstart, Grid g, double dmax2, int* __restrict__ corr,
                                                             float* __restrict__ key) {
  const int s = blockIdx.x * GICP_T + threadIdx.x;
  if (s >= ns) return;
  const float4 sp = SP[s];
  float qx, qy, qz, best;
  transform_f32(T, sp.x, sp.y, sp.z, qx, qy, qz);
  int bs;
  nn_search<true>(qx, qy, qz, TP, tstart, g, 1.0e300, best, bs);
  key[s] = best;
  corr[s] = (bs >= 0 && (double)best < dmax2) ? bs : -1;
}

constexpr int kGicpAcc = kAccum + 1;  // 21 upper-triangular H, 6 b, the cost, the number of kept correspondences (exact in a double: < 2^27)

// fast_gicp_impl.hpp:143-211 (the Mahalanobis matrices of update_correspondences and linearize) for the pair list of k_gicp_correspond:
// a = R p + t, e = b_j - a, M = (C_B[j] + R C_A[s] R^T)^-1 (the 3x3 block of the reference's 4x4 with RCR(3,3) = 1, M(3,3) = 0, :146-150),
// cost += e^T M e, J = [skew(a), -I], H += J^T M J, b += J^T M e; no weight.  M goes to Mout[a * ns + s] for the frozen cost.
// One lane per sorted source point: its 28 + 1 values are its term itself.
template <bool kGenA, bool kGenB>
__global__ void __launch_bounds__(GICP_T) k_gicp_terms(const float4* __restrict__ SP, int ns, const float4* __restrict__ TP, int nt, const int* __restrict__ corr,
                                                        const double* __restrict__ c6A, const double* __restrict__ nxA, const double* __restrict__ nyA,
                                                        const double* __restrict__ nzA, const double* __restrict__ c6B, const double* __restrict__ nxB,
                                                        const double* __restrict__ nyB, const double* __restrict__ nzB, Pose T, int want_H,
                                                        double* __restrict__ Mout, double* __restrict__ partials) {
  const int s = blockIdx.x * GICP_T + threadIdx.x;
  double acc[kGicpAcc];
#pragma unroll
  for (int a = 0; a < kGicpAcc; a++) acc[a] = 0.0;
  const int j = s < ns ? corr[s] : -1;
  if (j >= 0 && j < nt) {
    const float4 sp = SP[s], tp = TP[j];
    const double p0 = (double)sp.x, p1 = (double)sp.y, p2 = (double)sp.z;
    double CA[6], CB[6];
    point_cov6<kGenA>(c6A, nxA, nyA, nzA, ns, s, CA);
    point_cov6<kGenB>(c6B, nxB, nyB, nzB, nt, j, CB);
    // (R C_A R^T in place, not rgc_terms.h's rcrt6: behind a function boundary this kernel takes more SGPRs, see there)
    const double Cs[3][3] = {{CA[0], CA[1], CA[2]}, {CA[1], CA[3], CA[4]}, {CA[2], CA[4], CA[5]}};
    double RC[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) RC[a][b] = T.R[3 * a] * Cs[0][b] + T.R[3 * a + 1] * Cs[1][b] + T.R[3 * a + 2] * Cs[2][b];
    double S[6];
    {
      int u = 0;
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++) { S[u] = CB[u] + (RC[a][0] * T.R[3 * b] + RC[a][1] * T.R[3 * b + 1] + RC[a][2] * T.R[3 * b + 2]); u++; }
    }
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    inv_sym3(S, M);
#pragma unroll
    for (int a = 0; a < 6; a++) Mout[(size_t)a * ns + s] = M[a];
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const double e0 = (double)tp.x - q0, e1 = (double)tp.y - q1, e2 = (double)tp.z - q2;
    gn_term<false>(M, q0, q1, q2, e0, e1, e2, 1.0, want_H, acc);  // J = [skew(a) | -I], columns [rotation, translation] (:188-190); no weight
    acc[28] = 1.0;
  }
  block_sum_store<GICP_T>(acc, partials + (size_t)blockIdx.x * kGicpAcc);
}

// fast_gicp_impl.hpp:214-237 (compute_error): the pairs and the matrices of the last linearisation at another pose
__global__ void __launch_bounds__(GICP_T) k_gicp_error(const float4* __restrict__ SP, int ns, const float4* __restrict__ TP, int nt, const int* __restrict__ corr,
                                                        const double* __restrict__ Min, Pose T, double* __restrict__ partials) {
  const int s = blockIdx.x * GICP_T + threadIdx.x;
  double acc[1] = {0.0};
  const int j = s < ns ? corr[s] : -1;
  if (j >= 0 && j < nt) {
    const float4 sp = SP[s], tp = TP[j];
    const double p0 = (double)sp.x, p1 = (double)sp.y, p2 = (double)sp.z;
    double M[6];
#pragma unroll
    for (int a = 0; a < 6; a++) M[a] = Min[(size_t)a * ns + s];
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const double e0 = (double)tp.x - q0, e1 = (double)tp.y - q1, e2 = (double)tp.z - q2;
    const double Me0 = M[0] * e0 + M[1] * e1 + M[2] * e2;
    const double Me1 = M[1] * e0 + M[3] * e1 + M[4] * e2;
    const double Me2 = M[2] * e0 + M[4] * e1 + M[5] * e2;
    acc[0] = e0 * Me0 + e1 * Me1 + e2 * Me2;
  }
  block_sum_store<GICP_T>(acc, partials + blockIdx.x);
}

// the workgroups' rows folded in a fixed order, one wave per column (fold_column)
__global__ void __launch_bounds__(GICP_WAVE) k_gicp_fold(const double* __restrict__ partials, int nb, int ncol, double* __restrict__ out) {
  const int col = blockIdx.x, lane = threadIdx.x;
  const double t = fold_column(partials, nb, ncol, col, lane);
  if (lane == 0) out[col] = t;
}

// the pair list in CALLER order: idx[i] = original index of source point i's neighbour or -1, sq[i] = its key
__global__ void __launch_bounds__(GICP_T) k_gicp_export(const float4* __restrict__ SP, int ns, const float4* __restrict__ TP, int nt, const int* __restrict__ corr,
                                                         const float* __restrict__ key, int* __restrict__ idx, float* __restrict__ sq) {
  const int s = blockIdx.x * GICP_T + threadIdx.x;
  if (s >= ns) return;
  const int o = __float_as_int(SP[s].w);
  if (o < 0 || o >= ns) return;
  const int j = corr[s];
  idx[o] = (j >= 0 && j < nt) ? __float_as_int(TP[j].w) : -1;
  sq[o] = key[s];
}

void gicp_correspond(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, double dmax2, int* corr, float* key) {
  const int nb = gicp_blocks(src.n);
  if (nb > 0) hipLaunchKernelGGL(k_gicp_correspond, dim3(nb), dim3(GICP_T), 0, s, src.P, src.n, T, tgt.P, tgt.start, tgt.grid, dmax2, corr, key);
}

void gicp_terms(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const GicpCov& A, const GicpCov& B, Pose T, int want_H,
                double* M, double* partials, double* out29) {
  const int nb = gicp_blocks(src.n);
  if (nb <= 0) return;
#define GICP_LAUNCH(GA, GB) \
  hipLaunchKernelGGL((k_gicp_terms<GA, GB>), dim3(nb), dim3(GICP_T), 0, s, src.P, src.n, tgt.P, tgt.n, corr, A.c6, A.nx, A.ny, A.nz, B.c6, B.nx, B.ny, B.nz, T, want_H, M, partials)
  if (A.c6) { if (B.c6) GICP_LAUNCH(true, true); else GICP_LAUNCH(true, false); }
  else      { if (B.c6) GICP_LAUNCH(false, true); else GICP_LAUNCH(false, false); }
#undef GICP_LAUNCH
  hipLaunchKernelGGL(k_gicp_fold, dim3(kGicpAcc), dim3(GICP_WAVE), 0, s, partials, nb, kGicpAcc, out29);
}

void gicp_error(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const double* M, Pose T, double* partials, double* out1) {
  const int nb = gicp_blocks(src.n);
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_gicp_error, dim3(nb), dim3(GICP_T), 0, s, src.P, src.n, tgt.P, tgt.n, corr, M, T, partials);
  hipLaunchKernelGGL(k_gicp_fold, dim3(1), dim3(GICP_WAVE), 0, s, partials, nb, 1, out1);
}

void gicp_fold(hipStream_t s, const double* partials, int nb, int ncol, double* out) {
  if (nb > 0 && ncol > 0) hipLaunchKernelGGL(k_gicp_fold, dim3(ncol), dim3(GICP_WAVE), 0, s, partials, nb, ncol, out);
}

void gicp_export(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const float* key, int* idx, float* sq) {
  const int nb = gicp_blocks(src.n);
  if (nb > 0) hipLaunchKernelGGL(k_gicp_export, dim3(nb), dim3(GICP_T), 0, s, src.P, src.n, tgt.P, tgt.n, corr, key, idx, sq);
}

}  // namespace rgck
