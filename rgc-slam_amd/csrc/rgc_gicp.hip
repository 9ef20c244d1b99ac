// rgc_gicp.hip -- gfx950 kernels of FastGICP: GICP on an exact nearest neighbour per source point, under the kNN covariances of both clouds.
// Reference: fast_gicp::FastGICP (include/fast_gicp/gicp/fast_gicp.hpp, include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237); written from its
// formulas, in the project's arithmetic: the query and the search key in fp32 (never FMA-contracted: -ffp-contract=off), everything after
// them fp64, every sum in a fixed order, no floating-point atomics.  Citations are relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own: the device code of every other kernel of the library stays what it was.  Two kernels per linearisation
// rather than one: the fp32 search (its cube walk holds two dozen live registers and a loop) and the fp64 term (28 accumulators) each keep
// their registers to themselves -- no spill, no private segment, no accumulator registers.
#include "rgc_kernels.h"
#include "rgc_nn.h"

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
  const float x = sp.x, y = sp.y, z = sp.z;
  const float qx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  const float qy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  const float qz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
  float best;
  int bs;
  nn_search<true>(qx, qy, qz, TP, tstart, g, 1.0e300, best, bs);
  key[s] = best;
  corr[s] = (bs >= 0 && (double)best < dmax2) ? bs : -1;
}

// the covariance of sorted point s as its upper triangle (xx xy xz yy yz zz): the general route's six doubles (c6[a * n + s]), or the tuned
// route's unit normal expanded as the getters expand it, C = I - 0.999 n n^T (fast_gicp_impl.hpp:280-293)
template <bool kGeneral>
__device__ __forceinline__ void gicp_cov6(const double* __restrict__ c6, const double* __restrict__ nx, const double* __restrict__ ny,
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

// inverse of a symmetric 3x3 by its adjugate; false (M untouched) if the determinant is exactly zero
__device__ __forceinline__ bool gicp_inv_sym3(const double S[6], double M[6]) {
  const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  if (det == 0.0) return false;
  const double id = 1.0 / det;
  M[0] = c00 * id; M[1] = c01 * id; M[2] = c02 * id;
  M[3] = (a * f - c * c) * id; M[4] = (b * c - a * e) * id; M[5] = (a * d - b * b) * id;
  return true;
}

// Sum of the block's NACC accumulators in a FIXED order: the six shuffle steps of a wave, then the four waves ascending.  row: NACC doubles.
template <int NACC>
__device__ __forceinline__ void gicp_block_store(double (&acc)[NACC], double* __restrict__ row) {
  __shared__ double red[GICP_T / GICP_WAVE][NACC];
  const int lane = threadIdx.x & (GICP_WAVE - 1), w = threadIdx.x / GICP_WAVE;
#pragma unroll
  for (int a = 0; a < NACC; a++) {
    double v = acc[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) red[w][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < GICP_T / GICP_WAVE; j++) t += red[j][threadIdx.x];
    row[threadIdx.x] = t;
  }
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
    gicp_cov6<kGenA>(c6A, nxA, nyA, nzA, ns, s, CA);
    gicp_cov6<kGenB>(c6B, nxB, nyB, nzB, nt, j, CB);
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
    gicp_inv_sym3(S, M);
#pragma unroll
    for (int a = 0; a < 6; a++) Mout[(size_t)a * ns + s] = M[a];
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const double e0 = (double)tp.x - q0, e1 = (double)tp.y - q1, e2 = (double)tp.z - q2;
    const double Me0 = M[0] * e0 + M[1] * e1 + M[2] * e2;
    const double Me1 = M[1] * e0 + M[3] * e1 + M[4] * e2;
    const double Me2 = M[2] * e0 + M[4] * e1 + M[5] * e2;
    acc[27] = e0 * Me0 + e1 * Me1 + e2 * Me2;
    acc[28] = 1.0;
    if (want_H) {
      // J = [skew(a) | -I] (3 x 6), columns [rotation, translation] (:188-190)
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
          acc[u] = J[0][a] * MJ[0][c] + J[1][a] * MJ[1][c] + J[2][a] * MJ[2][c];
          u++;
        }
      }
#pragma unroll
      for (int a = 0; a < 6; a++) acc[21 + a] = J[0][a] * Me0 + J[1][a] * Me1 + J[2][a] * Me2;
    }
  }
  gicp_block_store<kGicpAcc>(acc, partials + (size_t)blockIdx.x * kGicpAcc);
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
  gicp_block_store<1>(acc, partials + blockIdx.x);
}

// the workgroups' rows folded in a fixed order, one wave per column: lane l adds rows l, l + 64, ... ascending, then the wave's shuffle tree
__global__ void __launch_bounds__(GICP_WAVE) k_gicp_fold(const double* __restrict__ partials, int nb, int ncol, double* __restrict__ out) {
  const int col = blockIdx.x, lane = threadIdx.x;
  double t = 0.0;
  for (int b = lane; b < nb; b += GICP_WAVE) t += partials[(size_t)b * ncol + col];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
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

void gicp_export(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const float* key, int* idx, float* sq) {
  const int nb = gicp_blocks(src.n);
  if (nb > 0) hipLaunchKernelGGL(k_gicp_export, dim3(nb), dim3(GICP_T), 0, s, src.P, src.n, tgt.P, tgt.n, corr, key, idx, sq);
}

}  // namespace rgck
