// rgc_ndt.hip -- gfx950 kernels of the NDT registration (P2D / D2D) on a Gaussian voxel map.  Reference: fast_gicp::NDTCuda, whose only body is
// CUDA (src/fast_gicp/cuda/ndt_cuda.cu, src/fast_gicp/cuda/ndt_compute_derivatives.cu, src/fast_gicp/cuda/gaussian_voxelmap.cu,
// src/fast_gicp/cuda/covariance_regularization.cu); written from its formulas, in the project's arithmetic: fp32 points, everything after them fp64,
// every sum in a fixed order, no floating-point atomics.  Citations are relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own, over the pieces every solver shares: the term, R C R^T and the block store with the term count are
// rgc_terms.h's, the inverse rgc_cov.h's.  Its own on purpose: ndt_jacobi_rot / ndt_min_eig (another threshold and closed form than rgc_cov.h's
// jacobi_rot) and k_ndt_fold (one lane adds the rows sequentially: another order than fold_column's).
#include "rgc_kernels.h"
#include "rgc_cov.h"
#include "rgc_terms.h"

#include <climits>

namespace rgck {

constexpr int NDT_T = 256;   // threads per workgroup of the term kernels
constexpr int NDT_WAVE = 64;

// One Jacobi rotation in the (P, Q) plane of the symmetric A, accumulated into V (columns = eigenvectors).  Every index is a template
// argument: A and V live in registers.
template <int P, int Q>
__device__ __forceinline__ void ndt_jacobi_rot(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q];
  if (fabs(apq) <= 1.0e-20 * (fabs(A[P][P]) + fabs(A[Q][Q]))) {  // nothing left to rotate away (a repeated eigenvalue of a diagonal block included)
    A[P][Q] = A[Q][P] = 0.0;
    return;
  }
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = cs * arp - sn * arq;
  A[R][Q] = A[Q][R] = sn * arp + cs * arq;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double vp = V[r][P], vq = V[r][Q];
    V[r][P] = cs * vp - sn * vq;
    V[r][Q] = sn * vp + cs * vq;
  }
}

// MIN_EIG (src/fast_gicp/cuda/covariance_regularization.cu:83-100): symmetric eigen-decomposition, every eigenvalue raised to at least 1e-3,
// recomposed -- and the inverse from the same factors (sum of v v^T / lambda), so that no term ever inverts a target covariance.
// Cyclic Jacobi: its eigenvectors are orthonormal to rounding whatever the spectrum, which is what the recomposition needs -- a voxel on a
// wall has two eigenvalues far above the clamp and one below, a voxel of seven collinear points two below and equal.
__device__ __forceinline__ void ndt_min_eig(const double S[6], double C[6], double Ci[6]) {
  double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 12; sweep++) {
    if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
    ndt_jacobi_rot<0, 1>(A, V);
    ndt_jacobi_rot<0, 2>(A, V);
    ndt_jacobi_rot<1, 2>(A, V);
  }
#pragma unroll
  for (int a = 0; a < 6; a++) { C[a] = 0.0; Ci[a] = 0.0; }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double l = fmax(A[k][k], 1.0e-3), li = 1.0 / l;
    int u = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = a; b < 3; b++) {
        const double vv = V[a][k] * V[b][k];
        C[u] += l * vv;
        Ci[u] += li * vv;
        u++;
      }
  }
}

// src/fast_gicp/cuda/gaussian_voxelmap.cu:122-148,178-198,209-231: per voxel n, mean = sum p / n, cov = (sum p p^T - mean (sum p)^T) / n (upper triangle,
// mirrored), the sums in ASCENDING point index -- the sorted array holds a cell's points in that order (k_rank_gather).  One lane per grid cell.
__global__ void __launch_bounds__(256) k_ndt_voxels(const float4* __restrict__ P, const int* __restrict__ start, int ncell, const int* __restrict__ cell_voxel,
                                                     double* __restrict__ vox, int* __restrict__ vox_cell) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= ncell) return;
  const int v = cell_voxel[cell];
  if (v < 0) return;
  const int s0 = start[cell], s1 = start[cell + 1];
  double s[3] = {0.0, 0.0, 0.0}, q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = s0; i < s1; i++) {
    const float4 p = P[i];
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    s[0] += x; s[1] += y; s[2] += z;
    q[0] += x * x; q[1] += x * y; q[2] += x * z; q[3] += y * y; q[4] += y * z; q[5] += z * z;
  }
  const double num = (double)(s1 - s0);
  const double m[3] = {s[0] / num, s[1] / num, s[2] / num};
  const double raw[6] = {(q[0] - m[0] * s[0]) / num, (q[1] - m[0] * s[1]) / num, (q[2] - m[0] * s[2]) / num,
                         (q[3] - m[1] * s[1]) / num, (q[4] - m[1] * s[2]) / num, (q[5] - m[2] * s[2]) / num};
  double C[6], Ci[6];
  ndt_min_eig(raw, C, Ci);
  double* rec = vox + (size_t)v * kNdtRec;
  rec[0] = m[0]; rec[1] = m[1]; rec[2] = m[2];
#pragma unroll
  for (int a = 0; a < 6; a++) { rec[3 + a] = C[a]; rec[10 + a] = Ci[a]; rec[16 + a] = raw[a]; }
  rec[9] = num;
  rec[22] = 0.0; rec[23] = 0.0;
  vox_cell[v] = cell;
}

__device__ __forceinline__ int ndt_coord(double x, double res) {
  const double u = floor(x / res - 0.5);
  return fabs(u) < 1.0e9 ? (int)u : INT_MIN;  // (a coordinate no grid holds: no voxel)
}

// The terms of one source element (src/fast_gicp/cuda/ndt_compute_derivatives.cu:50-91 P2D, :120-163 D2D) over every offset of the neighbour
// method (src/fast_gicp/cuda/find_voxel_correspondences.cu:55-60,92-110: each (element, offset) hit is a term of its own).
//   kD2D : the element is voxel i of the SOURCE's own map (mean, clamped covariance), M = (cov_B + R_lin cov_A R_lin^T)^-1;
//          else source point i, M = the inverse stored with the target voxel.
//   kFind: linearize -- the voxels are looked up at T and written to corr_v[o * n + i] (-1: none, or a voxel of n <= 6 points);
//          else compute_error -- the list of the last linearisation is read back.
// One lane per element; 21 + 6 + 1 accumulators per lane.
template <bool kD2D, bool kFind>
__global__ void __launch_bounds__(NDT_T) k_ndt_terms(const float* __restrict__ in, int stride_f, const double* __restrict__ svox, int n, Pose T, Pose Tlin, Grid g,
                                                      const int* __restrict__ cell_voxel, const double* __restrict__ vox, const int* __restrict__ offs, int noff,
                                                      int* __restrict__ corr_v, int want_H, double* __restrict__ partials, int* __restrict__ ipartials) {
  const int i = blockIdx.x * NDT_T + threadIdx.x;
  double acc[kAccum];
#pragma unroll
  for (int a = 0; a < kAccum; a++) acc[a] = 0.0;
  int nterm = 0;
  if (i < n) {
    double p0, p1, p2;
    double RCR[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (kD2D) {
      const double* sr = svox + (size_t)i * kNdtRec;
      p0 = sr[0]; p1 = sr[1]; p2 = sr[2];
      const double CA[6] = {sr[3], sr[4], sr[5], sr[6], sr[7], sr[8]};
      rcrt6(Tlin.R, CA, RCR);
    } else {
      const float* p = in + (size_t)i * stride_f;
      p0 = (double)p[0]; p1 = (double)p[1]; p2 = (double)p[2];
    }
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    int cx = 0, cy = 0, cz = 0;
    bool in_range = true;
    if (kFind) {
      cx = ndt_coord(q0, g.res); cy = ndt_coord(q1, g.res); cz = ndt_coord(q2, g.res);
      in_range = cx != INT_MIN && cy != INT_MIN && cz != INT_MIN;
      if (in_range) { cx -= g.minc[0]; cy -= g.minc[1]; cz -= g.minc[2]; }
    }
    const double res2 = g.res * g.res;
    for (int o = 0; o < noff; o++) {
      const size_t slot = (size_t)o * n + i;
      int v = -1;
      if (kFind) {
        const int x = cx + offs[3 * o], y = cy + offs[3 * o + 1], z = cz + offs[3 * o + 2];
        if (in_range && x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) v = cell_voxel[cell_index(g, x, y, z)];
        if (v >= 0 && !(vox[(size_t)v * kNdtRec + 9] > 6.0)) v = -1;  // num_points <= 6: no term (:61-63, :132-134)
        corr_v[slot] = v;
      } else {
        v = corr_v[slot];
      }
      if (v < 0) continue;
      const double* rec = vox + (size_t)v * kNdtRec;
      double M[6];
      if (kD2D) {
        double S[6];
#pragma unroll
        for (int a = 0; a < 6; a++) S[a] = rec[3 + a] + RCR[a];
        if (!inv_sym3(S, M)) {
#pragma unroll
          for (int a = 0; a < 6; a++) M[a] = 0.0;
        }
      } else {
#pragma unroll
        for (int a = 0; a < 6; a++) M[a] = rec[10 + a];
      }
      nterm++;
      const double e0 = rec[0] - q0, e1 = rec[1] - q1, e2 = rec[2] - q2;
      const double w = res2 / (res2 + (e0 * e0 + e1 * e1 + e2 * e2));  // Cauchy (:15-18,78,150)
      gn_term<true>(M, q0, q1, q2, e0, e1, e2, w, want_H, acc);  // cost += w e^T M e, H += w J^T M J, b += w J^T M e (:81-88)
    }
  }
  block_sum_count_store<NDT_T>(acc, nterm, partials + (size_t)blockIdx.x * kAccum, ipartials + blockIdx.x);
}

// the workgroups' rows in ascending order: out[0 .. kAccum) the sums, out[kAccum] the number of terms
__global__ void __launch_bounds__(NDT_WAVE) k_ndt_fold(const double* __restrict__ partials, const int* __restrict__ ipartials, int nb, double* __restrict__ out) {
  const int a = threadIdx.x;
  if (a < kAccum) {
    double t = 0.0;
    for (int b = 0; b < nb; b++) t += partials[(size_t)b * kAccum + a];
    out[a] = t;
  } else if (a == kAccum) {
    long long t = 0;
    for (int b = 0; b < nb; b++) t += ipartials[b];
    out[a] = (double)t;
  }
}

int ndt_blocks(int n) { return (n + NDT_T - 1) / NDT_T; }

void ndt_voxels(hipStream_t s, const SortedCloud& cl, const VoxelMap& vm) {
  const int ncell = cl.grid.ncell;
  if (ncell > 0) hipLaunchKernelGGL(k_ndt_voxels, dim3((ncell + 255) / 256), dim3(256), 0, s, cl.P, cl.start, ncell, vm.cell_voxel, vm.vox, vm.vox_cell);
}

void ndt_terms(hipStream_t s, int d2d, int find, const float* in, int stride_f, const double* svox, int n, Pose T, Pose Tlin, const Grid& g,
               const VoxelMap& vm, const int* offs, int noff, int* corr_v, int want_H, double* partials, int* ipartials, double* out29) {
  const int nb = ndt_blocks(n);
  if (nb <= 0) return;
#define NDT_LAUNCH(D, F) \
  hipLaunchKernelGGL((k_ndt_terms<D, F>), dim3(nb), dim3(NDT_T), 0, s, in, stride_f, svox, n, T, Tlin, g, vm.cell_voxel, vm.vox, offs, noff, corr_v, want_H, partials, ipartials)
  if (d2d) { if (find) NDT_LAUNCH(true, true); else NDT_LAUNCH(true, false); }
  else     { if (find) NDT_LAUNCH(false, true); else NDT_LAUNCH(false, false); }
#undef NDT_LAUNCH
  hipLaunchKernelGGL(k_ndt_fold, dim3(1), dim3(NDT_WAVE), 0, s, partials, ipartials, nb, out29);
}

}  // namespace rgck
