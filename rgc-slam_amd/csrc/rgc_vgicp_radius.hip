// rgc_vgicp_radius.hip -- gfx950 kernels of VGICP's DIRECT_RADIUS neighbour method: the linearisation of rgc_kernels.hip's linearize_point over an
// offset TABLE instead of the 1 / 7 / 27 offsets neighbor_offset encodes.  Reference: fast_gicp::FastVGICPCuda::setNeighborSearchMethod(method, radius)
// (include/fast_gicp/gicp/fast_vgicp_cuda.hpp:60, src/fast_gicp/cuda/fast_vgicp_cuda.cu:42-95: the table; src/fast_gicp/cuda/find_voxel_correspondences.cu
// :55-60,92-110: one correspondence per (point, offset) hit; src/fast_gicp/cuda/compute_derivatives.cu:50-92: the term); written from its formulas, in
// the project's arithmetic: fp64 after the fp32 points, every sum in a fixed order, no floating-point atomics, -ffp-contract=off.  Citations are
// relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own (every other code object stays what it was), over the pieces every solver shares: the term, R C R^T, the covariance of
// a sorted point, the shuffle-tree block store and the column fold are rgc_terms.h's, the inverse rgc_cov.h's.  What the linearisation freezes -- the
// voxel found and the Mahalanobis matrix per (offset, point), in the layout of rgck::Corr -- is what rgc_kernels.hip's k_error / k_error_dev read: the
// frozen cost needs no kernel here.  No spill, no private segment, no accumulator registers; nothing waits on another workgroup.
#include "rgc_kernels.h"
#include "rgc_cov.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int VR_T = 256;  // threads per workgroup
// Lanes per source point.  Every point does the SAME number of look-ups, 19 to 485 of them, so one lane per point leaves a 30 k-point scan at ~470
// long-running waves on 256 CUs; a group of G lanes shares a point, lane g taking offsets g, g + G, ...  The point is the FAST index of a
// workgroup's threads (thread t: point t % (VR_T / G), lane t / (VR_T / G)), so that the lanes of a wave hold consecutive points at the same (G <= 4)
// or at 64 * G / VR_T different offsets: the stores of the frozen list (corr_v[o * n + i], corr_M[(a * noff + o) * n + i]) coalesce over i, and
// sorted neighbours at one offset read neighbouring voxels.  The group's fold is part of the block store's fixed tree.  4 was the fastest of 1, 4,
// 8 and 16 at 19, 33 and 123 offsets on a 30 k-point scan (scripts/bench_vgicp_radius.py; EXPERIMENTS.md, "VGICP DIRECT_RADIUS").
#ifdef RGC_LAB_VR_GROUP  // developer build (-DRGC_LAB_VR_GROUP=1|4|8|16): the group sizes scripts/bench_vgicp_radius.py compares
constexpr int VR_GROUP = RGC_LAB_VR_GROUP;
#else
constexpr int VR_GROUP = 4;
#endif
static_assert(VR_GROUP >= 1 && VR_GROUP <= 64 && !(VR_GROUP & (VR_GROUP - 1)), "a power of two of lanes");
constexpr int VR_PPB = VR_T / VR_GROUP;  // points per workgroup

int vgicp_radius_blocks(int n) { return (n + VR_PPB - 1) / VR_PPB; }
int vgicp_radius_group() { return VR_GROUP; }

// R C_A R^T of a source point under its unit normal n, I - 0.999 (R n)(R n)^T: the expressions of the tuned route's linearisation (rgc_kernels.hip)
__device__ __forceinline__ void vr_rcrt6_of_normal(const Pose& T, const double a0, const double a1, const double a2, double (&CA)[6]) {
  const double r0 = T.R[0] * a0 + T.R[1] * a1 + T.R[2] * a2;
  const double r1 = T.R[3] * a0 + T.R[4] * a1 + T.R[5] * a2;
  const double r2 = T.R[6] * a0 + T.R[7] * a1 + T.R[8] * a2;
  CA[0] = 1.0 - 0.999 * r0 * r0; CA[1] = -0.999 * r0 * r1; CA[2] = -0.999 * r0 * r2;
  CA[3] = 1.0 - 0.999 * r1 * r1; CA[4] = -0.999 * r1 * r2; CA[5] = 1.0 - 0.999 * r2 * r2;
}

// FastVGICPCuda's update_correspondences + linearize for sorted source point i by its lane `lane` of G: the pose product and the point's cell exactly
// as linearize_point computes them, then for every offset o = lane, lane + G, ... of the table (offs[o]: x | y << 8 | z << 16, signed bytes) the
// bounds test, the look-up, S = C_B + R C_A R^T, its inverse (zero where S is singular), the term and the count; corr_v / corr_M as linearize_point
// leaves them.  kGeneral: R C_A R^T from the six entries c6 (the general route); else from the unit normal (the tuned route).
// Order of a sum: a lane's offsets ascending, then block_sum_count_store's tree over the workgroup (the lanes of a point among them), then k_vr_fold.
template <bool kGeneral>
__global__ void __launch_bounds__(VR_T)
k_vgicp_radius_linearize(const float4* __restrict__ P, const double* __restrict__ c6, const double* __restrict__ nx, const double* __restrict__ ny,
                         const double* __restrict__ nz, int n, Pose T, Grid g, const int* __restrict__ cell_voxel, const double* __restrict__ vox,
                         const int* __restrict__ offs, int noff, int* __restrict__ corr_v, double* __restrict__ corr_M, int want_H,
                         double* __restrict__ partials, int* __restrict__ ncorr_partials) {
  const int i = blockIdx.x * VR_PPB + (int)(threadIdx.x % VR_PPB), lane = (int)(threadIdx.x / VR_PPB);
  double acc[kAccum];
#pragma unroll
  for (int a = 0; a < kAccum; a++) acc[a] = 0.0;
  int ncorr = 0;
  if (i < n) {
    double CA[6];
    if (kGeneral) {
      double C[6];
      point_cov6<true>(c6, nullptr, nullptr, nullptr, n, i, C);
      rcrt6(T.R, C, CA);
    } else {
      vr_rcrt6_of_normal(T, nx[i], ny[i], nz[i], CA);
    }
    const float4 pp = P[i];
    const double p0 = (double)pp.x, p1 = (double)pp.y, p2 = (double)pp.z;
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const int cx = (int)floor(q0 / g.res - 0.5) - g.minc[0];
    const int cy = (int)floor(q1 / g.res - 0.5) - g.minc[1];
    const int cz = (int)floor(q2 / g.res - 0.5) - g.minc[2];
    for (int o = lane; o < noff; o += VR_GROUP) {
      const int w = offs[o];
      const int x = cx + (int)(signed char)(w & 0xff), y = cy + (int)(signed char)((w >> 8) & 0xff), z = cz + (int)(signed char)((w >> 16) & 0xff);
      int v = -1;
      if (x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) v = cell_voxel[cell_index(g, x, y, z)];
      corr_v[(size_t)o * n + i] = v;
      if (v < 0) continue;
      const double* rec = vox + (size_t)v * kVoxRec;
      double S[6], M[6];
#pragma unroll
      for (int a = 0; a < 6; a++) S[a] = rec[3 + a] + CA[a];
      if (!inv_sym3(S, M)) {
#pragma unroll
        for (int a = 0; a < 6; a++) M[a] = 0.0;
      }
#pragma unroll
      for (int a = 0; a < 6; a++) corr_M[((size_t)a * noff + o) * n + i] = M[a];
      ncorr++;
      const double e0 = rec[0] - q0, e1 = rec[1] - q1, e2 = rec[2] - q2;
      const double wgt = sqrt(rec[9]);
      gn_term<true>(M, q0, q1, q2, e0, e1, e2, wgt, want_H, acc);  // cost += w e^T M e, H += w J^T M J, b += w J^T M e
    }
  }
  block_sum_count_store<VR_T>(acc, ncorr, partials + (size_t)blockIdx.x * kAccum, ncorr_partials + blockIdx.x);
}

// the rows folded in a fixed order: workgroup a (one wave) owns sum a (fold_column); workgroup kAccum folds the integer counts
__global__ void __launch_bounds__(kWaveLanes) k_vr_fold(const double* __restrict__ partials, int nrows, double* __restrict__ out,
                                                        const int* __restrict__ ipartials, int* __restrict__ iout) {
  const int a = blockIdx.x, lane = threadIdx.x;
  if (a < kAccum) {
    const double s = fold_column(partials, nrows, kAccum, a, lane);
    if (lane == 0) out[a] = s;
  } else {
    int c = 0;
    for (int r = lane; r < nrows; r += kWaveLanes) c += ipartials[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (lane == 0) *iout = c;
  }
}

void vgicp_radius_linearize(hipStream_t s, const SortedCloud& src, const GicpCov& A, Pose T, const Grid& g, const VoxelMap& vm, const int* offs, int noff,
                            Corr corr, int want_H, double* partials, int* ncorr_partials, double* out28, int* out_ncorr) {
  const int nb = vgicp_radius_blocks(src.n);
  if (A.c6)
    hipLaunchKernelGGL((k_vgicp_radius_linearize<true>), dim3(nb), dim3(VR_T), 0, s, src.P, A.c6, A.nx, A.ny, A.nz, src.n, T, g, vm.cell_voxel, vm.vox, offs, noff,
                       corr.v, corr.M, want_H, partials, ncorr_partials);
  else
    hipLaunchKernelGGL((k_vgicp_radius_linearize<false>), dim3(nb), dim3(VR_T), 0, s, src.P, A.c6, A.nx, A.ny, A.nz, src.n, T, g, vm.cell_voxel, vm.vox, offs, noff,
                       corr.v, corr.M, want_H, partials, ncorr_partials);
  hipLaunchKernelGGL(k_vr_fold, dim3(kAccum + 1), dim3(kWaveLanes), 0, s, (const double*)partials, nb, out28, (const int*)ncorr_partials, out_ncorr);
}

}  // namespace rgck
