// rgc_rbf.hip -- RBF-kernel covariance estimation (the reference's NearestNeighborMethod::GPU_RBF_KERNEL,
// src/fast_gicp/cuda/covariance_estimation_rbf.cu:59-151): a point's covariance is the Gaussian-weighted second moment of every point of
// its cloud within max_dist, not the moment of its k nearest neighbours.
//
// For point i of the sorted cloud P (fp32) the ball is B(i) = { j : key(i, j) <= max_dist_sq }, key the fp32 ((dx*dx + dy*dy) + dz*dz) of
// rgc_nn.h (dist2, never contracted), max_dist_sq = (float)max_dist * (float)max_dist; i itself is a member (key 0).  In fp64, over the
// members in ASCENDING POSITION of the sorted array, one accumulator chain per point:
//     w_j = exp(-(double)(float)kernel_width * (double)key),  d_j = (double)P_j - (double)P_i  (exact),
//     S0 = sum w_j,  S1 = sum w_j d_j,  S2 = sum w_j d_j d_j^T,     m = S1 / S0,  cov = S2 / S0 - m m^T,
// then the selected RegularizationMethod (regularize6, shared with the kNN moment).  This is NormalDistribution::finalize (:46-52) with the
// origin shifted to P_i: the same matrix, without the cancellation the reference's unshifted fp32 sums suffer at map coordinates.
// Membership is decided by `key` alone and the order is the position's, so ANY superset of the ball gives the same bits: how the
// candidates are gathered (workgroup shape, tile size, the reach in cells) cannot show in the result.
//
// Candidates come from the cloud's own cell grid.  A workgroup takes a run of consecutive positions = a run of cells; for every (y, z)
// grid row within reach of the run it takes ONE contiguous span of the sorted array (cells of a row are consecutive), rows in ascending
// cell index, so the spans are disjoint and ascending.  Spans are staged through LDS in tiles; every lane owns one query and walks the
// tile (all lanes read the same LDS address: a broadcast, no bank conflict), holding S0, S1, S2 -- ten doubles -- in registers.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_cov.h"

namespace rgck {

constexpr int RBF_T = 64;      // queries of a workgroup: one wavefront, one lane per query
constexpr int RBF_TILE = 256;  // candidates staged per tile (4 KiB of LDS)

// reach: the largest cell offset (per axis) at which a member of some ball can lie -- floor(max_dist (1 + 2^-20) / res) + 1, rgcapi::rbf_reach;
// reach_dist = max_dist (1 + 2^-20): a cell offset of d >= 1 means a distance above (d - 1) res, and a key that ROUNDS onto max_dist_sq
// belongs to a distance below reach_dist
__global__ void __launch_bounds__(RBF_T)
k_rbf_cov6(const float4* __restrict__ P, const int* __restrict__ start, Grid g, int n, float max_dist_sq, double neg_width, int reach,
           double reach_dist, int method, double* __restrict__ c6, const int* __restrict__ guard) {
  __shared__ float4 tile[RBF_TILE];
  if (guard && *guard) return;
  const int lane = (int)threadIdx.x;
  const int i0 = (int)blockIdx.x * RBF_T;
  if (i0 >= n) return;
  const int i1 = min(i0 + RBF_T, n) - 1;
  const int i = i0 + lane;
  const bool live = i <= i1;
  const float4 q = P[live ? i : i1];
  // the run's box of cells: positions ascend with the cell index (x fastest, then y, then z), so the first and the last query bound it
  // (not rgc_nn.h's ball_block: the box of a RUN of queries widened by `reach` whole cells, not the cells of one query's q -+ reach)
  const float4 qa = P[i0], qb = P[i1];
  int lo[3] = {cell_coord(qa.x, g) - g.minc[0], cell_coord(qa.y, g) - g.minc[1], cell_coord(qa.z, g) - g.minc[2]};
  int hi[3] = {cell_coord(qb.x, g) - g.minc[0], cell_coord(qb.y, g) - g.minc[1], cell_coord(qb.z, g) - g.minc[2]};
  for (int a = 0; a < 3; a++) { lo[a] = min(max(lo[a], 0), g.dim[a] - 1); hi[a] = min(max(hi[a], lo[a]), g.dim[a] - 1); }
  if (lo[2] != hi[2]) { lo[1] = 0; hi[1] = g.dim[1] - 1; }
  if (lo[2] != hi[2] || lo[1] != hi[1]) { lo[0] = 0; hi[0] = g.dim[0] - 1; }
  const int z0 = max(lo[2] - reach, 0), z1 = (int)min((long long)hi[2] + reach, (long long)g.dim[2] - 1);
  const int y0 = max(lo[1] - reach, 0), y1 = (int)min((long long)hi[1] + reach, (long long)g.dim[1] - 1);
  const double R2 = reach_dist * reach_dist;

  double S0 = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0, Sxx = 0.0, Sxy = 0.0, Sxz = 0.0, Syy = 0.0, Syz = 0.0, Szz = 0.0;
  const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
  for (int z = z0; z <= z1; z++) {
    const int dzc = z < lo[2] ? lo[2] - z : (z > hi[2] ? z - hi[2] : 0);
    const double gz = dzc > 0 ? (double)(dzc - 1) * g.res : 0.0;
    for (int y = y0; y <= y1; y++) {
      const int dyc = y < lo[1] ? lo[1] - y : (y > hi[1] ? y - hi[1] : 0);
      const double gy = dyc > 0 ? (double)(dyc - 1) * g.res : 0.0;
      const double rem = R2 - (gy * gy + gz * gz);  // what is left for x: a row farther than reach_dist from every query holds no member
      if (rem < 0.0) continue;
      const double rxd = floor(sqrt(rem) / g.res) + 1.0;
      const int rx = rxd < (double)reach ? (int)rxd : reach;
      const int x0 = max(lo[0] - rx, 0), x1 = (int)min((long long)hi[0] + rx, (long long)g.dim[0] - 1);
      const int s0 = start[cell_index(g, x0, y, z)], s1 = start[cell_index(g, x1, y, z) + 1];
      for (int t0 = s0; t0 < s1; t0 += RBF_TILE) {
        const int cnt = min(RBF_TILE, s1 - t0);
        __syncthreads();  // the previous tile has been walked by every lane
        for (int u = lane; u < cnt; u += RBF_T) tile[u] = P[t0 + u];
        __syncthreads();
        if (live) {
          for (int u = 0; u < cnt; u++) {
            const float4 cp = tile[u];
            const float key = dist2(q.x, q.y, q.z, cp);
            if (key <= max_dist_sq) {
              const double w = exp(neg_width * (double)key);
              const double dx = (double)cp.x - qx, dy = (double)cp.y - qy, dz = (double)cp.z - qz;
              const double wx = w * dx, wy = w * dy, wz = w * dz;
              S0 += w;
              Sx += wx; Sy += wy; Sz += wz;
              Sxx += wx * dx; Sxy += wx * dy; Sxz += wx * dz;
              Syy += wy * dy; Syz += wy * dz; Szz += wz * dz;
            }
          }
        }
      }
    }
  }
  if (!live) return;
  // NormalDistribution::finalize, covariance_estimation_rbf.cu:46-52 (S0 >= 1: the point is a member of its own ball with weight 1)
  const double mx = Sx / S0, my = Sy / S0, mz = Sz / S0;
  const double S[6] = {Sxx / S0 - mx * mx, Sxy / S0 - mx * my, Sxz / S0 - mx * mz, Syy / S0 - my * my, Syz / S0 - my * mz, Szz / S0 - mz * mz};
  double C[6];
  regularize6(S, method, C);
  for (int a = 0; a < 6; a++) c6[(size_t)a * n + i] = C[a];
}

void rbf_cov6(hipStream_t s, const SortedCloud& cl, float kernel_width, float max_dist_sq, int reach, double reach_dist, int method, double* c6, const int* guard) {
  if (cl.n <= 0) return;
  hipLaunchKernelGGL(k_rbf_cov6, dim3((cl.n + RBF_T - 1) / RBF_T), dim3(RBF_T), 0, s, cl.P, cl.start, cl.grid, cl.n, max_dist_sq, -(double)kernel_width, reach,
                     reach_dist, method, c6, guard);
}

}  // namespace rgck
