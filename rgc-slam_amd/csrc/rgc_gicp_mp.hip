// rgc_gicp_mp.hip -- gfx950 kernels of FastGICPMultiPoints: GICP of every source point against the distance-weighted merge of EVERY target Gaussian
// within a radius of it.  Reference: fast_gicp::FastGICPMultiPoints (include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp,
// include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:92-221); written from its formulas, in the project's arithmetic: the query and the search
// key in fp32 (never FMA-contracted: -ffp-contract=off), everything after them fp64, every sum in a fixed order, no floating-point atomics.
// Citations are relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own, over the pieces every solver shares: the term (under W = M M), the covariance of a sorted point, the shuffle-tree
// block store and the column fold are rgc_terms.h's, the inverse rgc_cov.h's, the fp32 query and the ball's walk rgc_nn.h's.  The radius gather (k_gicp_mp_merge: fp32
// candidates, eleven fp64 accumulators) and the term (k_gicp_mp_terms: 30 accumulators) are two kernels, as in rgc_gicp.hip -- no spill, no private
// segment, no accumulator registers; nothing waits on another workgroup.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_cov.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int MP_T = 256;     // threads per workgroup
constexpr int MP_WAVE = 64;
// Lanes per query of the gather.  A query's neighbour count ranges from none to the whole target, so one lane per query leaves a wave waiting for
// its longest row; a group of lanes strides the candidates of one query and folds its accumulators in a fixed shuffle tree.  8 was the fastest of
// 1, 8, 16 and 64 on the measured clouds (30 k-point scans, 24 to 123 candidates per query; EXPERIMENTS.md, "FastGICPMultiPoints").
#ifdef RGC_LAB_MP_GROUP  // developer build (-DRGC_LAB_MP_GROUP=1|8|16|64): the group sizes scripts/bench_gicp_mp.py compares
constexpr int MP_GROUP = RGC_LAB_MP_GROUP;
#else
constexpr int MP_GROUP = 8;
#endif
static_assert(MP_GROUP >= 1 && MP_GROUP <= MP_WAVE && !(MP_GROUP & (MP_GROUP - 1)), "a power of two of lanes within a wave");

int gicp_mp_blocks(int n) { return (n + MP_T - 1) / MP_T; }

// Every candidate of the query q: the rows of the ball's block of cells (ball_block / ball_rows of rgc_nn.h, where reach = r (1 + 1e-5) is argued),
// one at a time.  Lane `lane` of a group of G takes every G-th candidate of the concatenated ranges (the carry-over rule).  f(i): sorted position i.
// Returns the number of candidates (of all lanes).
template <int G, typename F>
__device__ __forceinline__ int mp_walk(const double q[3], double reach, const int* __restrict__ tstart, const Grid& g, int lane, F&& f) {
  int cnt = 0;
  ball_rows<1>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&a)[1], const int (&b)[1]) {
    int i = first_carried<G>(a[0], lane, cnt);
    cnt += b[0] - a[0];
    for (; i < b[0]; i += G) f(i);
    return true;
  });
  return cnt;
}

constexpr int kMpMerged = kGicpMpMerged;  // count, sum of weights, mean (3), covariance (6: xx xy xz yy yz zz)

// fast_gicp_mp_impl.hpp:139-153 (update_correspondences: the radius search) and :180-195 (the merge of loss_ls) for sorted source point s, by a
// group of G lanes: N = every target point whose fp32 key ((dx dx + dy dy) + dz dz) < r2, strict (pcl::KdTreeFLANN::radiusSearch's rule, r2 =
// float(r r)); w = max(1e-3, min(1, 1 - float(sqrt(key)) / r)) (:184-185; the fp32 square root, correctly rounded: the fp64 root of an fp32 value
// rounded to fp32 is that); sw = sum w, mean = sum w b / sw, cov = sum w C_B / sw, fp64 (the reference's casts of the two to fp32 are not made).
// Order of a sum: a lane's candidates ascending in the sorted target, then the group's shuffle tree.  out: SoA [kMpMerged][ns], zeros behind a count
// of 0.  cand (nullable): candidates looked at per query.
template <int G, bool kGenB>
__global__ void __launch_bounds__(MP_T) k_gicp_mp_merge(const float4* __restrict__ SP, int ns, PoseF T, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                                        Grid g, int nt, float r2, double r, double reach, const double* __restrict__ c6B,
                                                        const double* __restrict__ nxB, const double* __restrict__ nyB, const double* __restrict__ nzB,
                                                        double* __restrict__ out, int* __restrict__ cand) {
  const int s = blockIdx.x * (MP_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  double acc[kMpMerged];
#pragma unroll
  for (int a = 0; a < kMpMerged; a++) acc[a] = 0.0;
  int ncand = 0;
  if (s < ns) {  // (a whole group takes this branch or none of it does)
    float qx, qy, qz;
    const float4 sp = SP[s];
    transform_f32(T, sp.x, sp.y, sp.z, qx, qy, qz);  // fast_gicp_mp_impl.hpp:141
    const double q[3] = {(double)qx, (double)qy, (double)qz};
    ncand = mp_walk<G>(q, reach, tstart, g, lane, [&](int i) {
      const float4 cp = point_at(TP, (unsigned)i << 4);
      const float key = dist2(qx, qy, qz, cp);
      if (key < r2) {
        const double w = fmax(1e-3, fmin(1.0, 1.0 - (double)(float)sqrt((double)key) / r));
        double C[6];
        point_cov6<kGenB>(c6B, nxB, nyB, nzB, nt, i, C);
        acc[0] += 1.0;
        acc[1] += w;
        acc[2] += w * (double)cp.x; acc[3] += w * (double)cp.y; acc[4] += w * (double)cp.z;
#pragma unroll
        for (int a = 0; a < 6; a++) acc[5 + a] += w * C[a];
      }
    });
  }
  if (G > 1) {
#pragma unroll
    for (int a = 0; a < kMpMerged; a++) {
      double v = acc[a];
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) v += __shfl_down(v, o, G);
      acc[a] = v;
    }
  }
  if (s < ns && lane == 0) {
    const bool any = acc[0] > 0.0;
    out[s] = acc[0];
    out[(size_t)ns + s] = acc[1];
#pragma unroll
    for (int a = 2; a < kMpMerged; a++) out[(size_t)a * ns + s] = any ? acc[a] / acc[1] : 0.0;
    if (cand) cand[s] = ncand;
  }
}

constexpr int kMpAcc = kGicpMpAcc;  // 21 upper-triangular H, 6 b, the cost, the source points with a neighbour, the neighbours (exact in a double: < 2^53)

// fast_gicp_mp_impl.hpp:197-213 for sorted source point s with a non-empty ball (:176): a = R p + t, d = mean_B - a, M = (cov_B + R C_A[s] R^T)^-1
// (the 3x3 block of the reference's 4x4 with RCR(3,3) = 1, :199-202), loss l = M d (:203,212), J = M [skew(a) | -I] (:205-209,213).  The system is
// plain Gauss-Newton over those rows: with D = [skew(a) | -I] and W = M M, cost += d^T W d, H += D^T W D, b += D^T W d -- the weighting is M SQUARED,
// the reference's definition, not GICP's M.  One lane per sorted source point.
template <bool kGenA>
__global__ void __launch_bounds__(MP_T) k_gicp_mp_terms(const float4* __restrict__ SP, int ns, const double* __restrict__ merged, const double* __restrict__ c6A,
                                                        const double* __restrict__ nxA, const double* __restrict__ nyA, const double* __restrict__ nzA, Pose T,
                                                        int want_H, double* __restrict__ partials) {
  const int s = blockIdx.x * MP_T + threadIdx.x;
  double acc[kMpAcc];
#pragma unroll
  for (int a = 0; a < kMpAcc; a++) acc[a] = 0.0;
  const double count = s < ns ? merged[s] : 0.0;
  if (count > 0.0) {
    const float4 sp = SP[s];
    const double p0 = (double)sp.x, p1 = (double)sp.y, p2 = (double)sp.z;
    double CA[6], S[6];
    point_cov6<kGenA>(c6A, nxA, nyA, nzA, ns, s, CA);
    // (R C_A R^T in place, as in k_gicp_terms and for its reason: rgc_terms.h, rcrt6)
    const double Cs[3][3] = {{CA[0], CA[1], CA[2]}, {CA[1], CA[3], CA[4]}, {CA[2], CA[4], CA[5]}};
    double RC[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) RC[a][b] = T.R[3 * a] * Cs[0][b] + T.R[3 * a + 1] * Cs[1][b] + T.R[3 * a + 2] * Cs[2][b];
    {
      int u = 0;
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++) {
          S[u] = merged[(size_t)(5 + u) * ns + s] + (RC[a][0] * T.R[3 * b] + RC[a][1] * T.R[3 * b + 1] + RC[a][2] * T.R[3 * b + 2]);
          u++;
        }
    }
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    inv_sym3(S, M);
    // W = M M (symmetric: M is)
    const double W[6] = {M[0] * M[0] + M[1] * M[1] + M[2] * M[2], M[0] * M[1] + M[1] * M[3] + M[2] * M[4], M[0] * M[2] + M[1] * M[4] + M[2] * M[5],
                         M[1] * M[1] + M[3] * M[3] + M[4] * M[4], M[1] * M[2] + M[3] * M[4] + M[4] * M[5], M[2] * M[2] + M[4] * M[4] + M[5] * M[5]};
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const double e0 = merged[(size_t)2 * ns + s] - q0, e1 = merged[(size_t)3 * ns + s] - q1, e2 = merged[(size_t)4 * ns + s] - q2;
    gn_term<false>(W, q0, q1, q2, e0, e1, e2, 1.0, want_H, acc);  // the term under W = M M; no weight
    acc[28] = 1.0;
    acc[29] = count;
  }
  block_sum_store<MP_T>(acc, partials + (size_t)blockIdx.x * kMpAcc);
}

// the workgroups' rows folded in a fixed order, one wave per column (fold_column)
__global__ void __launch_bounds__(MP_WAVE) k_gicp_mp_fold(const double* __restrict__ partials, int nb, int ncol, double* __restrict__ out) {
  const int col = blockIdx.x, lane = threadIdx.x;
  const double t = fold_column(partials, nb, ncol, col, lane);
  if (lane == 0) out[col] = t;
}

// the merge's results in CALLER order (each output nullable): count[i], sum_w[i], mean3[3 i ..], cov6[6 i ..] of source point i
__global__ void __launch_bounds__(MP_T) k_gicp_mp_export(const float4* __restrict__ SP, int ns, const double* __restrict__ merged, int* __restrict__ count,
                                                         double* __restrict__ sum_w, double* __restrict__ mean3, double* __restrict__ cov6) {
  const int s = blockIdx.x * MP_T + threadIdx.x;
  if (s >= ns) return;
  const int o = __float_as_int(SP[s].w);
  if (o < 0 || o >= ns) return;
  if (count) count[o] = (int)merged[s];
  if (sum_w) sum_w[o] = merged[(size_t)ns + s];
  if (mean3) {
#pragma unroll
    for (int a = 0; a < 3; a++) mean3[(size_t)3 * o + a] = merged[(size_t)(2 + a) * ns + s];
  }
  if (cov6) {
#pragma unroll
    for (int a = 0; a < 6; a++) cov6[(size_t)6 * o + a] = merged[(size_t)(5 + a) * ns + s];
  }
}

// the rows N_i in CSR form and caller order: off = the exclusive scan of the counts k_gicp_mp_export leaves (off[o] .. off[o + 1]); one lane per
// sorted source point walks its candidates again -- the same fp32 query, key and strict test as the merge -- and writes its members' original
// indices and keys, ascending in the sorted target (a fixed order: the same from run to run)
__global__ void __launch_bounds__(MP_T) k_gicp_mp_fill(const float4* __restrict__ SP, int ns, PoseF T, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                                       Grid g, float r2, double reach, const int* __restrict__ off, int* __restrict__ idx, float* __restrict__ sq) {
  const int s = blockIdx.x * MP_T + threadIdx.x;
  if (s >= ns) return;
  const float4 sp = SP[s];
  const int o = __float_as_int(sp.w);
  if (o < 0 || o >= ns) return;
  float qx, qy, qz;
  transform_f32(T, sp.x, sp.y, sp.z, qx, qy, qz);
  const double q[3] = {(double)qx, (double)qy, (double)qz};
  int at = off[o];
  const int end = off[o + 1];
  mp_walk<1>(q, reach, tstart, g, 0, [&](int i) {
    const float4 cp = point_at(TP, (unsigned)i << 4);
    const float key = dist2(qx, qy, qz, cp);
    if (key < r2 && at < end) {
      idx[at] = __float_as_int(cp.w);
      sq[at] = key;
      at++;
    }
  });
}

void gicp_mp_merge(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, const GicpCov& B, float r2, double r, double* merged, int* cand) {
  const long long lanes = (long long)src.n * MP_GROUP;
  const int nb = (int)((lanes + MP_T - 1) / MP_T);
  if (nb <= 0) return;
  const double reach = r * (1.0 + 1e-5);
  if (B.c6)
    hipLaunchKernelGGL((k_gicp_mp_merge<MP_GROUP, true>), dim3(nb), dim3(MP_T), 0, s, src.P, src.n, T, tgt.P, tgt.start, tgt.grid, tgt.n, r2, r, reach, B.c6, B.nx, B.ny,
                       B.nz, merged, cand);
  else
    hipLaunchKernelGGL((k_gicp_mp_merge<MP_GROUP, false>), dim3(nb), dim3(MP_T), 0, s, src.P, src.n, T, tgt.P, tgt.start, tgt.grid, tgt.n, r2, r, reach, B.c6, B.nx, B.ny,
                       B.nz, merged, cand);
}

void gicp_mp_terms(hipStream_t s, const SortedCloud& src, const double* merged, const GicpCov& A, Pose T, int want_H, double* partials, double* out30) {
  const int nb = gicp_mp_blocks(src.n);
  if (nb <= 0) return;
  if (A.c6) hipLaunchKernelGGL((k_gicp_mp_terms<true>), dim3(nb), dim3(MP_T), 0, s, src.P, src.n, merged, A.c6, A.nx, A.ny, A.nz, T, want_H, partials);
  else      hipLaunchKernelGGL((k_gicp_mp_terms<false>), dim3(nb), dim3(MP_T), 0, s, src.P, src.n, merged, A.c6, A.nx, A.ny, A.nz, T, want_H, partials);
  hipLaunchKernelGGL(k_gicp_mp_fold, dim3(kMpAcc), dim3(MP_WAVE), 0, s, partials, nb, kMpAcc, out30);
}

void gicp_mp_export(hipStream_t s, const SortedCloud& src, const double* merged, int* count, double* sum_w, double* mean3, double* cov6) {
  const int nb = gicp_mp_blocks(src.n);
  if (nb > 0) hipLaunchKernelGGL(k_gicp_mp_export, dim3(nb), dim3(MP_T), 0, s, src.P, src.n, merged, count, sum_w, mean3, cov6);
}

void gicp_mp_fill(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, float r2, double r, const int* off, int* idx, float* sq) {
  const int nb = gicp_mp_blocks(src.n);
  if (nb > 0)
    hipLaunchKernelGGL(k_gicp_mp_fill, dim3(nb), dim3(MP_T), 0, s, src.P, src.n, T, tgt.P, tgt.start, tgt.grid, r2, r * (1.0 + 1e-5), off, idx, sq);
}

}  // namespace rgck
