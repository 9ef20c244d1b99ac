// rgc_gicp_st.hip -- gfx950 kernels of FastGICPSingleThread: FastGICP whose correspondences are cached behind an anchor per source point.
// Reference: fast_gicp::FastGICPSingleThread (include/fast_gicp/gicp/fast_gicp_st.hpp:20-65, include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125);
// written from its formulas, in the project's arithmetic: the query, the search keys and the anchor in fp32 (never FMA-contracted:
// -ffp-contract=off), the skip test's roots rounded to fp32 and compared in fp64, everything after them fp64, every sum in a fixed order, no
// floating-point atomics.  Citations are relative to rgc_slam/ of the reference (ROBOT-WSC/RGC-SLAM).
// A translation unit of its own (rgc_gicp.hip's code object stays what it was), over the pieces every solver shares: the term, the covariance of a
// sorted point and the shuffle-tree block store are rgc_terms.h's, the inverse rgc_cov.h's, the fp32 query and the two-nearest search rgc_nn.h's;
// the frozen cost and the column fold are rgc_gicp.hip's own kernels (gicp_error, gicp_fold).  Three kernels per linearisation: the test (one
// lane per source point: query, skip test, compaction of the points to search), the search (one lane per LIST entry: the few points still
// searched late in a solve fill whole waves) and the term (one lane per source point; a searched lane computes and stores M, a skipped lane
// loads it).  No spill, no private segment, no accumulator registers; nothing waits on another workgroup.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_cov.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int ST_T = 256;     // threads per workgroup
constexpr int ST_WAVE = 64;

// fast_gicp_st_impl.hpp:44-54 for sorted source point s: q = T.cast<float>() * p_s (transform_f32); with an anchor a_s (first == 0), d =
// float(sqrt(dist2(q, a_s))), max_first = float(sqrt(key1)) + d, min_second = float(sqrt(key2)) - d, the roots correctly rounded to fp32 and
// the sums in fp64 (:47-49: Eigen's norm() and std::sqrt(float) are fp32, the additions promote); the point keeps everything it has iff
// max_first < min_second (:51, strict).  searched[s] = 0 / 1.  The points to search are appended to `list`: ballot and prefix per wave, one
// integer atomic per wave on *count (zero on entry).  The list's order varies from run to run; no result depends on it.
__global__ void __launch_bounds__(ST_T) k_gicpst_test(const float4* __restrict__ SP, int ns, PoseF T, int first, const float* __restrict__ key1,
                                                      const float* __restrict__ key2, const float4* __restrict__ anchor, int* __restrict__ searched,
                                                      int* __restrict__ list, int* __restrict__ count) {
  const int s = blockIdx.x * ST_T + threadIdx.x;
  bool take = false;
  if (s < ns) {
    take = true;
    if (!first) {
      const float4 sp = SP[s];
      float qx, qy, qz;
      transform_f32(T, sp.x, sp.y, sp.z, qx, qy, qz);
      const double d = (double)(float)sqrt((double)dist2(qx, qy, qz, anchor[s]));
      const double max_first = (double)(float)sqrt((double)key1[s]) + d;
      const double min_second = (double)(float)sqrt((double)key2[s]) - d;
      take = !(max_first < min_second);
    }
    searched[s] = take ? 1 : 0;
  }
  const unsigned long long mask = __ballot(take);  // (every lane of the wave is here: no lane has returned)
  const int lane = threadIdx.x & (ST_WAVE - 1);
  int base = 0;
  if (lane == 0 && mask) base = atomicAdd(count, __popcll(mask));
  base = __shfl(base, 0);
  const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
  if (take && at < ns) list[at] = s;  // (at < ns always: *count never exceeds the points taken -- the guard is for a count that was not zeroed)
}

// fast_gicp_st_impl.hpp:56-61 for list entry e (lanes and workgroups beyond *count exit: the launch is sized for ns, the host does not wait for
// the count): the two nearest target points of q (nn_search2), key1 / key2 their fp32 keys, corr = the nearest's position in the target's
// sorted array iff (double)key1 < d_max^2 (:58, strict) else -1, the anchor <- q (:61).
__global__ void __launch_bounds__(ST_T) k_gicpst_search(const float4* __restrict__ SP, int ns, PoseF T, const float4* __restrict__ TP,
                                                        const int* __restrict__ tstart, Grid g, double dmax2, const int* __restrict__ list,
                                                        const int* __restrict__ count, int* __restrict__ corr, float* __restrict__ key1,
                                                        float* __restrict__ key2, float4* __restrict__ anchor) {
  const int e = blockIdx.x * ST_T + threadIdx.x;
  if (e >= min(*count, ns)) return;
  const int s = list[e];
  if (s < 0 || s >= ns) return;
  const float4 sp = SP[s];
  float qx, qy, qz, best, second;
  transform_f32(T, sp.x, sp.y, sp.z, qx, qy, qz);
  int bs;
  nn_search2(qx, qy, qz, TP, tstart, g, best, bs, second);
  key1[s] = best;
  key2[s] = second;
  corr[s] = (bs >= 0 && (double)best < dmax2) ? bs : -1;
  anchor[s] = make_float4(qx, qy, qz, 0.f);
}

constexpr int kStAcc = kGicpStAcc;  // 21 upper-triangular H, 6 b, the cost, the kept pairs, the points searched (exact in a double: < 2^27)

// fast_gicp_st_impl.hpp:63-75 and :80-120: k_gicp_terms with ONE difference -- a searched lane computes M = (C_B[j] + R C_A[s] R^T)^-1 at this
// pose and stores it (:67-75), a skipped lane loads the M of the pose it was last searched at (:52 skips :56-75).  Then for every pair with
// corr >= 0: a = R p + t, e = b_j - a, cost += e^T M e, J = [skew(a), -I], H += J^T M J, b += J^T M e (:94-116); no weight.  The thirtieth sum is
// the number of points searched: the read-out comes back with the sums.  *count (the compaction's counter) is left at zero.
template <bool kGenA, bool kGenB>
__global__ void __launch_bounds__(ST_T) k_gicpst_terms(const float4* __restrict__ SP, int ns, const float4* __restrict__ TP, int nt, const int* __restrict__ corr,
                                                       const int* __restrict__ searched, const double* __restrict__ c6A, const double* __restrict__ nxA,
                                                       const double* __restrict__ nyA, const double* __restrict__ nzA, const double* __restrict__ c6B,
                                                       const double* __restrict__ nxB, const double* __restrict__ nyB, const double* __restrict__ nzB, Pose T,
                                                       int want_H, double* Mio, double* __restrict__ partials, int* __restrict__ count) {
  const int s = blockIdx.x * ST_T + threadIdx.x;
  if (s == 0) *count = 0;  // the search before this launch has read it; zero again for the next linearisation's test (no memset per linearisation)
  double acc[kStAcc];
#pragma unroll
  for (int a = 0; a < kStAcc; a++) acc[a] = 0.0;
  const int j = s < ns ? corr[s] : -1;
  const int fresh = s < ns ? searched[s] : 0;
  if (j >= 0 && j < nt) {
    const float4 sp = SP[s], tp = TP[j];
    const double p0 = (double)sp.x, p1 = (double)sp.y, p2 = (double)sp.z;
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (fresh) {
      double CA[6], CB[6];
      point_cov6<kGenA>(c6A, nxA, nyA, nzA, ns, s, CA);
      point_cov6<kGenB>(c6B, nxB, nyB, nzB, nt, j, CB);
      // (R C_A R^T in place, as in k_gicp_terms and for its reason: rgc_terms.h, rcrt6)
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
      inv_sym3(S, M);
#pragma unroll
      for (int a = 0; a < 6; a++) Mio[(size_t)a * ns + s] = M[a];
    } else {
#pragma unroll
      for (int a = 0; a < 6; a++) M[a] = Mio[(size_t)a * ns + s];
    }
    const double q0 = T.R[0] * p0 + T.R[1] * p1 + T.R[2] * p2 + T.t[0];
    const double q1 = T.R[3] * p0 + T.R[4] * p1 + T.R[5] * p2 + T.t[1];
    const double q2 = T.R[6] * p0 + T.R[7] * p1 + T.R[8] * p2 + T.t[2];
    const double e0 = (double)tp.x - q0, e1 = (double)tp.y - q1, e2 = (double)tp.z - q2;
    gn_term<false>(M, q0, q1, q2, e0, e1, e2, 1.0, want_H, acc);
    acc[28] = 1.0;
  }
  acc[29] = fresh ? 1.0 : 0.0;
  block_sum_store<ST_T>(acc, partials + (size_t)blockIdx.x * kStAcc);
}

// the state in CALLER order (each output nullable): idx[i] = original index of source point i's neighbour or -1, sq[i] / sq2[i] = its keys to
// the nearest and the second nearest at its anchor, was[i] = 1 iff the last linearisation searched it
__global__ void __launch_bounds__(ST_T) k_gicpst_export(const float4* __restrict__ SP, int ns, const float4* __restrict__ TP, int nt, const int* __restrict__ corr,
                                                        const float* __restrict__ key1, const float* __restrict__ key2, const int* __restrict__ searched,
                                                        int* __restrict__ idx, float* __restrict__ sq, float* __restrict__ sq2, int* __restrict__ was) {
  const int s = blockIdx.x * ST_T + threadIdx.x;
  if (s >= ns) return;
  const int o = __float_as_int(SP[s].w);
  if (o < 0 || o >= ns) return;
  if (idx) {
    const int j = corr[s];
    idx[o] = (j >= 0 && j < nt) ? __float_as_int(TP[j].w) : -1;
  }
  if (sq) sq[o] = key1[s];
  if (sq2) sq2[o] = key2[s];
  if (was) was[o] = searched[s];
}

void gicpst_correspond(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, double dmax2, int first, const GicpStState& st) {
  const int nb = gicp_blocks(src.n);
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_gicpst_test, dim3(nb), dim3(ST_T), 0, s, src.P, src.n, T, first, st.key1, st.key2, st.anchor, st.searched, st.list, st.count);
  hipLaunchKernelGGL(k_gicpst_search, dim3(nb), dim3(ST_T), 0, s, src.P, src.n, T, tgt.P, tgt.start, tgt.grid, dmax2, st.list, st.count, st.corr, st.key1,
                     st.key2, st.anchor);
}

void gicpst_terms(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const GicpStState& st, const GicpCov& A, const GicpCov& B, Pose T, int want_H,
                  double* partials, double* out30) {
  const int nb = gicp_blocks(src.n);
  if (nb <= 0) return;
#define GICPST_LAUNCH(GA, GB) \
  hipLaunchKernelGGL((k_gicpst_terms<GA, GB>), dim3(nb), dim3(ST_T), 0, s, src.P, src.n, tgt.P, tgt.n, st.corr, st.searched, A.c6, A.nx, A.ny, A.nz, B.c6, B.nx, B.ny, B.nz, T, want_H, st.M, partials, st.count)
  if (A.c6) { if (B.c6) GICPST_LAUNCH(true, true); else GICPST_LAUNCH(true, false); }
  else      { if (B.c6) GICPST_LAUNCH(false, true); else GICPST_LAUNCH(false, false); }
#undef GICPST_LAUNCH
  gicp_fold(s, partials, nb, kStAcc, out30);
}

void gicpst_export(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const GicpStState& st, int* idx, float* sq, float* sq2, int* was) {
  const int nb = gicp_blocks(src.n);
  if (nb > 0) hipLaunchKernelGGL(k_gicpst_export, dim3(nb), dim3(ST_T), 0, s, src.P, src.n, tgt.P, tgt.n, st.corr, st.key1, st.key2, st.searched, idx, sq, sq2, was);
}

}  // namespace rgck
