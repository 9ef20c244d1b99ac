// rgc_plane.hip -- gfx950 kernels of RANSAC plane segmentation (rgc_plane_*): pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE
// and SAC_RANSAC over a stream of hypotheses that is scored a BATCH at a time; the host (rgc_api_plane.hip) replays PCL's sequential loop over the
// batch's counts.  The semantics are stated in include/rgc_hip.h: the fp64 model of a triple, the strict fp32 score (never FMA-contracted:
// -ffp-contract=off), exact integer counts, fixed-order fp64 sums for the refinement.  No output bit depends on the launch shape or the batch size.
//
// k_pl_models       one lane per position of the batch: the triple (the caller's samples or plane_sample of rgc_plane.h), the fp64 model, the
//                   validity test (the cross product's bound, finiteness, the axis constraint), the fp32 model (four NaNs when invalid) and the
//                   count's start value (0, or -1 when invalid)
// k_pl_score<PPT>   the hot path.  A workgroup takes a tile of 256 PPT points into registers, walks the batch's models -- wave-uniform, read through
//                   scalar loads -- and counts each model's inliers by ballot and popcount per wave into LDS counters; it takes the tiles blockIdx.x,
//                   blockIdx.x + gridDim.x, ... (a trip count known at launch) and flushes with ONE integer atomicAdd per model and workgroup.
//                   Integer adds are exact and order-free.  Invalid models are skipped.  check != 0 (a call's first walk of the cloud): a
//                   non-finite coordinate sets the non-finite word
// k_pl_flag         flag[i] = point i is within the rule of the final model (inverted by negative), flag[n] = 0; the library's exclusive_scan and
//                   the outlier filters' k_outlier_emit follow
// k_pl_moments<P>   the refinement's fixed-order sums over the inliers in ascending input index, a row per block of 256 consecutive points
//                   (block_sum_store of rgc_terms.h): pass 1 (x, y, z, 1), pass 2 the six products of (p - centroid)
// k_pl_fold_centroid / k_pl_fold_fit   one wave per column (fold_column); then ONE lane: the centroid; S, eig3_sym of rgc_cov.h, the smallest
//                   eigenvector with the RANSAC normal's sign, d, the fp32 model
// No kernel spills, uses scratch or waits for another workgroup; every loop is bounded by a count known at launch; the only atomics are integer adds.
#include "rgc_plane.h"

#include <limits.h>

#include "rgc_cov.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int PL_T = 256;          // threads per workgroup
constexpr int PL_MAX_BLOCKS = 2048;  // k_pl_score's grid cap: the tiles behind it are taken in further passes
// Points per thread of k_pl_score: 1 for a scan-sized cloud (more workgroups than a 30 k-point cloud would otherwise give), 4 beyond
// (scripts/bench_plane.py, EXPERIMENTS.md "Plane segmentation")
#ifdef RGC_LAB_PLANE_PPT  // developer build (-DRGC_LAB_PLANE_PPT=1|2|4|8): that many points per thread at EVERY cloud size, for scripts/bench_plane.py
constexpr int PL_PPT_LARGE = RGC_LAB_PLANE_PPT;
constexpr int PL_SMALL_CLOUD = RGC_LAB_PLANE_PPT == 1 ? INT_MAX : 0;
#else
constexpr int PL_PPT_LARGE = 4;
constexpr int PL_SMALL_CLOUD = 1 << 16;
#endif
constexpr int PL_FETCH = 4;        // models k_pl_score fetches together

__device__ __forceinline__ bool pl_inlier(float a, float b, float c, float d, float x, float y, float z, float thr) {
  return fabsf(((a * x + b * y) + c * z) + d) < thr;
}
__device__ __forceinline__ double pl_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

__global__ void __launch_bounds__(PL_T) k_pl_models(const float* __restrict__ in, int stride_f, int n, PlaneStream st, float4* __restrict__ models,
                                                    int* __restrict__ counts) {
  const int j = blockIdx.x * PL_T + threadIdx.x;
  if (j >= st.batch) return;
  const unsigned long long t = st.t0 + (unsigned long long)j;
  int i0, i1, i2;
  if (st.samples) {
    i0 = st.samples[3 * t]; i1 = st.samples[3 * t + 1]; i2 = st.samples[3 * t + 2];
  } else {
    plane_sample(st.seed, t, n, i0, i1, i2);
  }
  // (the host has checked a caller's samples; the clamp keeps a wrong index inside the cloud all the same)
  i0 = min(max(i0, 0), n - 1); i1 = min(max(i1, 0), n - 1); i2 = min(max(i2, 0), n - 1);
  const float* a = in + (size_t)i0 * stride_f;
  const float* b = in + (size_t)i1 * stride_f;
  const float* c = in + (size_t)i2 * stride_f;
  const double p0x = a[0], p0y = a[1], p0z = a[2];
  const double e1x = (double)b[0] - p0x, e1y = (double)b[1] - p0y, e1z = (double)b[2] - p0z;
  const double e2x = (double)c[0] - p0x, e2y = (double)c[1] - p0y, e2z = (double)c[2] - p0z;
  const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const double cc = pl_dot(cx, cy, cz, cx, cy, cz), a1 = pl_dot(e1x, e1y, e1z, e1x, e1y, e1z), a2 = pl_dot(e2x, e2y, e2z, e2x, e2y, e2z);
  bool ok = cc > 1e-12 * (a1 * a2);
  const double len = sqrt(cc);
  const double nx = cx / len, ny = cy / len, nz = cz / len;
  const double d = -pl_dot(nx, ny, nz, p0x, p0y, p0z);
  const float4 m = make_float4((float)nx, (float)ny, (float)nz, (float)d);
  ok = ok && isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(d) && isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && isfinite(m.w);
  if (ok && st.use_axis) ok = !(fabs(pl_dot(nx, ny, nz, st.axis[0], st.axis[1], st.axis[2])) < st.cos_eps);
  const float qnan = __int_as_float(0x7fc00000);
  models[j] = ok ? m : make_float4(qnan, qnan, qnan, qnan);
  counts[j] = ok ? 0 : -1;
}

template <int PPT>
__global__ void __launch_bounds__(PL_T) k_pl_score(const float* __restrict__ in, int stride_f, int n, float thr, int batch, int passes, int check,
                                                   const float4* __restrict__ models, int* __restrict__ counts, int* __restrict__ nonfinite) {
  __shared__ int cnt[kPlaneMaxBatch];
  for (int j = threadIdx.x; j < batch; j += PL_T) cnt[j] = 0;
  __syncthreads();
  const int lane = threadIdx.x & (kWaveLanes - 1);
  const float qnan = __int_as_float(0x7fc00000);
  for (int pass = 0; pass < passes; pass++) {
    const long long base = ((long long)pass * gridDim.x + blockIdx.x) * (PL_T * PPT) + threadIdx.x;
    float x[PPT], y[PPT], z[PPT];
    bool bad = false;
#pragma unroll
    for (int u = 0; u < PPT; u++) {
      const long long i = base + (long long)u * PL_T;
      x[u] = y[u] = z[u] = qnan;  // (a slot behind the cloud is no model's inlier)
      if (i < n) {
        const float* p = in + (size_t)i * stride_f;
        x[u] = p[0]; y[u] = p[1]; z[u] = p[2];
        bad = bad || !(isfinite(x[u]) && isfinite(y[u]) && isfinite(z[u]));
      }
    }
    if (check && bad) nonfinite[0] = 1;
    if (base - threadIdx.x >= n) continue;  // (workgroup-uniform: the tile lies behind the cloud)
    for (int j0 = 0; j0 < batch; j0 += PL_FETCH) {
      float4 m[PL_FETCH];  // wave-uniform: scalar loads, PL_FETCH models in flight together
#pragma unroll
      for (int v = 0; v < PL_FETCH; v++) m[v] = models[min(j0 + v, batch - 1)];
#pragma unroll
      for (int v = 0; v < PL_FETCH; v++) {
        if (j0 + v >= batch || !(m[v].x == m[v].x)) continue;  // behind the batch, or an invalid position
        int c = 0;
#pragma unroll
        for (int u = 0; u < PPT; u++) c += __popcll(__ballot(pl_inlier(m[v].x, m[v].y, m[v].z, m[v].w, x[u], y[u], z[u], thr)));
        if (lane == 0 && c) atomicAdd(&cnt[j0 + v], c);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < batch; j += PL_T) {
    const int c = cnt[j];
    if (c) atomicAdd(&counts[j], c);
  }
}

__global__ void __launch_bounds__(PL_T) k_pl_flag(const float* __restrict__ in, int stride_f, int n, float thr, const PlaneFit* __restrict__ fit, int negative,
                                                  int* __restrict__ flag) {
  const int i = blockIdx.x * PL_T + threadIdx.x;
  if (i > n) return;
  bool keep = false;
  if (i < n) {
    const float4 m = fit->model;
    const float* p = in + (size_t)i * stride_f;
    keep = pl_inlier(m.x, m.y, m.z, m.w, p[0], p[1], p[2], thr) != (negative != 0);
  }
  flag[i] = keep ? 1 : 0;
}

// block b's row over the points [256 b, 256 b + 256): kPass = 1: (sum x, sum y, sum z, count) of the model's inliers; kPass = 2: the six products of
// (p - centroid), xx xy xz yy yz zz.  A point that is no inlier (or lies behind the cloud) adds +0.0
template <int kPass>
__global__ void __launch_bounds__(PL_T) k_pl_moments(const float* __restrict__ in, int stride_f, int n, float thr, const PlaneFit* __restrict__ fit,
                                                     double* __restrict__ partials) {
  constexpr int NACC = kPass == 1 ? 4 : 6;
  const int i = blockIdx.x * PL_T + threadIdx.x;
  const float4 m = fit->model;
  double acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.0;
  if (i < n) {
    const float* p = in + (size_t)i * stride_f;
    const float x = p[0], y = p[1], z = p[2];
    if (pl_inlier(m.x, m.y, m.z, m.w, x, y, z, thr)) {
      if constexpr (kPass == 1) {
        acc[0] = (double)x; acc[1] = (double)y; acc[2] = (double)z; acc[3] = 1.0;
      } else {
        const double dx = (double)x - fit->centroid[0], dy = (double)y - fit->centroid[1], dz = (double)z - fit->centroid[2];
        acc[0] = dx * dx; acc[1] = dx * dy; acc[2] = dx * dz; acc[3] = dy * dy; acc[4] = dy * dz; acc[5] = dz * dz;
      }
    }
  }
  block_sum_store<PL_T, NACC>(acc, partials + (size_t)blockIdx.x * NACC);
}

// one workgroup of four waves: wave w folds column w of pass 1's rows; then one lane posts the count and the centroid
__global__ void __launch_bounds__(4 * kWaveLanes) k_pl_fold_centroid(const double* __restrict__ partials, int nrows, PlaneFit* __restrict__ fit) {
  __shared__ double tot[4];
  const int w = threadIdx.x / kWaveLanes, lane = threadIdx.x & (kWaveLanes - 1);
  const double s = fold_column(partials, nrows, 4, w, lane);
  if (lane == 0) tot[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double count = tot[3];
    fit->count = count;
    fit->refined = 0;
    for (int a = 0; a < 3; a++) fit->centroid[a] = count >= 3.0 ? tot[a] / count : 0.0;
  }
}

// one workgroup of six waves: wave w folds column w of pass 2's rows; then one lane runs eig3_sym and posts the refined model
__global__ void __launch_bounds__(6 * kWaveLanes) k_pl_fold_fit(const double* __restrict__ partials, int nrows, PlaneFit* __restrict__ fit) {
  __shared__ double tot[6];
  const int w = threadIdx.x / kWaveLanes, lane = threadIdx.x & (kWaveLanes - 1);
  const double s = fold_column(partials, nrows, 6, w, lane);
  if (lane == 0) tot[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double count = fit->count;
    if (count >= 3.0) {
      double S[6], ev[3], V[3][3];
      int ord[3];
      for (int a = 0; a < 6; a++) { S[a] = tot[a] / count; fit->S[a] = S[a]; }
      eig3_sym(S, ev, V, ord);
      const int col = ord[2];  // the smallest eigenvalue's
      for (int a = 0; a < 3; a++) fit->ev[a] = ev[ord[2 - a]];  // ascending
      const float4 m0 = fit->model;
      double vx = col == 0 ? V[0][0] : (col == 1 ? V[0][1] : V[0][2]);
      double vy = col == 0 ? V[1][0] : (col == 1 ? V[1][1] : V[1][2]);
      double vz = col == 0 ? V[2][0] : (col == 1 ? V[2][1] : V[2][2]);
      if (pl_dot(vx, vy, vz, (double)m0.x, (double)m0.y, (double)m0.z) < 0.0) { vx = -vx; vy = -vy; vz = -vz; }
      const double d = -pl_dot(vx, vy, vz, fit->centroid[0], fit->centroid[1], fit->centroid[2]);
      const float4 m = make_float4((float)vx, (float)vy, (float)vz, (float)d);
      if (isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && isfinite(m.w)) {
        fit->model = m;
        fit->refined = 1;
      }
    }
  }
}

static int pl_blocks(long long n) { return (int)((n + PL_T - 1) / PL_T); }
static int pl_ppt(int n) { return n < PL_SMALL_CLOUD ? 1 : PL_PPT_LARGE; }

int plane_moment_rows(int n) { return pl_blocks(n); }

void plane_models(hipStream_t s, const float* in, int stride_f, int n, const PlaneStream& st, const PlaneBatch& b) {
  if (st.batch <= 0) return;
  hipLaunchKernelGGL(k_pl_models, dim3(pl_blocks(st.batch)), dim3(PL_T), 0, s, in, stride_f, n, st, b.models, b.counts);
}

void plane_score(hipStream_t s, const float* in, int stride_f, int n, float thr, int batch, int check, const PlaneBatch& b) {
  if (n <= 0 || batch < 0) return;  // (batch = 0: the non-finite walk alone)
  const int tile = PL_T * pl_ppt(n);
  const long long tiles = ((long long)n + tile - 1) / tile;
  const int nb = (int)(tiles < PL_MAX_BLOCKS ? tiles : PL_MAX_BLOCKS);
  const int passes = (int)((tiles + nb - 1) / nb);
  if (pl_ppt(n) == 1) hipLaunchKernelGGL((k_pl_score<1>), dim3(nb), dim3(PL_T), 0, s, in, stride_f, n, thr, batch, passes, check, b.models, b.counts, b.nonfinite);
  else hipLaunchKernelGGL((k_pl_score<PL_PPT_LARGE>), dim3(nb), dim3(PL_T), 0, s, in, stride_f, n, thr, batch, passes, check, b.models, b.counts, b.nonfinite);
}

void plane_refine(hipStream_t s, const float* in, int stride_f, int n, float thr, double* partials, PlaneFit* fit) {
  const int nb = pl_blocks(n);
  if (nb <= 0) return;
  hipLaunchKernelGGL((k_pl_moments<1>), dim3(nb), dim3(PL_T), 0, s, in, stride_f, n, thr, fit, partials);
  hipLaunchKernelGGL(k_pl_fold_centroid, dim3(1), dim3(4 * kWaveLanes), 0, s, partials, nb, fit);
  hipLaunchKernelGGL((k_pl_moments<2>), dim3(nb), dim3(PL_T), 0, s, in, stride_f, n, thr, fit, partials);
  hipLaunchKernelGGL(k_pl_fold_fit, dim3(1), dim3(6 * kWaveLanes), 0, s, partials, nb, fit);
}

void plane_flag(hipStream_t s, const float* in, int stride_f, int n, float thr, const PlaneFit* fit, int negative, int* flag) {
  hipLaunchKernelGGL(k_pl_flag, dim3(pl_blocks((long long)n + 1)), dim3(PL_T), 0, s, in, stride_f, n, thr, fit, negative, flag);
}

}  // namespace rgck
