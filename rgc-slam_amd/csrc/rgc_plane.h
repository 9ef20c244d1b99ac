// rgc_plane.h -- what the two files of RANSAC plane segmentation share (rgc_plane.hip: the kernels; rgc_api_plane.hip: the host side, rgc_plane_*):
// the counter-based sampler of the hypothesis stream, ONE definition for the host's rgc_plane_sample and the device's k_pl_models, the records that
// travel between them, and the launch wrappers.  The semantics are stated in include/rgc_hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace rgck {

constexpr int kPlaneMaxBatch = 1024;  // RGC_PLANE_MAX_BATCH: k_pl_score's LDS counters
constexpr int kPlaneRowCols = 6;      // doubles per row of the fixed-order sums' partials (pass 1 uses 4 of them)

__host__ __device__ inline unsigned long long plane_mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the triple of stream position t (include/rgc_hip.h: splitmix64 started at seed, its outputs 3t + 1 .. 3t + 3); n >= 3
__host__ __device__ inline void plane_sample(unsigned long long seed, unsigned long long t, int n, int& i0, int& i1, int& i2) {
  const unsigned long long g = 0x9E3779B97F4A7C15ull, un = (unsigned long long)n;
  const unsigned long long r0 = plane_mix64(seed + (3ull * t + 1ull) * g), r1 = plane_mix64(seed + (3ull * t + 2ull) * g), r2 = plane_mix64(seed + (3ull * t + 3ull) * g);
  const unsigned long long a = r0 % un, b = (a + 1ull + r1 % (un - 1ull)) % un;
  const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
  unsigned long long c = r2 % (un - 2ull);
  if (c >= lo) c++;
  if (c >= hi) c++;
  i0 = (int)a; i1 = (int)b; i2 = (int)c;
}

// what k_pl_models needs beside the cloud: where the triples come from and the axis constraint
struct PlaneStream {
  const int* samples;        // device, 3 ints per position, or nullptr: the generator
  unsigned long long seed;
  unsigned long long t0;     // the batch's first stream position
  int batch;                 // positions of this batch
  int use_axis;
  double axis[3];            // normalised
  double cos_eps;
};
// a batch on the device, ONE contiguous read-back: the non-finite word (and padding), the models, the counts
struct PlaneBatch {
  int* nonfinite;            // 4 ints: word 0 != 0: the cloud has a non-finite coordinate
  float4* models;            // batch models; an invalid position's is four NaNs
  int* counts;               // batch counts; an invalid position's is -1
};
// the final model and the refinement's intermediate results (device; read back once at the end of a call)
struct PlaneFit {
  float4 model;              // in: the best RANSAC model (uploaded); out: the model that selects the reported inliers
  int refined, pad;
  double count;              // inliers of the RANSAC model
  double centroid[3];
  double S[6];               // xx xy xz yy yz zz about the centroid, / count
  double ev[3];
};

void plane_models(hipStream_t s, const float* in, int stride_f, int n, const PlaneStream& st, const PlaneBatch& b);
// the hot path: the batch's counts over the whole cloud; check != 0: also the non-finite test of every coordinate
void plane_score(hipStream_t s, const float* in, int stride_f, int n, float thr, int batch, int check, const PlaneBatch& b);
int  plane_moment_rows(int n);   // rows of kPlaneRowCols doubles the refinement needs in `partials`
void plane_refine(hipStream_t s, const float* in, int stride_f, int n, float thr, double* partials, PlaneFit* fit);
// flag[i], i < n: point i is written (inlier of fit->model, inverted by negative); flag[n] = 0
void plane_flag(hipStream_t s, const float* in, int stride_f, int n, float thr, const PlaneFit* fit, int negative, int* flag);

}  // namespace rgck
