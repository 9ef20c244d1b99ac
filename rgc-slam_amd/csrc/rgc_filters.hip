// rgc_filters.hip -- gfx950 kernels of the outlier filters (rgc_outlier_*): pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval of a cloud
// against itself, on a grid of the filters' own (rgcapi::OutlierRecord).  The machinery is the search index's (rgc_search.hip, rgc_nn.h): the grid's
// contiguous row ranges, the fp32 key dist2 (never FMA-contracted: -ffp-contract=off), cube_bound, a group of lanes per point.  What is new is a
// consumer that never materialises the rows: the queries ARE the indexed points, walked in the grid's sorted order, and what leaves a group is one
// float (the mean distance) or one int (the ball's count) at the point's ORIGINAL index.  No output bit depends on the grid or the cell size.
//
// k_sor_meandist<KT, G>  the mean_k + 1 (<= KT) smallest KEYS of a sorted point, by a group of G lanes striding the row ranges of the cube of cells
//                        about its cell, with k_search_knn's running count, cube growth and cube_bound exit (the lists start over when the cube
//                        grows).  Each lane keeps an ascending list of KT 32-bit keys (non-negative fp32 bit patterns order as integers) in
//                        registers (list_insert of rgc_nn.h).  The G lists are merged by mean_k + 1 rounds of a group-wide minimum (of tied heads the lowest
//                        lane pops: equal keys have equal roots, the sum does not depend on who wins); the leader drops rank 0 (the point itself or
//                        a duplicate of it) and adds the roots of ranks 1 .. mean_k in fp64 in rank order as the merge proceeds.
// k_sor_stats / k_sor_fold  sum d and sum d d in fp64 IN INPUT-INDEX ORDER with the fixed-order sums of rgc_terms.h; then one lane computes mean,
//                        stddev and threshold and posts them: no host round trip between the passes
// k_ror_count<G, kExact> the members of a sorted point's ball (key < r2, strict), the ball walk of k_search_count, three rows fetched together; kExact = false: the group
//                        stops walking once its count exceeds min_neighbors (the decision is made; the count it writes is then a lower bound)
// k_outlier_flag         the decision of every point in input order (SOR: (double)d <= threshold; ROR: count - 1 >= min_neighbors; negative inverts)
// k_outlier_emit         (after the library's exclusive_scan of the flags) records and indices, ascending input index
// No kernel spills, uses scratch or waits for another workgroup; the only atomics are integer adds of the read-out words.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_terms.h"

namespace rgck {

constexpr int FL_T = 256;  // threads per workgroup
constexpr int FL_WAVE = 64;
// Lanes per point.  Measured for THIS kernel (scripts/bench_outlier.py, EXPERIMENTS.md "Outlier filters"), not inherited from k_search_knn
#ifdef RGC_LAB_OUTLIER_GROUP  // developer build (-DRGC_LAB_OUTLIER_GROUP=2|4|8): the group sizes scripts/bench_outlier.py compares
constexpr int FL_GROUP = RGC_LAB_OUTLIER_GROUP;
#else
constexpr int FL_GROUP = 4;
#endif
static_assert(FL_GROUP >= 2 && FL_GROUP <= 16 && !(FL_GROUP & (FL_GROUP - 1)), "a power of two of lanes, at most 16 (the merge's ballot mask)");
constexpr int FL_ROWS = 3;         // rows of cells whose ranges a group fetches together: a z-layer of the 3 x 3 x 3 block
constexpr unsigned kFlNone = ~0u;  // an empty list slot: behind every key (a key's bits are never 0xffffffff)

int outlier_group() { return FL_GROUP; }

// the read-out words (OutlierStats::words): the group leaders' sums of a workgroup -- a wave's shuffle tree, the waves' sums through LDS -- added into the
// workgroup's slot: one integer atomic per workgroup and word, spread over kStatSlots cache lines.  Called by every thread of the workgroup
__device__ __forceinline__ void fl_stats_add(OutlierStats* st, unsigned long long cand, unsigned long long grew) {
  __shared__ unsigned long long part[FL_T / FL_WAVE][2];
  cand = wave_sum_u64(cand);
  grew = wave_sum_u64(grew);
  if ((threadIdx.x & (FL_WAVE - 1)) == 0) {
    part[threadIdx.x / FL_WAVE][0] = cand;
    part[threadIdx.x / FL_WAVE][1] = grew;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0;
#pragma unroll
    for (int j = 0; j < FL_T / FL_WAVE; j++) t += part[j][threadIdx.x];
    if (t) atomicAdd(&st->words[blockIdx.x & (kStatSlots - 1)][threadIdx.x], t);
  }
}

template <int KT, int G>
__global__ void __launch_bounds__(FL_T) k_sor_meandist(const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g, int n, int k1, float* __restrict__ out_d,
                                                       OutlierStats* __restrict__ st) {
  const int si = blockIdx.x * (FL_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  const int shift = (threadIdx.x & (FL_WAVE - 1)) & ~(G - 1);  // the group's first lane within its wave
  unsigned long long cand = 0, grew = 0;
  if (si < n) {  // (a whole group takes this branch or none of it does)
    const float4 me = point_at(TP, (unsigned)si << 4);
    const float px = me.x, py = me.y, pz = me.z;
    const double q[3] = {(double)px, (double)py, (double)pz};
    // the point's own cell: it was sorted into the grid by this rule, so it lies inside
    const int c[3] = {cell_coord(px, g) - g.minc[0], cell_coord(py, g) - g.minc[1], cell_coord(pz, g) - g.minc[2]};
    int rmax, r;
    cube_first(c, g, r, rmax);  // (r = 1: the cell lies inside)
    unsigned L[KT];
    double sum = 0.0;
    for (;;) {
#pragma unroll
      for (int u = 0; u < KT; u++) L[u] = kFlNone;  // the lists start over at every cube
      int cnt = 0;
      cube_rows<FL_ROWS>(c, r, tstart, g, [&](const int (&ra)[FL_ROWS], const int (&rb)[FL_ROWS]) {
#pragma unroll
        for (int u = 0; u < FL_ROWS; u++) {
          int i = first_carried<G>(ra[u], lane, cnt);
          cnt += rb[u] - ra[u];
          for (; i < rb[u]; i += G) list_insert(L, __float_as_uint(dist2(px, py, pz, point_at(TP, (unsigned)i << 4))));
        }
        return true;
      });
      cand += (unsigned long long)cnt;
      // the G lists merged: k1 rounds of the group's minimum; of the lanes whose head it is the lowest pops
      int found = 0;
      unsigned kth_bits = 0x7f800000u;
      sum = 0.0;
      for (int j = 0; j < k1; j++) {
        const unsigned m = group_min<G>(L[0]);
        const bool any = m != kFlNone;
        const unsigned heads = (unsigned)(__ballot(any && m == L[0]) >> shift) & ((1u << G) - 1u);
        list_pop(L, any && lane == __ffs(heads) - 1);
        if (any) {
          found++;
          kth_bits = m;
          // rank 0 is the point itself or a duplicate of it (key 0): dropped.  sqrtf, correctly rounded, as (float)sqrt((double)key)
          if (j > 0) sum += (double)(float)sqrt((double)__uint_as_float(m));
        }
      }
      if (r >= rmax) break;  // the cube covers the grid: the row holds min(k1, n) = k1 entries (n > mean_k is the caller's)
      const double bound = cube_bound(g, c, q, r);
      if (bound == 1.0e300) break;
      const bool full = found == k1;
      const float kth = __uint_as_float(kth_bits);
      if (full && key_inside(kth, bound)) break;  // the K-TH entry is provably inside the cube
      grew = 1;
      r = cube_next(g, c, q, r, rmax, full, key_reach(kth));
    }
    if (lane == 0) {
      out_d[__float_as_int(me.w)] = (float)(sum / (double)(k1 - 1));
    } else {
      cand = 0;
      grew = 0;
    }
  }
  fl_stats_add(st, cand, grew);
}

// block b's row of the partial sums: (sum d, sum d d) over d[256 b .. 256 b + 256), in the fixed order of block_sum_store; d d is exact in fp64
__global__ void __launch_bounds__(FL_T) k_sor_stats(const float* __restrict__ d, int n, double* __restrict__ partials) {
  const int i = blockIdx.x * FL_T + threadIdx.x;
  const double v = i < n ? (double)d[i] : 0.0;
  double acc[2] = {v, v * v};
  block_sum_store<FL_T, 2>(acc, partials + (size_t)blockIdx.x * 2);
}

// one workgroup of two waves: wave w folds column w of the rows (fold_column), then one lane computes and posts the statistics
__global__ void __launch_bounds__(2 * FL_WAVE) k_sor_fold(const double* __restrict__ partials, int nrows, int n, double std_mul, OutlierStats* __restrict__ st) {
  __shared__ double tot[2];
  const int w = threadIdx.x / FL_WAVE, lane = threadIdx.x & (FL_WAVE - 1);
  const double s = fold_column(partials, nrows, 2, w, lane);
  if (lane == 0) tot[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = tot[0], sq_sum = tot[1], nn = (double)n;
    const double mean = sum / nn;
    const double variance = fmax((sq_sum - sum * sum / nn) / (nn - 1.0), 0.0);  // (PCL takes the root of a negative rounding residue: clamped here)
    const double stddev = sqrt(variance);
    st->mean = mean;
    st->stddev = stddev;
    st->threshold = mean + std_mul * stddev;
  }
}

template <int G, bool kExact>
__global__ void __launch_bounds__(FL_T) k_ror_count(const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g, int n, float r2, double reach, int min_nb,
                                                    int* __restrict__ out_cnt, OutlierStats* __restrict__ st) {
  const int si = blockIdx.x * (FL_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0;
  if (si < n) {
    const float4 me = point_at(TP, (unsigned)si << 4);
    const float px = me.x, py = me.y, pz = me.z;
    const double q[3] = {(double)px, (double)py, (double)pz};
    // the rows of the ball of radius `reach` about the point (ball_block / ball_rows of rgc_nn.h, where reach = r (1 + 1e-5) is argued), the in-step rule
    int mine = 0, total = 0, cnt = 0;
    ball_rows<FL_ROWS>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&ra)[FL_ROWS], const int (&rb)[FL_ROWS]) {
#pragma unroll
      for (int u = 0; u < FL_ROWS; u++) {
        cnt += rb[u] - ra[u];
        for (int i = first_in_step(ra[u], lane); i < rb[u]; i += G) mine += dist2(px, py, pz, point_at(TP, (unsigned)i << 4)) < r2 ? 1 : 0;
      }
      if (kExact) return true;
      // the decision is made once the group's count exceeds min_neighbors (count - 1 >= min_neighbors): once per batch of rows
      total = mine;
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) total += __shfl_xor(total, o, G);
      return total <= min_nb;
    });
    if (kExact) {
      total = mine;
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) total += __shfl_xor(total, o, G);
    }
    if (lane == 0) {
      out_cnt[__float_as_int(me.w)] = total;
      cand = (unsigned long long)cnt;
    }
  }
  fl_stats_add(st, cand, 0);
}

// flag[i], i < n: point i is kept; flag[n] = 0 (the scan's last offset is then the number kept).  d != nullptr: SOR against the posted threshold
__global__ void __launch_bounds__(FL_T) k_outlier_flag(const float* __restrict__ d, const int* __restrict__ cnt, int n, const OutlierStats* __restrict__ st, int min_nb,
                                                       int negative, int* __restrict__ flag) {
  const int i = blockIdx.x * FL_T + threadIdx.x;
  if (i > n) return;
  bool keep = false;
  if (i < n) {
    const bool inlier = d ? (double)d[i] <= st->threshold : cnt[i] - 1 >= min_nb;
    keep = inlier != (negative != 0);
  }
  flag[i] = keep ? 1 : 0;
}

// the kept points at their offsets: 16-byte records (x, y, z, c unchanged; c = 0 for a 12-byte stride) and input indices, each nullable
__global__ void __launch_bounds__(FL_T) k_outlier_emit(const float* __restrict__ in, int stride_f, int n, const int* __restrict__ flag, const int* __restrict__ off,
                                                       float* __restrict__ out, int* __restrict__ out_index) {
  const int i = blockIdx.x * FL_T + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int at = off[i];
  if (out) {
    const float* p = in + (size_t)i * stride_f;
    float* o = out + (size_t)at * 4;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    o[3] = stride_f > 3 ? p[3] : 0.f;
  }
  if (out_index) out_index[at] = i;
}

static int fl_group_blocks(int n) { return (int)(((long long)n * FL_GROUP + FL_T - 1) / FL_T); }
static int fl_blocks(long long n) { return (int)((n + FL_T - 1) / FL_T); }

int outlier_tier(int mean_k) { const int k1 = mean_k + 1; return k1 <= 4 ? 4 : (k1 <= 8 ? 8 : (k1 <= 16 ? 16 : (k1 <= 32 ? 32 : 64))); }
int outlier_stat_rows(int n) { return fl_blocks(n); }

void sor_meandist(hipStream_t s, const SortedCloud& cl, int mean_k, float* out_d, OutlierStats* st) {
  const int nb = fl_group_blocks(cl.n);
  if (nb <= 0) return;
#define RGC_FL_LAUNCH(KT) hipLaunchKernelGGL((k_sor_meandist<KT, FL_GROUP>), dim3(nb), dim3(FL_T), 0, s, cl.P, cl.start, cl.grid, cl.n, mean_k + 1, out_d, st)
  switch (outlier_tier(mean_k)) {
    case 4: RGC_FL_LAUNCH(4); break;
    case 8: RGC_FL_LAUNCH(8); break;
    case 16: RGC_FL_LAUNCH(16); break;
    case 32: RGC_FL_LAUNCH(32); break;
    default: RGC_FL_LAUNCH(64); break;
  }
#undef RGC_FL_LAUNCH
}

void sor_stats(hipStream_t s, const float* d, int n, double std_mul, double* partials, OutlierStats* st) {
  const int nb = fl_blocks(n);
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_sor_stats, dim3(nb), dim3(FL_T), 0, s, d, n, partials);
  hipLaunchKernelGGL(k_sor_fold, dim3(1), dim3(2 * FL_WAVE), 0, s, partials, nb, n, std_mul, st);
}

void ror_count(hipStream_t s, const SortedCloud& cl, float r2, double r, int min_nb, int exact, int* out_cnt, OutlierStats* st) {
  const int nb = fl_group_blocks(cl.n);
  if (nb <= 0) return;
  const double reach = r * (1.0 + 1e-5);
  if (exact) hipLaunchKernelGGL((k_ror_count<FL_GROUP, true>), dim3(nb), dim3(FL_T), 0, s, cl.P, cl.start, cl.grid, cl.n, r2, reach, min_nb, out_cnt, st);
  else hipLaunchKernelGGL((k_ror_count<FL_GROUP, false>), dim3(nb), dim3(FL_T), 0, s, cl.P, cl.start, cl.grid, cl.n, r2, reach, min_nb, out_cnt, st);
}

void outlier_flag(hipStream_t s, const float* d, const int* cnt, int n, const OutlierStats* st, int min_nb, int negative, int* flag) {
  hipLaunchKernelGGL(k_outlier_flag, dim3(fl_blocks((long long)n + 1)), dim3(FL_T), 0, s, d, cnt, n, st, min_nb, negative, flag);
}

void outlier_emit(hipStream_t s, const float* in, int stride_f, int n, const int* flag, const int* off, float* out, int* out_index) {
  if (n > 0 && (out || out_index)) hipLaunchKernelGGL(k_outlier_emit, dim3(fl_blocks(n)), dim3(FL_T), 0, s, in, stride_f, n, flag, off, out, out_index);
}

}  // namespace rgck
