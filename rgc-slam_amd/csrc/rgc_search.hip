// rgc_search.hip -- gfx950 kernels of the search index (rgc_search_*): pcl::KdTreeFLANN::nearestKSearch / radiusSearch for batches of arbitrary
// queries against a cloud of the library's own (a grid only).  The reference calls them in 13 places (relative to rgc_slam/ of the reference,
// ROBOT-WSC/RGC-SLAM): src/RGC_mapping.cpp:1097,1147,1196,1243 (5-NN in the feature maps), :1537,2157 (radius search over the key poses),
// include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:133,254, include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:56,
// include/fast_gicp/gicp/impl/fast_vgicp_cuda_impl.hpp:161, include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:145,148,233.
// The machinery is rgc_nn.h's: the grid's contiguous row ranges, the fp32 key dist2 (never FMA-contracted: -ffp-contract=off), cube_bound; the
// order of every result is ascending (key, original index), a total order, so a row does not depend on the grid, the cell size or the launch.
//
// k_search_knn<KT, G>   the k (<= KT) smallest of a query, by a group of G lanes striding the row ranges of a cube of cells (the running count
//                       carries over from row to row: short rows idle no lane).  Each lane keeps an ascending list of KT packed 64-bit entries
//                       (key bits << 32 | original index; non-negative fp32 bit patterns order as integers) in registers: every index into the
//                       list is a compile-time constant of a fully unrolled loop.  The G lists are merged by k rounds of a group-wide minimum
//                       (__shfl_xor); the winner pops its head.  A cube that does not prove the row complete GROWS AND THE LISTS START OVER:
//                       nothing is carried from the smaller cube, so a candidate seen again cannot enter a list twice.  Every exit bounds the
//                       K-TH entry: the row is complete when it is full and its k-th key lies provably inside the cube (the rule of key_inside,
//                       rgc_nn.h: cube_bound with the allowance for the fp32 key against the exact distance), or when the cube covers the grid (a row of
//                       min(k, n) entries ends there).  bounded != 0: the member test key < r2 joins, and a cube whose faces are beyond `reach`
//                       ends the search (nothing unscanned can be a member) -- radiusSearch with max_nn > 0; the rows come out sorted.
// k_search_compact      the bounded rows (fixed width) into CSR
// k_search_count<G>     radiusSearch without a cap, first walk: the members of every query's ball (key < r2, strict)
// k_search_fill<G>      ... second walk: the members as packed entries, ascending in the sorted target inside a row (a fixed order)
// k_search_sort_rows<W> one workgroup per row: a bitonic network over the row's entries in LDS, W entries at a time; a row longer than W then
//                       goes the long route, bottom-up two-way merges of the sorted windows through a global scratch row by the same workgroup
// k_search_unpack       packed entries -> idx, sq_dist
// No kernel spills, uses scratch or waits for another workgroup; the only atomics are integer adds / maxima of the read-out words.
#include "rgc_kernels.h"
#include "rgc_nn.h"

namespace rgck {

constexpr int SR_T = 256;  // threads per workgroup
constexpr int SR_WAVE = 64;
// Lanes per query.  Of 2, 4, 8 and 16, measured at 30 k queries against 30 k and 1 M points (100 to 140 candidates per query; EXPERIMENTS.md, "Search
// index"), 8 and 16 were slower at every shape; 2 is 10 to 15 % faster than 4 at k <= 5 and 25 % slower at k = 32.  4 is within 15 % of the best everywhere.
#ifdef RGC_LAB_SEARCH_GROUP  // developer build (-DRGC_LAB_SEARCH_GROUP=2|4|8|16): the group sizes scripts/bench_search.py compares
constexpr int SR_GROUP = RGC_LAB_SEARCH_GROUP;
#else
constexpr int SR_GROUP = 4;
#endif
static_assert(SR_GROUP >= 2 && SR_GROUP <= 16 && !(SR_GROUP & (SR_GROUP - 1)), "a power of two of lanes, at most 16 (the fill's ballot mask)");
constexpr unsigned long long kSrNone = ~0ull;  // an empty list slot: behind every entry (a key's bits are never 0xffffffff)
constexpr int SR_SMALL = 256;                  // rows up to this many members are sorted by the small instantiation of k_search_sort_rows

int search_group() { return SR_GROUP; }
int search_sort_window() { return kSearchSortWindow; }

__device__ __forceinline__ bool sr_finite(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// the read-out words (SearchStats): sums of a wave's group leaders, one integer atomic per wave and word
__device__ __forceinline__ void sr_stats_add(unsigned long long* word, unsigned long long v) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & (SR_WAVE - 1)) == 0 && v) atomicAdd(word, v);
}

// (The ONE kernel that keeps the cube walk, the list and the next-radius loop written out instead of rgc_nn.h's cube_rows / list_insert / cube_next:
// on those its KT = 32 instantiation measured 25 to 65 % slower in two separate visits -- EXPERIMENTS.md, "One grid walk" -- with the same registers
// and the same instruction mix.  The rules are rgc_nn.h's; a change to one of them there has to be made here too.)
template <int KT, int G>
__global__ void __launch_bounds__(SR_T) k_search_knn(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                                     Grid g, int k, int bounded, float r2, double reach, int* __restrict__ out_idx, float* __restrict__ out_sq,
                                                     int* __restrict__ out_cnt, SearchStats* __restrict__ st) {
  const int qi = blockIdx.x * (SR_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0, grew = 0, members = 0;
  if (qi < nq) {  // (a whole group takes this branch or none of it does)
    const float* qp = Q + (size_t)qi * qstride_f;
    const float px = qp[0], py = qp[1], pz = qp[2];
    int* row_idx = out_idx + (size_t)qi * k;
    float* row_sq = out_sq + (size_t)qi * k;
    if (!sr_finite(px, py, pz)) {  // nothing is indexed by a bad coordinate: the row is empty and the call is refused (SearchStats::nonfinite)
      if (lane == 0) { st->nonfinite = 1; out_cnt[qi] = 0; }
      for (int j = lane; j < k; j += G) { row_idx[j] = -1; row_sq[j] = INFINITY; }
    } else {
      const double q[3] = {(double)px, (double)py, (double)pz};
      int c[3], rmax = 0, r = 1;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        c[a] = cell_rel(q[a], g, a);
        rmax = max(rmax, max(c[a], g.dim[a] - 1 - c[a]));
        r = max(r, max(-c[a], c[a] - (g.dim[a] - 1)));  // (1 with the clamp: the first cube touches the grid)
      }
      unsigned long long L[KT];
      int found = 0;
      for (;;) {
#pragma unroll
        for (int u = 0; u < KT; u++) L[u] = kSrNone;  // the lists start over at every cube
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.dim[2] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.dim[1] - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.dim[0] - 1);
        int cnt = 0;
        for (int z = z0; z <= z1; z++)
          for (int y = y0; y <= y1; y++) {
            const int a = tstart[cell_index(g, x0, y, z)], b = tstart[cell_index(g, x1, y, z) + 1];
            int i = a + ((lane - cnt) & (G - 1));
            cnt += b - a;
            for (; i < b; i += G) {
              const float4 cp = point_at(TP, (unsigned)i << 4);
              const float key = dist2(px, py, pz, cp);
              const unsigned long long e = ((unsigned long long)__float_as_uint(key) << 32) | (unsigned)__float_as_int(cp.w);
              if ((!bounded || key < r2) && e < L[KT - 1]) {
#pragma unroll
                for (int u = KT - 1; u > 0; u--) L[u] = e < L[u - 1] ? L[u - 1] : (e < L[u] ? e : L[u]);
                L[0] = e < L[0] ? e : L[0];
              }
            }
          }
        cand += (unsigned long long)cnt;
        // the G lists merged: k rounds of the group's minimum; the winner (original indices are unique: one lane) pops its head
        found = 0;
        unsigned kth_bits = 0x7f800000u;
        for (int j = 0; j < k; j++) {
          unsigned long long m = L[0];
#pragma unroll
          for (int o = G / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, G);
            m = other < m ? other : m;
          }
          const bool any = m != kSrNone, win = any && m == L[0];
#pragma unroll
          for (int u = 0; u < KT - 1; u++) L[u] = win ? L[u + 1] : L[u];
          L[KT - 1] = win ? kSrNone : L[KT - 1];
          if (lane == (j & (G - 1))) {
            row_idx[j] = any ? (int)(unsigned)(m & 0xffffffffull) : -1;
            row_sq[j] = any ? __uint_as_float((unsigned)(m >> 32)) : INFINITY;
          }
          if (any) { found++; kth_bits = (unsigned)(m >> 32); }
        }
        if (r >= rmax) break;  // the cube covers the grid: the row holds min(k, members) entries
        const double bound = cube_bound(g, c, q, r);
        if (bound == 1.0e300) break;
        if (bounded && bound > reach) break;  // everything unscanned is farther than the ball reaches
        const bool full = found == k;
        const float kth = __uint_as_float(kth_bits);
        if (full && bound > 0.0 && (double)kth < bound * bound * (1.0 - 1e-5)) break;  // the K-TH entry is provably inside the cube
        grew = 1;
        int rn;
        if (full || bounded) {
          double need = full ? sqrt((double)kth) * (1.0 + 1e-5) : reach;
          if (bounded) need = fmin(need, reach);
          rn = r + 1;
          while (rn < rmax) {
            const double b = cube_bound(g, c, q, rn);
            if (b == 1.0e300 || b > need) break;
            rn++;
          }
        } else {
          rn = r + max(1, (r + 1) / 2);
        }
        r = min(rn, rmax);
      }
      if (lane == 0) {
        out_cnt[qi] = found;
        members = (unsigned long long)found;
      } else {
        cand = 0;
        grew = 0;
      }
    }
  }
  sr_stats_add(&st->candidates, cand);
  sr_stats_add(&st->grown, grew);
  sr_stats_add(&st->members, members);
}

// rows of `width` entries, cnt[q] of them taken, into CSR (off = the exclusive scan of cnt); sq nullable
__global__ void __launch_bounds__(SR_T) k_search_compact(const int* __restrict__ row_idx, const float* __restrict__ row_sq, const int* __restrict__ cnt,
                                                         const int* __restrict__ off, int nq, int width, int* __restrict__ idx, float* __restrict__ sq) {
  const size_t t = (size_t)blockIdx.x * SR_T + threadIdx.x;
  const size_t qi = t / (unsigned)width;
  const int j = (int)(t - qi * (unsigned)width);
  if (qi >= (size_t)nq || j >= cnt[qi]) return;
  const size_t at = (size_t)off[qi] + j;
  idx[at] = row_idx[t];
  if (sq) sq[at] = row_sq[t];
}

// The rows of the ball of radius `reach` about the query (ball_block / ball_rows of rgc_nn.h, where reach = r (1 + 1e-5) is argued), walked by a
// group of G lanes in steps of G candidates (the in-step rule): f(i, valid) is called by the whole group together, i = sorted position, valid = i is
// inside its row range.  Returns the number of candidates.
template <int G, typename F>
__device__ __forceinline__ int sr_ball_walk(const double q[3], double reach, const int* __restrict__ tstart, const Grid& g, int lane, F&& f) {
  int cnt = 0;
  ball_rows<1>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&a)[1], const int (&b)[1]) {
    cnt += b[0] - a[0];
    for (int i0 = a[0]; i0 < b[0]; i0 += G) f(first_in_step(i0, lane), first_in_step(i0, lane) < b[0]);
    return true;
  });
  return cnt;
}

template <int G>
__global__ void __launch_bounds__(SR_T) k_search_count(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                                       Grid g, float r2, double reach, int* __restrict__ out_cnt, SearchStats* __restrict__ st) {
  const int qi = blockIdx.x * (SR_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0, members = 0;
  if (qi < nq) {
    const float* qp = Q + (size_t)qi * qstride_f;
    const float px = qp[0], py = qp[1], pz = qp[2];
    int mine = 0;
    if (!sr_finite(px, py, pz)) {
      if (lane == 0) st->nonfinite = 1;
    } else {
      const double q[3] = {(double)px, (double)py, (double)pz};
      const int cnt = sr_ball_walk<G>(q, reach, tstart, g, lane, [&](int i, bool valid) {
        if (valid) mine += dist2(px, py, pz, point_at(TP, (unsigned)i << 4)) < r2 ? 1 : 0;
      });
      if (lane == 0) cand = (unsigned long long)cnt;
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, G);
    if (lane == 0) {
      out_cnt[qi] = mine;
      members = (unsigned long long)mine;
      atomicMax(&st->longest, mine);
    }
  }
  sr_stats_add(&st->candidates, cand);
  sr_stats_add(&st->members, members);
}

template <int G>
__global__ void __launch_bounds__(SR_T) k_search_fill(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                                      Grid g, float r2, double reach, const int* __restrict__ off, unsigned long long* __restrict__ ent) {
  const int qi = blockIdx.x * (SR_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  if (qi >= nq) return;
  const float* qp = Q + (size_t)qi * qstride_f;
  const float px = qp[0], py = qp[1], pz = qp[2];
  if (!sr_finite(px, py, pz)) return;
  const double q[3] = {(double)px, (double)py, (double)pz};
  int at = off[qi];
  const int end = off[qi + 1];
  const int shift = (threadIdx.x & (SR_WAVE - 1)) & ~(G - 1);  // the group's first lane within its wave
  sr_ball_walk<G>(q, reach, tstart, g, lane, [&](int i, bool valid) {
    float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
    float key = INFINITY;
    if (valid) {
      cp = point_at(TP, (unsigned)i << 4);
      key = dist2(px, py, pz, cp);
    }
    const bool member = valid && key < r2;
    // the members of this step, in lane order = ascending sorted position (the lanes of a group take every step together)
    const unsigned bits = (unsigned)(__ballot(member) >> shift) & ((1u << G) - 1u);
    const int pos = at + __popc(bits & ((1u << lane) - 1u));
    if (member && pos < end) ent[pos] = ((unsigned long long)__float_as_uint(key) << 32) | (unsigned)__float_as_int(cp.w);
    at += __popc(bits);
  });
}

// One workgroup per row of lo <= members (<= W where only_window): ascending packed entries, i.e. ascending (key, original index).  W entries at
// a time through a bitonic network in LDS (padded with kSrNone to a power of two); a longer row then merges its sorted windows bottom-up, two
// runs at a time, between the row and the same span of `tmp`: every element finds its place by a binary search in the other run (entries are
// unique: no ties), and the result is copied home if it ended in tmp.  The long route has to be correct, not fast.
template <int W>
__global__ void __launch_bounds__(SR_T) k_search_sort_rows(const int* __restrict__ off, int lo, int only_window, unsigned long long* ent, unsigned long long* tmp,
                                                           SearchStats* __restrict__ st) {
  __shared__ unsigned long long sh[W];
  const int a = off[blockIdx.x], len = off[blockIdx.x + 1] - a, tid = threadIdx.x;
  if (len < lo || (only_window && len > W)) return;  // (the whole workgroup)
  for (int w0 = 0; w0 < len; w0 += W) {
    const int m = min(W, len - w0);
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = tid; i < P; i += SR_T) sh[i] = i < m ? ent[(size_t)a + w0 + i] : kSrNone;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P; i += SR_T) {
          const int p = i ^ j;
          if (p > i) {
            const unsigned long long x = sh[i], y = sh[p];
            if ((x > y) == ((i & kk) == 0)) { sh[i] = y; sh[p] = x; }
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < m; i += SR_T) ent[(size_t)a + w0 + i] = sh[i];
    __syncthreads();
  }
  if (len <= W) return;
  if (tid == 0) atomicAdd(&st->rows_long, 1ull);
  unsigned long long* src = ent + a;
  unsigned long long* dst = tmp + a;
  for (long long run = W; run < len; run <<= 1) {  // (64-bit: twice a run may pass 2^31 before it passes the row)
    for (int i = tid; i < len; i += SR_T) {
      const long long q0 = i / (2 * run) * (2 * run);
      const int p0 = (int)q0, mid = (int)min(q0 + run, (long long)len), end = (int)min(q0 + 2 * run, (long long)len);
      const unsigned long long v = src[i];
      int s0 = i < mid ? mid : p0, s1 = i < mid ? end : mid;  // the other run: how many of it come before v
      const int base = s0;
      while (s0 < s1) {
        const int h = s0 + ((s1 - s0) >> 1);
        if (src[h] < v) s0 = h + 1; else s1 = h;
      }
      dst[(i < mid ? i : p0 + (i - mid)) + (s0 - base)] = v;
    }
    __syncthreads();
    unsigned long long* t = src; src = dst; dst = t;
  }
  if (src != ent + a)
    for (int i = tid; i < len; i += SR_T) ent[(size_t)a + i] = src[i];
}

__global__ void __launch_bounds__(SR_T) k_search_unpack(const unsigned long long* __restrict__ ent, long long total, int* __restrict__ idx, float* __restrict__ sq) {
  const long long i = (long long)blockIdx.x * SR_T + threadIdx.x;
  if (i >= total) return;
  const unsigned long long e = ent[i];
  idx[i] = (int)(unsigned)(e & 0xffffffffull);
  if (sq) sq[i] = __uint_as_float((unsigned)(e >> 32));
}

static int sr_group_blocks(int nq) { return (int)(((long long)nq * SR_GROUP + SR_T - 1) / SR_T); }

int search_tier(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32)); }

void search_knn(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, int k, int bounded, float r2, double r, int* out_idx, float* out_sq,
                int* out_cnt, SearchStats* st) {
  const int nb = sr_group_blocks(nq);
  if (nb <= 0) return;
  const double reach = r * (1.0 + 1e-5);
#define RGC_SR_LAUNCH(KT) \
  hipLaunchKernelGGL((k_search_knn<KT, SR_GROUP>), dim3(nb), dim3(SR_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, k, bounded, r2, reach, out_idx, out_sq, out_cnt, st)
  switch (search_tier(k)) {
    case 4: RGC_SR_LAUNCH(4); break;
    case 8: RGC_SR_LAUNCH(8); break;
    case 16: RGC_SR_LAUNCH(16); break;
    default: RGC_SR_LAUNCH(32); break;
  }
#undef RGC_SR_LAUNCH
}

void search_compact(hipStream_t s, const int* row_idx, const float* row_sq, const int* cnt, const int* off, int nq, int width, int* idx, float* sq) {
  const long long nb = ((long long)nq * width + SR_T - 1) / SR_T;
  if (nb > 0) hipLaunchKernelGGL(k_search_compact, dim3((unsigned)nb), dim3(SR_T), 0, s, row_idx, row_sq, cnt, off, nq, width, idx, sq);
}

void search_count(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, int* out_cnt, SearchStats* st) {
  const int nb = sr_group_blocks(nq);
  if (nb > 0) hipLaunchKernelGGL((k_search_count<SR_GROUP>), dim3(nb), dim3(SR_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, r2, r * (1.0 + 1e-5), out_cnt, st);
}

void search_fill(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, const int* off, unsigned long long* ent) {
  const int nb = sr_group_blocks(nq);
  if (nb > 0) hipLaunchKernelGGL((k_search_fill<SR_GROUP>), dim3(nb), dim3(SR_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, r2, r * (1.0 + 1e-5), off, ent);
}

void search_sort_rows(hipStream_t s, const int* off, int nq, int longest, unsigned long long* ent, unsigned long long* tmp, SearchStats* st) {
  if (nq <= 0 || longest < 2) return;
  hipLaunchKernelGGL((k_search_sort_rows<SR_SMALL>), dim3(nq), dim3(SR_T), 0, s, off, 2, 1, ent, tmp, st);
  if (longest > SR_SMALL) hipLaunchKernelGGL((k_search_sort_rows<kSearchSortWindow>), dim3(nq), dim3(SR_T), 0, s, off, SR_SMALL + 1, 0, ent, tmp, st);
}

void search_unpack(hipStream_t s, const unsigned long long* ent, long long total, int* idx, float* sq) {
  const long long nb = (total + SR_T - 1) / SR_T;
  if (nb > 0) hipLaunchKernelGGL(k_search_unpack, dim3((unsigned)nb), dim3(SR_T), 0, s, ent, total, idx, sq);
}

}  // namespace rgck
