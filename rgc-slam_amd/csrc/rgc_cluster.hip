// rgc_cluster.hip -- gfx950 kernels of Euclidean cluster extraction (rgc_cluster_*): pcl::EuclideanClusterExtraction of a cloud on a grid of its own
// (rgcapi::ClusterRecord).  The machinery is the outlier filters' (rgc_filters.hip, rgc_nn.h): the grid's contiguous row ranges, the fp32 key dist2 (never
// FMA-contracted: -ffp-contract=off), the strict key < r2 ball walk by a group of lanes per sorted point.  What is new is a consumer that LINKS instead
// of counting -- a lock-free union-find over the sorted positions -- and a stable global ordering of the result (an LSD radix sort; the library had no
// global sort).  No output bit depends on the grid, the cell size, the launch shape or the run: the leader of a component is its smallest ORIGINAL
// index, and every atomic is an integer one (CAS, min, add, max).
//
// k_cl_init        parent[x] = x, lead[x] = INT_MAX, size[x] = 0 over the sorted positions
// k_cl_link<G>     a group of G lanes per sorted point walks the block of cells its ball can touch (k_ror_count's walk: ball_rows of rgc_nn.h), only over sorted positions BELOW its
//                  own -- every edge is seen once -- and unites the two components of every member with key < r2 (cl_unite)
// k_cl_flatten     (a separate launch) every position points at its root
// k_cl_census      atomicMin of the ORIGINAL index and atomicAdd of the count into the root's slots, one pair per run of equal roots in a wave
// k_cl_assign      at the original index: the component's leader and size, "in a kept component", "the leader of a kept component"; components and
//                  the largest size go to the read-out words
// k_cl_emit        (after the library's exclusive_scan of the leader flags) the kept leaders, ascending input index, with the key n - size
// k_cl_radix_hist / k_cl_radix_scatter   one pass of a STABLE least-significant-digit radix sort of (key, value) pairs on an 8-bit digit: per-workgroup
//                  digit histograms, the library's exclusive_scan over them (digit-major), a scatter whose rank inside the workgroup is computed in
//                  LDS so that equal digits keep their order.  Used twice: the leaders by n - size (stable over ascending leaders = "size descending,
//                  leader ascending"), and the kept points, ascending in input index, by cluster rank (the rows of `indices`)
// k_cl_rank        the rank of every kept leader at its original index, the sizes in rank order (their scan is `offsets`)
// k_cl_labels      labels at the original index; the kept points compacted in input order with their cluster's rank as the key
//
// The union-find.  parent[] lives on sorted positions.  Invariant: parent[x] <= x at all times, and a non-root never becomes a root again.  The larger
// root is hooked under the smaller by atomicCAS(&parent[hi], hi, lo); a failed CAS means that root moved down: re-find from what the CAS returned and
// retry.  Under the invariant every find strictly descends and ends after at most n steps without any other wave's help: no kernel waits for another
// workgroup.  Path halving stores an ancestor into a non-root (a relaxed store: whichever of two racing ancestors lands is one).  parent[] is read with
// relaxed agent-scope atomic loads, so that no load is hoisted out of a loop; a STALE value is harmless -- it is an earlier ancestor of the same
// position (or the position itself), so it lies in the same component and obeys the invariant, and the CAS, which is decided where the word lives,
// is what a hook stands on.  Every unite carries ONE step budget of 3 n + 8 (both finds descend monotonically over all retries: <= 2 n steps; <= n
// failed hooks); past it the lane raises ClusterStats::err and leaves, and the host returns RGC_ERR_HIP and writes nothing: a logic error is an error
// code, never a kernel that runs until somebody's time limit.
// No kernel spills, uses scratch or accumulator registers.  Host round trips of a call: rgc_api_cluster.hip's header.
#include "rgc_kernels.h"
#include "rgc_nn.h"

namespace rgck {

constexpr int CL_T = 256;  // threads per workgroup
constexpr int CL_WAVE = 64;
// Lanes per point of k_cl_link.  Measured for THIS kernel (scripts/bench_cluster.py, EXPERIMENTS.md "Euclidean clustering"): 2 is the slowest on a 30 k-point
// scan and the fastest on a 1 M-point map, 8 the slowest on the map; 4 is never the worst: the compromise between the two cloud sizes, as for the outlier filters
#ifdef RGC_LAB_CLUSTER_GROUP  // developer build (-DRGC_LAB_CLUSTER_GROUP=2|4|8): the group sizes scripts/bench_cluster.py compares
constexpr int CL_GROUP = RGC_LAB_CLUSTER_GROUP;
#else
constexpr int CL_GROUP = 4;
#endif
static_assert(CL_GROUP >= 2 && CL_GROUP <= 16 && !(CL_GROUP & (CL_GROUP - 1)), "a power of two of lanes, at most 16");
constexpr int CL_ROWS = 3;  // rows of cells whose ranges a group fetches together
constexpr int CL_RADIX_V = 4;                      // rounds of a wave over its share of a tile
constexpr int CL_TILE = CL_T * CL_RADIX_V;         // pairs per workgroup of a radix pass
constexpr int CL_DIGITS = 256;
static_assert(CL_TILE == kClusterRadixTile && CL_DIGITS == kClusterRadixDigits && CL_DIGITS == CL_T, "one thread per digit folds the waves' counts");

int cluster_group() { return CL_GROUP; }

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x, halving the path on the way; budget: the caller's remaining steps (< 0 on return: exhausted)
__device__ __forceinline__ int cl_find(int* __restrict__ parent, int x, int& budget) {
  int p = cl_load(parent + x);
  while (p != x && budget >= 0) {
    const int gp = cl_load(parent + p);
    if (gp != p) cl_store(parent + x, gp);  // x is no root and never will be: any ancestor may stand here
    x = p;
    p = gp;
    budget--;
  }
  return x;
}

// the components of a and b made one; returns their common root as this lane last saw it (or -1: the budget ran out, *err raised)
__device__ __forceinline__ int cl_unite(int* __restrict__ parent, int a, int b, int n, int* __restrict__ err) {
  int budget = 3 * n + 8;
  while (budget >= 0) {
    a = cl_find(parent, a, budget);
    b = cl_find(parent, b, budget);
    if (budget < 0) break;
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old;  // hi had moved down to old < hi
    b = lo;
    budget--;
  }
  atomicOr(err, 1);
  return -1;
}

// the read-out words (ClusterStats::words): a workgroup's sums (words 0 and 1) and maximum (word 2) -- a wave's shuffle tree, the waves' through LDS --
// into the workgroup's slot: one integer atomic per workgroup and word.  Called by every thread of the workgroup
__device__ __forceinline__ void cl_stats_add(ClusterStats* st, unsigned long long w0, unsigned long long w1, unsigned long long mx) {
  __shared__ unsigned long long part[CL_T / CL_WAVE][3];
  w0 = wave_sum_u64(w0);
  w1 = wave_sum_u64(w1);
#pragma unroll
  for (int o = CL_WAVE / 2; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_down(mx, o, CL_WAVE);
    mx = t > mx ? t : mx;
  }
  if ((threadIdx.x & (CL_WAVE - 1)) == 0) {
    part[threadIdx.x / CL_WAVE][0] = w0;
    part[threadIdx.x / CL_WAVE][1] = w1;
    part[threadIdx.x / CL_WAVE][2] = mx;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
#pragma unroll
    for (int j = 0; j < CL_T / CL_WAVE; j++) t = threadIdx.x < 2 ? t + part[j][threadIdx.x] : (part[j][2] > t ? part[j][2] : t);
    unsigned long long* w = &st->words[blockIdx.x & (kStatSlots - 1)][threadIdx.x];
    if (t) {
      if (threadIdx.x < 2) atomicAdd(w, t);
      else atomicMax(w, t);
    }
  }
}

__global__ void __launch_bounds__(CL_T) k_cl_init(int n, int* __restrict__ parent, int* __restrict__ lead, int* __restrict__ size) {
  const int x = blockIdx.x * CL_T + threadIdx.x;
  if (x >= n) return;
  parent[x] = x;
  lead[x] = INT_MAX;
  size[x] = 0;
}

template <int G>
__global__ void __launch_bounds__(CL_T) k_cl_link(const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g, int n, float r2, double reach,
                                                  int* __restrict__ parent, ClusterStats* __restrict__ st) {
  const int si = blockIdx.x * (CL_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0;
  if (si < n) {
    const float4 me = point_at(TP, (unsigned)si << 4);
    const float px = me.x, py = me.y, pz = me.z;
    const double q[3] = {(double)px, (double)py, (double)pz};
    // the rows of the ball of radius `reach` about the point (ball_block / ball_rows of rgc_nn.h, where reach = r (1 + 1e-5) is argued), the in-step rule
    CellBlock B = ball_block(q, reach, g);
    // only the sorted positions below si are linked from here (the others link to si): the layers above the point's own hold none of them ...
    B.hi[2] = min(B.hi[2], cell_coord(pz, g) - g.minc[2]);
    int cnt = 0, root = si;  // root: a position of si's component, its root as this lane last saw it
    bool dead = false;       // the error route: a unite ran out of its budget, the lane leaves (after the batch of rows)
    ball_rows<CL_ROWS>(B, q, reach, tstart, g, [&](const int (&ra)[CL_ROWS], const int (&rb)[CL_ROWS]) {
#pragma unroll
      for (int u = 0; u < CL_ROWS; u++) {
        const int b = min(rb[u], si);  // ... and every row ends at si
        cnt += max(b - ra[u], 0);
        for (int i = first_in_step(ra[u], lane); i < b && !dead; i += G) {
          if (dist2(px, py, pz, point_at(TP, (unsigned)i << 4)) < r2 && cl_load(parent + i) != root) {
            const int r = cl_unite(parent, root, i, n, &st->err);
            dead = r < 0;
            root = dead ? root : r;
          }
        }
      }
      return !dead;
    });
    if (lane == 0) cand = (unsigned long long)cnt;
  }
  cl_stats_add(st, cand, 0, 0);
}

__global__ void __launch_bounds__(CL_T) k_cl_flatten(int n, int* __restrict__ parent, ClusterStats* __restrict__ st) {
  const int x = blockIdx.x * CL_T + threadIdx.x;
  if (x >= n) return;
  int r = x, p = cl_load(parent + r), budget = n + 8;
  while (p != r && budget >= 0) {  // (others flatten meanwhile: what is read is an ancestor either way)
    r = p;
    p = cl_load(parent + r);
    budget--;
  }
  if (budget < 0) atomicOr(&st->err, 2);
  else if (r != x) cl_store(parent + x, r);
}

// parent[] is flat.  A run of consecutive lanes with one root (neighbours in the sorted order mostly share theirs) posts ONE min and ONE add
__global__ void __launch_bounds__(CL_T) k_cl_census(const float4* __restrict__ TP, int n, const int* __restrict__ parent, int* __restrict__ lead, int* __restrict__ size) {
  const int x = blockIdx.x * CL_T + threadIdx.x, lane = threadIdx.x & (CL_WAVE - 1);
  const bool in = x < n;
  const int root = in ? parent[x] : -1 - lane;  // (past the end: a run of its own, never posted)
  int m = in ? __float_as_int(point_at(TP, (unsigned)min(x, n - 1) << 4).w) : INT_MAX;
  const int prev = __shfl_up(root, 1, CL_WAVE);
  const unsigned long long heads = __ballot(lane == 0 || prev != root);
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the run's first lane: the highest head at or below this one
#pragma unroll
  for (int o = 1; o < CL_WAVE; o <<= 1) {
    const int t = __shfl_up(m, o, CL_WAVE);
    if (lane - o >= start) m = min(m, t);
  }
  const bool last = lane == CL_WAVE - 1 || ((heads >> (lane + 1)) & 1ull);
  if (in && last) {
    atomicMin(lead + root, m);
    atomicAdd(size + root, lane - start + 1);
  }
}

// threads 0 .. n (thread n closes the two flag arrays with a 0: the scans' last offsets are then the totals)
__global__ void __launch_bounds__(CL_T) k_cl_assign(const float4* __restrict__ TP, int n, const int* __restrict__ parent, const int* __restrict__ lead,
                                                    const int* __restrict__ size, int min_size, int max_size, int* __restrict__ comp, int* __restrict__ csize,
                                                    int* __restrict__ flag_p, int* __restrict__ flag_l, ClusterStats* __restrict__ st) {
  const int x = blockIdx.x * CL_T + threadIdx.x;
  unsigned long long roots = 0, big = 0;
  if (x < n) {
    const int r = parent[x], i = __float_as_int(point_at(TP, (unsigned)x << 4).w);
    const int L = lead[r], sz = size[r];
    const bool kept = sz >= min_size && sz <= max_size;
    comp[i] = L;
    csize[i] = sz;
    flag_p[i] = kept ? 1 : 0;
    flag_l[i] = kept && L == i ? 1 : 0;
    roots = r == x ? 1 : 0;
    big = (unsigned long long)sz;
  } else if (x == n) {
    flag_p[n] = 0;
    flag_l[n] = 0;
  }
  cl_stats_add(st, 0, roots, big);
}

__global__ void __launch_bounds__(CL_T) k_cl_emit(int n, const int* __restrict__ flag_l, const int* __restrict__ off_l, const int* __restrict__ csize, int* __restrict__ key,
                                                  int* __restrict__ val) {
  const int i = blockIdx.x * CL_T + threadIdx.x;
  if (i >= n || !flag_l[i]) return;
  const int at = off_l[i];
  key[at] = n - csize[i];
  val[at] = i;
}

// hist[d * nblocks + b]: pairs of tile b whose digit is d (digit-major: the scan over the whole array is every (digit, tile)'s first slot)
__global__ void __launch_bounds__(CL_T) k_cl_radix_hist(const int* __restrict__ key, int m, int shift, int* __restrict__ hist) {
  __shared__ int h[CL_DIGITS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * CL_TILE;
#pragma unroll
  for (int v = 0; v < CL_RADIX_V; v++) {
    const int i = base + v * CL_T + threadIdx.x;
    if (i < m) atomicAdd(&h[((unsigned)key[i] >> shift) & (CL_DIGITS - 1)], 1);
  }
  __syncthreads();
  hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) hist[CL_DIGITS * gridDim.x] = 0;  // (the scan's closing entry)
}

// A tile's order is wave-major, then round, then lane: wave w owns pairs [w V 64, (w + 1) V 64) of the tile.  A pair's rank among the tile's pairs of
// its digit = the pairs of that digit in the waves before (folded by thread d for digit d) + those of its own wave's earlier rounds (the wave's running
// count in LDS) + those of the lower lanes of its round (eight ballots: the lanes whose digit agrees bit by bit)
__global__ void __launch_bounds__(CL_T) k_cl_radix_scatter(const int* __restrict__ key, const int* __restrict__ val, int m, int shift, const int* __restrict__ off,
                                                           int* __restrict__ key_out, int* __restrict__ val_out) {
  __shared__ int cnt[CL_T / CL_WAVE][CL_DIGITS];
  const int w = threadIdx.x / CL_WAVE, lane = threadIdx.x & (CL_WAVE - 1);
#pragma unroll
  for (int j = 0; j < CL_T / CL_WAVE; j++) cnt[j][threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * CL_TILE + w * (CL_RADIX_V * CL_WAVE);
  int k[CL_RADIX_V], x[CL_RADIX_V], rank[CL_RADIX_V];
#pragma unroll
  for (int v = 0; v < CL_RADIX_V; v++) {
    const int i = base + v * CL_WAVE + lane;
    const bool in = i < m;
    k[v] = in ? key[i] : 0;
    x[v] = in ? val[i] : 0;
    const int d = ((unsigned)k[v] >> shift) & (CL_DIGITS - 1);
    unsigned long long peers = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const unsigned long long has = __ballot(in && ((d >> b) & 1));
      peers &= ((d >> b) & 1) ? has : ~has;
    }
    const int before = __popcll(peers & ((1ull << lane) - 1ull));
    rank[v] = in ? cnt[w][d] + before : 0;
    __syncthreads();  // (every lane has read the running counts of this round ...)
    if (in && before == 0) cnt[w][d] += __popcll(peers);  // ... before the first lane of each digit advances them
    __syncthreads();
  }
  {  // thread d: the waves' counts of digit d become each wave's first slot of that digit
    int at = off[threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
    for (int j = 0; j < CL_T / CL_WAVE; j++) {
      const int c = cnt[j][threadIdx.x];
      cnt[j][threadIdx.x] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < CL_RADIX_V; v++) {
    const int i = base + v * CL_WAVE + lane;
    if (i < m) {
      const int at = cnt[w][((unsigned)k[v] >> shift) & (CL_DIGITS - 1)] + rank[v];
      key_out[at] = k[v];
      val_out[at] = x[v];
    }
  }
}

// threads 0 .. m: rank r's leader learns its rank, sizes[r] = its size; sizes[m] = 0 (the scan's last offset is then the number of clustered points)
__global__ void __launch_bounds__(CL_T) k_cl_rank(int n, int m, const int* __restrict__ key, const int* __restrict__ val, int* __restrict__ rank_at, int* __restrict__ sizes) {
  const int r = blockIdx.x * CL_T + threadIdx.x;
  if (r > m) return;
  if (r == m) {
    sizes[m] = 0;
    return;
  }
  rank_at[val[r]] = r;
  sizes[r] = n - key[r];
}

// labels (nullable) at the original index; pkey / pval (nullable together): the kept points in input order with their cluster's rank
__global__ void __launch_bounds__(CL_T) k_cl_labels(int n, const int* __restrict__ flag_p, const int* __restrict__ off_p, const int* __restrict__ comp,
                                                    const int* __restrict__ rank_at, int* __restrict__ labels, int* __restrict__ pkey, int* __restrict__ pval) {
  const int i = blockIdx.x * CL_T + threadIdx.x;
  if (i >= n) return;
  const bool kept = flag_p[i] != 0;
  const int lab = kept ? rank_at[comp[i]] : -1;
  if (labels) labels[i] = lab;
  if (kept && pkey) {
    const int at = off_p[i];
    pkey[at] = lab;
    pval[at] = i;
  }
}

static int cl_blocks(long long n, int per = CL_T) { return (int)((n + per - 1) / per); }

int cluster_radix_tiles(int m) { return cl_blocks(m, CL_TILE); }

void cluster_link(hipStream_t s, const SortedCloud& cl, float r2, double r, int* parent, int* lead, int* size, ClusterStats* st) {
  if (cl.n <= 0) return;
  hipLaunchKernelGGL(k_cl_init, dim3(cl_blocks(cl.n)), dim3(CL_T), 0, s, cl.n, parent, lead, size);
  hipLaunchKernelGGL((k_cl_link<CL_GROUP>), dim3(cl_blocks((long long)cl.n * CL_GROUP)), dim3(CL_T), 0, s, cl.P, cl.start, cl.grid, cl.n, r2, r * (1.0 + 1e-5), parent, st);
  hipLaunchKernelGGL(k_cl_flatten, dim3(cl_blocks(cl.n)), dim3(CL_T), 0, s, cl.n, parent, st);
  hipLaunchKernelGGL(k_cl_census, dim3(cl_blocks(cl.n)), dim3(CL_T), 0, s, cl.P, cl.n, parent, lead, size);
}

void cluster_assign(hipStream_t s, const SortedCloud& cl, const int* parent, const int* lead, const int* size, int min_size, int max_size, int* comp, int* csize,
                    int* flag_p, int* flag_l, ClusterStats* st) {
  hipLaunchKernelGGL(k_cl_assign, dim3(cl_blocks((long long)cl.n + 1)), dim3(CL_T), 0, s, cl.P, cl.n, parent, lead, size, min_size, max_size, comp, csize, flag_p, flag_l, st);
}

void cluster_emit(hipStream_t s, int n, const int* flag_l, const int* off_l, const int* csize, int* key, int* val) {
  if (n > 0) hipLaunchKernelGGL(k_cl_emit, dim3(cl_blocks(n)), dim3(CL_T), 0, s, n, flag_l, off_l, csize, key, val);
}

int cluster_radix_sort(hipStream_t s, int m, int bits, int* key[2], int* val[2], int* hist, int* hist_off, int* block_sums) {
  int cur = 0;
  if (m <= 1) return cur;
  const int nb = cluster_radix_tiles(m);
  for (int shift = 0; shift < bits; shift += 8, cur ^= 1) {
    hipLaunchKernelGGL(k_cl_radix_hist, dim3(nb), dim3(CL_T), 0, s, key[cur], m, shift, hist);
    exclusive_scan(s, hist, hist_off, CL_DIGITS * nb + 1, block_sums);
    hipLaunchKernelGGL(k_cl_radix_scatter, dim3(nb), dim3(CL_T), 0, s, key[cur], val[cur], m, shift, hist_off, key[cur ^ 1], val[cur ^ 1]);
  }
  return cur;
}

void cluster_rank(hipStream_t s, int n, int m, const int* key, const int* val, int* rank_at, int* sizes) {
  hipLaunchKernelGGL(k_cl_rank, dim3(cl_blocks((long long)m + 1)), dim3(CL_T), 0, s, n, m, key, val, rank_at, sizes);
}

void cluster_labels(hipStream_t s, int n, const int* flag_p, const int* off_p, const int* comp, const int* rank_at, int* labels, int* pkey, int* pval) {
  if (n > 0 && (labels || pkey)) hipLaunchKernelGGL(k_cl_labels, dim3(cl_blocks(n)), dim3(CL_T), 0, s, n, flag_p, off_p, comp, rank_at, labels, pkey, pval);
}

}  // namespace rgck
