// rgc_normals.hip -- gfx950 kernels of surface normal estimation (rgc_normal_*): pcl::NormalEstimation, a unit normal and a curvature per query from the
// second moment of its neighbourhood in a surface cloud, on a grid of the call's own (rgcapi::NormalRecord).  The machinery is shared: the grid walk, the
// per-lane (key, index) lists and cube_bound of rgc_nn.h, eig3_sym of rgc_cov.h, the shifted-origin fp64 moment of rgc_rbf.hip.  What is new is a
// consumer that joins them without materialising a row: what leaves a group of lanes is the normal, the curvature and (where asked for) the covariance,
// the centroid and the member count at the query's index.  The semantics are stated in include/rgc_hip.h.
//
// k_nrm_check            a query with a non-finite coordinate raises the flag word (a plain store of 1): the call is refused before anything is written
// k_nrm_knn<KT, G>       the min(k, n_surface) (<= KT) smallest (key, original index) entries of a query, by a group of G lanes striding the row ranges of
//                        the cube of cells about its cell -- k_search_knn's running count, cube growth and cube_bound exit through the helpers of rgc_nn.h
//                        (the lists start over when the cube grows).  Each lane keeps an ascending list of KT packed 64-bit entries in registers.  The G
//                        lists are merged by k rounds of a group-wide minimum (original indices are unique: one lane pops); as each rank pops, every lane
//                        of the group fetches that surface point (one address: a broadcast) and extends the SAME fp64 chain in ascending rank -- S1 = sum
//                        d, S2 = sum d d^T, d = (double)P - (double)q -- one rank behind the pop, so the fetch overlaps the next round of the merge.  No
//                        bit of the moment depends on the grid, the cell size or the launch shape.
// k_nrm_radius<G>        the members of a query's ball (key < r2, strict), the ball walk of k_ror_count (in step, three rows fetched together); every
//                        lane keeps its own chain of the unit-weight moment in the order it meets its members (ascending sorted position), and the G
//                        chains are added in lane order: a fixed order that is a function of the grid and the query alone.  The count is an integer.
// nrm_query              queries are an arbitrary array in input order; a cloud that is its own surface (a null query array) is walked in the grid's
//                        sorted order and written at the original indices, as the outlier filters walk theirs
// nrm_tail               both kernels' end: mean, centroid and covariance, eig3_sym, the column of the smallest eigenvalue (the last of the descending
//                        selection sort, exact ties included: min_eigenvector's rule, rgc_kernels.hip), the sign rule, the curvature, the stores.  Every
//                        lane of a group computes it (the lanes run in lockstep anyway), the leader stores.
// No kernel spills, uses scratch or waits for another workgroup; the only atomics are integer adds of the read-out words.
#include "rgc_kernels.h"
#include "rgc_nn.h"
#include "rgc_cov.h"

namespace rgck {

constexpr int NR_T = 256;  // threads per workgroup
constexpr int NR_WAVE = 64;
// Lanes per query, of the k route and of the radius route.  Chosen for THESE kernels (scripts/bench_normals.py, EXPERIMENTS.md "Normal estimation"), not
// inherited from k_search_knn or the outlier filters
#ifdef RGC_LAB_NORMAL_GROUP  // developer build (-DRGC_LAB_NORMAL_GROUP=2|4|8): the group sizes scripts/bench_normals.py compares
constexpr int NR_GROUP = RGC_LAB_NORMAL_GROUP;
#else
constexpr int NR_GROUP = 4;
#endif
#ifdef RGC_LAB_NORMAL_RADIUS_GROUP
constexpr int NR_RGROUP = RGC_LAB_NORMAL_RADIUS_GROUP;
#else
constexpr int NR_RGROUP = 4;
#endif
static_assert(NR_GROUP >= 2 && NR_GROUP <= 16 && !(NR_GROUP & (NR_GROUP - 1)), "a power of two of lanes, at most 16");
static_assert(NR_RGROUP >= 2 && NR_RGROUP <= 16 && !(NR_RGROUP & (NR_RGROUP - 1)), "a power of two of lanes, at most 16");
constexpr int NR_ROWS = 3;                     // rows of cells whose ranges a group fetches together: a z-layer of the 3 x 3 x 3 block
constexpr unsigned long long kNrNone = ~0ull;  // an empty list slot: behind every entry (a key's bits are never 0xffffffff)

int normal_group() { return NR_GROUP; }
int normal_radius_group() { return NR_RGROUP; }

// the read-out words (NormalStats::words: candidates, queries whose cube grew, valid queries): the group leaders' sums of a workgroup -- a wave's shuffle
// tree, the waves' sums through LDS -- added into the workgroup's slot, as the outlier filters' (fl_stats_add).  Called by every thread of the workgroup
__device__ __forceinline__ void nrm_stats_add(NormalStats* st, unsigned long long cand, unsigned long long grew, unsigned long long valid) {
  __shared__ unsigned long long part[NR_T / NR_WAVE][3];
  cand = wave_sum_u64(cand);
  grew = wave_sum_u64(grew);
  valid = wave_sum_u64(valid);
  if ((threadIdx.x & (NR_WAVE - 1)) == 0) {
    part[threadIdx.x / NR_WAVE][0] = cand;
    part[threadIdx.x / NR_WAVE][1] = grew;
    part[threadIdx.x / NR_WAVE][2] = valid;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
#pragma unroll
    for (int j = 0; j < NR_T / NR_WAVE; j++) t += part[j][threadIdx.x];
    if (t) atomicAdd(&st->words[blockIdx.x & (kStatSlots - 1)][threadIdx.x], t);
  }
}

// one member joins a chain: d = (double)P - (double)q per axis, S1 += d, S2 += d d^T (each product rounded, then added: never contracted)
__device__ __forceinline__ void nrm_add(const double q[3], float x, float y, float z, double (&S1)[3], double (&S2)[6]) {
  const double dx = (double)x - q[0], dy = (double)y - q[1], dz = (double)z - q[2];
  S1[0] += dx; S1[1] += dy; S1[2] += dz;
  S2[0] += dx * dx; S2[1] += dx * dy; S2[2] += dx * dz;
  S2[3] += dy * dy; S2[4] += dy * dz; S2[5] += dz * dz;
}

// The end of both kernels, for query qi with m members and their moments about q.  Returns 1 when the row is valid (m >= 3).
__device__ __forceinline__ unsigned long long nrm_tail(int qi, int m, const double q[3], const double (&S1)[3], const double (&S2)[6], const NormalSign& sg,
                                                       const NormalOut& out, bool leader) {
  if (m < 3) {  // PCL writes NaN and clears is_dense
    if (leader) {
      const float fn = __uint_as_float(0x7fc00000u);
      const double dn = (double)fn;
      if (out.n4)
        for (int a = 0; a < 4; a++) out.n4[(size_t)qi * 4 + a] = fn;
      if (out.cov6)
        for (int a = 0; a < 6; a++) out.cov6[(size_t)qi * 6 + a] = dn;
      if (out.cen)
        for (int a = 0; a < 3; a++) out.cen[(size_t)qi * 3 + a] = dn;
      if (out.cnt) out.cnt[qi] = m;
    }
    return 0;
  }
  const double mm = (double)m;
  const double mx = S1[0] / mm, my = S1[1] / mm, mz = S1[2] / mm;
  const double S[6] = {S2[0] / mm - mx * mx, S2[1] / mm - mx * my, S2[2] / mm - mx * mz, S2[3] / mm - my * my, S2[4] / mm - my * mz, S2[5] / mm - mz * mz};
  double ev[3], V[3][3];
  int ord[3];
  eig3_sym(S, ev, V, ord);
  const int c = ord[2];  // the smallest eigenvalue: the last of the descending selection sort, exact ties included
  double nx = c == 0 ? V[0][0] : (c == 1 ? V[0][1] : V[0][2]);
  double ny = c == 0 ? V[1][0] : (c == 1 ? V[1][1] : V[1][2]);
  double nz = c == 0 ? V[2][0] : (c == 1 ? V[2][1] : V[2][2]);
  const double lam = c == 0 ? ev[0] : (c == 1 ? ev[1] : ev[2]);
  const double trace = (S[0] + S[3]) + S[5];
  const float curvature = trace > 0.0 ? (float)(fabs(lam) / trace) : 0.f;
  bool neg;
  if (sg.flip) {  // flipNormalTowardsViewpoint: an exact 0 keeps the sign
    const double dot = (((double)sg.vx - q[0]) * nx + ((double)sg.vy - q[1]) * ny) + ((double)sg.vz - q[2]) * nz;
    neg = dot < 0.0;
  } else {  // the component of largest magnitude is made positive, the first one on ties
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    double big = nx, amax = ax;
    if (ay > amax) { big = ny; amax = ay; }
    if (az > amax) { big = nz; amax = az; }
    neg = big < 0.0;
  }
  if (neg) { nx = -nx; ny = -ny; nz = -nz; }
  if (leader) {
    if (out.n4) {  // (four stores: a caller's buffer need not be 16-byte aligned)
      float* o = out.n4 + (size_t)qi * 4;
      o[0] = (float)nx; o[1] = (float)ny; o[2] = (float)nz; o[3] = curvature;
    }
    if (out.cov6)
      for (int a = 0; a < 6; a++) out.cov6[(size_t)qi * 6 + a] = S[a];
    if (out.cen) {
      out.cen[(size_t)qi * 3 + 0] = q[0] + mx;
      out.cen[(size_t)qi * 3 + 1] = q[1] + my;
      out.cen[(size_t)qi * 3 + 2] = q[2] + mz;
    }
    if (out.cnt) out.cnt[qi] = m;
  }
  return 1;
}

// Query qi and the index its outputs go to.  Q != nullptr: record qi of the query array, written at qi.  Q == nullptr: the cloud is its own surface
// and the queries are walked in the GRID'S SORTED ORDER, as the outlier filters walk theirs -- the groups of a wave then share cells and candidates --
// query qi is sorted point qi, written at its ORIGINAL index.  No output bit depends on which: a query's result is a function of the query and the grid.
__device__ __forceinline__ int nrm_query(const float* __restrict__ Q, int qstride_f, const float4* __restrict__ TP, int qi, float& px, float& py, float& pz) {
  if (Q) {
    const float* qp = Q + (size_t)qi * qstride_f;
    px = qp[0]; py = qp[1]; pz = qp[2];
    return qi;
  }
  const float4 me = point_at(TP, (unsigned)qi << 4);
  px = me.x; py = me.y; pz = me.z;
  return __float_as_int(me.w);
}

__global__ void __launch_bounds__(NR_T) k_nrm_check(const float* __restrict__ Q, int qstride_f, int nq, int* __restrict__ flag) {
  const int qi = blockIdx.x * NR_T + threadIdx.x;
  if (qi >= nq) return;
  const float* qp = Q + (size_t)qi * qstride_f;
  if (!(fabsf(qp[0]) < INFINITY && fabsf(qp[1]) < INFINITY && fabsf(qp[2]) < INFINITY)) *flag = 1;
}

template <int KT, int G>
__global__ void __launch_bounds__(NR_T) k_nrm_knn(const float* __restrict__ Q, int qstride_f, int nq, const float* __restrict__ SP, int sstride_f, const float4* __restrict__ TP,
                                                  const int* __restrict__ tstart, Grid g, int k, NormalSign sg, NormalOut out, NormalStats* __restrict__ st) {
  const int qi = blockIdx.x * (NR_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0, grew = 0, valid = 0;
  if (qi < nq) {  // (a whole group takes this branch or none of it does)
    float px, py, pz;
    const int oi = nrm_query(Q, qstride_f, TP, qi, px, py, pz);
    const double q[3] = {(double)px, (double)py, (double)pz};
    // the query's cell, clamped to the grid's rim (cell_rel): a query may lie anywhere
    const int c[3] = {cell_rel(q[0], g, 0), cell_rel(q[1], g, 1), cell_rel(q[2], g, 2)};
    int rmax, r;
    cube_first(c, g, r, rmax);
    unsigned long long L[KT];
    double S1[3], S2[6];
    int found = 0;
    for (;;) {
#pragma unroll
      for (int u = 0; u < KT; u++) L[u] = kNrNone;  // the lists start over at every cube
      int cnt = 0;
      cube_rows<NR_ROWS>(c, r, tstart, g, [&](const int (&ra)[NR_ROWS], const int (&rb)[NR_ROWS]) {
#pragma unroll
        for (int u = 0; u < NR_ROWS; u++) {
          int i = first_carried<G>(ra[u], lane, cnt);
          cnt += rb[u] - ra[u];
          for (; i < rb[u]; i += G) {
            const float4 cp = point_at(TP, (unsigned)i << 4);
            list_insert(L, ((unsigned long long)__float_as_uint(dist2(px, py, pz, cp)) << 32) | (unsigned)__float_as_int(cp.w));
          }
        }
        return true;
      });
      cand += (unsigned long long)cnt;
      // the G lists merged: k rounds of the group's minimum; the winner (original indices are unique: one lane) pops its head.  The moment's chain runs
      // one rank behind: rank j's point is fetched while rank j + 1 is being found
      found = 0;
      unsigned kth_bits = 0x7f800000u;
#pragma unroll
      for (int a = 0; a < 3; a++) S1[a] = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) S2[a] = 0.0;
      float fx = 0.f, fy = 0.f, fz = 0.f;
      bool pending = false;
      for (int j = 0; j < k; j++) {
        const unsigned long long m = group_min<G>(L[0]);
        const bool any = m != kNrNone;
        list_pop(L, any && m == L[0]);
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (any) {
          const float* sp = SP + (size_t)(unsigned)(m & 0xffffffffull) * sstride_f;
          nx = sp[0]; ny = sp[1]; nz = sp[2];
          found++;
          kth_bits = (unsigned)(m >> 32);
        }
        if (pending) nrm_add(q, fx, fy, fz, S1, S2);
        fx = nx; fy = ny; fz = nz;
        pending = any;
      }
      if (pending) nrm_add(q, fx, fy, fz, S1, S2);
      if (r >= rmax) break;  // the cube covers the grid: the row holds min(k, n_surface) entries
      const double bound = cube_bound(g, c, q, r);
      if (bound == 1.0e300) break;
      const bool full = found == k;
      const float kth = __uint_as_float(kth_bits);
      if (full && key_inside(kth, bound)) break;  // the K-TH entry is provably inside the cube
      grew = 1;
      r = cube_next(g, c, q, r, rmax, full, key_reach(kth));
    }
    valid = nrm_tail(oi, found, q, S1, S2, sg, out, lane == 0);
    if (lane != 0) {
      cand = 0;
      grew = 0;
      valid = 0;
    }
  }
  nrm_stats_add(st, cand, grew, valid);
}

template <int G>
__global__ void __launch_bounds__(NR_T) k_nrm_radius(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g,
                                                     float r2, double reach, NormalSign sg, NormalOut out, NormalStats* __restrict__ st) {
  const int qi = blockIdx.x * (NR_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0, valid = 0;
  if (qi < nq) {
    float px, py, pz;
    const int oi = nrm_query(Q, qstride_f, TP, qi, px, py, pz);
    const double q[3] = {(double)px, (double)py, (double)pz};
    // the rows of the ball of radius `reach` about the query (ball_block / ball_rows of rgc_nn.h, where reach = r (1 + 1e-5) is argued), the in-step rule
    int mine = 0, cnt = 0;
    double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ball_rows<NR_ROWS>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&ra)[NR_ROWS], const int (&rb)[NR_ROWS]) {
#pragma unroll
      for (int u = 0; u < NR_ROWS; u++) {
        cnt += rb[u] - ra[u];
        for (int i = first_in_step(ra[u], lane); i < rb[u]; i += G) {
          const float4 cp = point_at(TP, (unsigned)i << 4);
          if (dist2(px, py, pz, cp) < r2) {
            mine++;
            nrm_add(q, cp.x, cp.y, cp.z, s1, s2);
          }
        }
      }
      return true;
    });
    // the G chains in lane order: ((lane 0 + lane 1) + lane 2) + ...; every lane of the group ends with the same bits
    int total = __shfl(mine, 0, G);
    double S1[3], S2[6];
#pragma unroll
    for (int a = 0; a < 3; a++) S1[a] = __shfl(s1[a], 0, G);
#pragma unroll
    for (int a = 0; a < 6; a++) S2[a] = __shfl(s2[a], 0, G);
#pragma unroll
    for (int l = 1; l < G; l++) {
      total += __shfl(mine, l, G);
#pragma unroll
      for (int a = 0; a < 3; a++) S1[a] += __shfl(s1[a], l, G);
#pragma unroll
      for (int a = 0; a < 6; a++) S2[a] += __shfl(s2[a], l, G);
    }
    valid = nrm_tail(oi, total, q, S1, S2, sg, out, lane == 0);
    if (lane == 0) cand = (unsigned long long)cnt;
    else valid = 0;
  }
  nrm_stats_add(st, cand, 0, valid);
}

static int nr_group_blocks(int nq, int group) { return (int)(((long long)nq * group + NR_T - 1) / NR_T); }

int normal_tier(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32)); }

void normal_check(hipStream_t s, const float* Q, int qstride_f, int nq, int* flag) {
  if (nq > 0) hipLaunchKernelGGL(k_nrm_check, dim3((nq + NR_T - 1) / NR_T), dim3(NR_T), 0, s, Q, qstride_f, nq, flag);
}

void normal_knn(hipStream_t s, const float* Q, int qstride_f, int nq, const float* SP, int sstride_f, const SortedCloud& cl, int k, const NormalSign& sg, const NormalOut& out,
                NormalStats* st) {
  const int nb = nr_group_blocks(nq, NR_GROUP);
  if (nb <= 0) return;
#define RGC_NR_LAUNCH(KT) \
  hipLaunchKernelGGL((k_nrm_knn<KT, NR_GROUP>), dim3(nb), dim3(NR_T), 0, s, Q, qstride_f, nq, SP, sstride_f, cl.P, cl.start, cl.grid, k, sg, out, st)
  switch (normal_tier(k)) {
    case 4: RGC_NR_LAUNCH(4); break;
    case 8: RGC_NR_LAUNCH(8); break;
    case 16: RGC_NR_LAUNCH(16); break;
    default: RGC_NR_LAUNCH(32); break;
  }
#undef RGC_NR_LAUNCH
}

void normal_radius(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, const NormalSign& sg, const NormalOut& out, NormalStats* st) {
  const int nb = nr_group_blocks(nq, NR_RGROUP);
  if (nb > 0) hipLaunchKernelGGL((k_nrm_radius<NR_RGROUP>), dim3(nb), dim3(NR_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, r2, r * (1.0 + 1e-5), sg, out, st);
}

}  // namespace rgck
