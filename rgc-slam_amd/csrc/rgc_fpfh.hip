// rgc_fpfh.hip -- gfx950 kernels of the FPFH descriptors (rgc_fpfh_*): pcl::FPFHEstimation, 33 bins per query from the normals of everything within a
// radius, on a grid of the call's own over the surface cloud (rgcapi::FpfhRecord).  The grid walk is rgc_nn.h's ball walk (in step, three rows fetched
// together), as k_nrm_radius uses it.  The semantics are stated in include/rgc_hip.h.
//
// k_fpfh_check           a query with a non-finite coordinate raises the flag word (a plain store of 1); the normals of the surface cloud, whatever their
//                        stride, become float4 records with w = 1 where the three components are finite, else 0: one 16-byte load per pair member
// k_fpfh_mark<G>         a separate surface only: the ball walk of every query; each member's SORTED position is flagged (plain stores of 1: every
//                        writer writes the same value).  The library's exclusive_scan and k_fpfh_list turn the flags into the ascending list of sorted
//                        positions whose SPFH a query needs
// k_fpfh_spfh<G>         G lanes per listed surface point (every point when the cloud is its own surface, in the grid's sorted order), each lane with the
//                        pair terms of its own ball members in fp64; the three bins of a pair are integer LDS adds into the point's row of 33 counters
//                        (row stride 33 dwords: rows start on different banks).  The workgroup then stores its rows, 132 contiguous bytes each, at the
//                        points' original indices, and the row sizes.  The counts are integers: no bit depends on the order, the grid or the launch
// k_fpfh_combine<G>      G lanes per query, bins to lanes: the group takes G consecutive candidates of a row together, a ballot over the group lists the
//                        accepted members, and they join one after another in ascending sorted position -- each is one contiguous 132-byte row of 33
//                        counts, the group's lanes load consecutive dwords of it, lane l adds ((count * inc) * w) in fp64 into its sums of bins l, l + G,
//                        ...: ONE chain per bin in the walk's order.  The three blocks are normalised to 100 and stored as floats in the same launch.
//                        (The other layout, members to lanes with 33 sums per lane folded in lane order, is in EXPERIMENTS.md "FPFH".)
// No kernel spills, uses scratch or waits for another workgroup; the only atomics are integer adds (LDS counters, the read-out words).
#include "rgc_kernels.h"
#include "rgc_nn.h"

namespace rgck {

constexpr int FP_T = 256;  // threads per workgroup
constexpr int FP_WAVE = 64;
// Lanes per surface point of the SPFH pass and per query of the combine pass (the mark pass walks the same balls as the combine pass and takes its
// group).  Chosen for THESE kernels (scripts/bench_fpfh.py, EXPERIMENTS.md "FPFH")
#ifdef RGC_LAB_FPFH_SPFH_GROUP  // developer build (-DRGC_LAB_FPFH_SPFH_GROUP=2|4|8|16, -DRGC_LAB_FPFH_COMBINE_GROUP=4|8|16|32): the group sizes scripts/bench_fpfh.py compares
constexpr int FP_SGROUP = RGC_LAB_FPFH_SPFH_GROUP;
#else
constexpr int FP_SGROUP = 16;
#endif
#ifdef RGC_LAB_FPFH_COMBINE_GROUP
constexpr int FP_CGROUP = RGC_LAB_FPFH_COMBINE_GROUP;
#else
constexpr int FP_CGROUP = 16;
#endif
static_assert(FP_SGROUP >= 2 && FP_SGROUP <= 16 && !(FP_SGROUP & (FP_SGROUP - 1)), "a power of two of lanes, at most 16");
static_assert(FP_CGROUP >= 2 && FP_CGROUP <= 32 && !(FP_CGROUP & (FP_CGROUP - 1)), "a power of two of lanes, at most 32");
constexpr int FP_ROWS = 3;  // rows of cells whose ranges a group fetches together

// the read-out words (FpfhStats::words): the group leaders' sums of a workgroup added into the workgroup's slot, as nrm_stats_add.  Called by every
// thread of the workgroup
__device__ __forceinline__ void fpfh_stats_add(FpfhStats* st, unsigned long long cand, unsigned long long pairs, unsigned long long valid) {
  __shared__ unsigned long long part[FP_T / FP_WAVE][3];
  cand = wave_sum_u64(cand);
  pairs = wave_sum_u64(pairs);
  valid = wave_sum_u64(valid);
  if ((threadIdx.x & (FP_WAVE - 1)) == 0) {
    part[threadIdx.x / FP_WAVE][0] = cand;
    part[threadIdx.x / FP_WAVE][1] = pairs;
    part[threadIdx.x / FP_WAVE][2] = valid;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
#pragma unroll
    for (int j = 0; j < FP_T / FP_WAVE; j++) t += part[j][threadIdx.x];
    if (t) atomicAdd(&st->words[blockIdx.x & (kStatSlots - 1)][threadIdx.x], t);
  }
}

// floor(11 x) clamped to 0 .. 10 (a NaN goes to 0: fmax drops it)
__device__ __forceinline__ int fpfh_bin(double x) { return (int)fmin(fmax(floor(11.0 * x), 0.0), 10.0); }

// The pair term of surface point s (normal a) with its ball member t (normal b), include/rgc_hip.h "Pair term": everything in fp64 from the fp32 inputs,
// never contracted.  false: the pair is skipped (vn == 0).  b1, b2, b3: the bins of f1, f2, f3
__device__ __forceinline__ bool fpfh_pair(const float4& s, const float4& a, const float4& t, const float4& b, int& b1, int& b2, int& b3) {
  double dx = (double)t.x - (double)s.x, dy = (double)t.y - (double)s.y, dz = (double)t.z - (double)s.z;
  const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
  const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
  const double c1 = (ax * dx + ay * dy) + az * dz, c2 = (bx * dx + by * dy) + bz * dz;
  const bool swap = fabs(c1) < fabs(c2);  // on the numerators
  const double ux = swap ? bx : ax, uy = swap ? by : ay, uz = swap ? bz : az;
  const double nx = swap ? ax : bx, ny = swap ? ay : by, nz = swap ? az : bz;
  dx = swap ? -dx : dx; dy = swap ? -dy : dy; dz = swap ? -dz : dz;
  const double f3 = (swap ? -c2 : c1) / f4;
  double vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;  // v = d x u
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  if (vn == 0.0) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;  // w = u x v
  const double f2 = (vx * nx + vy * ny) + vz * nz;
  const double f1 = atan2((wx * nx + wy * ny) + wz * nz, (ux * nx + uy * ny) + uz * nz);
  b1 = fpfh_bin((f1 + 3.14159265358979323846) * (1.0 / (2.0 * 3.14159265358979323846)));
  b2 = fpfh_bin((f2 + 1.0) * 0.5);
  b3 = fpfh_bin((f3 + 1.0) * 0.5);
  return true;
}

// the sum of an int over the G lanes of a group, in every lane
template <int G>
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

__global__ void __launch_bounds__(FP_T) k_fpfh_check(const float* __restrict__ Q, int qstride_f, int nq, const float* __restrict__ N, int nstride_f, int ns,
                                                     float4* __restrict__ N4, int* __restrict__ flag) {
  const int i = blockIdx.x * FP_T + threadIdx.x;
  if (Q && i < nq) {
    const float* qp = Q + (size_t)i * qstride_f;
    if (!(fabsf(qp[0]) < INFINITY && fabsf(qp[1]) < INFINITY && fabsf(qp[2]) < INFINITY)) *flag = 1;
  }
  if (i < ns) {
    const float* np = N + (size_t)i * nstride_f;
    const float x = np[0], y = np[1], z = np[2];
    const bool ok = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
    N4[i] = make_float4(x, y, z, ok ? 1.f : 0.f);
  }
}

template <int G>
__global__ void __launch_bounds__(FP_T) k_fpfh_mark(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g,
                                                    float r2, double reach, int* __restrict__ flag, FpfhStats* __restrict__ st) {
  const int qi = blockIdx.x * (FP_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0;
  if (qi < nq) {
    const float* qp = Q + (size_t)qi * qstride_f;
    const float px = qp[0], py = qp[1], pz = qp[2];
    const double q[3] = {(double)px, (double)py, (double)pz};
    int cnt = 0;
    ball_rows<FP_ROWS>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&ra)[FP_ROWS], const int (&rb)[FP_ROWS]) {
#pragma unroll
      for (int u = 0; u < FP_ROWS; u++) {
        cnt += rb[u] - ra[u];
        for (int i = first_in_step(ra[u], lane); i < rb[u]; i += G)
          if (dist2(px, py, pz, point_at(TP, (unsigned)i << 4)) < r2) flag[i] = 1;
      }
      return true;
    });
    if (lane == 0) cand = (unsigned long long)cnt;
  }
  fpfh_stats_add(st, cand, 0, 0);
}

__global__ void __launch_bounds__(FP_T) k_fpfh_list(const int* __restrict__ flag, const int* __restrict__ off, int ns, int* __restrict__ list) {
  const int i = blockIdx.x * FP_T + threadIdx.x;
  if (i < ns && flag[i]) list[off[i]] = i;
}

template <int G>
__global__ void __launch_bounds__(FP_T) k_fpfh_spfh(const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g, int ns, const int* __restrict__ list,
                                                    const int* __restrict__ n_list, const float4* __restrict__ N4, float r2, double reach, unsigned* __restrict__ spfh,
                                                    int* __restrict__ mout, FpfhStats* __restrict__ st) {
  constexpr int PTS = FP_T / G;  // surface points of a workgroup
  __shared__ unsigned row[PTS * kFpfhBins];
  __shared__ int at[PTS];  // the points' original indices, -1: no point
  const int grp = threadIdx.x / G, lane = threadIdx.x & (G - 1);
  const int nq = list ? *n_list : ns;
  if (blockIdx.x * PTS >= nq) return;  // (the whole workgroup: the launch is sized for the surface, a list may be far shorter)
  const int qi = blockIdx.x * PTS + grp;
  for (int e = threadIdx.x; e < PTS * kFpfhBins; e += FP_T) row[e] = 0;
  if (lane == 0) at[grp] = -1;
  __syncthreads();
  unsigned long long cand = 0, pairs = 0;
  if (qi < nq) {  // (a whole group takes this branch or none of it does)
    const float4 me = point_at(TP, (unsigned)(list ? list[qi] : qi) << 4);
    const int oi = __float_as_int(me.w);
    const float4 a = N4[oi];
    const bool valid = a.w != 0.f;
    const double q[3] = {(double)me.x, (double)me.y, (double)me.z};
    unsigned* const mine_row = row + grp * kFpfhBins;
    int mine = 0, cnt = 0, done = 0;
    ball_rows<FP_ROWS>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&ra)[FP_ROWS], const int (&rb)[FP_ROWS]) {
#pragma unroll
      for (int u = 0; u < FP_ROWS; u++) {
        cnt += rb[u] - ra[u];
        for (int i = first_in_step(ra[u], lane); i < rb[u]; i += G) {
          const float4 cp = point_at(TP, (unsigned)i << 4);
          const float key = dist2(me.x, me.y, me.z, cp);
          if (key < r2) {
            mine++;  // (a skipped pair still counts in the row size)
            if (valid && key != 0.f) {
              const float4 b = N4[__float_as_int(cp.w)];
              int b1, b2, b3;
              if (b.w != 0.f && fpfh_pair(me, a, cp, b, b1, b2, b3)) {
                atomicAdd(mine_row + b1, 1u);
                atomicAdd(mine_row + 11 + b2, 1u);
                atomicAdd(mine_row + 22 + b3, 1u);
                done++;
              }
            }
          }
        }
      }
      return true;
    });
    const int total = group_sum<G>(mine);
    if (lane == 0) {
      at[grp] = oi;
      mout[oi] = total;
      cand = (unsigned long long)cnt;
    }
    pairs = (unsigned long long)done;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < PTS * kFpfhBins; e += FP_T) {  // consecutive threads store consecutive dwords of a 132-byte row
    const int p = e / kFpfhBins, o = at[p];
    if (o >= 0) spfh[(size_t)o * kFpfhBins + (e - p * kFpfhBins)] = row[e];
  }
  fpfh_stats_add(st, cand, pairs, 0);
}

template <int G>
__global__ void __launch_bounds__(FP_T) k_fpfh_combine(const float* __restrict__ Q, int qstride_f, int nq, const float4* __restrict__ TP, const int* __restrict__ tstart, Grid g,
                                                       const unsigned* __restrict__ spfh, const int* __restrict__ msurf, float r2, double reach, float* __restrict__ out,
                                                       int* __restrict__ cnt_out, FpfhStats* __restrict__ st) {
  const int qi = blockIdx.x * (FP_T / G) + threadIdx.x / G, lane = threadIdx.x & (G - 1);
  unsigned long long cand = 0, valid = 0;
  if (qi < nq) {
    // the query and the index its outputs go to: record qi of Q, or (Q == nullptr) sorted point qi written at its original index (nrm_query's rule)
    float px, py, pz;
    int oi = qi;
    if (Q) {
      const float* qp = Q + (size_t)qi * qstride_f;
      px = qp[0]; py = qp[1]; pz = qp[2];
    } else {
      const float4 me = point_at(TP, (unsigned)qi << 4);
      px = me.x; py = me.y; pz = me.z;
      oi = __float_as_int(me.w);
    }
    const double q[3] = {(double)px, (double)py, (double)pz};
    // bins to lanes: lane l keeps the sums of bins l, l + G, l + 2 G ...; the group takes G consecutive candidates together, and the accepted ones join
    // one after another in ascending sorted position, every lane loading its bins of the member's 132-byte row (the group's lanes: consecutive dwords)
    constexpr int SLOTS = (kFpfhBins + G - 1) / G;
    double F[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; k++) F[k] = 0.0;
    const int shift = (threadIdx.x & (FP_WAVE - 1)) & ~(G - 1);  // the group's first lane in its wave
    int mine = 0, cnt = 0;
    ball_rows<FP_ROWS>(ball_block(q, reach, g), q, reach, tstart, g, [&](const int (&ra)[FP_ROWS], const int (&rb)[FP_ROWS]) {
#pragma unroll
      for (int u = 0; u < FP_ROWS; u++) {
        cnt += rb[u] - ra[u];
        for (int i0 = ra[u]; i0 < rb[u]; i0 += G) {  // (every lane of the group makes every round: the ballot and the shuffles need them all)
          const int i = min(i0 + lane, rb[u] - 1);
          const float4 cp = point_at(TP, (unsigned)i << 4);
          const float key = dist2(px, py, pz, cp);
          const bool member = i0 + lane < rb[u] && key < r2;
          mine += member;
          const int j = __float_as_int(cp.w);
          const int mj = member && key != 0.f ? msurf[j] : 0;  // (a row of one member, and an invalid point's, hold zeros: nothing to add)
          unsigned todo = (unsigned)(__ballot(mj > 1) >> shift) & (G == 32 ? ~0u : (1u << (G & 31)) - 1u);
          while (todo) {
            const int l = __ffs(todo) - 1;
            todo &= todo - 1;
            const int jl = __shfl(j, l, G), ml = __shfl(mj, l, G);
            const float kl = __shfl(key, l, G);
            const double w = 1.0 / (double)kl, inc = 100.0 / (double)(ml - 1);
            const unsigned* __restrict__ rowj = spfh + (size_t)jl * kFpfhBins;
#pragma unroll
            for (int k = 0; k < SLOTS; k++)
              if (k * G + lane < kFpfhBins) F[k] += ((double)rowj[k * G + lane] * inc) * w;
          }
        }
      }
      return true;
    });
    const int total = group_sum<G>(mine);
    if (out) {
      // the three block sums in ascending bin, in every lane: bin b sits in slot b / G of lane b % G
      double sum[3];
#pragma unroll
      for (int blk = 0; blk < 3; blk++) {
        sum[blk] = __shfl(F[(blk * 11) / G], (blk * 11) % G, G);
#pragma unroll
        for (int b = blk * 11 + 1; b < blk * 11 + 11; b++) sum[blk] += __shfl(F[b / G], b % G, G);
      }
      float* const o = out + (size_t)oi * kFpfhBins;
#pragma unroll
      for (int k = 0; k < SLOTS; k++) {
        const int b = k * G + lane;
        if (b < kFpfhBins) {
          const double sb = b < 11 ? sum[0] : (b < 22 ? sum[1] : sum[2]);
          o[b] = total == 0 ? __uint_as_float(0x7fc00000u) : (sb != 0.0 ? (float)(F[k] * (100.0 / sb)) : 0.f);
        }
      }
    }
    if (lane == 0) {
      if (cnt_out) cnt_out[oi] = total;
      cand = (unsigned long long)cnt;
      valid = total > 0;
    }
  }
  fpfh_stats_add(st, cand, 0, valid);
}

static int fp_group_blocks(int nq, int group) { return (int)(((long long)nq * group + FP_T - 1) / FP_T); }

void fpfh_check(hipStream_t s, const float* Q, int qstride_f, int nq, const float* N, int nstride_f, int ns, float4* N4, int* flag) {
  const int n = Q && nq > ns ? nq : ns;
  if (n > 0) hipLaunchKernelGGL(k_fpfh_check, dim3((n + FP_T - 1) / FP_T), dim3(FP_T), 0, s, Q, qstride_f, nq, N, nstride_f, ns, N4, flag);
}

void fpfh_mark(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, int* flag, FpfhStats* st) {
  const int nb = fp_group_blocks(nq, FP_CGROUP);
  if (nb > 0) hipLaunchKernelGGL((k_fpfh_mark<FP_CGROUP>), dim3(nb), dim3(FP_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, r2, r * (1.0 + 1e-5), flag, st);
}

void fpfh_list(hipStream_t s, const int* flag, const int* off, int ns, int* list) {
  if (ns > 0) hipLaunchKernelGGL(k_fpfh_list, dim3((ns + FP_T - 1) / FP_T), dim3(FP_T), 0, s, flag, off, ns, list);
}

void fpfh_spfh(hipStream_t s, const SortedCloud& cl, const int* list, const int* n_list, const float4* N4, float r2, double r, unsigned* spfh, int* m, FpfhStats* st) {
  const int nb = fp_group_blocks(cl.n, FP_SGROUP);  // (a list's length stays on the device: the groups beyond it find nothing to do)
  if (nb > 0) hipLaunchKernelGGL((k_fpfh_spfh<FP_SGROUP>), dim3(nb), dim3(FP_T), 0, s, cl.P, cl.start, cl.grid, cl.n, list, n_list, N4, r2, r * (1.0 + 1e-5), spfh, m, st);
}

void fpfh_combine(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, const unsigned* spfh, const int* m, float r2, double r, float* out, int* cnt,
                  FpfhStats* st) {
  const int nb = fp_group_blocks(nq, FP_CGROUP);
  if (nb > 0) hipLaunchKernelGGL((k_fpfh_combine<FP_CGROUP>), dim3(nb), dim3(FP_T), 0, s, Q, qstride_f, nq, cl.P, cl.start, cl.grid, spfh, m, r2, r * (1.0 + 1e-5), out, cnt, st);
}

}  // namespace rgck
