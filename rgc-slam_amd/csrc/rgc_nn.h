// rgc_nn.h -- the exact nearest-neighbour search on a cloud's grid (sorted float4 points, cell starts) and the device helpers it is made of,
// shared by the translation units that search: rgc_kernels.hip (k_fitness, k_icp_accumulate, the kNN kernels use the helpers), rgc_gicp.hip
// (k_gicp_correspond), rgc_gicp_st.hip (k_gicpst_search: nn_search2, the nearest and the second nearest), and the four that walk a ball or a
// growing cube by a group of lanes -- rgc_gicp_mp.hip (the radius gather), rgc_search.hip, rgc_filters.hip, rgc_cluster.hip: "the grid walk"
// below; transform_f32 is the fp32 query of all of them.  Everything here is
// __forceinline__: each kernel inlines its own copy, the device code of a translation unit that included these definitions in place is
// unchanged.  Compile with -ffp-contract=off (dist2).
#pragma once
#include "rgc_kernels.h"

#include <limits.h>

namespace rgck {

// Cell of grid g (absolute, before - minc) along one axis: floor(x / res - 0.5), without the fp64 division when the cell size is a
// power of two (the product is then the same double).
__device__ __forceinline__ int cell_coord(float x, const Grid& g) {
  const double u = g.inv_res != 0.0 ? (double)x * g.inv_res - 0.5 : (double)x / g.res - 0.5;
  return (int)floor(u);
}
// lower wall of cell c (relative) along axis a; the upper wall is + g.res
__device__ __forceinline__ double cell_wall(const Grid& g, int a, int c) { return ((double)(c + g.minc[a]) + 0.5) * g.res; }

// distance from the query to the faces of the cube of cells [c-r, c+r] that are not grid borders; 1e300 if none
__device__ __forceinline__ double cube_bound(const Grid& g, const int c[3], const double q[3], int r) {
  double bound = 1.0e300;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (c[a] - r > 0) bound = fmin(bound, q[a] - cell_wall(g, a, c[a] - r));
    if (c[a] + r < g.dim[a] - 1) bound = fmin(bound, cell_wall(g, a, c[a] + r + 1) - q[a]);
  }
  return bound;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dist2(float px, float py, float pz, const float4& c) {
  // (dx*dx + dy*dy) + dz*dz like flann::L2_Simple<float>; never contracted (-ffp-contract=off).  x and y go through the
  // packed fp32 pipe as ONE pair -- the loaded {x, y} already sits in an aligned register pair -- so the distance is
  // v_pk_add, v_pk_mul, v_sub, v_mul, v_add, v_add: six VALU ops per candidate (each lane rounds exactly as before).
  const f32x2 cxy = {c.x, c.y}, pxy = {px, py};
  const f32x2 d = pxy - cxy;
  const f32x2 dd = d * d;
  const float dz = pz - c.z;
  return (dd.x + dd.y) + dz * dz;
}

// the fp32 query of a search: T.cast<float>() * p with the association ((m0 x + m1 y) + m2 z) + m3 per row, never contracted -- the one
// definition of k_fitness, k_transform_f32, k_gicp_correspond and the FastGICPMultiPoints gather
__device__ __forceinline__ void transform_f32(const PoseF& T, float x, float y, float z, float& qx, float& qy, float& qz) {
  qx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  qy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  qz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
}

// sorted point at a 32-bit BYTE offset: base in SGPRs + one VGPR offset, no 64-bit address arithmetic per candidate
// (n <= 2^27 points is enforced at the API, so 16 n fits)
__device__ __forceinline__ float4 point_at(const float4* __restrict__ P, unsigned byte_off) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(P) + byte_off);
}

// Cells of one (y,z) grid row are consecutive in the sorted array, so the candidates of the cube of cells
// [c-r, c+r]^3 are (2r+1)^2 CONTIGUOUS ranges: two start[] loads per row instead of two per cell, and no walk
// through empty cells (the 1-NN searches of C8 / f4).
template <typename F>
__device__ __forceinline__ void for_each_cube_row(const Grid& g, const int c[3], int r, const int* __restrict__ start, F&& f) {
  const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.dim[2] - 1);
  const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.dim[1] - 1);
  const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.dim[0] - 1);
  if (x0 > x1) return;
  for (int z = z0; z <= z1; z++) {
    int y = y0;
    for (; y + 3 <= y1; y += 4) {  // four rows per step: eight independent start[] loads in flight
      int a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        a[u] = start[cell_index(g, x0, y + u, z)];
        b[u] = start[cell_index(g, x1, y + u, z) + 1];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) f(a[u], b[u]);
    }
    for (; y <= y1; y++) f(start[cell_index(g, x0, y, z)], start[cell_index(g, x1, y, z) + 1]);
  }
}

// ---- The grid walk shared by the search index, the outlier filters, Euclidean clustering and the FastGICPMultiPoints gather (rgc_search.hip,
// rgc_filters.hip, rgc_cluster.hip, rgc_gicp_mp.hip): a block of cells as batches of contiguous row ranges, the growing cube's three rules, the
// per-lane sorted list.  Every argument for completeness is written here, once.  ("The shared grid walk")

// The cell of coordinate x along axis a, relative to the grid, clamped in fp64 to [-1, dim]: a query far outside the grid must not overflow the int.
// Inside the grid this is cell_coord - minc.  A clamped cell is a cell nearer the grid than the coordinate's own: the cubes about it, clipped to the
// grid, are cubes of cells all the same, and cube_bound measures their faces from the query's true coordinates.
__device__ __forceinline__ int cell_rel(double x, const Grid& g, int a) {
  const double u = floor(g.inv_res != 0.0 ? x * g.inv_res - 0.5 : x / g.res - 0.5) - (double)g.minc[a];
  return (int)fmin(fmax(u, -1.0), (double)g.dim[a]);
}

struct CellBlock { int lo[3], hi[3]; bool empty; };  // cells lo .. hi per axis, clipped to the grid; empty: it misses the grid

// The part of the grid the ball of radius `reach` about q can touch: per axis the cells of q - reach and q + reach.  reach = r (1 + 1e-5), set by
// the launch wrappers: a point whose fp32 key is below r2 lies within r (1 + 3 * 2^-24) of the query in exact arithmetic (the key's three products and
// two sums round by 2^-24 each, the differences of fp32 coordinates at most as much again), and it lies in the cell its own coordinates name (the
// grid's rule, cell_coord) -- so no member of the ball is outside this block.  A cell too many costs candidates; a cell too few would be a wrong answer.
__device__ __forceinline__ CellBlock ball_block(const double q[3], double reach, const Grid& g) {
  CellBlock B;
  B.empty = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    B.lo[a] = max(cell_rel(q[a] - reach, g, a), 0);
    B.hi[a] = min(cell_rel(q[a] + reach, g, a), g.dim[a] - 1);
    B.empty = B.empty || B.lo[a] > B.hi[a];
  }
  return B;
}
// the cube of cells [c - r, c + r]^3
__device__ __forceinline__ CellBlock cube_block(const int c[3], int r, const Grid& g) {
  CellBlock B;
  B.empty = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    B.lo[a] = max(c[a] - r, 0);
    B.hi[a] = min(c[a] + r, g.dim[a] - 1);
    B.empty = B.empty || B.lo[a] > B.hi[a];
  }
  return B;
}
// distance from x to the cell c of axis a (0 inside it)
__device__ __forceinline__ double cell_gap(const Grid& g, int a, int c, double x) {
  const double wall = cell_wall(g, a, c);
  return fmax(0.0, fmax(wall - x, x - (wall + g.res)));
}

// The row ranges of a block: cells of one (y, z) row are consecutive in the sorted array (for_each_cube_row), so the block is (hi_y - lo_y + 1)
// (hi_z - lo_z + 1) ranges [a, b) of sorted positions.  ORDER: z ascending, inside a layer y ascending.  ROWS ranges are fetched together (one round
// trip, not one per row) and handed to f(a[ROWS], b[ROWS]); a row past the block's last takes its neighbour's start and is EMPTY (b = a).  kBall: a row
// whose gap to q exceeds the reach (gy^2 + gz^2 > reach2) is empty too; with ROWS = 1 it is not fetched at all.  f returns false to end the
// walk: an early exit acts once per batch, never inside one.
template <int ROWS, bool kBall, typename F>
__device__ __forceinline__ void block_rows(const CellBlock& B, const double q[3], double reach2, const int* __restrict__ start, const Grid& g, F&& f) {
  if (B.empty) return;
  for (int z = B.lo[2]; z <= B.hi[2]; z++) {
    const double gz = kBall ? cell_gap(g, 2, z, q[2]) : 0.0;
    for (int yb = B.lo[1]; yb <= B.hi[1]; yb += ROWS) {
      bool in[ROWS], any = false;
#pragma unroll
      for (int u = 0; u < ROWS; u++) {
        in[u] = yb + u <= B.hi[1];
        if (kBall) {
          const double gy = cell_gap(g, 1, min(yb + u, B.hi[1]), q[1]);
          in[u] = in[u] && gy * gy + gz * gz <= reach2;
        }
        any = any || in[u];
      }
      if (kBall && ROWS == 1 && !any) continue;  // (ROWS > 1: the fetches do not wait for the gap test, it only chooses between b and a)
      int a[ROWS], b[ROWS];
#pragma unroll
      for (int u = 0; u < ROWS; u++) {
        const int y = min(yb + u, B.hi[1]);
        a[u] = start[cell_index(g, B.lo[0], y, z)];
        const int e = start[cell_index(g, B.hi[0], y, z) + 1];
        b[u] = in[u] ? e : a[u];
      }
      if (!f(a, b)) return;
    }
  }
}
// the rows of the ball of radius `reach` about q (rows beyond the gap are empty), and of the cube [c - r, c + r]^3
template <int ROWS, typename F>
__device__ __forceinline__ void ball_rows(const CellBlock& B, const double q[3], double reach, const int* __restrict__ start, const Grid& g, F&& f) {
  block_rows<ROWS, true>(B, q, reach * reach, start, g, f);
}
template <int ROWS, typename F>
__device__ __forceinline__ void cube_rows(const int c[3], int r, const int* __restrict__ start, const Grid& g, F&& f) {
  block_rows<ROWS, false>(cube_block(c, r, g), nullptr, 0.0, start, g, f);
}

// How the G lanes of a group share the candidates of a row [a, b): a lane's first candidate; it then strides by G.  The two rules give every lane
// other candidates, so they fix the ORDER of a lane's floating-point sums: a kernel keeps the rule it has.
//   carry-over  the running count `before` of the rows so far carries over: the concatenated ranges are dealt round robin, short rows idle no lane
//               (mp_walk, k_search_knn, k_sor_meandist)
//   in step     every row starts at lane 0: the group takes G consecutive candidates together, which a ballot over the group can then order
//               (search_ball_walk, k_ror_count, k_cl_link)
template <int G> __device__ __forceinline__ int first_carried(int a, int lane, int before) { return a + ((lane - before) & (G - 1)); }
__device__ __forceinline__ int first_in_step(int a, int lane) { return a + lane; }

// The growing cube.  A search that wants the `need` nearest walks the cube [c - r, c + r]^3, and either proves its answer complete or takes a larger cube.
// cube_first: the first radius -- 1, or the first cube that touches the grid when the cell lies outside it -- and rmax, the cube that covers the grid.
__device__ __forceinline__ void cube_first(const int c[3], const Grid& g, int& r, int& rmax) {
  r = 1;
  rmax = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rmax = max(rmax, max(c[a], g.dim[a] - 1 - c[a]));
    r = max(r, max(-c[a], c[a] - (g.dim[a] - 1)));
  }
}
// "The key lies provably inside the cube whose nearest inner face is `bound` away" (cube_bound): everything unscanned is at least `bound` from the
// query.  The fp32 key stands for an exact squared distance it differs from by a few 2^-24 relative (ball_block); the allowance 1 - 1e-5 is far
// wider than that, so a key that passes is inside in exact arithmetic too -- and so is every tie of it.
__device__ __forceinline__ bool key_inside(float key, double bound) { return bound > 0.0 && (double)key < bound * bound * (1.0 - 1e-5); }
// the distance a cube's faces must exceed for key_inside to hold of `key`: its root, with the allowance 1 + 1e-5 the other way round
__device__ __forceinline__ double key_reach(float key) { return sqrt((double)key) * (1.0 + 1e-5); }
// The next radius after r: known (a distance `need` to prove is at hand): the smallest cube whose faces are beyond `need` -- every cube between is
// walked in vain; else nothing bounds the answer yet and the cube grows by half.  Never beyond rmax.
__device__ __forceinline__ int cube_next(const Grid& g, const int c[3], const double q[3], int r, int rmax, bool known, double need) {
  int rn;
  if (known) {
    rn = r + 1;
    while (rn < rmax) {
      const double b = cube_bound(g, c, q, rn);
      if (b == 1.0e300 || b > need) break;
      rn++;
    }
  } else {
    rn = r + max(1, (r + 1) / 2);
  }
  return min(rn, rmax);
}

// A lane's ascending list of KT entries in registers (E: an unsigned integer whose order is the entries'; an empty slot holds E's maximum): every
// index is a compile-time constant of a fully unrolled loop.  list_insert compares with the tail first: most candidates end there once the list is
// warm.  list_pop drops the head where `win`.  group_min: the minimum over the G lanes of a group.
template <int KT, typename E>
__device__ __forceinline__ void list_insert(E (&L)[KT], E e) {
  if (e < L[KT - 1]) {
#pragma unroll
    for (int u = KT - 1; u > 0; u--) L[u] = e < L[u - 1] ? L[u - 1] : (e < L[u] ? e : L[u]);
    L[0] = e < L[0] ? e : L[0];
  }
}
template <int KT, typename E>
__device__ __forceinline__ void list_pop(E (&L)[KT], bool win) {
#pragma unroll
  for (int u = 0; u < KT - 1; u++) L[u] = win ? L[u + 1] : L[u];
  L[KT - 1] = win ? (E)~(E)0 : L[KT - 1];
}
template <int G, typename E>
__device__ __forceinline__ E group_min(E m) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const E other = __shfl_xor(m, o, G);
    m = other < m ? other : m;
  }
  return m;
}
// the sum over a wave's 64 lanes, in lane 0 (the read-out words: integer sums)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// The skeleton of the exact searches below: own cell first (an aligned point's nearest map point is usually closer than its cell walls), then the
// rows of the 3x3x3 block the ball of what was found reaches, else a cube of cells that grows (cube_first / key_inside / cube_next) until the answer
// is provably inside it.  take(cp, s) folds candidate cp at sorted position s into the caller's answer; key() is the squared distance EVERY exit
// bounds (INFINITY: nothing bounds the answer yet).  take must be idempotent: the clamped tail loads of scan and the re-scans of a growing cube show
// it a candidate again.  kCap: the search also ends once everything unscanned is farther than cap_r, and `unresolved` (nullable) makes it give up
// instead of growing the cube beyond its first size.
template <bool kCap, typename Take, typename Key>
__device__ __forceinline__ void nn_walk(float px, float py, float pz, const float4* __restrict__ TP, const int* __restrict__ tstart, const Grid& g,
                                        double cap_r, bool* unresolved, Take&& take, Key&& key) {
  const int c[3] = {cell_coord(px, g) - g.minc[0], cell_coord(py, g) - g.minc[1], cell_coord(pz, g) - g.minc[2]};
  const double q[3] = {(double)px, (double)py, (double)pz};
  int rmax, r;
  cube_first(c, g, r, rmax);
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; a++) inside = inside && c[a] >= 0 && c[a] < g.dim[a];
  auto scan = [&](int s0, int s1) {
    int s = s0;
    unsigned off = (unsigned)s0 << 4;
    for (; s + 8 <= s1; s += 8, off += 128) {  // eight loads in flight: this search is a chain of memory round trips
      float4 cc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) cc[u] = point_at(TP, off + 16u * u);
#pragma unroll
      for (int u = 0; u < 8; u++) take(cc[u], s + u);
    }
    if (s < s1) {  // 1..7 left: clamped loads (a repeated candidate changes nothing: take is idempotent)
      const int last = s1 - 1;
      float4 cc[7];
#pragma unroll
      for (int u = 0; u < 7; u++) cc[u] = point_at(TP, (unsigned)min(s + u, last) << 4);
#pragma unroll
      for (int u = 0; u < 7; u++) take(cc[u], min(s + u, last));
    }
  };
  if (inside) {
    const int own = cell_index(g, c[0], c[1], c[2]);
    const int o0 = tstart[own], o1 = tstart[own + 1];
    scan(o0, o1);
    const float k0 = key();
    if (k0 < INFINITY) {
      const double bound = cube_bound(g, c, q, 0);
      if (bound == 1.0e300 || key_inside(k0, bound)) return;
      // What the own cell gave bounds the search ball: of the 26 neighbouring cells only those the ball reaches can hold anything that changes the
      // answer (an equal-distance tie included) -- usually one to three of them, not the whole 3x3x3 block.  All their row ranges are fetched
      // together (one round trip), then scanned.  If the ball pokes out of the block the general loop below takes over.
      const double b1 = cube_bound(g, c, q, 1);
      if (b1 == 1.0e300 || key_inside(k0, b1)) {
        const double rad2 = (double)k0 * (1.0 + 1e-5);
        double wl[3], wh[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double wall = cell_wall(g, a, c[a]);
          wl[a] = q[a] - wall;
          wh[a] = wall + g.res - q[a];
        }
        int ra[9], rb[9];
#pragma unroll
        for (int r = 0; r < 9; r++) {
          const int dy = r % 3 - 1, dz = r / 3 - 1;
          const int y = c[1] + dy, z = c[2] + dz;
          const double gy = dy < 0 ? wl[1] : (dy > 0 ? wh[1] : 0.0), gz = dz < 0 ? wl[2] : (dz > 0 ? wh[2] : 0.0);
          const double m = gy * gy + gz * gz;
          const bool need = y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2] && m <= rad2;
          const int xa = (c[0] > 0 && wl[0] * wl[0] + m <= rad2) ? c[0] - 1 : c[0];
          const int xb = (c[0] < g.dim[0] - 1 && wh[0] * wh[0] + m <= rad2) ? c[0] + 1 : c[0];
          ra[r] = need ? tstart[cell_index(g, xa, y, z)] : 0;
          rb[r] = need ? tstart[cell_index(g, xb, y, z) + 1] : 0;
        }
#pragma unroll
        for (int r = 0; r < 9; r++) {
          if (r == 4) {  // the own row: its own cell has been scanned
            if (ra[4] < o0) scan(ra[4], o0);
            if (rb[4] > o1) scan(o1, rb[4]);
          } else if (rb[r] > ra[r]) {
            scan(ra[r], rb[r]);
          }
        }
        return;
      }
    }
  }
  for (;;) {
    // cube [c-r, c+r]^3 as contiguous row ranges of the sorted target (re-scans change nothing)
    for_each_cube_row(g, c, r, tstart, scan);
    if (r >= rmax) break;
    const double bound = cube_bound(g, c, q, r);
    if (bound == 1.0e300) break;
    if (kCap && bound > cap_r) break;  // everything unscanned is farther than the cap
    const float kk = key();
    if (kk < INFINITY && key_inside(kk, bound)) break;
    if (kCap && unresolved) {
      *unresolved = true;
      return;
    }
    r = cube_next(g, c, q, r, rmax, kk < INFINITY, key_reach(kk));
  }
}

// Exact nearest neighbour of (px,py,pz) in the sorted target (nn_walk), or everything within cap_r of it: the cube stops growing once the unscanned
// region is farther than cap_r (then nothing within cap_r is missing).  Ties: smaller original index.
// best = squared distance (INFINITY if none found), bs = position in the sorted array (-1 if none; only tracked if kIndex:
// the fitness score needs the distance alone, and the index bookkeeping costs it a third of its time).
// unresolved (nullable): instead of growing the cube beyond its first size the search gives up and sets the flag -- the caller has a
// cheaper way for what is left (a small map: the whole wave scans all of it, fitness_wave)
template <bool kIndex>
__device__ __forceinline__ void nn_search(float px, float py, float pz, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                          const Grid& g, double cap_r, float& best, int& bs, bool* unresolved = nullptr) {
  best = INFINITY;
  bs = -1;
  int bo = INT_MAX;
  nn_walk<true>(px, py, pz, TP, tstart, g, cap_r, unresolved,
                [&](const float4& cp, int s) {
                  const float d = dist2(px, py, pz, cp);
                  if (kIndex) {
                    const int o = __float_as_int(cp.w);
                    if (d < best || (d == best && o < bo)) { best = d; bs = s; bo = o; }
                  } else {
                    best = fminf(best, d);
                  }
                },
                [&] { return best; });
}

// Exact nearest AND second-nearest neighbour of (px,py,pz) in the sorted target (FastGICPSingleThread's nearestKSearch(pt, 2),
// fast_gicp_st_impl.hpp:56-60): nn_walk over the two smallest candidates under the total order (key, original index).  best / bs = the smallest's
// key and sorted position (ties to the smaller original index, as nn_search), second = the second smallest key of the multiset of keys (== best
// where the nearest is tied or duplicated; INFINITY when the target holds one point).
// The update is IDEMPOTENT: original indices are unique, so a candidate seen again IS (best, bo) or (second, so) or ranks behind both, and
// changes nothing.  Every exit bounds SECOND, not best: a ball that holds the nearest alone proves nothing about the second nearest (one point of
// the own cell bounds nothing).  second >= best, so the ball of second holds every candidate for either (an equal-key tie of best with a smaller
// index included).  No cap, no giving up.
__device__ __forceinline__ void nn_search2(float px, float py, float pz, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                           const Grid& g, float& best, int& bs, float& second) {
  best = second = INFINITY;
  bs = -1;
  int bo = INT_MAX, so = INT_MAX;
  nn_walk<false>(px, py, pz, TP, tstart, g, 0.0, nullptr,
                 [&](const float4& cp, int s) {
                   const float d = dist2(px, py, pz, cp);
                   const int o = __float_as_int(cp.w);
                   // (selects of values, not branches over which variable to write: the compiler kept the pairs in registers only this way)
                   const bool first = d < best || (d == best && o < bo);
                   const bool next = !first && o != bo && (d < second || (d == second && o < so));
                   second = first ? best : (next ? d : second);
                   so = first ? bo : (next ? o : so);
                   best = first ? d : best;
                   bs = first ? s : bs;
                   bo = first ? o : bo;
                 },
                 [&] { return second; });
}

}  // namespace rgck
