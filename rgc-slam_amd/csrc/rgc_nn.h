// rgc_nn.h -- the exact nearest-neighbour search on a cloud's grid (sorted float4 points, cell starts) and the device helpers it is made of,
// shared by the translation units that search: rgc_kernels.hip (k_fitness, k_icp_accumulate, the kNN kernels use the helpers), rgc_gicp.hip
// (k_gicp_correspond), rgc_gicp_st.hip (k_gicpst_search: nn_search2, the nearest and the second nearest) and rgc_gicp_mp.hip (the radius
// gather); transform_f32 is the fp32 query of all of them.  Everything here is
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

// Exact nearest neighbour of (px,py,pz) in the sorted target: own cell first (an aligned point's nearest map point is usually
// closer than its cell walls), else a cube of cells that grows until the best distance is provably inside it -- or until the
// unscanned region is farther than cap_r (then nothing within cap_r is missing).  Ties: smaller original index.
// best = squared distance (INFINITY if none found), bs = position in the sorted array (-1 if none; only tracked if kIndex:
// the fitness score needs the distance alone, and the index bookkeeping costs it a third of its time).
// unresolved (nullable): instead of growing the cube beyond its first size the search gives up and sets the flag -- the caller has a
// cheaper way for what is left (a small map: the whole wave scans all of it, fitness_wave)
template <bool kIndex>
__device__ __forceinline__ void nn_search(float px, float py, float pz, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                          const Grid& g, double cap_r, float& best, int& bs, bool* unresolved = nullptr) {
  const int c[3] = {cell_coord(px, g) - g.minc[0], cell_coord(py, g) - g.minc[1], cell_coord(pz, g) - g.minc[2]};
  const double q[3] = {(double)px, (double)py, (double)pz};
  int rmax = 0, r = 1;
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rmax = max(rmax, max(c[a], g.dim[a] - 1 - c[a]));
    r = max(r, max(-c[a], c[a] - (g.dim[a] - 1)));  // first cube that touches the grid when the query lies outside
    inside = inside && c[a] >= 0 && c[a] < g.dim[a];
  }
  best = INFINITY;
  bs = -1;
  int bo = INT_MAX;
  auto take = [&](const float4& cp, int s) {
    const float d = dist2(px, py, pz, cp);
    if (kIndex) {
      const int o = __float_as_int(cp.w);
      if (d < best || (d == best && o < bo)) { best = d; bs = s; bo = o; }
    } else {
      best = fminf(best, d);
    }
  };
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
    if (s < s1) {  // 1..7 left: clamped loads (a repeated candidate changes neither the minimum nor its index)
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
    if (best < INFINITY) {
      const double bound = cube_bound(g, c, q, 0);
      if (bound == 1.0e300 || (bound > 0.0 && (double)best < bound * bound * (1.0 - 1e-5))) return;
      // The nearest point of the own cell bounds the search ball: of the 26 neighbouring cells only those the ball reaches can hold
      // anything nearer (or an equal-distance tie) -- usually one to three of them, not the whole 3x3x3 block.  All their row ranges
      // are fetched together (one round trip), then scanned.  If the ball pokes out of the block the general loop below takes over.
      const double b1 = cube_bound(g, c, q, 1);
      if (b1 == 1.0e300 || (b1 > 0.0 && (double)best < b1 * b1 * (1.0 - 1e-5))) {
        const double rad2 = (double)best * (1.0 + 1e-5);
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
    // cube [c-r, c+r]^3 as contiguous row ranges of the sorted target (the minimum only improves on re-scans)
    for_each_cube_row(g, c, r, tstart, scan);
    if (r >= rmax) break;
    const double bound = cube_bound(g, c, q, r);
    if (bound == 1.0e300) break;
    if (bound > cap_r) break;  // everything unscanned is farther than the cap
    int rn;
    if (best < INFINITY) {
      if (bound > 0.0 && (double)best < bound * bound * (1.0 - 1e-5)) break;
    }
    if (unresolved) {
      *unresolved = true;
      return;
    }
    if (best < INFINITY) {
      const double need = sqrt((double)best) * (1.0 + 1e-5);
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
}

// Exact nearest AND second-nearest neighbour of (px,py,pz) in the sorted target (FastGICPSingleThread's nearestKSearch(pt, 2),
// fast_gicp_st_impl.hpp:56-60): nn_search's own-cell-first and cube-walk structure over the two smallest candidates under the total order
// (key, original index).  best / bs = the smallest's key and sorted position (ties to the smaller original index, as nn_search), second = the
// second smallest key of the multiset of keys (== best where the nearest is tied or duplicated; INFINITY when the target holds one point).
// The update is IDEMPOTENT: original indices are unique, so a candidate seen again IS (best, bo) or (second, so) or ranks behind both, and
// changes nothing -- the clamped tail loads of scan and the re-scans of a growing cube cannot count a point twice into second.
// Every early exit bounds SECOND, not best: a ball that holds the nearest alone proves nothing about the second nearest.  second >= best, so
// the ball of second holds every candidate for either (an equal-key tie of best with a smaller index included).
__device__ __forceinline__ void nn_search2(float px, float py, float pz, const float4* __restrict__ TP, const int* __restrict__ tstart,
                                           const Grid& g, float& best, int& bs, float& second) {
  const int c[3] = {cell_coord(px, g) - g.minc[0], cell_coord(py, g) - g.minc[1], cell_coord(pz, g) - g.minc[2]};
  const double q[3] = {(double)px, (double)py, (double)pz};
  int rmax = 0, r = 1;
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rmax = max(rmax, max(c[a], g.dim[a] - 1 - c[a]));
    r = max(r, max(-c[a], c[a] - (g.dim[a] - 1)));  // first cube that touches the grid when the query lies outside
    inside = inside && c[a] >= 0 && c[a] < g.dim[a];
  }
  best = second = INFINITY;
  bs = -1;
  int bo = INT_MAX, so = INT_MAX;
  auto take = [&](const float4& cp, int s) {
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
  };
  auto scan = [&](int s0, int s1) {
    int s = s0;
    unsigned off = (unsigned)s0 << 4;
    for (; s + 8 <= s1; s += 8, off += 128) {  // eight loads in flight, as nn_search
      float4 cc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) cc[u] = point_at(TP, off + 16u * u);
#pragma unroll
      for (int u = 0; u < 8; u++) take(cc[u], s + u);
    }
    if (s < s1) {  // 1..7 left: clamped loads (a repeated candidate changes nothing: the update is idempotent)
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
    if (second < INFINITY) {  // (two points of the own cell at least: one alone bounds nothing)
      const double bound = cube_bound(g, c, q, 0);
      if (bound == 1.0e300 || (bound > 0.0 && (double)second < bound * bound * (1.0 - 1e-5))) return;
      // the ball of the SECOND nearest of the own cell: only the neighbouring cells it reaches can hold a point that changes either of the two
      const double b1 = cube_bound(g, c, q, 1);
      if (b1 == 1.0e300 || (b1 > 0.0 && (double)second < b1 * b1 * (1.0 - 1e-5))) {
        const double rad2 = (double)second * (1.0 + 1e-5);
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
    // cube [c-r, c+r]^3 as contiguous row ranges of the sorted target (a re-scanned candidate changes nothing)
    for_each_cube_row(g, c, r, tstart, scan);
    if (r >= rmax) break;
    const double bound = cube_bound(g, c, q, r);
    if (bound == 1.0e300) break;
    int rn;
    if (second < INFINITY) {
      if (bound > 0.0 && (double)second < bound * bound * (1.0 - 1e-5)) break;
      const double need = sqrt((double)second) * (1.0 + 1e-5);
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
}

}  // namespace rgck
