// rgc_kernels.h -- launch wrappers of the gfx950 kernels (internal; the public boundary is include/rgc_hip.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

namespace rgck {

// Dense voxel-aligned grid: cell c (per axis) covers [(c + minc + 0.5) * res, (c + minc + 1.5) * res): this is fast_gicp's
// voxel_coord = floor(x / res - 0.5) (fast_vgicp_voxel.hpp:158-160) shifted by minc, so the exact-kNN search grid and the Gaussian
// voxel map of the target are the SAME partition.
struct Grid {
  int minc[3];
  int dim[3];
  double res;      // cell size
  int ncell;
  double inv_res;  // 1 / res when res is a power of two (x / res == x * inv_res bit for bit), else 0: see grid_inv_res()
};
inline double grid_inv_res(double res) {
  int e;
  return std::frexp(res, &e) == 0.5 ? 1.0 / res : 0.0;
}
inline Grid make_grid(const int minc[3], const int dim[3], double res) {
  Grid g{};
  double nc = 1.0;
  for (int a = 0; a < 3; a++) { g.minc[a] = minc[a]; g.dim[a] = dim[a]; nc *= (double)dim[a]; }
  g.res = res;
  g.inv_res = grid_inv_res(res);
  g.ncell = nc <= 2.0e9 ? (int)nc : -1;
  return g;
}
// Cell order: x fastest (a grid row = the cells of one (y, z) = one contiguous range of the sorted array), then y, then z.
// (x, z, y was measured: 43 MB of HBM traffic per 1 M-query kNN launch instead of 73, but the launch 3 % slower -- the populated
// neighbour rows of a surface are the y-neighbours, which that order moves apart; the kernel is bound by instruction issue, not bytes.)
__host__ __device__ __forceinline__ int cell_index(const Grid& g, int cx, int cy, int cz) { return (cz * g.dim[1] + cy) * g.dim[0] + cx; }
// ... and its inverse: the integer cell coordinates (minc included) of cell ci
inline void cell_coords(const Grid& g, int ci, int out3[3]) {
  out3[0] = ci % g.dim[0] + g.minc[0];
  out3[1] = (ci / g.dim[0]) % g.dim[1] + g.minc[1];
  out3[2] = ci / (g.dim[0] * g.dim[1]) + g.minc[2];
}

struct Pose {  // row-major rotation + translation, fp64 (Eigen::Isometry3d in the reference)
  double R[9];
  double t[3];
};
struct PoseF {  // fp32 4x4 rows 0..2 (pcl::transformPointCloud in the reference)
  float m[12];
};

struct Quat { double x, y, z, w; };
// B9 folded into the counting pass of a cloud's preparation (count_cells): point i is read from src, re-expressed as q * p + t with
// k_transform_q's arithmetic, stored to the cloud's own buffer (x, y, z, intensity) and counted -- one pass over the map less
// copy / epoch / frame (nullable): the library's own copy of the source map, compared with it bit for bit (x, y, z) on the way; a point that
// differs is taken over and *epoch = frame says "the map is not the one the neighbour lists were made for" (KnnCache)
// force: the copy is not to be trusted (first frame of a buffer): *epoch = frame whatever the comparison says
struct Reframe { const float* src; int src_stride_f; Quat q; double t[3]; float4* copy; int* epoch; int frame; int force; };
// The neighbour-list cache of a map that is handed over by rgc_set_target_reframed again and again (round 5, second half).  A rigid
// re-expression does not change who a point's k nearest neighbours are -- only the fp32 rounding of the coordinates can, and only where
// the k-th and the (k+1)-th neighbour (or the edge of what the 3x3x3 block proves) are that close.  Points are named by their RANK: the
// position in the sorted array of the frame that built the lists (neighbours have nearby ranks in every later frame too: look-ups by rank
// are as local as look-ups by position).  Per rank: the k neighbours' ranks as that frame's exact search found them (nbr, 4 k bytes), the
// top bit of the first one a CERTIFICATE: the gap behind the
// k-th neighbour exceeded what rounding in any two frames can bridge (list_certified).  A certified query of an unchanged map takes its
// neighbours from the list (knn_point_cached: no search); the others -- on the todo lists since the frame that built the lists -- are
// searched exactly as before.  "Unchanged" is verified, not assumed: the counting pass compares the map with the library's own copy, bit
// for bit (Reframe); a frame that finds a difference searches everything and builds the lists again.
struct KnnCache {
  int* nbr = nullptr;        // [n][k] ranks of the k nearest neighbours of the point of rank r, in no particular order
  int* rank_of = nullptr;    // [n] rank of original point o (written by the frame that builds the lists, k_rank_gather)
  int* pos_of = nullptr;     // [n] this frame's position of rank r in the sorted array (k_rank_gather)
  int* qrank = nullptr;      // [n] ... and the rank of the point at position i
  const int* epoch = nullptr;  // *epoch == frame: the map changed this frame (or the lists are not trusted)
  int* overflow = nullptr;   // overflow[(frame - 1) & 1] == frame - 1: the previous frame's rebuild ran out of room in a todo list: rebuild again
  int frame = 0;
  int* todo = nullptr;       // kTodoLists lists of ranks of the queries without a certificate, todo_cap entries each
  int* todo_cnt = nullptr;   // ... their lengths (emptied by k_place in a frame that rebuilds)
  int todo_cap = 0;
  float cert_slack = 0.f;    // metres: what the coordinates' fp32 rounding in two frames can move a distance by, twice (4 sqrt(3) ulp of the largest coordinate)
};
constexpr int kTodoLists = 64;
struct LmIn { double x0[16]; double lambda; double init_factor; };
struct LmState {  // device-resident state of LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-172)
  double x0[16], lambda, nu, y0, yi, H[36], b[6], d[6], delta[16], xi[16], Hfin[36];
  double rot_eps, trans_eps, init_factor;
  int phase, done, conv, failed, outer, inner, n_lin, n_err, ncorr, ticketA, ticketB, max_outer, max_inner, has_fit;
  double fit_sum;                // sum of squared NN distances at the final pose (k_fitness_lm)
  int nvox, def_t, def_s, pad;   // frame counters carried home with the state; pad = grid guards, map | scan << 8
  int gen, cmd, mode, cur;       // step kernels: mode, valid correspondence buffer; gen: the posted solve's number (host image); cmd: -1 in image 0 = a resident solve gave up (lm_solve_hand_over), else 0; ticketA: unused
  float src_sq; int pad2;        // sum over the scan's grid cells of count^2 (how crowded its cells are; steers the scan's cell size); pad2: the lazy target's miss flag
  int lazy_nq, lazy_ncell;       // lazy target: listed queries / cells of this frame (size the next frame's launches)
};
struct LmInit { double x0[16], rot_eps, trans_eps, init_factor; int max_outer, max_inner; };
// Mapped host memory: the final pose of a solve, posted by its deciding launch BEFORE that launch computes the score (C8) -- a caller that
// needs only the pose to go on (the next frame's target of a dependent sequence, rgc_align_end_reframe) starts ~25 us earlier; pad / pad2:
// the grid guards and the lazy target's miss flag as the finished state will carry them; gen: the solve's number, written last
struct LmEarly { double x0[16]; int pad, pad2, outer, gen; };
// The LM area: one per context, zeroed once (rgc_align_begin).  Launch j of a chained solve reads image[(j - 1) & 1] and leaves image[j & 1];
// the resident solve leaves image[0].  Behind the images, the words that belong to neither:
//   miss     the lazy target's miss flag ("a look-up hit an occupied voxel outside the part that was built"), set by any workgroup of any
//            launch of a solve, taken into the finished state (pad2) and cleared by whoever finishes it
//   ticket   of the score's fold (the one launch of a solve whose workgroups hand rows to each other)
//   give_up  the resident solve's: the number of the solve a workgroup gave up on (a wait ran out, or RGC_LM_GIVE_UP_AT)
//   flags    the resident solve's, one per workgroup, {solve number, try number}: written by that workgroup alone
constexpr int kLmSolveMaxGroups = 512;
struct LmArea {
  LmState image[2];
  char pad0[3 * 1024 - 2 * sizeof(LmState)];  // the loose words open the area's fourth KiB ...
  int miss, ticket;
  unsigned give_up;
  char pad1[1024 - 3 * sizeof(int)];          // ... and the flags its second half
  unsigned long long flags[kLmSolveMaxGroups];
};
static_assert(offsetof(LmArea, image) == 0 && offsetof(LmArea, image[1]) == sizeof(LmState), "the two state images lead the area");
static_assert(offsetof(LmArea, miss) == 3072 && offsetof(LmArea, ticket) == 3076 && offsetof(LmArea, give_up) == 3080, "the loose words of the LM area");
static_assert(offsetof(LmArea, flags) == 4096, "a flag per workgroup of the resident solve");
constexpr int kLmAreaBytes = sizeof(LmArea);
static_assert(kLmAreaBytes == 8192, "the LM area");
// The context's small scratch (rgc_ctx::d_small, and h_small, its pinned mirror of the same layout): 48 ints.
struct SmallBlock {  // what measures or guards one cloud's grid (k_bbox, k_count): the box's accumulators and the flag word
  int lo[3], hi[3];
  int guard;         // != 0: non-finite points (k_bbox) / the cloud left its speculative grid (k_count)
  union { int nvox; float sum_sq; };  // the map: its voxel count (the cell scan); the scan: the sum over its cells of count^2
};
struct LeafRows { int box5[5]; int res[3]; };        // the leaf filter's rows chain (rgck::vg_rows) on the leaf block: res[1] is the block's guard
struct MapregCounts { int staged8[8]; int n[4]; };   // the mapping registration's factor counts (host mirror only) on the front-end's words
struct SmallWords {
  SmallBlock map;    // [0..7]
  int ncorr;         // [8] correspondences of the last linearize launch
  int unused[7];
  SmallBlock scan;   // [16..23]
  union { SmallBlock leaf; LeafRows leaf_rows; };  // [24..31] the leaf filter: its bounding-box pass, then its rows chain
  // [32..47] the front-end stages 16 ints here (host mirror, copied to its own flag block); the box of a map about to be re-framed is
  // measured here (rgc_set_target_reframed); the mapping registration reads its four counts back into host words 40..43.  All three are
  // enqueued on the context's MAIN stream, and each call waits for that stream before it reads the host words: the stream orders them.
  union { int fe[16]; SmallBlock hint; MapregCounts mapreg; };
  __host__ __device__ SmallBlock* block(bool is_target) { return is_target ? &map : &scan; }
};
static_assert(offsetof(SmallWords, map.guard) == 6 * 4 && offsetof(SmallWords, map.nvox) == 7 * 4 && offsetof(SmallWords, ncorr) == 8 * 4, "the map's block");
static_assert(offsetof(SmallWords, scan) == 16 * 4 && offsetof(SmallWords, scan.guard) == 22 * 4 && offsetof(SmallWords, scan.sum_sq) == 23 * 4, "the scan's block");
static_assert(offsetof(SmallWords, leaf) == 24 * 4 && offsetof(SmallWords, leaf_rows.res) == 29 * 4 && offsetof(SmallWords, leaf.guard) == 30 * 4, "the leaf filter's block");
static_assert(offsetof(SmallWords, fe) == 32 * 4 && offsetof(SmallWords, hint) == 32 * 4 && offsetof(SmallWords, mapreg.n) == 40 * 4, "the front-end's words");
static_assert(sizeof(SmallBlock) == 8 * 4 && sizeof(SmallWords) == 48 * 4, "48 ints");
struct FeParams { int n_scans; double min_range, max_range; };
struct LeafGrid { int minb[3]; int div[3]; };  // pcl::VoxelGrid leaf grid

constexpr int kAccum = 28;  // 21 upper-triangular H + 6 b + 1 cost
constexpr int kVoxRec = 10; // mean(3) cov6(6) num(1), doubles

// ---- typed views of a prepared cloud's device buffers: what the wrappers below take (rgcapi::Cloud builds them, rgc_ctx.h) ----
// Sorted points are float4 {x, y, z, original index (int bits)} grouped by grid cell; start[]: a cell's first point (ncell + 1 entries).
struct SortedCloud { const float4* P; const int* start; Grid grid; int n; };
struct Normals { double* nx; double* ny; double* nz; };  // the unit normal of every sorted point (its PLANE covariance is I - 0.999 n n^T)
// the Gaussian voxel map laid out on a cloud's grid: a cell's voxel id (< 0: empty), kVoxRec doubles per voxel, a voxel's cell
struct VoxelMap { const int* cell_voxel; double* vox; int* vox_cell; };
// the bulk kNN launch's deferred-query buffer (deferred_bytes(n) bytes) and the guard of the cloud's grid (nullable): set, the kernels stand still
struct DeferredBuf { void* buf; const int* guard; };
struct Corr { int* v; double* M; };  // what a linearisation freezes per source point and offset: the voxel found and the Mahalanobis matrix (6 doubles)
// ---- grid build ----
void bbox(hipStream_t s, const float* in, int stride_f, int n, double res, int* mm6, int* flags, int hi = 0);
// rf (nullable): in[] is first WRITTEN from rf->src (see Reframe; in must then be a 16-byte-stride device buffer this call may write)
void count_cells(hipStream_t s, const float* in, int stride_f, int n, Grid g, int* cell_of, int* slot_of, int* cnt, int hi = 0, int* guard = nullptr,
                 const Reframe* rf = nullptr);
// cnt: n = cells + 1 entries; block_sums: >= 8 * (n / 2048 + 2) bytes; cell_voxel (n - 1 ints) and nvox may be null
// consumes the counters: cnt[0..n) is left ZERO
void scan_cells(hipStream_t s, int* cnt, int* start, int n, void* block_sums, int* cell_voxel, int* nvox, int hi = 0,
                float* sum_sq = nullptr /* += sum of count^2, nullable */);
// order_tmp: n 64-bit records {original index, position in the cell, cell population} (k_place)
void place(hipStream_t s, int n, const int* cell_of, const int* slot_of, const int* start, unsigned long long* order_tmp, int hi = 0,
           const KnnCache* cache = nullptr /* its todo lists are emptied on the way in a frame that rebuilds them */);
void exclusive_scan(hipStream_t s, const int* in, int* out, int n, int* block_sums /* >= n/2048+2 */, int hi = 0);
// cache (nullable): KnnCache::rank_of (a frame that builds the lists) or pos_of and qrank (any other), written on the way
void rank_gather(hipStream_t s, const float* in, int stride_f, int n, const int* cell_of, const int* start,
                 const unsigned long long* order_tmp, float4* P, int* zero_me = nullptr, int hi = 0, const KnnCache* cache = nullptr);
// ---- C2: exact kNN + PLANE covariance -> unit normal ----
// bulk kernel (one lane per query; defers what it cannot finish) then the cooperative kernel (one wave per deferred query).
// deferred: deferred_bytes(n) bytes, whose first int (the count) must be 0 on entry (rank_gather's zero_me)
size_t deferred_bytes(int n);
// Seeds of the map's search (knn_point_seeded): seed[original point index] = an upper bound of the k-th squared distance the last search
// of that point found (>= 1e30: none); slack = how much a k-th distance may have grown since, in metres; warm = a search has written
// them.  Results do not depend on the seeds' values (a search they do not serve runs again without them).
struct KnnSeeds {
  float* seed = nullptr;
  float slack = 0.f;
  bool warm = false;
  KnnCache cache;  // (nbr == nullptr: no lists)
};
bool knn_seeds_apply(int n, int k);  // the seeded search exists for this cloud size and k
constexpr int kDeferredSlotEmptyByte = 0x80;
// What a bulk launch may be asked for beyond the search itself; the defaults mean "absent", a call site sets its own fields only.
struct KnnBulkOpts {
  int wide_r = 0;  // 2: the four-lanes-per-query search on the 5^3 block whatever the cloud (a sparse map)
  // the dense map's launch only (knn_bulk_times_itself): the launch's own start / stop times go into these events
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // lazy target (dense-map launch only): the queries listed in qlist[0 .. *nq) are searched, nothing else; q_est sizes the launch
  const int *qlist = nullptr, *nq = nullptr;
  int q_est = 0;
  KnnSeeds seeds;
  // > 0, the scan's launch and the map's with `fuse`: that many waves at the end of the launch resolve the deferred queries as they are published
  // (no knn_coop launch behind it).  The deferred buffer's entry words must hold kDeferredSlotEmptyByte bytes on entry; the readers leave them so.
  int coop_waves = 0;
  // The dense map's launch over the whole map (target, wide_r == 0, no query list, not the seeded kernel: knn_bulk_fuses_voxels; ignored
  // elsewhere) can do the voxel stage's work itself: every workgroup builds the voxel records of the cells that start and end among its 256
  // sorted points, from the normals it has in registers, and the launch's last workgroups resolve the deferred queries (coop_waves).
  // voxel_seams then finishes the map: the cells that cross a workgroup boundary and the voxels of the deferred queries.
  VoxelMap fuse{};  // (vox == nullptr: not asked for)
};
// what knn_bulk would do with these options, answered by the function that picks the launch's variant
bool knn_bulk_fuses_voxels(bool is_target, int n, int k, const KnnBulkOpts& o);  // it would honour a `fuse`
bool knn_bulk_times_itself(bool is_target, int n, int k, const KnnBulkOpts& o);  // it would honour ev0 / ev1
void knn_bulk(hipStream_t s, bool is_target, const SortedCloud& cl, int k, const DeferredBuf& df, const Normals& nrm, const KnnBulkOpts& o = KnnBulkOpts{});
// lazy target: stamp the cells of the map's grid within `margin` cells of the cell each point of the cloud `in` falls into under T and list the
// occupied ones (cell_list: their first sorted point; qlist: all their points; counts[0] / [1]: the lists' sizes, zeroed by rank_gather)
// guard (nullable): the map's (DeferredBuf::guard) -- set: nothing is listed
void footprint(hipStream_t s, const float* in, int stride_f, int n, Pose T, const SortedCloud& map, int* need, int stamp, int margin, int* qlist,
               int* cell_list, int* counts, const int* guard = nullptr);
// ... and the voxel pass over the listed cells, the map's deferred queries resolved beside it (k_voxel_cells_coop); voxel_patch follows
void voxel_cells_coop(hipStream_t s, const SortedCloud& cl, const Normals& nrm, const VoxelMap& vm, int k, const DeferredBuf& df, int waves,
                      const int* cell_list, const int* ncells, int cells_est, const KnnSeeds& seeds = KnnSeeds{});
// waves: one-wave workgroups that share the deferred list (clamped to [32, 8192])
void knn_coop(hipStream_t s, bool is_target, const SortedCloud& cl, int k, const DeferredBuf& df, const Normals& nrm, int waves, const KnnSeeds& seeds = KnnSeeds{});
// ---- C3: Gaussian voxel map ----
void voxel_build(hipStream_t s, const SortedCloud& cl, const Normals& nrm, const VoxelMap& vm);
// voxel_build and knn_coop (target) in one launch, followed by voxel_patch: see k_voxel_build_coop
void voxel_build_coop(hipStream_t s, const SortedCloud& cl, const Normals& nrm, const VoxelMap& vm, int k, const DeferredBuf& df, int waves, const KnnSeeds& seeds = KnnSeeds{});
// the voxels that hold a deferred query, recomputed: lets the cooperative search run BESIDE voxel_build; lanes: about
// the number of deferred queries (grid-stride loop, clamped to [64, 4096])
void voxel_patch(hipStream_t s, const SortedCloud& cl, const Normals& nrm, const VoxelMap& vm, const DeferredBuf& df, int lanes,
                 hipEvent_t done = nullptr /* signalled by the launch's own completion */);
// behind a knn_bulk that fused the voxel stage (KnnBulkOpts::fuse): the cells that cross a boundary between two of its workgroups and the voxels
// of the deferred queries (k_voxel_seams); patch_waves: about the number of deferred queries (they stride over the list)
void voxel_seams(hipStream_t s, const SortedCloud& cl, const Normals& nrm, const VoxelMap& vm, const DeferredBuf& df, int patch_waves, hipEvent_t done = nullptr);
// ---- C4/C5/C6 ---- (src at T against the target's voxel map vm on its grid g)
void linearize(hipStream_t s, const SortedCloud& src, const Normals& nrm, Pose T, const Grid& g, const VoxelMap& vm, int noff, Corr corr, int want_H,
               double* partials, int* ncorr_partials, double* out28, int* out_ncorr);
// ---- the general covariance route (rgc_set_regularization_method other than PLANE, VoxelAccumulationMode::MULTIPLICATIVE): every point
// through the cooperative search, a regularised 3x3 per point (c6: six doubles, SoA c6[a * n + i], sorted order) instead of a unit normal;
// unoptimised by design.  method = rgc_regularization_method; guard (nullable): a tripped speculative-grid guard makes the kernels stand still
void knn_cov6(hipStream_t s, const SortedCloud& cl, int k, int method, double* c6, const int* guard);
// ... or, rgc_set_covariance_estimation(RGC_COV_RBF), the Gaussian-weighted moment of every point within max_dist (rgc_rbf.hip: semantics there).
// reach: cells per axis a ball can span, reach_dist: the distance that bound was made for (rgcapi::rbf_reach)
void rbf_cov6(hipStream_t s, const SortedCloud& cl, float kernel_width, float max_dist_sq, int reach, double reach_dist, int method, double* c6, const int* guard);
void voxel_build_general(hipStream_t s, const SortedCloud& cl, const double* c6, const VoxelMap& vm, int multiplicative, const int* guard);
void linearize_general(hipStream_t s, const SortedCloud& src, const double* c6, Pose T, const Grid& g, const VoxelMap& vm, int noff, Corr corr,
                       int want_H, double* partials, int* ncorr_partials, double* out28, int* out_ncorr);
void unsort6(hipStream_t s, const double* c6, const float4* P, int n, double* out9);
void sort6(hipStream_t s, const double* in9, const float4* P, int n, double* c6);
void compute_error(hipStream_t s, const float4* P, int n, Pose T, const double* vox, int noff, Corr corr, double* partials, double* out1);
void lm_try(hipStream_t s, double* out, const int* ncorr, LmIn in);
void compute_error_dev(hipStream_t s, const float4* P, int n, const double* Tdev, const double* vox, int noff, Corr corr, double* partials, double* out1);
// What a solve on the device works on, filled once per solve (rgcapi: lm_enqueue_batch).  area: the LM area, zeroed once.  partials: 2 * linearize_blocks(src.n) rows of kAccum + 2 doubles (the chained launches
// alternate between the halves).  corr: the two correspondence buffers, the finished state's `cur` the valid one.
struct LmArgs {
  SortedCloud src; Normals nrm;  // the scan
  SortedCloud tgt; VoxelMap vm;  // the map: its grid and voxels; its sorted points for the score
  int noff;
  Corr corr[2];
  double* partials; LmArea* area;
  SmallWords* small; const void* segs_t; const void* segs_s;  // the frame's counters, carried home with the state: the small scratch (nullable), the clouds' deferred buffers
  LmState* h_post; int seq;      // mapped host memory (nullable): a finished state is posted there, then seq in its `gen`; seq > 0: post when done; < 0: when done AND scored
  double* fit_partials;          // non-null: the score is chained to the solve -- the launch whose decision ends it scores the final pose (as does a launch on a finished solve without a score)
  // lazy target: the target is built for the cells stamped lazy_stamp in lazy_need[] only -- a look-up of any other occupied voxel
  // raises LmState::pad2; lazy_counts: the lists' sizes, carried home in LmState::lazy_nq / lazy_ncell
  const int* lazy_need; int lazy_stamp; const int* lazy_counts;
  LmEarly* h_early;              // mapped host memory (nullable): the deciding launch posts the final pose there before it scores it
};
// launch number j of a solve of the device-chained LM (k_lm_step; 0 opens the solve and takes *open) reads image (j - 1) & 1 and leaves image j & 1
inline LmState* lm_image(LmArea* area, int j_last) { return &area->image[j_last & 1]; }
void lm_step(hipStream_t s, const LmArgs& a, int j, const LmInit* open);
// The whole solve in ONE resident launch (see k_lm_solve); the finished state is left in image 0.  The caller keeps
// linearize_blocks(src.n) <= min(the device's CU count, kLmSolveMaxGroups) -- all of them resident at once -- and finds a solve that gave up
// (a bounded wait ran out; give_up_at >= 0: workgroup 0 at that try, without waiting) as a stream that drained with nothing posted.
// seq != 0 always: its magnitude tags the hand-over's words.
// The longest a workgroup waits for the others' rows, in ticks of the 100 MHz wall clock: 2 ms.  The workgroups of a solve are placed as
// CU slots free up, so a wait can last as long as the longest kernel that may hold the slots: the map's kNN launch of a c-main frame, ~165 us.
// Twelve times that, and still a bound on what a lost frame costs (the chained solve that follows takes ~0.15 ms).
constexpr unsigned long long kLmSolveWaitTicks = 200000;
void lm_solve_resident(hipStream_t s, const LmArgs& a, const LmInit& open, int give_up_at);
// a map of at most 32768 points is scanned whole by the wave for a query its first cube does not settle
void fitness_lm(hipStream_t s, const SortedCloud& src, LmState* st, const SortedCloud& tgt, double* partials, LmState* h_post = nullptr, int seq = 0);
// ---- f1: mapping-node feature registration (RGC_mapping.cpp:1069-1358) ----
// factor record = 8 doubles per feature: edge {a[3], b[3], var, valid}, plane {n[3], d, 0, 0, var, valid}
struct MapregAssoc {  // one association loop: feature set (n x 4: x,y,z,weight), its pose, the map grid it is matched against
  const float* feat; int n; int edge;
  Quat q; double t[3];
  const float4* P; const int* start; Grid g;
  double* fac; int* nvalid;  // nvalid nullable: += factors created
};
void mapreg_associate(hipStream_t s, const MapregAssoc* sets, int nsets /* <= 4, one launch */);
int mapreg_blocks(int ne, int np);
// both poses in one launch.  feat/fac/nfeat: {corner cur, surf cur, corner last, surf last}; x14 = q_cur t_cur q_last t_last;
// out56 = per pose {21 upper-triangular H, 6 g, robust cost} (H, g only if want_H); partials: 2 * 28 * max mapreg_blocks doubles
void mapreg_terms(hipStream_t s, const float* const feat[4], const double* const fac[4], const int nfeat[4], const double x14[14], double huber_a,
                  int want_H, double* partials, double* out56);
// ---- f4: one ICP iteration (1-NN correspondences within max_dist + the sums of the rigid fit); out28[0..16] = n, sum p, sum q, sum p q^T, sum d^2
void icp_accumulate(hipStream_t s, const float4* SP, int ns, const SortedCloud& tgt, double max_dist, double* partials, double* out28);
// ---- C8 ----
// scan_small_map: a map of at most 32768 points is scanned whole by the wave for a query its first cube does not settle (as fitness_lm does)
void fitness(hipStream_t s, const float4* SP, int ns, PoseF T, const SortedCloud& tgt, double* partials, double* out1, bool scan_small_map = false);
// ---- misc ----
void transform_f32(hipStream_t s, const float* in, int stride_f, int n, PoseF T, float* out, int out_stride_f);
void unsort3(hipStream_t s, const double* a, const double* b, const double* c, const float4* P, int n, double* out3);
void sort3(hipStream_t s, const double* in3, const float4* P, int n, double* a, double* b, double* c);
int  linearize_blocks(int n);
int  fitness_blocks(int n);
// ---- B2 / B3 / B9 (rgc_pre.hip) ----
// ---- f3: sensor_msgs/PointCloud2 <-> device arrays; fields in the order x, y, z, intensity, ring, time (offset < 0: absent) ----
struct Pc2Layout { int point_step; int off[6]; int type[6]; int big_endian; };
void pc2_unpack(hipStream_t s, const unsigned char* data, int n, const Pc2Layout& L, float4* xyzi, int* ring, float* time);
void pc2_pack(hipStream_t s, const float* in, int cols, int n, int kind, unsigned char* out);
void deskew(hipStream_t s, float* xyzi, int stride_f, int n, Quat qinv, const double t[3]);
void transform_q(hipStream_t s, const float* in, int stride_f, int n, Quat q, const double t[3], float* out, int ostride_f);
// f5 (rgc_keyframes.hip): one launch re-expresses and concatenates a selection of stored keyframe clouds.  One KfSegment per (keyframe, kind)
// with points: src (16-byte points, body frame), n of them, written to out[out0 ..) as q * p + t (transform_q's arithmetic).  blk0[s] = first
// workgroup (kKfBlock points each) of segment s, blk0[nseg] = nblocks.  seg / blk0: device memory.
constexpr int kKfBlock = 256;
struct KfSegment { const float4* src; int n; int out0; Quat q; double t[3]; };
void kf_assemble(hipStream_t s, const KfSegment* seg, const int* blk0, int nseg, int nblocks, float4* out);
// the keyframe selections' radius gate over the mirror of the key positions (pos[p] = {x, y, z, p}): flag[p] (nullable) = d2 < r2, small[0] += the
// number inside; loop != 0: the 64-bit word at small + 2 takes the minimum of (bits of d2) << 32 | p over the positions that are inside, have
// |travel[p] - travel_last| > thr and ids[p] >= min_id.  small: four words, {0, 0, ~0, ~0} on entry
void kf_gate(hipStream_t s, const float4* pos, const float* travel, const int* ids, int n, const float q[3], float r2, int loop, float travel_last, float thr,
             int min_id, int* flag, unsigned* small);
// out[scan[p]] = pos[p] for every flagged p (scan = the exclusive scan of flag)
void kf_compact(hipStream_t s, const float4* pos, const int* flag, const int* scan, int n, float4* out);
// ---- 4-DoF pose graph over the key poses (rgc_pgo.hip; PoseGraphOptimize4DoF, src/RGC_mapping.cpp:2303-2466) ----
// The graph on the device.  Positions 0 .. n_nodes - 1, 4 unknowns each {yaw in degrees, t}; edges: the n_nodes - 1 odometry edges e = n
// (n -> n + 1), then the used loops; ij: 2 ints per edge, meas: 6 doubles per edge {m[3], rel_yaw, pitch, roll}; fixed: the constant
// position or -1.  inc_start[n_nodes + 1] / inc: per node its loops in ascending order (loop * 2 + side, side 1 = the node is the edge's j).
// sep[n_sep]: the separators in ascending order (sep[0] = 0), sep_of[n_nodes]: a position's index in sep or -1.
constexpr int kPgoBlock = 256, kPgoDenseBlock = 1024;
constexpr int kPgoTerm = 64;     // doubles per edge record (k_pgo_edges)
constexpr int kPgoWs = 52;       // doubles per position kept between k_pgo_segments and k_pgo_backsub
constexpr int kPgoSlot = 56;     // doubles per segment handed to k_pgo_dense
constexpr int kPgoMaxSep = 384;  // separators the dense stage takes (its two LDS vectors: 2 x 4 x kPgoMaxSep doubles)
struct PgoGraph { int n_nodes, n_edges, fixed, n_sep; const int *ij, *inc_start, *inc, *sep, *sep_of; const double* meas; };
// residuals, Jacobian products (terms: kPgoTerm doubles per edge), the diagonal blocks D (16 per node) and g (4 per node), out2 = {cost, max |g|}
void pgo_evaluate(hipStream_t s, const PgoGraph& G, const double* x, double* terms, double* D, double* g, double* out2);
// d (4 per node) of (H + clamp(diag H, 1e-6, 1e32) / radius) d = -g; ws: kPgoWs doubles per node, slots: kPgoSlot per separator, M: (4 n_sep)^2
// doubles; flag[0] is raised (never cleared) where the system is not positive definite
void pgo_solve(hipStream_t s, const PgoGraph& G, const double* terms, const double* D, const double* g, double radius, double* ws, double* slots, double* M, double* d,
               int* flag);
// x_new = Plus(x, d); out3 = {model decrease, |d|^2, |x_new|^2 over the free parameters}; part: 4 doubles per node
void pgo_step(hipStream_t s, const PgoGraph& G, const double* terms, const double* D, const double* g, const double* x, const double* d, double* x_new, double* part,
              double* out3);
// ---- NDT registration on a Gaussian voxel map (rgc_ndt.hip; fast_gicp::NDTCuda, src/fast_gicp/cuda/ndt_cuda.cu) ----
// voxel record = kNdtRec doubles: mean(3), covariance after MIN_EIG (6: xx xy xz yy yz zz), number of points, its inverse (6), the covariance
// before MIN_EIG (6), two unused.  The voxels are those of the grid's occupied cells (cell_voxel / vox_cell as for the VGICP map).
constexpr int kNdtRec = 24;
void ndt_voxels(hipStream_t s, const SortedCloud& cl, const VoxelMap& vm);
int  ndt_blocks(int n);
// the terms of n source elements (d2d: the records svox of the source's own map; else the points in / stride_f) against the target map
// (g, vm) at T.  find != 0: the voxels at T + offs[3 * o ..] are looked up and written to corr_v[o * n + i]; else that list is
// read.  Tlin: the pose of the last linearisation (its rotation enters the D2D matrices).  partials: ndt_blocks(n) rows of kAccum doubles,
// ipartials: as many ints; out29: the 28 sums and the number of terms.
void ndt_terms(hipStream_t s, int d2d, int find, const float* in, int stride_f, const double* svox, int n, Pose T, Pose Tlin, const Grid& g,
               const VoxelMap& vm, const int* offs, int noff, int* corr_v, int want_H, double* partials, int* ipartials, double* out29);
// ---- FastGICP: GICP on exact nearest-neighbour correspondences (rgc_gicp.hip; fast_gicp::FastGICP, include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237) ----
// the covariances of a prepared cloud, in its sorted order: c6 (the general route: six doubles per point, SoA) or, c6 == nullptr, its unit normal
struct GicpCov { const double* c6; const double* nx; const double* ny; const double* nz; };
int  gicp_blocks(int n);
// the exact nearest target point of every source point at T (fp32, nn_search): corr[s] = its sorted position or -1 (key >= dmax2), key[s] =
// the squared distance; s = the source's sorted order
void gicp_correspond(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, double dmax2, int* corr, float* key);
// the terms of that pair list at T: M (6 * src.n doubles, SoA) <- the Mahalanobis matrices; partials: gicp_blocks(src.n) rows of kAccum + 1
// doubles; out29: the 28 sums and the number of pairs.  A / B: the source's / the target's covariances
void gicp_terms(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const GicpCov& A, const GicpCov& B, Pose T, int want_H,
                double* M, double* partials, double* out29);
// the cost of the same pairs under the same matrices at another pose
void gicp_error(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const double* M, Pose T, double* partials, double* out1);
// the pair list in caller order: idx[i] = the neighbour's original index or -1, sq[i] = the key
void gicp_export(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const int* corr, const float* key, int* idx, float* sq);
// nb rows of ncol doubles folded to out[ncol] in a fixed order (k_gicp_fold: one wave per column)
void gicp_fold(hipStream_t s, const double* partials, int nb, int ncol, double* out);
// ---- FastGICPSingleThread: GICP with anchor-cached correspondences (rgc_gicp_st.hip; fast_gicp::FastGICPSingleThread,
// include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125) ----
constexpr int kGicpStAcc = kAccum + 2;  // the 28 sums, the kept pairs, the points searched
// the per-point state in the source's sorted order (src.n entries each; M: 6 * src.n doubles, SoA; anchor.w unused) and the compaction's
// scratch: searched (0 / 1 of the last linearisation), list (the points it searched, in no fixed order), count (one int: how many)
struct GicpStState { int* corr; float* key1; float* key2; float4* anchor; double* M; int* searched; int* list; int* count; };
// the skip test of every source point at T and the two-nearest search of those that fail it (first != 0: of all of them); *st.count must be
// zero on entry (in stream order) and holds the number searched afterwards, until gicpst_terms zeroes it again
void gicpst_correspond(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, double dmax2, int first, const GicpStState& st);
// the terms of the state at T (M computed and stored where searched, loaded elsewhere); partials: gicp_blocks(src.n) rows of kGicpStAcc
// doubles; out30: the sums (the 28, the kept pairs, the points searched).  Leaves *st.count at zero
void gicpst_terms(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const GicpStState& st, const GicpCov& A, const GicpCov& B, Pose T, int want_H,
                  double* partials, double* out30);
// the state in caller order (each output nullable)
void gicpst_export(hipStream_t s, const SortedCloud& src, const SortedCloud& tgt, const GicpStState& st, int* idx, float* sq, float* sq2, int* was);
// ---- FastGICPMultiPoints: GICP on radius-merged target distributions (rgc_gicp_mp.hip; fast_gicp::FastGICPMultiPoints,
// include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:92-221) ----
constexpr int kGicpMpMerged = 11;  // per source point: neighbours, sum of weights, merged mean (3), merged covariance (6)
constexpr int kGicpMpAcc = kAccum + 2;  // the 28 sums, the source points with a neighbour, the neighbours
int  gicp_mp_blocks(int n);
// the exact radius gather at T (fp32 query and key, key < r2 strict) and the weighted merge of the members' Gaussians: merged = SoA
// [kGicpMpMerged][src.n] in the source's sorted order; cand (nullable): candidates looked at per source point.  B: the target's covariances
void gicp_mp_merge(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, const GicpCov& B, float r2, double r, double* merged, int* cand);
// the terms of the merged list at T; partials: gicp_mp_blocks(src.n) rows of kGicpMpAcc doubles; out30: the sums.  A: the source's covariances
void gicp_mp_terms(hipStream_t s, const SortedCloud& src, const double* merged, const GicpCov& A, Pose T, int want_H, double* partials, double* out30);
// the merged list in caller order (each output nullable): count[i], sum_w[i], mean3[3 i ..], cov6[6 i ..]
void gicp_mp_export(hipStream_t s, const SortedCloud& src, const double* merged, int* count, double* sum_w, double* mean3, double* cov6);
// the members themselves: off = the exclusive scan of the caller-order counts (src.n + 1 entries); idx / sq: original target index and key
void gicp_mp_fill(hipStream_t s, const SortedCloud& src, PoseF T, const SortedCloud& tgt, float r2, double r, const int* off, int* idx, float* sq);
// ---- VGICP's DIRECT_RADIUS neighbour method (rgc_vgicp_radius.hip; fast_gicp::FastVGICPCuda::setNeighborSearchMethod(method, radius),
// src/fast_gicp/cuda/fast_vgicp_cuda.cu:42-95) ----
int  vgicp_radius_blocks(int n);   // workgroups (rows of partials) of a linearisation of n source points
int  vgicp_radius_group();         // lanes per source point of this build
// one table entry: the three offsets as signed bytes, x | y << 8 | z << 16 (|offset| <= ceil(radius) <= 5 under RGC_NDT_MAX_OFFSETS)
inline int vgicp_radius_pack(int x, int y, int z) { return (x & 0xff) | ((y & 0xff) << 8) | ((z & 0xff) << 16); }
// linearize / linearize_general over the table offs[0 .. noff) (device memory): A.c6 != nullptr = the general route's six entries, else the unit
// normal.  corr: noff * src.n entries as linearize leaves them; partials: vgicp_radius_blocks(src.n) rows of kAccum doubles, ncorr_partials: as many ints
void vgicp_radius_linearize(hipStream_t s, const SortedCloud& src, const GicpCov& A, Pose T, const Grid& g, const VoxelMap& vm, const int* offs, int noff,
                            Corr corr, int want_H, double* partials, int* ncorr_partials, double* out28, int* out_ncorr);
// ---- the search index (rgc_search.hip; pcl::KdTreeFLANN::nearestKSearch / radiusSearch, e.g. src/RGC_mapping.cpp:1097,1537) ----
// The read-out words of one query call, zeroed by the caller: candidates looked at, queries whose cube grew, members found, rows that took the sort's
// long route; nonfinite != 0: a query had a non-finite coordinate (its row is empty); longest: the longest row of search_count
struct SearchStats { unsigned long long candidates, grown, members, rows_long; int nonfinite, longest; };
constexpr int kSearchMaxK = 32;           // the largest list tier of k_search_knn
// Rows up to this many members are sorted in one pass of k_search_sort_rows: 4096 packed 64-bit entries = 32 KiB of the CU's 160 KiB of LDS, so
// four workgroups fit on a CU beside the 2 KiB small instantiation's
constexpr int kSearchSortWindow = 4096;
int  search_group();         // lanes per query of this build
int  search_sort_window();
int  search_tier(int k);     // the list length k_search_knn runs k with: 4, 8, 16 or 32
// queries: Q[i * qstride_f + 0..2].  Row i of out_idx / out_sq (k entries each): the min(k, members) smallest under (key, original index), -1 / +inf
// behind them; out_cnt[i]: how many.  bounded != 0: members are the points with key < r2 (r: the radius r2 was made from), else every point
void search_knn(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, int k, int bounded, float r2, double r, int* out_idx, float* out_sq,
                int* out_cnt, SearchStats* st);
// search_knn's rows into CSR: off = the exclusive scan of cnt; sq nullable
void search_compact(hipStream_t s, const int* row_idx, const float* row_sq, const int* cnt, const int* off, int nq, int width, int* idx, float* sq);
// the uncapped radius search: the members per query, then (off = the exclusive scan of the counts) the members as packed entries
// (key bits << 32 | original index), ascending in the sorted cloud inside a row
void search_count(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, int* out_cnt, SearchStats* st);
void search_fill(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, const int* off, unsigned long long* ent);
// every row ascending; longest: the longest row (SearchStats::longest); tmp: as many entries as ent (read only where a row exceeds the window)
void search_sort_rows(hipStream_t s, const int* off, int nq, int longest, unsigned long long* ent, unsigned long long* tmp, SearchStats* st);
void search_unpack(hipStream_t s, const unsigned long long* ent, long long total, int* idx, float* sq /* nullable */);
// ---- the outlier filters (rgc_outlier_*, rgc_filters.hip): a cloud against itself on a grid of its own; every output at the ORIGINAL index ----
// What a call reads back: SOR's statistics as k_sor_fold posts them, and the read-out words -- indexed points looked at (word 0), points whose cube of cells
// grew (word 1) -- as kStatSlots partial sums a cache line apart: a workgroup adds its sums into slot (block & (kStatSlots - 1)), the host adds the
// slots.  (One word for every wave of a launch to add into serialises the launch: at 1 M points the kernels' time was the atomics', whatever the walk did.)
// The clusters', the normals' and the descriptors' read-out words are laid out the same way, behind heads of their own
constexpr int kStatSlots = 32;
using StatWords = unsigned long long[kStatSlots][8];
struct OutlierStats { double mean, stddev, threshold, pad; StatWords words; };
constexpr int kOutlierMaxMeanK = 63;  // mean_k + 1 entries: the largest list tier of k_sor_meandist
int  outlier_group();          // lanes per point of this build
int  outlier_tier(int mean_k); // the list length k_sor_meandist runs mean_k with: 4, 8, 16, 32 or 64
int  outlier_stat_rows(int n); // rows of two doubles sor_stats needs in `partials`
// out_d[i] = (float)(sum over ranks 1 .. mean_k of (double)sqrtf(key) / mean_k), the ranks of point i's ascending keys over the whole cloud (itself rank 0)
void sor_meandist(hipStream_t s, const SortedCloud& cl, int mean_k, float* out_d, OutlierStats* st);
// sum d and sum d d in input-index order (fixed order), then st->mean / stddev / threshold = mean + std_mul stddev (variance clamped at 0)
void sor_stats(hipStream_t s, const float* d, int n, double std_mul, double* partials, OutlierStats* st);
// out_cnt[i] = the points with key < r2 about point i (itself one of them; r: the radius r2 was made from); exact == 0: a lower bound > min_nb where the
// count exceeds min_nb (the walk stops there)
void ror_count(hipStream_t s, const SortedCloud& cl, float r2, double r, int min_nb, int exact, int* out_cnt, OutlierStats* st);
// flag[0 .. n]: kept (flag[n] = 0); d != nullptr: (double)d[i] <= st->threshold, else cnt[i] - 1 >= min_nb; negative inverts
void outlier_flag(hipStream_t s, const float* d, const int* cnt, int n, const OutlierStats* st, int min_nb, int negative, int* flag);
// off = the exclusive scan of flag: the kept points' 16-byte records (c = 0 for a 12-byte stride) and input indices in ascending input index; each nullable
void outlier_emit(hipStream_t s, const float* in, int stride_f, int n, const int* flag, const int* off, float* out, int* out_index);
// ---- Euclidean cluster extraction (rgc_cluster_*, rgc_cluster.hip): the connected components of the key < r2 graph of a cloud on a grid of its own ----
// What a call reads back: the error word (!= 0: a find / unite loop ran past its iteration cap -- a logic error, RGC_ERR_HIP) and the read-out words as
// kStatSlots partial results a cache line apart, as OutlierStats': word 0 indexed points looked at (summed), word 1 components (summed), word 2 the
// largest component's size (the slots' maximum)
struct ClusterStats { int err; int pad[15]; StatWords words; };
constexpr int kClusterRadixTile = 1024;   // pairs per workgroup of a radix pass
constexpr int kClusterRadixDigits = 256;  // 8-bit digits
int  cluster_group();              // lanes per point of this build's linking kernel
int  cluster_radix_tiles(int m);   // workgroups of a radix pass over m pairs: hist / hist_off hold kClusterRadixDigits * tiles + 1 ints
// parent / lead / size: n ints each, on SORTED positions.  After this chain parent[x] is x's root, lead[root] the component's smallest ORIGINAL index,
// size[root] its points.  r: the tolerance r2 was made from
void cluster_link(hipStream_t s, const SortedCloud& cl, float r2, double r, int* parent, int* lead, int* size, ClusterStats* st);
// at the ORIGINAL index i: comp[i] the leader of i's component, csize[i] its size, flag_p[i] = min_size <= size <= max_size, flag_l[i] = flag_p[i] and
// i is the leader; flag_p[n] = flag_l[n] = 0.  Components and the largest size go to st
void cluster_assign(hipStream_t s, const SortedCloud& cl, const int* parent, const int* lead, const int* size, int min_size, int max_size, int* comp, int* csize,
                    int* flag_p, int* flag_l, ClusterStats* st);
// off_l = the exclusive scan of flag_l: the kept leaders in ascending input index, key = n - size, val = the leader
void cluster_emit(hipStream_t s, int n, const int* flag_l, const int* off_l, const int* csize, int* key, int* val);
// a STABLE ascending sort of m (key, val) pairs on the low `bits` bits of the key, ceil(bits / 8) passes between key[0] / val[0] and key[1] / val[1];
// returns which of the two holds the result (0 when no pass was needed: bits = 0 or m <= 1).  block_sums: as exclusive_scan's for the histogram
int  cluster_radix_sort(hipStream_t s, int m, int bits, int* key[2], int* val[2], int* hist, int* hist_off, int* block_sums);
// rank_at[val[r]] = r, sizes[r] = n - key[r] for r < m; sizes[m] = 0
void cluster_rank(hipStream_t s, int n, int m, const int* key, const int* val, int* rank_at, int* sizes);
// labels[i] (nullable) = flag_p[i] ? rank_at[comp[i]] : -1; pkey / pval (nullable together) at off_p[i]: that rank and i, for the kept points
void cluster_labels(hipStream_t s, int n, const int* flag_p, const int* off_p, const int* comp, const int* rank_at, int* labels, int* pkey, int* pval);
// ---- surface normal estimation (rgc_normal_*, rgc_normals.hip): a normal and a curvature per query from its neighbourhood in a surface cloud's grid ----
// What a call reads back: the queries' non-finite flag and the read-out words as kStatSlots partial sums a cache line apart, as OutlierStats': word 0
// indexed points looked at, word 1 queries whose cube of cells grew (k route), word 2 valid queries (three members or more)
struct NormalStats { int nonfinite; int pad[15]; StatWords words; };
struct NormalSign { float vx, vy, vz; int flip; };                  // the viewpoint and the sign rule (rgc_normal_params)
struct NormalOut { float* n4; double* cov6; double* cen; int* cnt; };  // per query, each nullable: (nx, ny, nz, curvature), {xx,xy,xz,yy,yz,zz}, the centroid, the members
int  normal_group();         // lanes per query of this build's k route ...
int  normal_radius_group();  // ... and radius route
int  normal_tier(int k);     // the list length k_nrm_knn runs k with: 4, 8, 16 or 32
// *flag = 1 if a query has a non-finite coordinate (untouched otherwise)
void normal_check(hipStream_t s, const float* Q, int qstride_f, int nq, int* flag);
// the k route: the min(k, cl.n) smallest (key, original index) of every query; SP / sstride_f: the surface cloud's records at their ORIGINAL indices.
// Q == nullptr (both routes): the queries are the cloud's own points (nq = cl.n), walked in the grid's sorted order, each written at its original index
void normal_knn(hipStream_t s, const float* Q, int qstride_f, int nq, const float* SP, int sstride_f, const SortedCloud& cl, int k, const NormalSign& sg, const NormalOut& out,
                NormalStats* st);
// the radius route: every member with key < r2 (r: the radius r2 was made from)
void normal_radius(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, const NormalSign& sg, const NormalOut& out, NormalStats* st);
// ---- FPFH descriptors (rgc_fpfh_*, rgc_fpfh.hip): 33 bins per query from the normals of a surface cloud's balls, in two passes over its grid ----
// What a call reads back, as NormalStats: word 0 indexed points looked at (every pass), word 1 non-skipped pair terms, word 2 queries with a member
constexpr int kFpfhBins = 33;
struct FpfhStats { int nonfinite; int pad[15]; StatWords words; };
// *flag = 1 if a query has a non-finite coordinate (Q nullable: the cloud is its own surface, its grid build checks it); N4[i] = the normal of surface
// point i with w = 1 where its three components are finite, else 0
void fpfh_check(hipStream_t s, const float* Q, int qstride_f, int nq, const float* N, int nstride_f, int ns, float4* N4, int* flag);
// flag[sorted position] = 1 for every member (key < r2) of some query's ball; flag[0 .. cl.n] was zeroed by the caller
void fpfh_mark(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, float r2, double r, int* flag, FpfhStats* st);
// list[off[i]] = i for every flagged sorted position i (off = the exclusive scan of flag)
void fpfh_list(hipStream_t s, const int* flag, const int* off, int ns, int* list);
// the SPFH counts (33 per point) and row sizes of the listed sorted positions (list == nullptr: of every point), written at the points' ORIGINAL indices;
// n_list: the list's length, on the device
void fpfh_spfh(hipStream_t s, const SortedCloud& cl, const int* list, const int* n_list, const float4* N4, float r2, double r, unsigned* spfh, int* m, FpfhStats* st);
// the descriptors (out, nullable: 33 floats per query) and row sizes (cnt, nullable).  Q == nullptr: the queries are the cloud's own points, walked in
// the grid's sorted order, each written at its original index
void fpfh_combine(hipStream_t s, const float* Q, int qstride_f, int nq, const SortedCloud& cl, const unsigned* spfh, const int* m, float r2, double r, float* out, int* cnt,
                  FpfhStats* st);
void vg_bbox(hipStream_t s, const float* in, int stride_f, int n, float inv, int* mm6, int* flags);
// sparse leaf grids: counting sort over (y, z) rows, rank by (leaf x, index) inside a row -- the whole filter as one chain of launches.
// edge > 0: g is a box kept from an earlier cloud (see rgc_pre.hip).  res[0] <- flags of this run (1 non-finite point, 2 point outside g,
// 4 point within `edge` leaves of g's faces), res[1] = the live flag word (must be 0 on entry, is 0 on exit), res[2] <- number of leaves.
// dense != 0: the counting sort runs over the leaves themselves ("rows" below = leaves; dense clouds).
// row_block_sums: 8 bytes x (rows / 2048 + 2); head_block_sums: n / 2048 + 2 ints; cnt: rows + 1 zeros, left at zero.
// seg_shift: the counting sort's bucket is 2^seg_shift leaves of a grid row (0: the leaf itself, 31: the whole row); cnt / start: rows x vg_segments() + 1 entries
int vg_segments(const LeafGrid& g, int seg_shift);
// returns true when the chain used the packed record (k_vg_rows_place<true> / k_vg_rows_rank<true>), false for the unpacked one
bool vg_rows(hipStream_t s, const float* in, int stride_f, int n, float inv, LeafGrid g, int edge, int seg_shift, int* row_of, int* lx, int* slot_then_pos, int* cnt,
             int* start, void* row_block_sums, unsigned long long* tmp, int* order, unsigned long long* leaf, int* head_block_sums, float* out,
             int* res, int mode = 0, float leafsz = 0.f, int* out_index = nullptr);
// mode of the chain's last launch: the leaf's centroid (pcl::VoxelGrid), or the member nearest the leaf's centre with its input index in
// out_index (nullable) (pcl::UniformSampling; leafsz = the leaf size the centre is computed with)
constexpr int kVgModeCentroid = 0, kVgModePick = 1;
// UniformSampling's unfiltered copy: out = the points' bits, out_index (nullable) = the identity
void us_copy(hipStream_t s, const float* in, int stride_f, int n, float* out, int* out_index);

// ---- A1-A8 front-end (rgc_frontend.hip) ----
int fe_blocks(int n);
int fe_slot_ints();
void fe_filter(hipStream_t s, const float* in, int stride_f, int n, FeParams p, int* ring, int* st, int* rank_in_block, int* blk_hist);  // + per-block ring ranks / histograms
void fe_half(hipStream_t s, const float* in, int stride_f, int n, const int* ring, int* st);
void fe_bucket(hipStream_t s, const float* in, int stride_f, int n, int NS, const int* ring, int* rank_in_block, int* blk_hist, int* meta,
               const int* st, float4* C, int* inum2, int* z0, int* z1, int* z2, int* z3);  // z0..z3: four per-point arrays zeroed on the way (n ints each)
// cs: the launch's bound; csp (nullable): the sweep's size on the device (meta[128]), read by the kernels -- the host need not know it
void fe_stencils(hipStream_t s, const float4* C, int cs, const int* csp, float* range_vec, float* scan_angle, const int* inum2, int* inum, float* curv,
                 float* curv2, float* icurv, float* dsrc, float* osrc, int* picked);
void fe_ground(hipStream_t s, const float4* C, int cs, const int* csp, int NS, const float* range_vec, const int* meta, int* gmark, int* mult, int* seedcnt,
               double* partials, double* out11, double* fit);   // ... the ground sums into out11 and their plane fit into fit[16], on the device
// the distance sums into out2[2]
void fe_ground_dist(hipStream_t s, const float4* C, int cs, const int* csp, const int* mult, const double* fit, double* partials, double* out2);
void fe_ground_list(hipStream_t s, const float4* C, int cs, const int* csp, int NS, const float* range_vec, const int* meta, const int* seedcnt,
                    const int* seedpos, float4* out, int cap);
void fe_select(hipStream_t s, const float4* C, int NS, const int* meta, const float* curv, const float* curv2, const float* icurv, const int* inum,
               const int* gmark, int* picked, int* ipicked, int* label, int* ilabel, int* slots, int* flags, int max_ring /* points in the largest ring: sizes the LDS window */,
               int* sorted_curv, int* sorted_icurv /* cs ints each: per-sector sorted point indices (scratch) */);
void fe_emit(hipStream_t s, const float4* C, int NS, const int* slots, const float* dsrc, const float* osrc, float* sharp, float* flat, float* inten,
             int cap, int* counts);

#ifdef RGC_LAB_TURN
void lab_turn(unsigned long long* out8);
#endif
#if defined(RGC_LAB) || defined(RGC_LAB_BLK)
void lab_blocks(long long* out65536);  // developer build: {start, end, XCC, first query} of every workgroup of the map's bulk kNN launch
#endif
#ifdef RGC_LAB
void lab_lm_ts(unsigned long long* out16, hipStream_t s);  // developer build: phase timestamps of k_lm_step
void lab_why(int* out8);
void lab_declines(int* out16);                              // developer build: why knn_point_seeded declined, per lane (and resets)
void lab_iters(unsigned long long* out8);                   // developer build: wave-level loop counts of the map's bulk kNN kernel (and resets them)
void lab_wave_ts(long long* out16384, hipStream_t s);       // developer build: start / end of the scan kNN launch's waves
#endif
}  // namespace rgck
