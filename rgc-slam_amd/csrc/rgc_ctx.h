// rgc_ctx.h -- internal to librgc_hip.so: what the host files of the C-ABI (rgc_api*.hip, one per subsystem) share.  The build-flag defaults, the context
// (struct rgc_ctx: opaque to callers, include/rgc_hip.h) with a record per subsystem beside the VGICP core's loose state, and the helpers more than one of those
// files calls, in namespace rgcapi (-fvisibility=hidden keeps them out of the dynamic symbol table).  DESIGN.md says which file holds what.
#pragma once
#include "../../include/rgc_hip.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <mutex>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "rgc_kernels.h"

namespace rgcapi {

// Build-time switches (RGC_EXTRA_FLAGS=-D...): alternative routes to the SAME results, kept for A/B measurements.  A caller's
// process reads RGC_LM_IMPL, RGC_VOXEL_IMPL, RGC_LM_GIVE_UP_AT, RGC_SPEC_GRID, RGC_KNN_SEEDS, RGC_KNN_CACHE (a context's initial rgc_set_knn_reuse mode), RGC_TRACE_ALLOC, RGC_TRACE_CACHE, RGC_CHECK_POINTERS,
// RGC_FORCE_GENERAL (the odometer's settings on the general covariance route: a cross-check) and the
// three scheduling switches RGC_JOIN_SPIN_US / RGC_PREP_EVENT_EXT / RGC_COOP_STREAM from the environment, once, in rgc_create.
#ifndef RGC_LM_POST
#define RGC_LM_POST 1          // 0: rgc_align_end always waits for the stream and its copy of the state (round 2)
#endif
#ifndef RGC_FE_SPEC
#define RGC_FE_SPEC 1          // 0: the front-end reads every sweep's size back before its stencil kernels
#endif
#ifndef RGC_SOLVE_BEHIND_MAP
#define RGC_SOLVE_BEHIND_MAP 1 // 0: the solve always on the scan's (high-priority) stream (round 2)
#endif
#ifndef RGC_KNN_SEEDS
#define RGC_KNN_SEEDS 1        // 0: the map's exact search never starts from the previous search's k-th distances (round 4)
#endif
#ifndef RGC_COOP_STREAM
#define RGC_COOP_STREAM 0      // 1: the scan's deferred queries are resolved by waiting waves at the end of its bulk kNN launch (coop_stream): a frame at a time
                               // 3 % faster, a sequence on two contexts 9 % slower (the waiting waves hold slots the other context's map wants); measured, off
#endif
#ifndef RGC_PREP_EVENT_EXT
#define RGC_PREP_EVENT_EXT 1
#endif
#ifndef RGC_JOIN_SPIN_US
#define RGC_JOIN_SPIN_US 300
#endif
#ifndef RGC_EARLY_POSE
#define RGC_EARLY_POSE 1       // 0: rgc_align_end_reframe waits for a solve's score before it enqueues the next frame's target (round 5)
#endif
#ifndef RGC_KNN_CACHE
#define RGC_KNN_CACHE 1        // 0: no neighbour lists (rgck::KnnCache): every frame searches the whole map, seeded
#endif
#ifndef RGC_MAP_WIDE_R
#define RGC_MAP_WIDE_R 2       // block radius of the bulk kNN launch for a sparse map (0 = off, 2)
#endif
#ifndef RGC_MAP_WIDE
#define RGC_MAP_WIDE 0.25      // ... taken when the map has fewer points per grid cell than this
#endif
#ifndef RGC_SRC_RES
#define RGC_SRC_RES 0.0        // fixed cell size of the scan's kNN grid (0 = adaptive)
#endif
static_assert(RGC_MAP_WIDE_R == 0 || RGC_MAP_WIDE_R == 2, "RGC_MAP_WIDE_R: 0 or 2");
constexpr int kProfKinds = RGC_K_COUNT;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool borrowed = false;  // p belongs to another context (rgc_share_target): never freed, never grown here
  template <class T> T* as() const { return static_cast<T*>(p); }  // the one place the host files turn a buffer into a typed pointer
};

struct Cloud {
  // input (device copy owned by ctx, or caller's device pointer)
  const float* in = nullptr;
  int stride_f = 0;
  int n = 0;
  bool ready = false;  // grid + normals (+ voxels for the target) enqueued
  bool covs_user = false;  // the normals were given by the caller (rgc_set_source/target_covariances), not computed from the neighbours
  DevBuf in_copy, cell_of, slot_of, cnt, start, block_sums, order_tmp, P, nx, ny, nz;  // P: sorted float4 {x,y,z,orig idx}
  DevBuf c6;            // the general covariance route only (general_route()): six doubles per point, SoA, instead of the normal
  bool general = false; // this cloud was prepared on the general route (its covariances are in c6, nx / ny / nz hold nothing)
  DevBuf segs;  // deferred-query list of the bulk kNN kernel: [count, pad x15][query n][bound n]
  int deferred_seen = -1;  // deferred count of the last cloud whose count came home (sizes the next cooperative launch)
  rgck::Grid grid{};   // the search grid: sorted array P, start[]; for the target also the voxel grid cell_voxel[] is laid out on
  // speculative grid (voxel level): the previous cloud's grid, widened, re-used without the bounding-box round trip; k_count guards it
  rgck::Grid spec_grid{};
  bool spec_ok = false;    // spec_grid is usable
  bool spec_used = false;  // this cloud was prepared on spec_grid and its guard has not been read yet
  bool reframe_pending = false;  // in[] has not been written yet: the next preparation produces it from rf (rgc_set_target_reframed)
  rgck::Reframe rf{};
  size_t cnt_clean = 0;    // cnt[0 .. cnt_clean) is known to be zero (the cell scan leaves the counters it consumed at zero)
  const void* cnt_seen = nullptr;  // the allocation cnt_clean refers to
  // target only
  DevBuf cell_voxel, vox, vox_cell;
  int nvox = -1;
  // lazy target (rgc_set_target_lazy): 0 = covariances and voxel map complete; 1 = the grid is built, nothing else (the solve's guess
  // decides which part is needed); 2 = built for the cells stamped need_stamp in `need` only
  int lazy = 0;
  DevBuf need, qlist, cell_list;  // one stamp per grid cell; the listed queries (points) and cells of this frame (k_footprint)
  int need_stamp = 0;
  const void* need_seen = nullptr;  // the allocation the stamps refer to
  int lazy_nq_seen = -1, lazy_ncell_seen = -1;  // the previous frame's list sizes (they size this frame's launches)
  // seeds of the exact search (rgck::KnnSeeds): kept while the target is a re-expression of the SAME buffer (rgc_set_target_reframed: the
  // key is the buffer it re-frames), one float per original point
  DevBuf seed;
  const void* seed_key = nullptr;
  int seed_n = 0;
  bool seed_on = false;    // this cloud's searches read and write them
  bool seed_warm = false;  // ... and some search has written them
  float seed_slack = 0.f;
  // the neighbour-list cache on top of the seeds (rgck::KnnCache): the same key, the same life
  DevBuf nbr, rank_of, pos_of, qrank, map_copy, todo, cache_small;  // cache_small: kTodoLists list lengths, the epoch word, the overflow word
  bool cache_on = false;    // this preparation compares the map with map_copy and its searches read / write the lists
  bool cache_live = false;  // the LAST preparation's searches ran with the lists attached (otherwise they are stale: the next frame starts over)
  int cache_frame = 0;
  int cache_e2 = 0;         // binary exponent of the largest coordinate the certificates were issued for
  int cache_e2_low = 0;     // frames in a row whose coordinates stayed below it
  int cache_e2_low_max = 0; // ... and the largest exponent among them
  int todo_cap = 0;
  bool slots_clean = false;        // segs' entry words hold the "empty slot" pattern (the scan's deferred queries resolved inside its bulk launch, and the dense map's)
  const void* slots_seen = nullptr;  // ... of this allocation
  size_t slots_cap = 0;              // ... at this capacity
  bool prepared_recorded = false;  // the preparation's last launch carried the context's tgt_prepared event (no record packet behind it)
  bool cache_searched_lists = false;  // the last preparation's search was the seeded launch that reads the lists (rgc_stats::searched_target)
  int searched_known = -1;            // rgc_stats::searched_target of this preparation once it has been fetched (-1: not yet)
  rgck::SortedCloud sorted() const { return {P.as<const float4>(), start.as<const int>(), grid, n}; }  // the typed views the launch wrappers take (rgc_kernels.h)
  rgck::Normals normals() const { return {nx.as<double>(), ny.as<double>(), nz.as<double>()}; }
  rgck::VoxelMap voxels() const { return {cell_voxel.as<const int>(), vox.as<double>(), vox_cell.as<int>()}; }
  rgck::DeferredBuf deferred(const int* guard /* of the cloud's grid, nullable: guard_of, rgc_api.hip */) const { return {segs.p, guard}; }
};

// ---- the registration methods beside VGICP: what each keeps between its calls.  bufs(): its device buffers, once (rgc_destroy walks them);
// pinned(): its page-locked host mirrors; clouds(): its clouds.  `valid` = the frozen state is that of the present clouds and settings
struct NoLists {  // a record derives from it and states only the lists it has
  std::vector<void*> pinned() { return {}; }
  std::vector<Cloud*> clouds() { return {}; }
};
struct Sums : NoLists {  // where a method's term kernels fold to: per-block partials, the folded sums, their pinned mirror (32 doubles)
  DevBuf partials, out;
  double* h_out = nullptr;
  std::vector<DevBuf*> bufs() { return {&partials, &out}; }
  std::vector<void*> pinned() { return {h_out}; }
};

// NDT registration (rgc_ndt_*): two clouds of its own (0 target, 1 source) with their grids and voxel maps (Cloud::cell_voxel / vox / vox_cell,
// records of rgck::kNdtRec doubles), the offsets of the neighbour method, the frozen term list of the last linearisation
struct NdtRecord {
  rgc_ndt_params prm{1.0, RGC_NDT_D2D, RGC_NDT_DIRECT7, 0.0};
  Cloud cl[2];
  bool set[2] = {false, false};       // a cloud has been handed over (its points are in Cloud::in_copy, 12-byte stride)
  bool built[2] = {false, false};     // ... and its voxel map is built, at resolution built_res
  double built_res[2] = {0.0, 0.0};
  std::vector<int> offs_h;            // 3 ints per offset, the order of the reference's list
  DevBuf offs, corr, ipartials, small;
  Sums sums;
  bool offs_dirty = true;
  int* h_small = nullptr;             // pinned: 8 ints
  bool valid = false;                 // corr holds the list of n elements x noff offsets made under mode at Tlin
  int n = 0, noff = 0, mode = 0, terms = 0;
  double Tlin[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<DevBuf*> bufs() { return {&offs, &corr, &ipartials, &small, &sums.partials, &sums.out}; }
  std::vector<void*> pinned() { return {sums.h_out, h_small}; }
  std::vector<Cloud*> clouds() { return {&cl[0], &cl[1]}; }
};

// FastGICP (rgc_gicp_*) on the context's own source and target: the pair list of the last rgc_gicp_linearize (per sorted source point the
// neighbour's position in the target's sorted array or -1, and the fp32 key) and its Mahalanobis matrices
struct GicpRecord : NoLists {
  double dmax = (double)FLT_MAX;      // corr_dist_threshold_ (fast_gicp_impl.hpp:18: std::numeric_limits<float>::max())
  DevBuf corr, key, M;
  bool valid = false;
  int n = 0, kept = 0;
  std::vector<DevBuf*> bufs() { return {&corr, &key, &M}; }
};

// FastGICPSingleThread (rgc_gicpst_*) on the same clouds: per sorted source point the pair, the keys to the nearest and the second nearest at
// its anchor, the anchor and the Mahalanobis matrix of the pose it was last searched at (rgck::GicpStState), the compaction's list and
// counter.  valid covers the anchors: it falls on rgc_gicpst_reset and at the start of rgc_gicpst_align too; the next linearisation then
// searches every point
struct GicpStRecord : NoLists {
  DevBuf corr, key1, key2, anchor, M, searched, list, count;
  bool valid = false;
  int n = 0, kept = 0, searched_n = 0;
  std::vector<DevBuf*> bufs() { return {&corr, &key1, &key2, &anchor, &M, &searched, &list, &count}; }
};

// FastGICPMultiPoints (rgc_gicpmp_*) on the same clouds: the merged list of the last rgc_gicpmp_linearize (rgck::kGicpMpMerged doubles per sorted
// source point), the fp32 pose and radius it was made under (the read-out of the members walks the candidates again).  valid falls on
// rgc_gicpmp_set_params too
struct GicpMpRecord : NoLists {
  rgc_gicp_mp_params prm{0.5, 64, 1e-5, 1e-5};
  DevBuf merged, cand, scratch;
  Sums sums;
  bool valid = false;
  int n = 0, points = 0;
  long long pairs = 0;
  float T32[16] = {0};
  std::vector<DevBuf*> bufs() { return {&merged, &cand, &scratch, &sums.partials, &sums.out}; }
  std::vector<void*> pinned() { return {sums.h_out}; }
};

// ---- the cloud operations (search index, outlier filters, clusters, plane, normals, FPFH): what each keeps between its calls, released like the
// methods' records above.  The helpers of their common call frame are declared below (rgc_api_search.hip)
// What five of them hold alike: a cloud used for its grid only (independent of the context's source and target, and of each other's), the read-out
// words on the device -- the 8 ints of the grid's measurement, the call's own words at kFrameWordsAt, what the kernels post at kFrameStatsAt -- their
// pinned mirror, and the cell-size knob (rgc_*_set_cell: 0 = the search index's automatic rule; the search index takes its cell with the cloud)
struct OpFrame {
  Cloud cl;
  DevBuf small;
  unsigned char* h = nullptr;
  double cell = 0.0;
};
struct FrameLists {  // what a record around one OpFrame lists beside its buffers
  OpFrame f;
  std::vector<void*> pinned() { return {f.h}; }
  std::vector<Cloud*> clouds() { return {&f.cl}; }
};
constexpr size_t kFrameBytes = 4096, kFrameWordsAt = 32, kFrameStatsAt = 64;
template <class T> T* stats(const OpFrame& f) {
  static_assert(kFrameStatsAt + sizeof(T) <= kFrameBytes, "the read-out words fit");
  return reinterpret_cast<T*>(f.small.as<unsigned char>() + kFrameStatsAt);
}
template <class T> const T* host_stats(const OpFrame& f) { return reinterpret_cast<const T*>(f.h + kFrameStatsAt); }
inline int* host_words(const OpFrame& f) { return reinterpret_cast<int*>(f.h + kFrameWordsAt); }  // the call's own words in the mirror

// What emit_selected works on (the outlier filters, the plane's extraction): the flags in input order, their scan and its block sums, a host
// caller's records and indices
struct Selection {
  DevBuf flag, off, bs, out, idx;
};

// The search index (rgc_search_*, rgc_api_search.hip): the indexed cloud (a host caller's points in Cloud::in_copy); the staged host queries, the query
// calls' scratch (counts, offsets, block sums, fixed-width rows, packed entries and the long sort's second row, the results of a host caller); the
// mirror holds rgck::SearchStats
struct SearchRecord : FrameLists {
  bool set = false;
  rgc_search_info info{};
  DevBuf q, cnt, off, bs, row_idx, row_sq, ent, tmp, idx, sq;
  std::vector<DevBuf*> bufs() { return {&f.small, &q, &cnt, &off, &bs, &row_idx, &row_sq, &ent, &tmp, &idx, &sq}; }
};

// The outlier filters (rgc_outlier_*, rgc_api_filters.hip): a host caller's staged records, the mean distances / counts, the selection, the
// fixed-order sums' rows; the mirror holds the number kept and rgck::OutlierStats
struct OutlierRecord : FrameLists {
  rgc_outlier_info info{};
  DevBuf in, val, partials;
  Selection sel;
  std::vector<DevBuf*> bufs() { return {&f.small, &in, &val, &partials, &sel.flag, &sel.off, &sel.bs, &sel.out, &sel.idx}; }
};

// Euclidean cluster extraction (rgc_cluster_*, rgc_api_cluster.hip): a host caller's staged records; the int arrays of a call carved from ONE buffer
// (the union-find, the per-point and per-cluster tables, the radix sort's two pairs of arrays, a host caller's results); the radix histograms and
// the scans' block sums; the mirror holds the two counts and rgck::ClusterStats
struct ClusterRecord : FrameLists {
  rgc_cluster_info info{};
  DevBuf in, work, hist, bs;
  std::vector<DevBuf*> bufs() { return {&f.small, &in, &work, &hist, &bs}; }
};

// RANSAC plane segmentation (rgc_plane_*, rgc_api_plane.hip), no grid: a host caller's staged records and samples; a batch's non-finite word, models
// and counts (one contiguous read-back) with their pinned mirror of 32 KiB, which also holds the final rgck::PlaneFit and the number written; the
// fixed-order sums' rows; the fit; the selection
struct PlaneRecord : NoLists {
  rgc_plane_info info{};
  int batch = 0;  // rgc_plane_set_batch: 0 = automatic
  DevBuf in, samples, bat, rows, fit;
  Selection sel;
  unsigned char* h = nullptr;
  std::vector<DevBuf*> bufs() { return {&in, &samples, &bat, &rows, &fit, &sel.flag, &sel.off, &sel.bs, &sel.out, &sel.idx}; }
  std::vector<void*> pinned() { return {h}; }
};

// Surface normal estimation (rgc_normal_*, rgc_api_normals.hip): the surface cloud's grid; a host caller's staged queries and surface (12-byte
// records) and results; the mirror holds the queries' flag and rgck::NormalStats
struct NormalRecord : FrameLists {
  rgc_normal_info info{};
  DevBuf q, surf, n4, cov, cen, cnt;
  std::vector<DevBuf*> bufs() { return {&f.small, &q, &surf, &n4, &cov, &cen, &cnt}; }
};

// FPFH descriptors (rgc_fpfh_*, rgc_api_fpfh.hip): the surface cloud's grid; a host caller's staged queries, surface and normals (12-byte records);
// the normals as float4 with their validity in w; the marks of a separate surface, their scan, its block sums and the list of marked sorted
// positions; the SPFH counts and row sizes (scratch when the caller does not ask for them), a host caller's descriptors and counts; the mirror
// holds the queries' flag, the list's length and rgck::FpfhStats
struct FpfhRecord : FrameLists {
  rgc_fpfh_info info{};
  DevBuf q, surf, nrm, n4, flag, off, bs, list, spfh, m, out, cnt;
  std::vector<DevBuf*> bufs() { return {&f.small, &q, &surf, &nrm, &n4, &flag, &off, &bs, &list, &spfh, &m, &out, &cnt}; }
};

// ---- the mapping side and the stages around the registration, released like the records above.  PinnedBuf: a pinned host buffer that grows (ensure_pinned)
struct PinnedBuf { unsigned char* p = nullptr; size_t cap = 0; };

// f1, the mapping node's feature registration (rgc_mapreg_*, rgc_api_mapreg.hip): the corner / surf feature maps (grid only, kMapregCell), the four
// feature sets (0/1 corner/surf of the current pose, 2/3 of the last) with their factors (8 doubles each), the term kernels' per-block rows, and 16 ints:
// [0, 8) a measured grid's scratch, [8, 12) the factor counts.  small is BORROWED by rgc_icp_align for its target's grid (prepare_map_grid)
struct MapregRecord : NoLists {
  Cloud map[2];
  DevBuf feat[4], fac[4], partials, small;
  std::vector<DevBuf*> bufs() { return {&feat[0], &feat[1], &feat[2], &feat[3], &fac[0], &fac[1], &fac[2], &fac[3], &partials, &small}; }
  std::vector<Cloud*> clouds() { return {&map[0], &map[1]}; }
};

// f2, the rolling local map (rgc_map_*, rgc_api_map.hip).  World-frame points (relative to origin, x,y,z,intensity, 16 B) of the live keyframes as
// contiguous segments in insertion order in store[cur]; the other buffer is the compaction / re-basing target.  target: the committed, filtered map
struct RollingMapRecord : NoLists {
  struct MapKf { int id; size_t off; int n; double t[3]; };
  DevBuf store[2], target;
  int cur = 0, next_id = 0;
  size_t n = 0;
  std::vector<MapKf> kf;
  double origin[3] = {0, 0, 0};
  bool dirty = false;     // keyframes changed since the last commit
  bool bound = false;     // the context's target IS the committed map (rgc_set_target* unbinds it)
  float leaf = 0.f;       // of the last commit, which left ntarget points
  int ntarget = 0;
  unsigned long long rev = 0;
  std::vector<DevBuf*> bufs() { return {&store[0], &store[1], &target}; }
};

// f5, the mapping node's keyframe store (rgc_kf_*, rgc_api_keyframes.hip; the pose graph reads recs and index).  Body-frame points (x,y,z,c, 16 B) per
// kind in store[kind], a keyframe's clouds as one contiguous run each; the key poses (and the quaternions the reference's chain makes of them) stay on
// the host and travel with every assembly's segment table (table; h_table its pinned staging, rewritten or freed only after `uploaded`); raw / filt: the
// assembly when it is not written to the caller's buffer.  The selections: a device mirror of the key positions, float4 {x, y, z, position}, with the
// travelled distances and the ids beside it -- uploaded when rev has moved since mirror_rev -- and their scratch
struct KeyframeRecord : NoLists {
  struct KfRec { int id; size_t off[RGC_KF_KINDS]; int n[RGC_KF_KINDS]; rgc_kf_pose pose; double q[4];
                 float travel, travel_angle; };  // travelled distance / angle up to this keyframe, fixed at its push (src/RGC_mapping.cpp:1887-1908)
  DevBuf store[RGC_KF_KINDS];
  size_t n[RGC_KF_KINDS] = {0, 0, 0};
  std::vector<KfRec> recs;
  std::unordered_map<int, int> index;   // id -> position in recs
  unsigned long long rev = 0;
  DevBuf table, raw, filt;
  PinnedBuf h_table;
  hipEvent_t uploaded = nullptr;        // (created in rgc_create, destroyed in rgc_destroy)
  bool upload_pending = false;
  DevBuf pos, travel, ids, flag, scan, bsum, sel, sel_out, small;
  unsigned long long mirror_rev = ~0ull;   // the revision the mirror holds
  std::vector<DevBuf*> bufs() { return {&store[0], &store[1], &store[2], &table, &raw, &filt, &pos, &travel, &ids, &flag, &scan, &bsum, &sel, &sel_out, &small}; }
  std::vector<void*> pinned() { return {h_table.p}; }
};

// The 4-DoF pose graph over the store's key poses (rgc_pgo_*, rgc_api_pgo.hip): the graph's index tables, every double array of a solve (two
// evaluations: the accepted state and the candidate), the separators' dense system
struct PgoRecord : NoLists {
  DevBuf i, d, M;
  std::vector<DevBuf*> bufs() { return {&i, &d, &M}; }
};

// The leaf filter and the staging of B2 / B3 / B9 (rgc_voxelgrid*, rgc_uniform_sampling, stage_in: rgc_api_pre.hip).  in / out: a host caller's cloud
// on its way to the device and a result on its way back; the rows chain's arrays; us_index: the winners' indices of a host caller; aux: the chain's
// grid scratch; the leaf boxes of earlier clouds by leaf size; the one filter in flight between rgc_voxelgrid_begin and _end with its event and its
// three pinned result ints; the route of the last finished filter.  BORROWED for the length of a call: `in` by every entry point that stages a host
// cloud (stage_in) and by rgc_pc2_unpack; `out` by rgc_transform_cloud, rgc_pc2_* and rgc_icp_align (its moving source); `aux` by rgc_icp_align (its target)
struct LeafFilterRecord {
  struct VgBox { float leaf = 0.f; bool valid = false; rgck::LeafGrid g{}; };
  struct VgPending { bool active = false, ready = false; const float* d_in = nullptr; int n = 0, stride_bytes = 0; float leaf = 0.f; float* d_out = nullptr;
                     rgck::LeafGrid g{};  // the leaf grid the pending filter was enqueued on
                     int n_out = 0;
                     rgc_vg_route route{}; };  // what rgc_voxelgrid_route reports once the pending filter is ended
  DevBuf in, out, order, pos, tmp, leaf, us_index;
  Cloud aux;
  VgBox box[4];
  int box_next = 0;
  bool flags_clean = false;  // d_small->leaf.guard is known to be zero (a finished rows chain leaves it so)
  VgPending pend;
  rgc_vg_route route{};
  hipEvent_t done = nullptr;  // (created in rgc_create, destroyed in rgc_destroy)
  int* h_res = nullptr;
  std::vector<DevBuf*> bufs() { return {&in, &out, &order, &pos, &tmp, &leaf, &us_index}; }
  std::vector<void*> pinned() { return {h_res}; }
  std::vector<Cloud*> clouds() { return {&aux}; }
};

// The A1-A8 front end (rgc_frontend*, rgc_api_frontend.hip): a sweep's arrays, one buffer each (frontend_impl sizes them), the pinned staging of its small
// read-backs and feature clouds (a pageable copy is staged by the runtime anyway, one blocking hop per call), what the previous sweep leaves for the next
enum FeBuf { FE_RING, FE_RANK, FE_HIST, FE_META, FE_ST, FE_CL, FE_INUM2, FE_INUM, FE_RANGE, FE_ANGLE, FE_CURV, FE_CURV2, FE_ICURV, FE_DSRC, FE_OSRC, FE_PICK, FE_IPICK, FE_LAB, FE_ILAB, FE_GMARK, FE_MULT,
             FE_SCNT, FE_SPOS, FE_PART, FE_OUTD, FE_SLOTS, FE_FLAGS, FE_SHARP, FE_FLAT, FE_INTEN, FE_GLIST, FE_BSUM, FE_SORTC, FE_SORTI, kFeBufs };
struct FrontendRecord : NoLists {
  DevBuf buf[kFeBufs];
  PinnedBuf stage;
  bool spec_on = RGC_FE_SPEC != 0;  // (build flag) 0: read every sweep's size back before its stencil kernels
  int last_ns = 0, last_max_ring = 0;  // the previous sweep's scan lines and largest ring: sizes the next sweep's launches without a read-back
  int n_cloud = 0;                  // points of the last front-end's ring-major cloud (buf[FE_CL]), for rgc_frontend_cloud_device
  std::vector<DevBuf*> bufs() { std::vector<DevBuf*> v; for (DevBuf& b : buf) v.push_back(&b); return v; }
  std::vector<void*> pinned() { return {stage.p}; }
};

struct ProfRegion {
  hipEvent_t a, b;
  int kind;
  long long points;
};

}  // namespace rgcapi

using rgcapi::Cloud;
using rgcapi::DevBuf;
using rgcapi::kProfKinds;
using rgcapi::ProfRegion;

struct rgc_ctx {
  int device = 0;
  rgc_params prm{};
  hipStream_t stream = nullptr;   // main stream: target preprocessing, LM loop, fitness, getters
  hipStream_t stream2 = nullptr;  // source preprocessing runs here, concurrently with the (much larger) target's
  hipEvent_t src_ready = nullptr; // recorded on stream2 after the source is prepared
  hipEvent_t tgt_ready = nullptr; // recorded on the main stream at rgc_align_begin: the solve (on stream2) waits for the map's preparation
  hipEvent_t main_mark = nullptr; // recorded on the main stream before a source is prepared: stream2 waits for it (producers on rgc_stream())
  bool src_pending = false;       // main stream has not yet been ordered after src_ready
  bool mark_valid = false, main_has_target_prep = false;  // main_mark recorded; a map preparation was enqueued after it and may still run
  bool main_late_producer = false;  // ... and something that may WRITE a scan buffer (rgc_upload) was enqueued on the main stream behind it
  char err[512] = {0};
  Cloud src, tgt;
  // per-correspondence state frozen by linearize (fast_vgicp_impl.hpp:104-115)
  DevBuf corr_v, corr_M, partials, ipartials;
  DevBuf corr_v2, corr_M2;    // second correspondence buffer of the chained LM (speculative linearisation); corr_v / corr_M
                              // always name the VALID one after a solve
  int corr_noff = 0, corr_n = 0;
  bool corr_valid = false;
  // RGC_DIRECT_RADIUS (rgc_set_neighbor_search; prm.neighbor_method carries the method): the stored radius, its offset table (3 ints per offset, the
  // reference's order: neighbor_offsets_of) and the table on the device (one packed int per offset, rgck::vgicp_radius_pack), uploaded when it changed
  double nbr_radius = 0.0;
  std::vector<int> vr_offs_h, vr_packed_h;
  DevBuf vr_offs;
  bool vr_offs_dirty = true;
  // small device scratch + pinned host mirrors
  rgck::SmallWords* d_small = nullptr;  // the map's and the scan's blocks, ncorr, the leaf filter's block, the front-end's words
  double* d_out = nullptr;    // 28 doubles
  rgck::SmallWords* h_small = nullptr;  // pinned, same layout
  double* h_out = nullptr;    // pinned
  DevBuf scratch;             // getters
  DevBuf lm_state;            // the LM area (rgck::LmArea): the solve's two state images and the loose words behind them
  bool deferred_known = false;  // stats.deferred_* are those of the current clouds (carried home by the last align)
  DevBuf fit_partials;        // fitness rows when it is chained behind the LM slots
  rgck::LmState* h_lm = nullptr;  // pinned mirror (the stream-ordered copy behind every batch of LM launches)
  rgck::LmState* h_post = nullptr; // mapped host memory the DEVICE writes a finished solve's state into, then the solve's number into its `gen`
  rgck::LmState* d_post = nullptr; // ... its device address
  rgck::LmEarly* h_early = nullptr, *d_early = nullptr;  // mapped host memory / its device address: a solve's final pose, posted before its score (rgc_align_end_reframe)
  int lazy_margin = 0;             // rgc_set_target_lazy: > 0 = the target's covariances / voxels are built only where the solve can look (cells of margin)
  hipEvent_t src_in_ready = nullptr;  // recorded on stream2 behind a HOST scan's upload: the lazy target's footprint pass (main stream) reads the scan's input
  bool src_in_pending = false;
  int lm_seq = 0;                  // number of the pending solve (1, 2, ...)
  int lm_j = 0;                    // launches enqueued for it so far (rgck::lm_step's launch number: the state image alternates with it)
  rgck::LmState lm_res{};          // the finished solve's state as rgc_align_end took it (from h_post or h_lm): nothing writes it asynchronously
  hipEvent_t lm_mid = nullptr;     // recorded on the solve's stream behind its expected launches: the spare ones, on the context's other stream, wait for it
  hipEvent_t lm_tail = nullptr;    // recorded behind every batch of LM launches (and its copy into h_lm) on the stream they went to
  hipStream_t lm_tail_stream = nullptr;  // ... that stream: a solve enqueued on the OTHER stream waits for lm_tail first
  bool post_on = RGC_LM_POST != 0; // (build flag) 0: always wait for the stream and its copy, as in round 2
  struct { bool active = false; bool want_fitness = false; float guess[16]; rgck::LmInit in; int batch = 0; } pend;  // rgc_align_begin .. rgc_align_end (in, batch: what a chained solve of the same problem opens with)
  struct { bool on = false; int rc = 0; float T[16]; double H[36]; double fitness = 0; int iterations = 0, converged = 0, lm_failed = 0; bool has_fit = false; } gen_res;  // general route: rgc_align_begin solves at once, rgc_align_end hands this over
  int lm_last_outer = 0;      // outer iterations of the previous solve: sizes the next blind batch
  bool small_clean[2] = {false, false};  // d_small->map / d_small->scan holds its initial image (the last solve's first step restored it)
  hipStream_t solve_stream = nullptr;  // where the pending solve was enqueued (rgc_align_begin)
  bool solve_behind_map = RGC_SOLVE_BEHIND_MAP != 0;  // (build flag) 0: the solve always on the scan's (high-priority) stream, as in round 2
  bool lm_chained = false;    // RGC_LM_IMPL=chained: the solve as a chain of step launches (k_lm_step), never as one resident launch (k_lm_solve)
  int lm_give_up_at = -1;     // RGC_LM_GIVE_UP_AT=<try> (a test hook): the resident solve's workgroup 0 gives up at that try, without waiting
  int cu_count = 0;           // the device's compute units: the resident solve runs with at most one workgroup per CU
  bool lm_resident = false;   // the solve in flight went out as one resident launch
  int voxel_impl = 0;         // RGC_VOXEL_IMPL: 1 "separate", the voxel stage and the map's cooperative search always in launches of their own (k_voxel_build_coop,
                              // k_voxel_patch); 2 "fused", inside the dense map's kNN launch (rgck::KnnBulkOpts::fuse) wherever that launch runs; 0 (unset): fused on a
                              // context whose scans are held behind another context's target (src_held: a pipelined sequence), separate elsewhere
  bool src_held = false;      // the scan prepared last on this context was held by rgc_hold_source_until_target_of (src_hold_pending: the call came, the scan has not yet)
  bool src_hold_pending = false;
  bool lm_host = false;       // RGC_LM_IMPL=host: host-driven LM loop over the public fine-seam kernels (cross-check of the device-chained one)
  bool spec_on = true;        // RGC_SPEC_GRID=0 turns the speculative grid off
  bool coop_stream_on = RGC_COOP_STREAM != 0;  // (build flag; RGC_COOP_STREAM in the environment) the scan's deferred queries inside its bulk kNN launch
  bool prep_event_ext = RGC_PREP_EVENT_EXT != 0;  // (build flag; RGC_PREP_EVENT_EXT in the environment) the map's last launch signals tgt_prepared itself
  int join_spin_us = RGC_JOIN_SPIN_US;  // (build flag; RGC_JOIN_SPIN_US in the environment) how long the host waits for an almost-ready scan instead of putting a barrier into the map's stream (join_source)
  bool cache_on = RGC_KNN_CACHE != 0;  // (build flag; RGC_KNN_CACHE=0 in the environment) the neighbour lists of an unchanged map on top of the seeds
  bool seeds_on = RGC_KNN_SEEDS != 0;  // (build flag; RGC_KNN_SEEDS=0 in the environment) 0: every search of a re-framed map starts without a bound, as before round 5
  int reg_method = RGC_REG_PLANE, voxel_mode = RGC_VOXEL_ADDITIVE;  // as selected by the caller, implemented or not (rgc_set_regularization_method)
  // rgc_set_covariance_estimation / rgc_set_rbf_kernel: RGC_COV_RBF takes a point's covariance from the Gaussian-weighted moment of its ball
  // (rgc_rbf.hip) on the general route; the kernel as the caller gave it, max_dist already resolved (<= 0 -> 5 kernel_width)
  int cov_method = RGC_COV_KNN;
  double rbf_width = 0.5, rbf_max_dist = 3.0;  // fast_vgicp_cuda_impl.hpp:31
  bool test_fail_cache_alloc = false;  // RGC_TEST_FAIL_CACHE_ALLOC in the environment (rgc_create)
  bool force_general = false;          // RGC_FORCE_GENERAL=1 in the environment (rgc_create): PLANE / ADDITIVE on the general route too (a test's cross-check of the two routes)
  bool cache_dropped = false;          // the lists' buffers did not fit on the device: the context went down to the seeds by itself (rgc_get_knn_reuse)
  bool check_ptrs = false;             // RGC_CHECK_POINTERS in the environment (rgc_create): every pointer a caller calls "device" is looked up before it is used (check_device_range)
  bool trace_cache = false;            // RGC_TRACE_CACHE in the environment (rgc_create): rgc_get_stats reports the lists' state on stderr
  double src_res = RGC_SRC_RES;  // (build flag) fixed cell size of the SCAN's kNN grid (only the map's grid must be the voxel grid); 0 = adaptive
  int map_wide_r = RGC_MAP_WIDE_R;          // (build flag; 0 = off, 2) block radius of the bulk kNN launch for a sparse map
  double map_wide_density = RGC_MAP_WIDE;   // (build flag) ... when the map has fewer points per grid cell than this
  double src_res_auto = 0.0;  // adaptive cell size of the scan's kNN grid, steered by how crowded its cells were in the previous frame (0 = voxel_res)
  // Bounding boxes the library knows WITHOUT measuring: rgc_set_target_reframed maps the input's box (measured once per input buffer)
  // through the transform it applies -- the box of a sub-map re-framed by a new pose (RGC_odometer.cpp:1248-1256) follows from the
  // pose.  The target's preparation takes its grid from the hint: no bounding-box kernel, no host round trip, and no speculative-grid
  // miss when the re-framed map's box swings with the vehicle's yaw.  k_count's guard still checks it.
  struct BoxHint { const void* p = nullptr; int n = 0; double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; double reach_xy = 0, reach_z = 0; } box_hint[4];
  int box_hint_next = 0;
  unsigned long long tgt_generation = 0;   // bumped whenever this context prepares a target (what borrowers check)
  const rgc_ctx* tgt_owner = nullptr;      // rgc_share_target: whose target this context aliases, and at which generation
  unsigned long long tgt_owner_gen = 0, tgt_owner_uid = 0;
  unsigned long long uid = 0;              // process-wide, never re-used
  hipEvent_t tgt_prepared = nullptr;       // recorded on the main stream behind every target preparation (rgc_hold_source_until_target_of of another context waits for it)
  hipEvent_t src_read_done = nullptr;      // recorded on the main stream behind a kernel that reads the source's INPUT buffer (rgc_get_aligned*)
  bool src_read_pending = false;           // ... and not yet waited for by the stream a host source is copied on
  // The mapping side and the stages around the registration, each in a record of its own (rgcapi::MapregRecord and the five below it)
  rgcapi::MapregRecord mapreg;
  rgcapi::RollingMapRecord map;
  rgcapi::KeyframeRecord kfs;
  rgcapi::PgoRecord pgo;
  rgcapi::LeafFilterRecord vg;
  rgcapi::FrontendRecord fe;
  // The registration methods beside VGICP, each in a record of its own (rgcapi::NdtRecord and the three below it): NDT on two clouds of its own, the three GICP variants on the
  // context's source and target.  gicp_sums is the fixed-order sums' scratch of FastGICP and FastGICPSingleThread, which never run at the same time.
  rgcapi::NdtRecord ndt;
  rgcapi::Sums gicp_sums;
  rgcapi::GicpRecord gicp;
  rgcapi::GicpStRecord gicp_st;
  rgcapi::GicpMpRecord gicp_mp;
  // The cloud operations, each in a record of its own (rgcapi::SearchRecord and the five below it)
  rgcapi::SearchRecord search;
  rgcapi::OutlierRecord outlier;
  rgcapi::ClusterRecord cluster;
  rgcapi::PlaneRecord plane;
  rgcapi::NormalRecord normal;
  rgcapi::FpfhRecord fpfh;
  rgc_stats stats{};
  // profiling
  bool prof_on = false;
  unsigned prof_mask = ~0u;
  std::vector<ProfRegion> prof_open;
  std::vector<hipEvent_t> ev_pool;
  long long prof_launches[kProfKinds] = {0};
  double prof_ms[kProfKinds] = {0};
  long long prof_points[kProfKinds] = {0};
};

namespace rgcapi {

// What invalidates a frozen linearisation, in one place: VGICP's correspondences and the state of every method on the context's own clouds.  They
// fall together wherever a cloud is set, cleared, swapped, shared, given covariances or prepared again (NDT has clouds of its own: ndt_drop_terms)
inline void drop_frozen(rgc_ctx* c) { c->corr_valid = c->gicp.valid = c->gicp_st.valid = c->gicp_mp.valid = false; }

#define HIPCHK(c, expr)                                                                                    \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) {                                                                                \
      (void)hipGetLastError(); /* the runtime keeps a failed call's error until it is read: reported HERE, it must not surface again   \
                                  from the hipGetLastError() of the next, unrelated call (tests/fuzz/fuzz_bad_args.py) */             \
      return rgcapi::fail((c), RGC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);               \
    }                                                                                                      \
  } while (0)

// ---- rgc_api.hip: errors, buffers, the clouds' preparation, the registration core ----
int fail(rgc_ctx* c, int code, const char* fmt, ...);
int ensure(rgc_ctx* c, DevBuf& b, size_t bytes);
int ensure_pinned(rgc_ctx* c, PinnedBuf& b, size_t need, size_t grow_to);  // what b held is dropped; it grows to grow_to (>= need: each caller's own amount)
// room for `points` 16-byte points in a store that holds `held` (the rolling map's, the keyframe store's): half again, 1 MiB at least; preserve: they move along
int grow_store(rgc_ctx* c, DevBuf& b, size_t held, size_t points, bool preserve);
int check_device_range(rgc_ctx* c, const void* p, size_t bytes, const char* what);
bool ctx_alive(const rgc_ctx* c);
const rgc_ctx::BoxHint* find_hint(const rgc_ctx* c, const void* p, int n);
void put_hint(rgc_ctx* c, const void* p, int n, const double lo[3], const double hi[3], double reach_xy = 0, double reach_z = 0);
void hint_from_leaf_grid(rgc_ctx* c, const float* out /* device, or the caller's host buffer */, int n_out, const rgck::LeafGrid& g, float leaf);
bool map_prep_finished(rgc_ctx* c);
// rf (nullable, device clouds only): xyz has not been written yet -- the preparation produces it from rf (rgc_set_target_reframed)
int set_cloud(rgc_ctx* c, Cloud& cl, bool is_target, const float* xyz, int n, int stride_bytes, bool on_device, const rgck::Reframe* rf = nullptr);
// The grid of a cloud that is no VGICP target (a feature map, the ICP target, an NDT voxel map): its bounding box measured (one round
// trip), the points counting-sorted into that box's cells of size `cell`.  dsm / hsm: eight scratch ints on the device / the host;
// with_voxels: cell_voxel[] too, and the voxel count in dsm[7] (not read back here); name / grid_name: the cloud in the two error messages
int build_measured_grid(rgc_ctx* c, Cloud& cl, double cell, int* dsm, int* hsm, bool with_voxels, const char* name, const char* grid_name);
rgck::Pose pose_from(const double T[16]);
rgck::PoseF posef_from(const float T[16]);
int check_target_owner(rgc_ctx* c);
int need_inputs(rgc_ctx* c, bool validate = true);
int do_fitness(rgc_ctx* c, const float T[16], double* out);
// the 28 sums a linearisation folds to (21 of H's upper triangle by rows, 6 of b, the cost) -> the full symmetric H and b
void unpack_system(const double sums[28], double H[36], double b[6]);

// between rgc_align_begin and rgc_align_end -- on the general route too, where the solve has already run and its result waits to be handed over:
// the same calls are refused on both routes
inline bool solve_in_flight(const rgc_ctx* c) { return c->pend.active || c->gen_res.on; }
// the fewest points a cloud may have: k for the k nearest neighbours, one under RBF (a point is a member of its own ball)
inline int min_cloud_points(const rgc_ctx* c) { return c->cov_method == RGC_COV_RBF ? 1 : c->prm.k_correspondences; }
// what every entry point that takes a strided cloud accepts: x, y, z as floats at the head of each record
inline bool stride_ok(int stride_bytes) { return stride_bytes >= 12 && !(stride_bytes & 3) && stride_bytes <= 4096; }
// ... and where the fourth float is read too (x, y, z, intensity or class)
inline bool stride4_ok(int stride_bytes) { return stride_bytes >= 16 && stride_ok(stride_bytes); }
// the rotation and translation rows of a row-major 4x4 (or 3x4) pose
template <class T>
inline bool pose12_finite(const T* m) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(m[i])) return false;
  return true;
}

// ---- rgc_api_pre.hip ----
int stage_in(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, const float** d_in);
// rgc_voxelgrid after its argument checks (nothing runs for n == 0, or behind a refusal rc the caller already has), its route recorded for rgc_voxelgrid_route
int voxelgrid_routed(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, float leaf, float* out_xyzi, int* n_out, int on_device,
                     int mode = rgck::kVgModeCentroid, int* out_index = nullptr, int rc = RGC_OK);  // mode = rgck::kVgModePick: UniformSampling, out_index (nullable) as out_xyzi
// rgc_api_mapreg.hip.  A caller's strided cloud, host or device, as a grid-only cloud: a device caller's pointer is looked up (what_device names it in the refusal),
// a host caller's records are uploaded into cl.in_copy, both through x, y, z of the last record; then cl's measured grid at `cell` (the feature maps, the ICP target)
int grid_strided_cloud(rgc_ctx* c, Cloud& cl, const float* p, int n, int stride_bytes, bool on_device, double cell, const char* what_device);

// ---- rgc_api_search.hip: the call frame of the cloud operations (the records above) ----
// the frame's device words and their pinned mirror (kFrameBytes each), allocated once
int frame_open(rgc_ctx* c, OpFrame& f);
// The frame's cloud pointed at d for the length of the call and its measured grid built, as the search index's (build_search_grid: RGC_ERR_NONFINITE before
// anything is indexed; the frame's cell knob > 0 is the cell size, RGC_ERR_GRID_TOO_LARGE beyond max_cells; 0 selects it by the rule include/rgc_hip.h
// states for rgc_search_set_cloud).  who: the entry point, name / grid_name: the cloud, in the error messages.  The caller's pointer is not kept,
// whatever happens.  *cell: the cell size used; f.cl.grid and f.cl.sorted() are the call's to read afterwards
int index_cloud(rgc_ctx* c, OpFrame& f, const float* d, int stride_f, int n, const char* who, const char* name, const char* grid_name, double* cell);
// a cloud on the device: the caller's pointer, or a host caller's records packed to 12 bytes in `stage`
int stage_cloud(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, DevBuf& stage, const char* what, const float** d, int* stride_f);
// What is read of n whole records: through x, y, z of the last one, and through its fourth float too when records are written out from records that
// have one (`fourth`).  stage_records: the caller's device pointer, or a host caller's records up to there in `stage`; the stride stays the caller's
inline size_t record_bytes(int n, int stride_bytes, bool fourth) { return (size_t)n * stride_bytes - (stride_bytes - (fourth && stride_bytes >= 16 ? 16 : 12)); }
int stage_records(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, bool fourth, DevBuf& stage, const char* what, const float** d);
// Where an output goes on the device: the caller's buffer, or scratch for a host caller; nullptr when it is not asked for -- unless the call
// `need`s it as scratch anyway (the filters' per-point value, FPFH's first pass)
template <class T>
int place_output(rgc_ctx* c, T* user, size_t bytes, int on_device, DevBuf& scratch, const char* what, T** d, bool need = false) {
  *d = nullptr;
  if (!user && !need) return RGC_OK;
  int rc;
  if (user && on_device) {
    if ((rc = check_device_range(c, user, bytes, what))) return rc;
    *d = user;
    return RGC_OK;
  }
  if ((rc = ensure(c, scratch, bytes))) return rc;
  *d = scratch.as<T>();
  return RGC_OK;
}
// a result on its way to the caller, behind the call's launches: a download, or a copy on the device for a device caller (dst nullable)
int copy_out(rgc_ctx* c, void* dst, const void* src, size_t bytes, int on_device);
// offsets[0] = 0 (nullable): all a call without points writes
int write_empty_offsets(rgc_ctx* c, int* offsets, int on_device);
// the selection's int arrays for n points: the flags, their scan, its block sums (out / idx are placed by the caller: place_output)
int selection_scratch(rgc_ctx* c, Selection& sel, int n);
// The tail that turns sel.flag into records: the scan, the records and indices (outlier_emit), then ONE read-back -- the call's own read-out
// (home.h <- home.d, nullable) and the number kept (*home.h_kept, pinned) -- and the wait.  A host caller's kept rows are enqueued behind it: the
// caller waits for them, behind whatever else it downloads
struct EmitTo {  // where the records and indices go (each pair nullable together): on the device, and a host caller's own arrays
  float* d_out;
  int* d_index;
  float* out_xyzc;
  int* out_index;
};
struct EmitHome {  // what comes home behind the chain
  void* h;
  const void* d;
  size_t bytes;
  int* h_kept;
};
int emit_selected(rgc_ctx* c, Selection& sel, const float* d_in, int stride_f, int n, int on_device, const EmitTo& to, const EmitHome& home);
// what the four rgc_*_set_cell share
int set_cell_of(rgc_ctx* c, double* knob, double cell, const char* who);
// the read-out words' slots folded: word k's sum, or its maximum
inline unsigned long long sum_words(const rgck::StatWords& w, int k) {
  unsigned long long a = 0;
  for (int j = 0; j < rgck::kStatSlots; j++) a += w[j][k];
  return a;
}
inline unsigned long long max_words(const rgck::StatWords& w, int k) {
  unsigned long long a = 0;
  for (int j = 0; j < rgck::kStatSlots; j++) a = w[j][k] > a ? w[j][k] : a;
  return a;
}

// ---- rgc_api_lsq.hip: the LM driver of every registration method ----
// A registration problem as the driver sees it.  Either linearize + error (the driver makes the first try of an outer iteration itself, on
// the host), or linearize_try + error: the linearisation at x0 AND that first try in one call (rgc_align: one enqueue, the try on the
// device; lambda < 0 on entry = not initialised yet, *lambda_used = the one the try used).
struct LmSystem {
  int (*linearize)(rgc_ctx* c, const double T[16], double* H, double* b, double* cost);
  int (*error)(rgc_ctx* c, const double T[16], double* cost);
  int (*linearize_try)(rgc_ctx* c, const double x0[16], double lambda, double H[36], double b[6], double* y0, double d[6], double xi[16],
                       double* lambda_used, double* yi);
  bool (*may_linearize)(const double x0[16]);  // nullable; false: nothing can be linearised at this pose -- the solve ends as failed
};
struct LmResult {
  double x0[16], Hfin[36];  // the final pose and final_hessian_
  float fin[16];            // ... the pose as the caller gets it (lsq_registration_impl.hpp:77)
  int iters;                // outer iterations started
  bool conv, failed;
  void open(const float guess[16]) {  // x0 = the guess, final_hessian_.setIdentity() (lsq_registration_impl.hpp:21), nothing decided yet
    for (int i = 0; i < 12; i++) x0[i] = (double)guess[i];
    x0[12] = x0[13] = x0[14] = 0.0;
    x0[15] = 1.0;
    memset(Hfin, 0, sizeof(Hfin));
    for (int i = 0; i < 6; i++) Hfin[i * 7] = 1.0;
    conv = failed = false;
    iters = 0;
  }
  void write(float final_T[16], double final_H[36], int* iterations, int* converged, int* lm_failed) const {  // (each nullable)
    if (final_T) memcpy(final_T, fin, sizeof(fin));
    if (final_H) memcpy(final_H, Hfin, sizeof(Hfin));
    if (iterations) *iterations = iters;
    if (converged) *converged = conv ? 1 : 0;
    if (lm_failed) *lm_failed = failed ? 1 : 0;
  }
};
// computeTransformation from `guess` under c->prm's limits; an error of a system call ends it with that code (r is not complete then)
int lm_solve(rgc_ctx* c, const LmSystem& sys, const float guess[16], LmResult* r);
// the k folded sums of a method (s.out, behind its launches on the context's stream) in s.h_out, the launches checked; read_system: those of a
// linearisation (k >= 28) -- H and b out of them when both are wanted, and the cost (each nullable)
int read_sums(rgc_ctx* c, const Sums& s, int k);
int read_system(rgc_ctx* c, const Sums& s, int k, double* H, double* b, double* cost);
// The offsets of a fast_gicp::NeighborSearchMethod (0 DIRECT27, 1 DIRECT7, 2 DIRECT1, 3 DIRECT_RADIUS: include/fast_gicp/gicp/gicp_settings.hpp:8) in
// the reference's order, 3 ints per offset -- the ONE generator of NDT's list (src/fast_gicp/cuda/ndt_cuda.cu:35-88) and VGICP's
// (src/fast_gicp/cuda/fast_vgicp_cuda.cu:42-95), which are the same lists.  cap: the most offsets a caller takes (kMaxNeighborOffsets for a list
// a kernel is to walk); false: the radius has more (o is incomplete then).  The radius is read under method 3 only and must be finite and >= 0.
constexpr int kMaxNeighborOffsets = RGC_NDT_MAX_OFFSETS;  // the cap of both lists, under its one name
bool neighbor_offsets_of(int method, double radius, std::vector<int>& o, int cap = kMaxNeighborOffsets);

}  // namespace rgcapi
