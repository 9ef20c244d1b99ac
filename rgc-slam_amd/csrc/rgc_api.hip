// rgc_api.hip -- host side of librgc_hip.so, the core: context, device buffers, the clouds' preparation, the VGICP registration
// (rgc_align*, rgc_linearize, ...), its getters and setters, statistics and profiling.  The per-point work is in rgc_kernels.hip (the
// linearisation under RGC_DIRECT_RADIUS: rgc_vgicp_radius.hip).  The
// rest of the C-ABI of include/rgc_hip.h is in one rgc_api_*.hip per subsystem (the table in DESIGN.md), among them rgc_api_lsq.hip
// (the LM driver of lsq_registration_impl.hpp:53-172 that rgc_align's host route shares with NDT and FastGICP); rgc_ctx.h is what they share.
//
// No CPU fallback exists: every entry point fails with RGC_ERR_HIP when the HIP runtime / device is missing.
// Reference citations are relative to /root/reference/rgc_slam/.
#include "rgc_ctx.h"

// Contexts alive in this process: a context that borrows another one's target (rgc_share_target) checks its owner here before every
// solve, so that an owner destroyed too early is an error message and not a read of freed memory.
static std::mutex g_live_mutex;
static std::unordered_set<const rgc_ctx*> g_live;
static std::atomic<unsigned long long> g_next_uid{1};  // contexts are told apart by this, not by their address (an address is re-used)

namespace rgcapi {

constexpr int kMaxK = 32;
// Events that only order streams of ONE device against each other: no timing, and a device-scope release when recorded (the default is a
// system-scope one -- the L2s written back so that the HOST may read what came before; nobody's host does behind these).
constexpr unsigned kDevEvent = hipEventDisableTiming | hipEventReleaseToDevice;

bool ctx_alive(const rgc_ctx* c) {
  std::lock_guard<std::mutex> lk(g_live_mutex);
  return g_live.count(c) != 0;
}

int fail(rgc_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

// The odometer's settings (PLANE, ADDITIVE: fast_gicp_impl.hpp:20, fast_vgicp_impl.hpp:24) run on the tuned kernels, which keep a point's
// covariance as the unit normal of I - 0.999 n n^T.  Every other RegularizationMethod, and VoxelAccumulationMode::MULTIPLICATIVE, runs on
// the GENERAL route: every point through the cooperative search with a regularised 3x3 per point (rgck::knn_cov6), a plain voxel pass, and
// the host-driven LM loop over a linearisation that takes the full source covariance.  Unoptimised; the same entry points, the same results
// as the reference's arithmetic for those settings (fast_gicp_impl.hpp:262-293, fast_vgicp_voxel.hpp:76-99).
// RBF covariance estimation (rgc_set_covariance_estimation) hands out a 3x3 per point too, whatever the regularisation.
static bool general_route(const rgc_ctx* c) {
  return c->force_general || c->reg_method != RGC_REG_PLANE || c->voxel_mode == RGC_VOXEL_MULTIPLICATIVE || c->cov_method == RGC_COV_RBF;
}

static bool trace_alloc() { static const bool on = getenv("RGC_TRACE_ALLOC") != nullptr; return on; }  // developer aid: which buffer grew, and when
int ensure(rgc_ctx* c, DevBuf& b, size_t bytes) {
  if (b.borrowed) { b.p = nullptr; b.cap = 0; b.borrowed = false; }  // an alias is dropped, never resized: this context gets its own buffer
  if (bytes <= b.cap && b.p) return RGC_OK;
  if (b.p) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  // head-room: clouds of similar size arrive every frame, and a re-allocation costs a device synchronisation plus hipFree /
  // hipMalloc (hundreds of microseconds: 10 % of the first 20 frames of a sequence when buffers crept up by 1/8 at a time).
  // HBM is not the scarce resource here: half again for anything below 256 MB, an eighth above.
  size_t want = bytes + (bytes < ((size_t)256 << 20) ? bytes / 2 : bytes / 8) + 256;
  HIPCHK(c, hipMalloc(&b.p, want));
  b.cap = want;
  if (trace_alloc()) fprintf(stderr, "[rgc] buffer at ctx+%ld grew to %zu bytes (asked %zu)\n", (long)((char*)&b - (char*)c), want, bytes);
  return RGC_OK;
}

int ensure_pinned(rgc_ctx* c, PinnedBuf& b, size_t need, size_t grow_to) {
  if (need <= b.cap) return RGC_OK;
  if (b.p) { HIPCHK(c, hipHostFree(b.p)); b.p = nullptr; b.cap = 0; }
  HIPCHK(c, hipHostMalloc((void**)&b.p, grow_to, hipHostMallocDefault));
  b.cap = grow_to;
  return RGC_OK;
}

int grow_store(rgc_ctx* c, DevBuf& b, size_t held, size_t points, bool preserve) {
  const size_t bytes = points * 16;
  if (bytes <= b.cap && b.p) return RGC_OK;
  void* np = nullptr;
  const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
  HIPCHK(c, hipMalloc(&np, want));
  if (b.p) {
    if (preserve && held) HIPCHK(c, hipMemcpyAsync(np, b.p, held * 16, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(b.p));
  }
  b.p = np;
  b.cap = want;
  return RGC_OK;
}

// An integrator's aid (RGC_CHECK_POINTERS=1; off by default: a look-up per pointer per call, microseconds on a frame's critical path): is what
// the caller calls a device buffer one -- device memory of THIS context's device, with room for `bytes` behind p?  A host pointer handed to
// a *_device entry, a buffer of another GPU, a count larger than the allocation: RGC_ERR_INVALID instead of a memory fault on the device.
int check_device_range(rgc_ctx* c, const void* p, size_t bytes, const char* what) {
  if (!c->check_ptrs || !p) return RGC_OK;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, RGC_ERR_INVALID, "%s: %p is not memory the HIP runtime knows (a host pointer passed as a device pointer?)", what, p);
  }
  if (at.type != hipMemoryTypeDevice) return fail(c, RGC_ERR_INVALID, "%s: %p is not device memory", what, p);
  if (at.device != c->device) return fail(c, RGC_ERR_INVALID, "%s: %p lives on device %d, the context on device %d", what, p, at.device, c->device);
  void* base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return RGC_OK; }
  const size_t off = (size_t)((const char*)p - (const char*)base);
  if (off + bytes > size) return fail(c, RGC_ERR_INVALID, "%s: %zu bytes asked of an allocation that has %zu behind %p", what, bytes, size - off, p);
  return RGC_OK;
}

static void release(DevBuf& b) {
  if (b.p && !b.borrowed) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  b.borrowed = false;
}

// the buffers of a target that a borrower aliases (rgc_share_target)
static std::vector<DevBuf*> shared_bufs(Cloud& cl) {
  return {&cl.in_copy, &cl.cell_of, &cl.slot_of, &cl.cnt, &cl.start, &cl.block_sums, &cl.order_tmp, &cl.P, &cl.nx, &cl.ny, &cl.nz, &cl.segs,
          &cl.cell_voxel, &cl.vox, &cl.vox_cell, &cl.c6};
}
static void release_cloud(Cloud& cl) {
  for (DevBuf* b : shared_bufs(cl)) release(*b);
  for (DevBuf* b : {&cl.need, &cl.qlist, &cl.cell_list, &cl.seed, &cl.nbr, &cl.rank_of, &cl.pos_of, &cl.qrank, &cl.map_copy, &cl.todo, &cl.cache_small}) release(*b);
}
// a record of a subsystem (rgc_ctx.h): its device buffers, its pinned mirrors, its clouds
template <class Record>
static void release_record(Record& r) {
  for (DevBuf* b : r.bufs()) release(*b);
  for (void* p : r.pinned())
    if (p) (void)hipHostFree(p);
  for (Cloud* cl : r.clouds()) release_cloud(*cl);
}

// ---- profiling regions (HIP events on the context's stream) ----
static bool profiled(const rgc_ctx* c, int kind) { return c->prof_on && ((c->prof_mask >> kind) & 1u); }  // the profile is on and wants this kind of region
namespace {
struct ProfScope {
  rgc_ctx* c;
  bool on, records;  // records == false: the region's one launch fills r.a / r.b with its own start / stop times (hipExtLaunchKernelGGL)
  ProfRegion r{};
  hipStream_t st;
  ProfScope(rgc_ctx* ctx, int kind, long long points, hipStream_t stream = nullptr, bool records_ = true)
      : c(ctx), on(profiled(ctx, kind)), records(records_), st(stream ? stream : ctx->stream) {
    if (!on) return;
    auto get = [&](hipEvent_t* e) {
      if (!c->ev_pool.empty()) { *e = c->ev_pool.back(); c->ev_pool.pop_back(); return true; }
      return hipEventCreate(e) == hipSuccess;
    };
    if (!get(&r.a)) { on = false; return; }
    if (!get(&r.b)) { c->ev_pool.push_back(r.a); on = false; return; }
    r.kind = kind;
    r.points = points;
    if (records) (void)hipEventRecord(r.a, st);
  }
  ~ProfScope() {
    if (!on) return;
    if (records) (void)hipEventRecord(r.b, st);
    c->prof_open.push_back(r);
  }
};
}  // namespace

static void prof_collect(rgc_ctx* c) {
  for (auto& r : c->prof_open) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      c->prof_launches[r.kind]++;
      c->prof_ms[r.kind] += (double)ms;
      c->prof_points[r.kind] += r.points;
    }
    c->ev_pool.push_back(r.a);
    c->ev_pool.push_back(r.b);
  }
  c->prof_open.clear();
}

// RGC_DIRECT_RADIUS: the context's offset table (made from the stored radius where no rgc_set_neighbor_search has made it yet: a radius that was
// stored has passed that call's checks, and the initial 0.0 is the own cell alone)
static bool radius_method(const rgc_ctx* c) { return c->prm.neighbor_method == RGC_DIRECT_RADIUS; }
static const std::vector<int>& radius_table(rgc_ctx* c) {
  if (c->vr_offs_h.empty()) { neighbor_offsets_of(RGC_DIRECT_RADIUS, c->nbr_radius, c->vr_offs_h); c->vr_offs_dirty = true; }
  return c->vr_offs_h;
}
static int noff_of(rgc_ctx* c) {
  const int method = c->prm.neighbor_method;
  if (method == RGC_DIRECT_RADIUS) return (int)radius_table(c).size() / 3;
  return method == RGC_DIRECT1 ? 1 : (method == RGC_DIRECT7 ? 7 : 27);
}

static int check_params(rgc_ctx* c, const rgc_params* p) {
  if (!(p->voxel_res > 0.0) || !std::isfinite(p->voxel_res)) return fail(c, RGC_ERR_INVALID, "voxel_res must be > 0");
  if (p->k_correspondences < 2 || p->k_correspondences > kMaxK) return fail(c, RGC_ERR_INVALID, "k_correspondences must be in [2,%d]", kMaxK);
  if (p->neighbor_method < RGC_DIRECT27 || p->neighbor_method > RGC_DIRECT_RADIUS) return fail(c, RGC_ERR_INVALID, "bad neighbor_method");
  // RGC_DIRECT_RADIUS needs a radius, which this block does not carry: it is SELECTED by rgc_set_neighbor_search alone.  While it is the
  // selection a block that names it is taken (what rgc_get_params handed out comes back: get / modify / set keeps it, with the stored radius)
  if (p->neighbor_method == RGC_DIRECT_RADIUS && c->prm.neighbor_method != RGC_DIRECT_RADIUS)
    return fail(c, RGC_ERR_INVALID, "RGC_DIRECT_RADIUS is selected with rgc_set_neighbor_search (it takes the radius)");
  if (p->max_iterations < 0 || p->lm_max_iterations < 1) return fail(c, RGC_ERR_INVALID, "bad iteration limits");
  if (!(p->rotation_eps > 0) || !(p->translation_eps > 0)) return fail(c, RGC_ERR_INVALID, "epsilons must be > 0");
  if (p->max_cells < 1) return fail(c, RGC_ERR_INVALID, "max_cells must be >= 1");
  return RGC_OK;
}

const rgc_ctx::BoxHint* find_hint(const rgc_ctx* c, const void* p, int n) {
  for (const auto& h : c->box_hint)
    if (h.p == p && h.n == n && p) return &h;
  return nullptr;
}
void put_hint(rgc_ctx* c, const void* p, int n, const double lo[3], const double hi[3], double reach_xy, double reach_z) {
  rgc_ctx::BoxHint* h = nullptr;
  for (auto& e : c->box_hint)
    if (e.p == p) h = &e;  // a buffer has one box
  if (!h) { h = &c->box_hint[c->box_hint_next]; c->box_hint_next = (c->box_hint_next + 1) % 4; }
  h->p = p; h->n = n;
  h->reach_xy = reach_xy; h->reach_z = reach_z;
  for (int a = 0; a < 3; a++) { h->lo[a] = lo[a]; h->hi[a] = hi[a]; }
}
static void drop_hints(rgc_ctx* c) {
  for (auto& e : c->box_hint) e.p = nullptr;
}
// The leaf filter's output lies inside the leaf grid it was sorted on (a leaf's centroid lies in the leaf): a box the library knows without
// measuring.  rgc_set_target_device on that buffer takes its grid from it -- the node's sub-map (three keyframes through the 0.3 m filter)
// changes its bounding box with every keyframe, and a target that left the previous target's widened grid cost a second preparation and a
// second solve (the node's 1.4 ms frames among 0.63 ms ones).
void hint_from_leaf_grid(rgc_ctx* c, const float* out /* device, or the caller's host buffer */, int n_out, const rgck::LeafGrid& g, float leaf) {
  if (!c->spec_on || n_out <= 0) return;
  double lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = (double)g.minb[a] * (double)leaf - 1.0e-3;
    hi[a] = ((double)g.minb[a] + (double)g.div[a]) * (double)leaf + 1.0e-3;
  }
  put_hint(c, out, n_out, lo, hi);
}

// Has the map preparation enqueued last on the main stream finished?  Asked of the event recorded behind it -- NOT of the stream:
// hipStreamQuery on a stream whose last command is a kernel puts a marker packet with a completion signal behind it (a system-scope
// release in front of whatever is enqueued next: ~10 us between the map's last kernel and the solve's first step, every frame).
bool map_prep_finished(rgc_ctx* c) {
  const hipError_t q = hipEventQuery(c->tgt_prepared);
  if (q != hipSuccess) (void)hipGetLastError();  // ("not ready" is an answer, not an error to be found by a later check)
  return q == hipSuccess;
}

static int cloud_covariances(rgc_ctx* c, Cloud& cl, bool is_target);
// a sparse map (points per cell of its grid below map_wide_density) takes the wider block of the bulk kNN launch, see k_knn_sp_wide
static int map_wide_r_of(const rgc_ctx* c, const Cloud& cl) {
  return (c->map_wide_r > 0 && (double)cl.n < c->map_wide_density * (double)cl.grid.ncell) ? c->map_wide_r : 0;
}
static rgck::KnnSeeds cloud_seeds(const Cloud& cl, bool is_target);

// ---- one place per rule ----
// the guard of a cloud's grid (its block of the context's small scratch, rgck::SmallWords::block) as the cloud's kernels take it: while the
// cloud sits on a speculative (or hinted) grid whose guard has not been read yet
static int* guard_of(rgc_ctx* c, const Cloud& cl, bool is_target) { return cl.spec_used ? &c->d_small->block(is_target)->guard : nullptr; }
// Launch sizes from the deferred count of the previous cloud prepared here (consecutive clouds of a sequence defer about the same queries;
// n / 64 for the first one): the waves of a cooperative search, and the waves that patch the voxels of the deferred queries
static int coop_waves_est(const Cloud& cl) { return cl.deferred_seen >= 0 ? cl.deferred_seen + cl.deferred_seen / 4 + 32 : cl.n / 64 + 32; }
static int patch_waves_est(const Cloud& cl) { return cl.deferred_seen >= 0 ? 2 * cl.deferred_seen + 64 : cl.n; }
// the voxel records of a map of cl.n points on a grid of ncell cells: at most one voxel per point and per cell
static int ensure_voxel_table(rgc_ctx* c, Cloud& cl, int ncell) {
  const size_t vmax = (size_t)(cl.n < ncell ? cl.n : ncell);
  int rc;
  if ((rc = ensure(c, cl.vox, sizeof(double) * rgck::kVoxRec * vmax))) return rc;
  return ensure(c, cl.vox_cell, sizeof(int) * vmax);
}
// what a linearisation of n source points freezes and folds: corr_v / corr_M for noff offsets, row_doubles per workgroup in partials
static int ensure_corr(rgc_ctx* c, int n, int noff, size_t row_doubles) {
  // (RGC_DIRECT_RADIUS: a workgroup of its linearisation takes fewer points -- more rows than k_error's, which folds into the same buffer)
  const size_t nb = (size_t)std::max(rgck::linearize_blocks(n), radius_method(c) ? rgck::vgicp_radius_blocks(n) : 0);
  int rc;
  if ((rc = ensure(c, c->corr_v, sizeof(int) * (size_t)n * noff))) return rc;
  if ((rc = ensure(c, c->corr_M, sizeof(double) * 6 * (size_t)n * noff))) return rc;
  if ((rc = ensure(c, c->partials, sizeof(double) * row_doubles * nb))) return rc;
  return ensure(c, c->ipartials, sizeof(int) * nb);
}
static rgck::Corr corr_of(const rgc_ctx* c) { return {c->corr_v.as<int>(), c->corr_M.as<double>()}; }

// ---- C1-C3: grid + exact-kNN covariances (+ voxel map for the target), all enqueued on the stream: prepare_cloud and its stages ----
// The first cloud of a context costs one host<->device round trip -- the 6-int bounding box the dense grid is sized from; later
// clouds re-use the previous (widened) grid speculatively and need none (see prep_known_grid).
// Stage 1, stream ordering.  The scan is prepared on stream2, concurrently with the map's preparation on the main stream.  Whatever
// produced the scan was enqueued on the main stream (rgc_upload, the front-end, a caller's own kernels on rgc_stream()): stream2 waits for
// a mark recorded on the main stream BEFORE this frame's map preparation was enqueued (waiting for the map's kNN launch would serialise
// the two) -- i.e. at rgc_set_target*, or here when no map preparation is pending.  See rgc_set_source_device in rgc_hip.h.
static int prep_order_streams(rgc_ctx* c, bool is_target) {
  if (!is_target && c->main_has_target_prep && map_prep_finished(c)) c->main_has_target_prep = false;  // it has drained
  // (The map's own mark sits in FRONT of its counting pass: an event record between two kernels of one stream holds the second one back
  // ~5.8 us; in front of the frame's first launch it is processed while the GPU waits for the host anyway.)
  if (is_target || !c->main_has_target_prep || c->main_late_producer) {
    HIPCHK(c, hipEventRecord(c->main_mark, c->stream));
    c->mark_valid = true;
    c->main_late_producer = false;
  }
  if (is_target) c->main_has_target_prep = true;
  else if (c->mark_valid) HIPCHK(c, hipStreamWaitEvent(c->stream2, c->main_mark, 0));
  return RGC_OK;
}

// Stage 2, grid choice: cl.grid <- the grid where one is to be had without measuring, guarded by k_count (returns true): that of a box the
// library knows (*hint_out) or the speculative one; neither, the cloud's own box is measured (prep_measured_grid, behind the reuse set-up,
// whose launches go first).
// Speculative grid: consecutive clouds of a sequence cover (almost) the same cells, so the previous grid -- widened by two
// cells in x and y, one in z -- is re-used WITHOUT the bounding-box kernel and its host round trip (the only synchronisation
// between setInputTarget and the end of align).  A larger bounding grid changes nothing in the results: cells keep their
// relative order (voxel ids come from the cell scan), neighbourhoods are the same.  k_count guards it; the guard comes home
// with the LM state (or is read by the first other consumer) and a miss re-prepares the cloud on its own bounding box.
static bool prep_known_grid(rgc_ctx* c, Cloud& cl, bool is_target, bool force_bbox, double res, const rgc_ctx::BoxHint** hint_out) {
  const rgc_ctx::BoxHint*& hint = *hint_out;
  const bool spec = c->spec_on && !c->lm_host && cl.spec_ok && cl.spec_grid.res == res && !force_bbox;
  hint = (is_target && c->spec_on && !c->lm_host && !force_bbox) ? find_hint(c, cl.in, cl.n) : nullptr;
  if (hint)  // (a box that is not one -- it was derived from a pose that was not finite -- is no hint: the float -> int conversions below are undefined on it)
    for (int a = 0; a < 3; a++)
      if (!(std::isfinite(hint->lo[a]) && std::isfinite(hint->hi[a]) && hint->hi[a] >= hint->lo[a] && std::fabs(hint->lo[a]) <= 1.0e8 &&
            std::fabs(hint->hi[a]) <= 1.0e8)) { hint = nullptr; break; }
  if (hint) {  // the box is known (rgc_set_target_reframed / rgc_transform_cloud): its cells plus one on every side, guarded like a speculative grid
    int lo[3], dm[3];
    double ncell = 1.0;
    for (int a = 0; a < 3; a++) {
      lo[a] = (int)std::floor(hint->lo[a] / res - 0.5) - 1;
      dm[a] = (int)std::floor(hint->hi[a] / res - 0.5) + 1 - lo[a] + 1;
      ncell *= (double)dm[a];
    }
    if (ncell <= (double)c->prm.max_cells && ncell <= 2.0e9) cl.grid = rgck::make_grid(lo, dm, res);
    else hint = nullptr;
  }
  if (hint) {
    cl.spec_ok = true;
    cl.spec_grid = cl.grid;
  } else if (spec) {
    cl.grid = cl.spec_grid;
  }
  return hint || spec;
}
// ... the measured grid: the bounding-box kernel and its round trip, and the grid the NEXT cloud will try
static int prep_measured_grid(rgc_ctx* c, Cloud& cl, bool is_target, double res, hipStream_t s) {
  rgck::SmallBlock* dsm = c->d_small->block(is_target);
  rgck::SmallBlock* hsm = c->h_small->block(is_target);
  rgck::Grid g{};
  rgck::bbox(s, cl.in, cl.stride_f, cl.n, res, dsm->lo, &dsm->guard, is_target ? 0 : 1);
  HIPCHK(c, hipMemcpyAsync(hsm, dsm, offsetof(rgck::SmallBlock, nvox), hipMemcpyDeviceToHost, s));  // (box and guard)
  HIPCHK(c, hipStreamSynchronize(s));
  if (hsm->guard) return fail(c, RGC_ERR_NONFINITE, "%s cloud contains non-finite or absurd coordinates", is_target ? "target" : "source");
  double ncell = 1.0;
  for (int a = 0; a < 3; a++) {
    g.minc[a] = hsm->lo[a];
    g.dim[a] = hsm->hi[a] - hsm->lo[a] + 1;
    ncell *= (double)g.dim[a];
  }
  if (ncell > (double)c->prm.max_cells || ncell > 2.0e9)
    return fail(c, RGC_ERR_GRID_TOO_LARGE, "%s grid %d x %d x %d exceeds max_cells", is_target ? "target" : "source", g.dim[0], g.dim[1], g.dim[2]);
  g.res = res;
  g.inv_res = rgck::grid_inv_res(res);
  g.ncell = (int)ncell;
  cl.grid = g;
  // The grid the NEXT cloud will try.  The map's box is stable and its grid large: 2 / 2 / 1 cells of margin.  A raw scan's box
  // jumps with every far return, but it stays inside the sensor's range envelope and its grid is small: 16 / 16 / 4 cells of
  // margin, united with the box tried before (a miss costs the scan's whole preparation and a second solve, so the box only
  // ever grows -- at most to four times the measured one).
  rgck::Grid w = g;
  double wcell = 1.0;
  for (int a = 0; a < 3; a++) {
    const int m = is_target ? (a < 2 ? 2 : 1) : (a < 2 ? 16 : 4);
    int lo = g.minc[a] - m, hi = g.minc[a] + g.dim[a] - 1 + m;
    if (!is_target && cl.spec_ok && cl.spec_grid.res == g.res) {
      lo = std::min(lo, cl.spec_grid.minc[a]);
      hi = std::max(hi, cl.spec_grid.minc[a] + cl.spec_grid.dim[a] - 1);
    }
    w.minc[a] = lo; w.dim[a] = hi - lo + 1;
    wcell *= (double)w.dim[a];
  }
  if (!is_target && wcell > 4.0 * ncell + 1.0e6) {  // the union ran away (a sequence that really moves its box): start over from this cloud
    wcell = 1.0;
    for (int a = 0; a < 3; a++) { const int m = a < 2 ? 16 : 4; w.minc[a] = g.minc[a] - m; w.dim[a] = g.dim[a] + 2 * m; wcell *= (double)w.dim[a]; }
  }
  w.ncell = (int)wcell;
  cl.spec_ok = wcell <= (double)c->prm.max_cells && wcell <= 2.0e9;
  cl.spec_grid = w;
  if (cl.spec_ok) {  // its cell arrays now, in the frame that is slow anyway, not in the next one
    const size_t wc1 = (size_t)w.ncell + 1;
    int rc;
    if ((rc = ensure(c, cl.cnt, sizeof(int) * wc1 + 256))) return rc;
    if ((rc = ensure(c, cl.start, sizeof(int) * wc1))) return rc;
    if ((rc = ensure(c, cl.block_sums, sizeof(long long) * (wc1 / 2048 + 2)))) return rc;
    if (is_target && (rc = ensure(c, cl.cell_voxel, sizeof(int) * (size_t)w.ncell))) return rc;
    // ... and the voxel table (80 B per cell of a map denser than its grid: 1.3 GB at 16 M cells -- growing it in the next
    // frame, when the widened grid is first used, was a 77 ms allocation inside c5's three timed frames on a fresh box)
    if (is_target && (rc = ensure_voxel_table(c, cl, w.ncell))) return rc;
  }
  return RGC_OK;
}
// ... the neighbour lists on top of the seeds (rgck::KnnCache): their buffers, the certificates' exponent, the frame number, the copy of the map the
// counting pass compares it with (cl.rf).  An optimisation: if the device cannot hold them (112 B per point) the context goes down to the seeds.
static int prep_lists(rgc_ctx* c, Cloud& cl, hipStream_t s, double maxabs, double res) {
  const int n = cl.n;
  const size_t cap = (size_t)std::max(256, n / (4 * rgck::kTodoLists) + 1);
  const size_t want[7] = {sizeof(int) * (size_t)n * 20, sizeof(int) * (size_t)n, sizeof(int) * (size_t)n, sizeof(int) * (size_t)n,
                          sizeof(float4) * (size_t)n, sizeof(int) * cap * rgck::kTodoLists, sizeof(int) * (rgck::kTodoLists + 16)};
  DevBuf* bufs[7] = {&cl.nbr, &cl.pos_of, &cl.rank_of, &cl.qrank, &cl.map_copy, &cl.todo, &cl.cache_small};
  bool lists = true;
  for (int b = 0; b < 7 && lists; b++)
    if (ensure(c, *bufs[b], want[b]) != RGC_OK) lists = false;
  if (c->test_fail_cache_alloc) lists = false;  // (RGC_TEST_FAIL_CACHE_ALLOC at rgc_create: a test's way to walk the path below, as if the device were full)
  if (!lists) {
    (void)hipGetLastError();
    for (DevBuf* b : bufs) release(*b);
    c->cache_on = false;
    c->cache_dropped = true;
    cl.cache_live = false;
    if (trace_alloc()) fprintf(stderr, "[rgc] neighbour lists of %d points do not fit on the device: this context keeps seeds only from here on\n", n);
    return RGC_OK;
  }
  bool fresh = !cl.seed_warm || !cl.cache_live || !cl.nbr.p;
  cl.todo_cap = (int)cap;
  int ce2;  // (a cell of margin around the box, as the grid has)
  (void)std::frexp(1.5 * maxabs + 2.0 * res, &ce2);
  // larger coordinates than the certificates allow for: issue them again.  Smaller ones for sixteen frames in a row: new certificates
  // need the smaller gap only (the old ones, issued for a wider one, stand).
  if (fresh || ce2 > cl.cache_e2) { cl.cache_e2 = ce2; fresh = true; }
  if (ce2 < cl.cache_e2) {
    cl.cache_e2_low_max = cl.cache_e2_low ? std::max(cl.cache_e2_low_max, ce2) : ce2;
    if (++cl.cache_e2_low >= 16) { cl.cache_e2 = cl.cache_e2_low_max; cl.cache_e2_low = 0; }  // (the largest of those sixteen frames)
  } else {
    cl.cache_e2_low = 0;
  }
  if (cl.cache_frame >= (1 << 30)) { cl.cache_frame = 0; fresh = true; }
  cl.cache_frame++;
  if (fresh) HIPCHK(c, hipMemsetAsync(cl.cache_small.p, 0, sizeof(int) * (rgck::kTodoLists + 16), s));  // (list lengths, epoch, overflow)
  cl.rf.copy = cl.map_copy.as<float4>();
  cl.rf.epoch = cl.cache_small.as<int>() + rgck::kTodoLists;
  cl.rf.frame = cl.cache_frame;
  cl.rf.force = fresh ? 1 : 0;
  cl.cache_on = true;
  return RGC_OK;
}

// Stage 3, reuse set-up.  A re-framed map (rgc_set_target_reframed) has not been written yet: with its box known the counting pass
// produces it on the way (fuse_reframe: one pass over the map and one launch less); any other route measures the cloud first and needs
// it in memory.  Seeds of the exact search: a re-framed map is the point set of cl.rf.src moved rigidly, so what the last search of that
// buffer found bounds this one (rgck::KnnSeeds; exactness does not depend on it).  Any other target: no seeds.
static int prep_reuse(rgc_ctx* c, Cloud& cl, bool is_target, hipStream_t s, const rgc_ctx::BoxHint* hint, bool fuse_reframe, double res) {
  const int n = cl.n;
  const bool own_target = is_target && &cl == &c->tgt;
  if (cl.reframe_pending && !fuse_reframe)
    rgck::transform_q(s, cl.rf.src, cl.rf.src_stride_f, n, cl.rf.q, cl.rf.t, const_cast<float*>(cl.in), 4);
  cl.seed_on = false;
  if (own_target && cl.reframe_pending && c->seeds_on && !general_route(c) && rgck::knn_seeds_apply(n, c->prm.k_correspondences)) {
    int rc;
    if (cl.seed_key != (const void*)cl.rf.src || cl.seed_n != n || !cl.seed.p) {
      if ((rc = ensure(c, cl.seed, sizeof(float) * (size_t)n))) return rc;
      HIPCHK(c, hipMemsetAsync(cl.seed.p, 0x7f, sizeof(float) * (size_t)n, s));  // 3.4e38: "no seed"
      cl.seed_key = cl.rf.src;
      cl.seed_n = n;
      cl.seed_warm = false;
    }
    cl.seed_on = true;
    // the coordinates' fp32 rounding, twice (two frames), on either end of a distance: 4 ulp of the largest coordinate of the box
    double maxabs = 1.0;
    if (hint) for (int a = 0; a < 3; a++) maxabs = std::max(maxabs, std::max(std::fabs(hint->lo[a]), std::fabs(hint->hi[a])));
    else maxabs = 1024.0;
    int e2;
    (void)std::frexp(1.5 * maxabs, &e2);
    cl.seed_slack = (float)(4.0 * std::ldexp(1.0, e2 - 24));
    // The neighbour lists on top: the counting pass that produces the map compares it with the library's copy on the way, so only that
    // route has them; a lazy target searches a part of the map per frame and keeps none.
    // (the certificate's error budget is that of a RIGID motion: reframe_point applies v + 2w(u x v) + 2u x (u x v) as Eigen does, without
    // normalising q, so |q|^2 - 1 shows up as a relative error of that order on every distance.  1e-9 is far inside the 4e-6 the
    // certificate allows for and is met by any quaternion normalised in fp64; one normalised in fp32 gets seeds, not lists.)
    const double qn = cl.rf.q.x * cl.rf.q.x + cl.rf.q.y * cl.rf.q.y + cl.rf.q.z * cl.rf.q.z + cl.rf.q.w * cl.rf.q.w;
    cl.cache_on = false;
    if (c->cache_on && fuse_reframe && c->lazy_margin <= 0 && std::fabs(qn - 1.0) < 1.0e-9 && (rc = prep_lists(c, cl, s, maxabs, res))) return rc;
  } else if (own_target) {
    cl.seed_key = nullptr;
    cl.cache_on = false;
  }
  if (own_target) {
    cl.cache_live = false;  // (set again by the search that attaches the lists, cloud_covariances)
    cl.searched_known = -1;
    if (!cl.cache_on) { cl.rf.copy = nullptr; cl.rf.epoch = nullptr; }
  }
  cl.reframe_pending = false;
  return RGC_OK;
}

// Stage 4, buffer sizing: everything the grid build and the search write, and the counters known to be zero
static int prep_size_buffers(rgc_ctx* c, Cloud& cl, bool is_target, hipStream_t s, const rgc_ctx::BoxHint* hint) {
  const int n = cl.n;
  const rgck::Grid& g = cl.grid;
  const size_t nc1 = (size_t)g.ncell + 1;  // counters (+ sentinel)
  int rc;
  for (DevBuf* b : {&cl.cell_of, &cl.slot_of})
    if ((rc = ensure(c, *b, sizeof(int) * n))) return rc;
  // (a hinted box is that of a map re-framed by the vehicle's pose: as the yaw changes it swings between the map's own box and one
  // with twice the cells -- the cell arrays are sized for the largest it can get, once, not grown a few per cent per frame)
  size_t want_cells = nc1;
  if (hint && hint->reach_xy > 0) {
    const double e = hint->reach_xy / g.res + 6.0, ez = hint->reach_z / g.res + 6.0;
    const double cells = e * e * ez * 1.05;
    if (cells < 2.0e9 && cells <= (double)c->prm.max_cells && (size_t)cells > want_cells) want_cells = (size_t)cells;
  }
  if ((rc = ensure(c, cl.cnt, sizeof(int) * want_cells + 256))) return rc;
  if ((rc = ensure(c, cl.start, sizeof(int) * want_cells))) return rc;
  if ((rc = ensure(c, cl.block_sums, sizeof(long long) * (want_cells / 2048 + 2)))) return rc;
  if ((rc = ensure(c, cl.order_tmp, sizeof(long long) * n))) return rc;
  if ((rc = ensure(c, cl.P, sizeof(float4) * ((size_t)n + 4)))) return rc;
  if ((rc = ensure(c, cl.segs, rgck::deferred_bytes(n)))) return rc;
  for (DevBuf* b : {&cl.nx, &cl.ny, &cl.nz})
    if ((rc = ensure(c, *b, sizeof(double) * n))) return rc;
  if (is_target && (rc = ensure(c, cl.cell_voxel, sizeof(int) * want_cells))) return rc;  // (want_cells > ncell)
  if (cl.cnt.p != cl.cnt_seen) { cl.cnt_clean = 0; cl.cnt_seen = cl.cnt.p; }  // re-allocated: contents unknown
  if (cl.cnt_clean < nc1) {  // first use or a larger grid; afterwards the scan leaves the counters clean: no fill kernel per frame
    const size_t fill = std::min(cl.cnt.cap, (sizeof(int) * nc1 + 255) & ~(size_t)255);
    HIPCHK(c, hipMemsetAsync(cl.cnt.p, 0, fill, s));
    cl.cnt_clean = fill / sizeof(int);
  }  // (a smaller grid leaves the counters beyond it as clean as they were: a re-framed map's box breathes with the yaw)
  return RGC_OK;
}

// Stage 5, the grid-build chain: count (a re-framed map is produced on the way), scan, place, gather
static void prep_build_grid(rgc_ctx* c, Cloud& cl, bool is_target, hipStream_t s, bool fuse_reframe) {
  const int n = cl.n, hi = is_target ? 0 : 1;  // the scan's kernels share CUs with the map's kNN launch: raised wave priority
  int *cell_of = cl.cell_of.as<int>(), *start = cl.start.as<int>();
  rgck::count_cells(s, cl.in, cl.stride_f, n, cl.grid, cell_of, cl.slot_of.as<int>(), cl.cnt.as<int>(), hi, guard_of(c, cl, is_target), fuse_reframe ? &cl.rf : nullptr);
  rgck::scan_cells(s, cl.cnt.as<int>(), start, cl.grid.ncell + 1, cl.block_sums.p, is_target ? cl.cell_voxel.as<int>() : nullptr,
                   is_target ? &c->d_small->map.nvox : nullptr, hi, is_target ? nullptr : &c->d_small->scan.sum_sq);
  const bool with_cache = is_target && &cl == &c->tgt && cl.cache_on;
  const rgck::KnnSeeds sd = cloud_seeds(cl, is_target);
  rgck::place(s, n, cell_of, cl.slot_of.as<int>(), start, cl.order_tmp.as<unsigned long long>(), hi, with_cache ? &sd.cache : nullptr);
  rgck::rank_gather(s, cl.in, cl.stride_f, n, cell_of, start, cl.order_tmp.as<unsigned long long>(), cl.P.as<float4>(), cl.segs.as<int>(), hi,
                    with_cache ? &sd.cache : nullptr);
}

static int prepare_cloud(rgc_ctx* c, Cloud& cl, bool is_target, bool force_bbox = false) {
  if (!is_target && &cl == &c->src) { c->src_held = c->src_hold_pending; c->src_hold_pending = false; }  // was THIS scan held? (the same contexts may run a frame at a time later)
  const int n = cl.n;
  cl.covs_user = false;
  if (is_target && &cl == &c->tgt) {
    c->tgt_generation++;       // borrowers of the previous target must share again
    c->tgt_owner = nullptr;    // (a borrowed target's aliases are dropped buffer by buffer in ensure())
  }
  hipStream_t s = is_target ? c->stream : c->stream2;
  int rc;
  if ((rc = prep_order_streams(c, is_target))) return rc;
  {
    ProfScope ps(c, RGC_K_GRID, n, s);
    // the cloud's whole block: bbox accumulators + guard, and the map's voxel counter / the scan's sum of count^2, a float accumulated by
    // the cell scan (ncorr, behind the map's block, stays untouched)
    // ... unless the previous solve's first step has already put the block back to this image on the device (reinit_small_blocks)
    if (!c->small_clean[is_target ? 0 : 1]) {
      const int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
      static_assert(sizeof(init) == sizeof(rgck::SmallBlock), "a block's initial image");
      memcpy(c->h_small->block(is_target), init, sizeof(init));
      HIPCHK(c, hipMemcpyAsync(c->d_small->block(is_target), c->h_small->block(is_target), sizeof(init), hipMemcpyHostToDevice, s));
    }
    c->small_clean[is_target ? 0 : 1] = false;  // this preparation uses it
    // The scan's kNN grid need not be the voxel grid (only the map's doubles as the voxel map), and the exact search returns the
    // same neighbours on any grid: a raw 64-beam sweep puts thousands of points into the 1 m cells near the sensor (every query
    // scans its whole cell: O(c^2)), so its cell size follows the crowding measured on the previous frame of the sequence.
    const double res = is_target ? c->prm.voxel_res : (c->src_res > 0.0 ? c->src_res : (c->src_res_auto > 0.0 ? c->src_res_auto : c->prm.voxel_res));
    const rgc_ctx::BoxHint* hint = nullptr;
    const bool guarded = prep_known_grid(c, cl, is_target, force_bbox, res, &hint);
    const bool fuse_reframe = cl.reframe_pending && hint != nullptr && cl.stride_f == 4 && ((uintptr_t)cl.in & 15) == 0;  // (k_count<true> stores float4)
    if ((rc = prep_reuse(c, cl, is_target, s, hint, fuse_reframe, res))) return rc;
    cl.spec_used = guarded;
    if (!guarded && (rc = prep_measured_grid(c, cl, is_target, res, s))) return rc;
    if ((rc = prep_size_buffers(c, cl, is_target, s, hint))) return rc;
    prep_build_grid(c, cl, is_target, s, fuse_reframe);
  }
  cl.lazy = 0;
  if (is_target && &cl == &c->tgt && c->lazy_margin > 0 && !c->lm_host && !general_route(c) && map_wide_r_of(c, cl) == 0) {
    // lazy target: which part of the map needs covariances and voxels is decided by the solve's guess (rgc_align_begin: lazy_build);
    // any other consumer completes the map first (validate_clouds)
    if ((rc = ensure_voxel_table(c, cl, cl.grid.ncell))) return rc;
    cl.lazy = 1;
    cl.nvox = -1;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->tgt_prepared, s));
    cl.ready = true;
    return RGC_OK;
  }
  cl.prepared_recorded = false;
  if ((rc = cloud_covariances(c, cl, is_target))) return rc;
  HIPCHK(c, hipGetLastError());
  if (!is_target) {
    HIPCHK(c, hipEventRecord(c->src_ready, s));
    c->src_pending = true;
  } else if (!cl.prepared_recorded) {  // (otherwise the map's last launch carries the event, cloud_covariances)
    HIPCHK(c, hipEventRecord(c->tgt_prepared, s));
  }
  cl.ready = true;
  return RGC_OK;
}

static rgck::KnnSeeds cloud_seeds(const Cloud& cl, bool is_target) {
  rgck::KnnSeeds sd;
  if (is_target && cl.seed_on) {
    sd.seed = cl.seed.as<float>(); sd.slack = cl.seed_slack; sd.warm = cl.seed_warm;
    if (cl.cache_on) {
      rgck::KnnCache& kc = sd.cache;
      kc.nbr = cl.nbr.as<int>();
      kc.pos_of = cl.pos_of.as<int>();
      kc.rank_of = cl.rank_of.as<int>();
      kc.qrank = cl.qrank.as<int>();
      kc.todo = cl.todo.as<int>();
      kc.todo_cnt = cl.cache_small.as<int>();
      kc.epoch = cl.cache_small.as<int>() + rgck::kTodoLists;
      kc.overflow = cl.cache_small.as<int>() + rgck::kTodoLists + 1;
      kc.frame = cl.cache_frame;
      kc.todo_cap = cl.todo_cap;
      // what the coordinates' fp32 rounding in two frames can move a distance by, twice: 4 sqrt(3) ulp of the largest coordinate, and a tenth
      kc.cert_slack = (float)(4.0 * 1.7320508 * 1.1 * std::ldexp(1.0, cl.cache_e2 - 24));
    }
  }
  return sd;
}

// How many cells of grid g (per axis) a ball of max_dist can span beyond its centre's cell.  The fp32 key of a pair can ROUND DOWN onto
// max_dist_sq: res = 1, max_dist = 3, x = nextafter(1, 0) in cell 0 and a neighbour at x = 4 in cell 4 have dx = 3.0f and key 9 -- a member
// four cells away.  A member lies within max_dist (1 + 2^-20) of its centre (*reach_dist; the key's three roundings are 2^-22 of it), and a
// cell offset of d needs a distance above (d - 1) res: d <= floor(reach_dist / res) + 1.  Clamped to the grid's largest dimension.
static int rbf_reach(const rgck::Grid& g, double max_dist, double* reach_dist) {
  const double R = max_dist * (1.0 + 0x1p-20);
  *reach_dist = R;
  int dmax = 1;
  for (int a = 0; a < 3; a++) dmax = g.dim[a] > dmax ? g.dim[a] : dmax;
  const double r = std::floor(R / g.res) + 1.0;
  return r < (double)dmax ? (int)r : dmax;  // (also when r is infinite)
}

// The deferred list's entry words as the launches that resolve the deferred queries themselves need them on entry (coop_stream): "empty".
// The WHOLE allocation is filled, once: the buffer keeps its head-room from cloud to cloud, and a larger cloud that still fits it has its
// entries where a smaller one's launches never wrote.  The readers put "empty" back, so the words stay clean until a plain list is
// written over them (slots_clean = false).
static int slots_make_clean(rgc_ctx* c, Cloud& cl, hipStream_t s) {
  if (cl.slots_clean && cl.slots_seen == cl.segs.p && cl.slots_cap == cl.segs.cap) return RGC_OK;  // (a new allocation may come back at the old address)
  HIPCHK(c, hipMemsetAsync(cl.segs.as<int>() + 16, rgck::kDeferredSlotEmptyByte, cl.segs.cap - 16 * sizeof(int), s));
  cl.slots_clean = true;
  cl.slots_seen = cl.segs.p;
  cl.slots_cap = cl.segs.cap;
  return RGC_OK;
}

// The general covariance route (general_route above): every point through the cooperative search (or its RBF ball), a 3x3 per point, a
// plain voxel pass.  (The deferred-list counter is zeroed by the grid build and stays zero: no query is deferred on this route.)
static int cloud_covariances_general(rgc_ctx* c, Cloud& cl, bool is_target, hipStream_t s) {
  const int n = cl.n;
  int rc;
  if ((rc = ensure(c, cl.c6, sizeof(double) * 6 * (size_t)n))) return rc;
  const int* guard = guard_of(c, cl, is_target);
  {
    ProfScope ps(c, is_target ? RGC_K_KNN_COV : RGC_K_KNN_COV_SRC, n, s);
    if (c->cov_method == RGC_COV_RBF) {
      const float md = (float)c->rbf_max_dist;
      double reach_dist;
      const int reach = rbf_reach(cl.grid, c->rbf_max_dist, &reach_dist);
      rgck::rbf_cov6(s, cl.sorted(), (float)c->rbf_width, md * md, reach, reach_dist, c->reg_method, cl.c6.as<double>(), guard);
    } else {
      rgck::knn_cov6(s, cl.sorted(), c->prm.k_correspondences, c->reg_method, cl.c6.as<double>(), guard);
    }
  }
  if (is_target) {
    if ((rc = ensure_voxel_table(c, cl, cl.grid.ncell))) return rc;
    ProfScope ps(c, RGC_K_VOXEL, n);
    rgck::voxel_build_general(s, cl.sorted(), cl.c6.as<double>(), cl.voxels(), c->voxel_mode == RGC_VOXEL_MULTIPLICATIVE ? 1 : 0, guard);
    cl.nvox = -1;
    cl.cache_searched_lists = false;
  }
  return RGC_OK;
}

// How a cloud's covariances (and the map's voxels) are enqueued, decided before anything is: what the bulk launch is asked for beyond the
// search (`bulk`: the sparse map's wider block, the seeds) and which stages go inside it.
struct CovRoute {
  rgck::KnnBulkOpts bulk;
  // The dense map's launch (the dominant kernel) is timed by ITS OWN start / stop times (hipExtLaunchKernelGGL fills the two events):
  // two hipEventRecord packets around it cost ~3 % of a frame of a dependent sequence on two contexts (bench.py's timed region).
  bool self_timed;
  // The dense map's launch over the whole map also builds the voxel records of its workgroups' own cells and resolves its deferred
  // queries in-launch (rgck::KnnBulkOpts::fuse; voxel_seams behind it) -- unless the stage-by-stage profile wants the voxel or the cooperative
  // stage apart, or RGC_VOXEL_IMPL=separate.  A target shared or bound to the rolling map keeps the stages apart as well.
  // Nor, unless RGC_VOXEL_IMPL=fused, a context whose last scan was not held behind another context's target (rgc_hold_source_until_target_of:
  // a pipelined sequence).  There the scan is prepared on the second stream BESIDE this launch, and its one-wave search (154 VGPRs: 160
  // allocated) gets onto a SIMD when ONE of the map's five 88-register waves retires (72 + 88 free) -- with the cooperative waves inlined
  // the map's kernel allocates 96, two must retire, and the scan's search took 160 us instead of 91: a frame one at a time 11 % slower
  // (EXPERIMENTS.md round 16).  A pipelined context prepares its scan under the other context's solve, not beside its own map's search.
  bool fused;
  // the scan: its deferred queries are resolved by the last workgroups of the same launch (coop_stream) -- unless the stage-by-stage
  // profile wants the two apart
  bool stream_coop;
};
static CovRoute cov_route(const rgc_ctx* c, const Cloud& cl, bool is_target) {
  const int n = cl.n, k = c->prm.k_correspondences;
  CovRoute r{};
  r.bulk.wide_r = is_target ? map_wide_r_of(c, cl) : 0;
  r.bulk.seeds = cloud_seeds(cl, is_target);
  r.self_timed = profiled(c, is_target ? RGC_K_KNN_COV : RGC_K_KNN_COV_SRC) && rgck::knn_bulk_times_itself(is_target, n, k, r.bulk);
  const bool stage_prof = profiled(c, RGC_K_VOXEL) || profiled(c, RGC_K_KNN_COOP);
  const bool want = c->voxel_impl == 2 || (c->voxel_impl == 0 && c->src_held);
  r.fused = is_target && &cl == &c->tgt && !c->tgt_owner && !c->map.bound && want && !stage_prof && k <= 32 && rgck::knn_bulk_fuses_voxels(true, n, k, r.bulk);
  r.stream_coop = !is_target && c->coop_stream_on && k <= 32 && !profiled(c, RGC_K_KNN_COOP_SRC);
  return r;
}

// C2 / C3 of a cloud whose grid is built: exact-kNN covariances (+ the Gaussian voxel map for the target), enqueued on the cloud's stream.
static int cloud_covariances(rgc_ctx* c, Cloud& cl, bool is_target) {
  const int n = cl.n, k = c->prm.k_correspondences;
  hipStream_t s = is_target ? c->stream : c->stream2;
  int rc;
  cl.general = general_route(c);
  if (cl.general) return cloud_covariances_general(c, cl, is_target, s);
  const CovRoute rt = cov_route(c, cl, is_target);
  rgck::KnnBulkOpts o = rt.bulk;
  if (rt.fused) {
    if ((rc = ensure_voxel_table(c, cl, cl.grid.ncell))) return rc;  // (the launch writes the voxel records: allocated here, not below)
    o.fuse = cl.voxels();
  }
  // a launch that resolves its deferred queries itself needs the entry words "empty" on entry: filled once per allocation, the readers
  // put it back.  Any other writes the plain list over the slots (a cloud can change roles: rgc_swap_source_and_target)
  if (rt.fused || rt.stream_coop) {
    if ((rc = slots_make_clean(c, cl, s))) return rc;
    o.coop_waves = coop_waves_est(cl);
  } else {
    cl.slots_clean = false;
  }
  const rgck::SortedCloud sc = cl.sorted();
  const rgck::Normals nrm = cl.normals();
  const rgck::DeferredBuf df = cl.deferred(guard_of(c, cl, is_target));
  {
    ProfScope ps(c, is_target ? RGC_K_KNN_COV : RGC_K_KNN_COV_SRC, n, s, /*records=*/!rt.self_timed);
    if (rt.self_timed && ps.on) { o.ev0 = ps.r.a; o.ev1 = ps.r.b; }
    rgck::knn_bulk(s, is_target, sc, k, df, nrm, o);
  }
  if (is_target) cl.cache_searched_lists = o.seeds.cache.nbr && o.seeds.warm && o.wide_r == 0;
  if (o.seeds.seed && o.wide_r == 0) {
    cl.seed_warm = true;
    if (o.seeds.cache.nbr) cl.cache_live = true;
  }
  // The map's deferred queries (~100 of a million, one wave each: 20 us of latency) are resolved in the SAME launch as the voxel map's
  // build (k_voxel_build_coop); the few voxels that hold one are recomputed behind it (k_voxel_patch).  (`fused`: inside the bulk launch
  // itself, and the voxel map with them; k_voxel_seams finishes it.)  The scan has no voxel map: its chain stays serial.
  if (!is_target && !rt.stream_coop) {
    ProfScope ps(c, RGC_K_KNN_COOP_SRC, n, s);
    rgck::knn_coop(s, false, sc, k, df, nrm, coop_waves_est(cl));
  }
  if (is_target) {
    if ((rc = ensure_voxel_table(c, cl, cl.grid.ncell))) return rc;
    const rgck::VoxelMap vm = cl.voxels();
    ProfScope ps(c, RGC_K_VOXEL, n);
    if (rt.fused) {
      rgck::voxel_seams(s, sc, nrm, vm, df, patch_waves_est(cl), c->prep_event_ext ? c->tgt_prepared : nullptr);
      cl.prepared_recorded = c->prep_event_ext;
    } else {
      rgck::voxel_build_coop(s, sc, nrm, vm, k, df, coop_waves_est(cl), o.seeds);
      cl.prepared_recorded = c->prep_event_ext && &cl == &c->tgt;
      rgck::voxel_patch(s, sc, nrm, vm, df, patch_waves_est(cl), cl.prepared_recorded ? c->tgt_prepared : nullptr);
    }
    cl.nvox = -1;  // fetched lazily
  }
  return RGC_OK;
}

// Lazy target, at rgc_align_begin: the cells within lazy_margin cells of where the scan falls at the guess are stamped (the look-up's own
// arithmetic), and covariances + voxels are built for those only -- at c-main 8 % of the map's points at a margin of two cells.  The
// solve checks every look-up (linearize_point): one that lands on an occupied voxel outside the stamped set makes rgc_align_end
// complete the map and solve again, so the result is the full build's bit for bit either way.
static int lazy_build(rgc_ctx* c, const float guess[16]) {
  Cloud& cl = c->tgt;
  hipStream_t s = c->stream;
  int rc;
  const int n = cl.n, k = c->prm.k_correspondences;
  const size_t cells = (size_t)cl.grid.ncell;
  if ((rc = ensure(c, cl.need, sizeof(int) * cells + 256))) return rc;
  if ((rc = ensure(c, cl.qlist, sizeof(int) * (size_t)n + 256))) return rc;
  if ((rc = ensure(c, cl.cell_list, sizeof(int) * (size_t)n + 256))) return rc;
  cl.need_stamp++;
  if (cl.need.p != cl.need_seen || cl.need_stamp > 0x3fffffff) {  // a new allocation (or the stamps ran out): start over from a clean array
    HIPCHK(c, hipMemsetAsync(cl.need.p, 0, cl.need.cap, s));
    cl.need_seen = cl.need.p;
    cl.need_stamp = 1;
  }
  if (c->src_in_pending) {  // the scan came from the host: its upload ran on stream2
    HIPCHK(c, hipStreamWaitEvent(s, c->src_in_ready, 0));
    c->src_in_pending = false;
  }
  double T[16];
  for (int i = 0; i < 16; i++) T[i] = (double)guess[i];
  int* counts = cl.segs.as<int>() + 1;  // [0] listed queries, [1] listed cells: behind the deferred-query counter, zeroed with it by k_rank_gather
  const rgck::SortedCloud sc = cl.sorted();
  const rgck::Normals nrm = cl.normals();
  const rgck::VoxelMap vm = cl.voxels();
  const rgck::DeferredBuf df = cl.deferred(guard_of(c, cl, true));
  rgck::footprint(s, c->src.in, c->src.stride_f, c->src.n, pose_from(T), sc, cl.need.as<int>(), cl.need_stamp, c->lazy_margin, cl.qlist.as<int>(),
                  cl.cell_list.as<int>(), counts, df.guard);
  const int c_est = cl.lazy_ncell_seen >= 0 ? cl.lazy_ncell_seen + cl.lazy_ncell_seen / 4 + 1024 : n / 8 + 1024;
  cl.slots_clean = false;  // (the plain deferred list is written over the entry words)
  {
    rgck::KnnBulkOpts o;
    o.qlist = cl.qlist.as<int>();
    o.nq = counts;
    o.q_est = cl.lazy_nq_seen >= 0 ? cl.lazy_nq_seen + cl.lazy_nq_seen / 4 + 4096 : n;
    o.seeds = cloud_seeds(cl, true);
    ProfScope ps(c, RGC_K_KNN_COV, n, s);
    rgck::knn_bulk(s, true, sc, k, df, nrm, o);
    if (cl.seed_on) cl.seed_warm = true;
  }
  {
    ProfScope ps(c, RGC_K_VOXEL, n);
    rgck::voxel_cells_coop(s, sc, nrm, vm, k, df, coop_waves_est(cl), cl.cell_list.as<int>(), counts + 1, c_est, cloud_seeds(cl, true));
    rgck::voxel_patch(s, sc, nrm, vm, df, patch_waves_est(cl));
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->tgt_prepared, s));  // (the map's preparation ends HERE now: what the solve goes behind, what another context's held scan waits for)
  cl.lazy = 2;
  return RGC_OK;
}

// every consumer of the target other than the chained solve: the whole map, as without the lazy mode
static int complete_target(rgc_ctx* c) {
  Cloud& cl = c->tgt;
  if (!cl.ready || cl.lazy == 0 || c->tgt_owner) return RGC_OK;
  HIPCHK(c, hipMemsetAsync(cl.segs.p, 0, 3 * sizeof(int), c->stream));  // the deferred-query counter of the bulk launch, and the lazy lists' sizes behind it (the launch's count-out word)
  int rc = cloud_covariances(c, cl, true);
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->tgt_prepared, c->stream));
  cl.lazy = 0;
  // (corr_valid stays as it is: the completed map has the voxel ids and records of the part a solve has used, bit for bit, so the
  // correspondences that solve froze are still the ones rgc_compute_error needs -- as after a solve on a fully built target)
  c->deferred_known = false;
  c->main_has_target_prep = true;
  return RGC_OK;
}

int set_cloud(rgc_ctx* c, Cloud& cl, bool is_target, const float* xyz, int n, int stride_bytes, bool on_device, const rgck::Reframe* rf) {
  if (!c) return RGC_ERR_INVALID;
  cl.reframe_pending = false;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  cl.ready = false;
  cl.n = 0;
  drop_frozen(c);
  c->deferred_known = false;
  if (is_target) c->map.bound = false;
  if (!xyz || n < 0) return fail(c, RGC_ERR_INVALID, "null cloud");
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (n > (1 << 27)) return fail(c, RGC_ERR_INVALID, "cloud has %d points, the limit is 2^27 (32-bit byte offsets into the sorted array)", n);
  if (n < min_cloud_points(c))
    return fail(c, RGC_ERR_TOO_FEW_POINTS, "%s cloud has %d points, need >= k = %d", is_target ? "target" : "source", n, c->prm.k_correspondences);
  HIPCHK(c, hipSetDevice(c->device));
  const int stride_f = stride_bytes / 4;
  if (on_device) { const int rk = check_device_range(c, xyz, record_bytes(n, stride_bytes, false), is_target ? "target cloud" : "source cloud"); if (rk) return rk; }
  if (on_device) {
    cl.in = xyz;
    if (!is_target) c->src_in_pending = false;  // (no upload of this scan to wait for)
  } else {
    const size_t bytes = (size_t)n * stride_bytes;
    int rc = ensure(c, cl.in_copy, bytes);
    if (rc) return rc;
    if (!is_target && c->src_read_pending) {  // a kernel on the main stream still reads the previous scan out of this buffer (rgc_get_aligned_device)
      HIPCHK(c, hipStreamWaitEvent(c->stream2, c->src_read_done, 0));
      c->src_read_pending = false;
    }
    // pageable host memory: hipMemcpyAsync stages and returns once the source has been consumed
    HIPCHK(c, hipMemcpyAsync(cl.in_copy.p, xyz, bytes - (stride_bytes - 12), hipMemcpyHostToDevice, is_target ? c->stream : c->stream2));
    if (!is_target) {  // (a lazy target's footprint pass reads the scan's input on the main stream -- whenever rgc_set_target_lazy was called)
      HIPCHK(c, hipEventRecord(c->src_in_ready, c->stream2));
      c->src_in_pending = true;
    }
    cl.in = cl.in_copy.as<const float>();
    // (a box known for the caller's HOST buffer -- the leaf filter's output, rgc_voxelgrid -- goes with the cloud to its device copy)
    if (is_target) {
      if (const rgc_ctx::BoxHint* h = find_hint(c, xyz, n)) { const rgc_ctx::BoxHint hh = *h; put_hint(c, cl.in, n, hh.lo, hh.hi); }
      else for (auto& e : c->box_hint) if (e.p == (const void*)cl.in) e.p = nullptr;  // (the staging buffer's last cloud's box says nothing about this one)
    }
  }
  cl.stride_f = stride_f;
  cl.n = n;
  if (rf && on_device) { cl.rf = *rf; cl.reframe_pending = true; }
  int rc = prepare_cloud(c, cl, is_target);
  if (rc) { cl.n = 0; return rc; }
  if (is_target) { c->stats.n_target = n; c->stats.target_cells = cl.grid.ncell; }
  else { c->stats.n_source = n; c->stats.source_cells = cl.grid.ncell; }
  return RGC_OK;
}

rgck::Pose pose_from(const double T[16]) {
  rgck::Pose P;
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) P.R[a * 3 + b] = T[a * 4 + b];
    P.t[a] = T[a * 4 + 3];
  }
  return P;
}
rgck::PoseF posef_from(const float T[16]) {
  rgck::PoseF P;
  for (int a = 0; a < 12; a++) P.m[a] = T[a];
  return P;
}

// order the main stream after the source preprocessing (which runs on stream2)
static int join_source(rgc_ctx* c) {
  if (c->src_pending) {
    // (a scan prepared ahead -- two contexts taking turns -- has usually finished by now: then no barrier packet goes into the main
    // stream at all; a dependency that has to be resolved across streams costs ~10 us in front of the kernel behind it, even a met one)
    // A scan that is ALMOST ready -- two contexts taking turns: its cooperative search is still running beside the map's preparation --
    // is waited for here, on the host, for as long as the map's preparation is still running anyway (bounded: join_spin_us): the solve's
    // launches are not needed in the queue before that, and the host has nothing else to do until the solve ends.
    bool ready = hipEventQuery(c->src_ready) == hipSuccess;
    if (!ready && c->join_spin_us > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      for (;;) {
        (void)hipGetLastError();
        if (hipEventQuery(c->src_ready) == hipSuccess) { ready = true; break; }
        if (map_prep_finished(c)) break;
        if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > (double)c->join_spin_us) break;
        __builtin_ia32_pause();  // (a sibling hyper-thread may be driving another sequence's context)
      }
    }
    if (!ready) {
      (void)hipGetLastError();  // ("not ready" is an answer, not an error to be found by a later check)
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->src_ready, 0));
    }
    c->src_pending = false;
  }
  return RGC_OK;
}

// Guards of speculative grids (bit 0: non-finite point, bit 1: point outside the grid).  Returns < 0 on error, 1 if a cloud had
// to be prepared again on its own bounding box (whatever was computed from it must be redone), 0 if everything stands.
static int resolve_guards(rgc_ctx* c, int guard_t, int guard_s) {
  int redo = 0;
  Cloud* cl[2] = {&c->tgt, &c->src};
  const int gd[2] = {guard_t, guard_s};
  for (int a = 0; a < 2; a++) {
    if (!cl[a]->spec_used) continue;
    cl[a]->spec_used = false;
    if (!cl[a]->ready || cl[a]->n <= 0) continue;  // (a cloud cleared since -- rgc_clear_source / _target --: its guard word is the last cloud's, there is nothing to prepare again)
    if (!gd[a]) continue;
    cl[a]->ready = false;
    drop_frozen(c);
    c->deferred_known = false;
    if (gd[a] & 1) { cl[a]->n = 0; return fail(c, RGC_ERR_NONFINITE, "%s cloud contains non-finite or absurd coordinates", a == 0 ? "target" : "source"); }
    if (trace_alloc()) fprintf(stderr, "[rgc] %s cloud left its speculative grid: prepared again\n", a == 0 ? "target" : "source");
    if (a == 0) drop_hints(c);  // (a hinted box that did not hold: its buffer was rewritten behind the library's back -- measure again)
    int rc = prepare_cloud(c, *cl[a], a == 0, /*force_bbox=*/true);
    if (rc) { cl[a]->n = 0; return rc; }
    redo = 1;
  }
  return redo;
}

// A borrowed target (rgc_share_target) is only as good as its owner: alive (the same context, not a new one at its address) and not
// prepared again since.  Called by EVERY consumer of c->tgt -- the solve, the fine seam, the fitness score, the getters.
int check_target_owner(rgc_ctx* c) {
  if (!c->tgt_owner) return RGC_OK;
  bool alive;
  unsigned long long owner_gen = 0;
  {
    std::lock_guard<std::mutex> lk(g_live_mutex);  // (the owner is only looked at while it cannot be destroyed)
    alive = g_live.count(c->tgt_owner) != 0 && c->tgt_owner->uid == c->tgt_owner_uid;
    if (alive) owner_gen = c->tgt_owner->tgt_generation;
  }
  if (!alive) {  // its device buffers are gone with it
    c->tgt_owner = nullptr;
    for (DevBuf* b : shared_bufs(c->tgt)) release(*b);
    c->tgt.ready = false;
    c->tgt.n = 0;
    return fail(c, RGC_ERR_NO_INPUT, "the context whose target this one shared has been destroyed");
  }
  if (owner_gen != c->tgt_owner_gen)
    return fail(c, RGC_ERR_INVALID, "the shared target was rebuilt by its owner: rgc_share_target again");
  return RGC_OK;
}

// for every consumer except rgc_align (which gets the guards with its state read-back): one synchronisation, once per cloud
static int validate_clouds(rgc_ctx* c, bool whole_target = true) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  { int rc = check_target_owner(c); if (rc) return rc; }
  // The guards FIRST: a lazy target whose speculative grid did not hold must be prepared again on its own box BEFORE it is completed -- the
  // completion's kernels leave at once on a tripped guard, and the re-preparation behind it would put back an unbuilt lazy target that
  // nobody completes any more (a target replaced while a scan is set, then read through a getter: tests/fuzz/fuzz_api.py found it).
  if ((c->tgt.ready && c->tgt.spec_used) || (c->src.ready && c->src.spec_used)) {
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipMemcpyAsync(&c->h_small->map.guard, &c->d_small->map.guard, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->h_small->scan.guard, &c->d_small->scan.guard, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int r = resolve_guards(c, c->tgt.spec_used ? c->h_small->map.guard : 0, c->src.spec_used ? c->h_small->scan.guard : 0);
    if (r < 0) return r;
  }
  if (whole_target) { int rc = complete_target(c); if (rc) return rc; }  // (lazy target: whoever comes this way reads covariances or voxels the solve may not have needed)
  return RGC_OK;
}

int need_inputs(rgc_ctx* c, bool validate) {
  if (!c) return RGC_ERR_INVALID;
  if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "source and target must be set first");
  if (validate) {
    int rc = validate_clouds(c);
    if (rc) return rc;
    if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "source and target must be set first");
  }
  return join_source(c);
}

void unpack_system(const double sums[28], double H[36], double b[6]) {
  int u = 0;
  for (int a = 0; a < 6; a++)
    for (int d = a; d < 6; d++) {
      H[a * 6 + d] = sums[u];
      H[d * 6 + a] = sums[u];
      u++;
    }
  for (int a = 0; a < 6; a++) b[a] = sums[21 + a];
}

// the scan linearised at T against the map's voxels, on the route the scan was prepared on: the 28 sums to d_out, the count to d_small->ncorr
// RGC_DIRECT_RADIUS: over the offset table, a group of lanes per source point (rgc_vgicp_radius.hip); the table goes to the device when it has
// changed since the last linearisation (in stream order on the context's stream: behind every launch that reads the former one)
static int enqueue_linearize(rgc_ctx* c, const double T[16], int noff, int want_H) {
  const Cloud& src = c->src;
  double* partials = c->partials.as<double>();
  int* ipartials = c->ipartials.as<int>();
  if (radius_method(c)) {
    const std::vector<int>& tab = radius_table(c);
    if (c->vr_offs_dirty || !c->vr_offs.p) {
      int rc = ensure(c, c->vr_offs, sizeof(int) * (size_t)kMaxNeighborOffsets);
      if (rc) return rc;
      // (the packed copy lives in the context: the asynchronous copy may read it after this call; every linearisation ends in a synchronisation
      // of the stream, so the next selection finds it read)
      c->vr_packed_h.resize((size_t)noff);
      for (int o = 0; o < noff; o++) c->vr_packed_h[o] = rgck::vgicp_radius_pack(tab[3 * o], tab[3 * o + 1], tab[3 * o + 2]);
      HIPCHK(c, hipMemcpyAsync(c->vr_offs.p, c->vr_packed_h.data(), sizeof(int) * (size_t)noff, hipMemcpyHostToDevice, c->stream));
      c->vr_offs_dirty = false;
    }
    const rgck::GicpCov A{src.general ? src.c6.as<const double>() : nullptr, src.nx.as<const double>(), src.ny.as<const double>(), src.nz.as<const double>()};
    rgck::vgicp_radius_linearize(c->stream, src.sorted(), A, pose_from(T), c->tgt.grid, c->tgt.voxels(), c->vr_offs.as<const int>(), noff, corr_of(c), want_H,
                                 partials, ipartials, c->d_out, &c->d_small->ncorr);
    return RGC_OK;
  }
  if (src.general)
    rgck::linearize_general(c->stream, src.sorted(), src.c6.as<double>(), pose_from(T), c->tgt.grid, c->tgt.voxels(), noff, corr_of(c), want_H, partials,
                            ipartials, c->d_out, &c->d_small->ncorr);
  else
    rgck::linearize(c->stream, src.sorted(), src.normals(), pose_from(T), c->tgt.grid, c->tgt.voxels(), noff, corr_of(c), want_H, partials, ipartials,
                    c->d_out, &c->d_small->ncorr);
  return RGC_OK;
}
// the first ndoubles of the output block, home (one synchronisation)
static int fetch_out(rgc_ctx* c, size_t ndoubles) {
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double) * ndoubles, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}
static int do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  int rc = need_inputs(c);
  if (rc) return rc;
  const int n = c->src.n, noff = noff_of(c);
  if ((rc = ensure_corr(c, n, noff, rgck::kAccum))) return rc;
  const int want = (H && b) ? 1 : 0;
  {
    ProfScope ps(c, RGC_K_LINEARIZE, n);
    if ((rc = enqueue_linearize(c, T, noff, want))) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double) * rgck::kAccum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&c->h_small->ncorr, &c->d_small->ncorr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  c->corr_noff = noff;
  c->corr_n = n;
  c->corr_valid = true;
  c->stats.n_corr = c->h_small->ncorr;
  c->stats.n_linearize++;
  if (want) unpack_system(c->h_out, H, b);
  if (cost) *cost = c->h_out[27];
  return RGC_OK;
}

// One enqueue per outer LM iteration: linearize at x0, fold, FIRST LM try on the device (solve, so3_exp, xi = delta*x0),
// compute_error at xi, fold -- then a single 57-double read-back.  lambda < 0: lambda = factor * max|H_ii| on the device.
static int do_linearize_try(rgc_ctx* c, const double x0[16], double lambda, double H[36], double b[6], double* y0, double d[6], double xi[16],
                     double* lambda_used, double* yi) {
  int rc = need_inputs(c);
  if (rc) return rc;
  const int n = c->src.n, noff = noff_of(c);
  if ((rc = ensure_corr(c, n, noff, rgck::kAccum))) return rc;
  rgck::LmIn in;
  for (int i = 0; i < 16; i++) in.x0[i] = x0[i];
  in.lambda = lambda;
  in.init_factor = c->prm.lm_init_lambda_factor;
  {
    ProfScope ps(c, RGC_K_LINEARIZE, n);
    if ((rc = enqueue_linearize(c, x0, noff, 1))) return rc;
    rgck::lm_try(c->stream, c->d_out, &c->d_small->ncorr, in);
  }
  {
    ProfScope ps(c, RGC_K_ERROR, n);
    rgck::compute_error_dev(c->stream, c->src.P.as<const float4>(), n, c->d_out + 38, c->tgt.vox.as<const double>(), noff, corr_of(c),
                            c->partials.as<double>(), c->d_out + 56);
  }
  if ((rc = fetch_out(c, 57))) return rc;
  c->corr_noff = noff;
  c->corr_n = n;
  c->corr_valid = true;
  c->stats.n_corr = (int)c->h_out[28];
  c->stats.n_linearize++;
  c->stats.n_error++;
  unpack_system(c->h_out, H, b);
  *y0 = c->h_out[27];
  for (int a = 0; a < 6; a++) d[a] = c->h_out[32 + a];
  for (int a = 0; a < 16; a++) xi[a] = c->h_out[38 + a];
  *lambda_used = c->h_out[54];
  *yi = c->h_out[56];
  return RGC_OK;
}

static int do_error(rgc_ctx* c, const double T[16], double* cost) {
  int rc = need_inputs(c);
  if (rc) return rc;
  if (!c->corr_valid) return fail(c, RGC_ERR_INVALID, "rgc_compute_error needs a preceding rgc_linearize");
  const int n = c->corr_n;
  {
    ProfScope ps(c, RGC_K_ERROR, n);
    rgck::compute_error(c->stream, c->src.P.as<const float4>(), n, pose_from(T), c->tgt.vox.as<const double>(), c->corr_noff, corr_of(c),
                        c->partials.as<double>(), c->d_out);
  }
  if ((rc = fetch_out(c, 1))) return rc;
  c->stats.n_error++;
  *cost = c->h_out[0];
  return RGC_OK;
}

int do_fitness(rgc_ctx* c, const float T[16], double* out) {
  int rc = need_inputs(c);
  if (rc) return rc;
  const int n = c->src.n;
  if ((rc = ensure(c, c->partials, sizeof(double) * (size_t)rgck::fitness_blocks(n) + 64))) return rc;
  {
    ProfScope ps(c, RGC_K_FITNESS, n);
    rgck::fitness(c->stream, c->src.P.as<const float4>(), n, posef_from(T), c->tgt.sorted(), c->partials.as<double>(), c->d_out, /*scan_small_map=*/true);
  }
  if ((rc = fetch_out(c, 1))) return rc;
  *out = c->h_out[0] / (double)n;
  return RGC_OK;
}

// ---- the measured grid of the clouds that are no VGICP target (rgc_ctx.h) ----
int build_measured_grid(rgc_ctx* c, Cloud& cl, double cell, int* dsm, int* hsm, bool with_voxels, const char* name, const char* grid_name) {
  const int n = cl.n;
  hipStream_t s = c->stream;
  int rc;
  const size_t words = with_voxels ? 8 : 7;  // bbox accumulators + flag (+ the voxel counter)
  const int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
  memcpy(hsm, init, sizeof(init));
  HIPCHK(c, hipMemcpyAsync(dsm, hsm, words * sizeof(int), hipMemcpyHostToDevice, s));
  rgck::bbox(s, cl.in, cl.stride_f, n, cell, dsm, dsm + 6);
  HIPCHK(c, hipMemcpyAsync(hsm, dsm, words * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (hsm[6]) return fail(c, RGC_ERR_NONFINITE, "%s contains non-finite or absurd coordinates", name);
  int minc[3], dim[3];
  double ncell = 1.0;
  for (int a = 0; a < 3; a++) {
    minc[a] = hsm[a];
    dim[a] = hsm[3 + a] - hsm[a] + 1;
    ncell *= (double)dim[a];
  }
  if (ncell > (double)c->prm.max_cells || ncell > 2.0e9) return fail(c, RGC_ERR_GRID_TOO_LARGE, "%s exceeds max_cells", grid_name);
  const rgck::Grid g = rgck::make_grid(minc, dim, cell);
  cl.grid = g;
  const size_t nc1 = (size_t)g.ncell + 1;
  if ((rc = ensure(c, cl.cell_of, sizeof(int) * n))) return rc;
  if ((rc = ensure(c, cl.slot_of, sizeof(int) * n))) return rc;
  if ((rc = ensure(c, cl.cnt, sizeof(int) * nc1 + 256))) return rc;
  if ((rc = ensure(c, cl.start, sizeof(int) * nc1))) return rc;
  if (with_voxels && (rc = ensure(c, cl.cell_voxel, sizeof(int) * nc1))) return rc;
  if ((rc = ensure(c, cl.block_sums, sizeof(long long) * (nc1 / 2048 + 2)))) return rc;
  if ((rc = ensure(c, cl.order_tmp, sizeof(long long) * n))) return rc;
  if ((rc = ensure(c, cl.P, sizeof(float4) * ((size_t)n + 4)))) return rc;
  HIPCHK(c, hipMemsetAsync(cl.cnt.p, 0, (sizeof(int) * nc1 + 255) & ~(size_t)255, s));
  rgck::count_cells(s, cl.in, cl.stride_f, n, g, cl.cell_of.as<int>(), cl.slot_of.as<int>(), cl.cnt.as<int>());
  rgck::scan_cells(s, cl.cnt.as<int>(), cl.start.as<int>(), (int)nc1, cl.block_sums.p, with_voxels ? cl.cell_voxel.as<int>() : nullptr, with_voxels ? dsm + 7 : nullptr);
  rgck::place(s, n, cl.cell_of.as<int>(), cl.slot_of.as<int>(), cl.start.as<int>(), cl.order_tmp.as<unsigned long long>());
  rgck::rank_gather(s, cl.in, cl.stride_f, n, cl.cell_of.as<int>(), cl.start.as<int>(), cl.order_tmp.as<unsigned long long>(), cl.P.as<float4>());
  return RGC_OK;
}

}  // namespace rgcapi

using namespace rgcapi;

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

void rgc_default_params(rgc_params* p) {
  if (!p) return;
  p->voxel_res = 1.0;
  p->max_iterations = 25;
  p->lm_max_iterations = 10;
  p->rotation_eps = 2e-3;
  p->translation_eps = 1e-6;
  p->lm_init_lambda_factor = 1e-9;
  p->k_correspondences = 20;
  p->neighbor_method = RGC_DIRECT1;
  p->max_cells = 1ll << 29;
}

const char* rgc_version(void) { return "rgc_hip 0.1 (gfx950)"; }

const char* rgc_status_string(int s) {
  switch (s) {
    case RGC_OK: return "ok";
    case RGC_ERR_INVALID: return "invalid argument";
    case RGC_ERR_HIP: return "HIP runtime error";
    case RGC_ERR_TOO_FEW_POINTS: return "too few points";
    case RGC_ERR_GRID_TOO_LARGE: return "grid too large";
    case RGC_ERR_NO_INPUT: return "no input cloud";
    case RGC_ERR_NONFINITE: return "non-finite input";
    case RGC_ERR_UNSUPPORTED: return "unsupported setting selected";
  }
  return "unknown";
}

int rgc_create(int hip_device, const rgc_params* params, rgc_ctx** out) {
  if (!out) return RGC_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipSetDevice(hip_device) != hipSuccess) return RGC_ERR_HIP;
  rgc_ctx* c = new (std::nothrow) rgc_ctx();
  if (!c) return RGC_ERR_HIP;
  c->device = hip_device;
  rgc_default_params(&c->prm);
  if (params) {
    int rc = check_params(c, params);
    if (rc) { delete c; return rc; }
    c->prm = *params;
  }
  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
  {  // the source's small kernels must not queue behind the map's 15k-wave kNN launch: highest stream priority
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    ok = ok && hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, hi) == hipSuccess;
  }
  ok = ok && hipEventCreateWithFlags(&c->lm_mid, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->src_in_ready, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->src_ready, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->main_mark, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->tgt_ready, kDevEvent) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->d_small, sizeof(rgck::SmallWords)) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->d_out, 64 * sizeof(double)) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->h_small, sizeof(rgck::SmallWords), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->h_out, 64 * sizeof(double), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->h_lm, sizeof(rgck::LmState), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->h_post, sizeof(rgck::LmState), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
  if (ok) {
    memset(c->h_post, 0, sizeof(rgck::LmState));
    if (hipHostGetDevicePointer((void**)&c->d_post, c->h_post, 0) != hipSuccess) c->d_post = nullptr;  // (no fast path then)
  }
  if (ok && hipHostMalloc((void**)&c->h_early, sizeof(rgck::LmEarly), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
    memset(c->h_early, 0, sizeof(rgck::LmEarly));
    if (hipHostGetDevicePointer((void**)&c->d_early, c->h_early, 0) != hipSuccess) c->d_early = nullptr;  // (no early pose then)
  }
  c->uid = g_next_uid.fetch_add(1);
  ok = ok && hipEventCreateWithFlags(&c->src_read_done, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->lm_tail, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->tgt_prepared, kDevEvent) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->vg.done, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->vg.h_res, 4 * sizeof(int), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->kfs.uploaded, hipEventDisableTiming) == hipSuccess;
  if (const char* e = getenv("RGC_SPEC_GRID")) c->spec_on = atoi(e) != 0;
  if (const char* e = getenv("RGC_KNN_SEEDS")) c->seeds_on = atoi(e) != 0;
  if (const char* e = getenv("RGC_KNN_CACHE")) c->cache_on = atoi(e) != 0;
  if (!c->seeds_on) c->cache_on = false;  // (the lists sit on top of the seeds)
  c->trace_cache = getenv("RGC_TRACE_CACHE") != nullptr;
  if (const char* e = getenv("RGC_CHECK_POINTERS")) c->check_ptrs = atoi(e) != 0;
  if (const char* e = getenv("RGC_FORCE_GENERAL")) c->force_general = atoi(e) != 0;
  c->test_fail_cache_alloc = getenv("RGC_TEST_FAIL_CACHE_ALLOC") != nullptr;
  if (const char* e = getenv("RGC_JOIN_SPIN_US")) c->join_spin_us = atoi(e);
  if (const char* e = getenv("RGC_PREP_EVENT_EXT")) c->prep_event_ext = atoi(e) != 0;
  if (const char* e = getenv("RGC_COOP_STREAM")) c->coop_stream_on = atoi(e) != 0;
  if (const char* e = getenv("RGC_VOXEL_IMPL")) c->voxel_impl = strcmp(e, "separate") == 0 ? 1 : (strcmp(e, "fused") == 0 ? 2 : 0);
  if (const char* e = getenv("RGC_LM_IMPL")) { c->lm_host = strcmp(e, "host") == 0; c->lm_chained = strcmp(e, "chained") == 0; }
  if (const char* e = getenv("RGC_LM_GIVE_UP_AT")) c->lm_give_up_at = atoi(e);
  if (hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess) c->cu_count = 0;
  if (!ok) { rgc_destroy(c); return RGC_ERR_HIP; }
  { std::lock_guard<std::mutex> lk(g_live_mutex); g_live.insert(c); }
  *out = c;
  return RGC_OK;
}

void rgc_destroy(rgc_ctx* c) {
  if (!c) return;
  { std::lock_guard<std::mutex> lk(g_live_mutex); g_live.erase(c); }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  prof_collect(c);
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  release_cloud(c->src);
  release_cloud(c->tgt);
  // the VGICP core, the one subsystem without a record (its two clouds above, the small words and mirrors below); everything else through its record
  for (DevBuf* b : {&c->corr_v, &c->corr_M, &c->corr_v2, &c->corr_M2, &c->partials, &c->ipartials, &c->scratch, &c->lm_state, &c->fit_partials, &c->vr_offs}) release(*b);
  if (c->d_small) (void)hipFree(c->d_small);
  if (c->d_out) (void)hipFree(c->d_out);
  if (c->h_small) (void)hipHostFree(c->h_small);
  if (c->h_out) (void)hipHostFree(c->h_out);
  if (c->h_lm) (void)hipHostFree(c->h_lm);
  if (c->h_post) (void)hipHostFree(c->h_post);
  if (c->h_early) (void)hipHostFree(c->h_early);
  if (c->vg.done) (void)hipEventDestroy(c->vg.done);
  release_record(c->mapreg);
  release_record(c->map);
  release_record(c->kfs);
  release_record(c->pgo);
  release_record(c->vg);
  release_record(c->fe);
  release_record(c->ndt);
  release_record(c->gicp_sums);
  release_record(c->gicp);
  release_record(c->gicp_st);
  release_record(c->gicp_mp);
  release_record(c->search);
  release_record(c->outlier);
  release_record(c->cluster);
  release_record(c->plane);
  release_record(c->normal);
  release_record(c->fpfh);
  if (c->kfs.uploaded) (void)hipEventDestroy(c->kfs.uploaded);
  if (c->src_ready) (void)hipEventDestroy(c->src_ready);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->main_mark) (void)hipEventDestroy(c->main_mark);
  if (c->tgt_ready) (void)hipEventDestroy(c->tgt_ready);
  if (c->src_read_done) (void)hipEventDestroy(c->src_read_done);
  if (c->lm_tail) (void)hipEventDestroy(c->lm_tail);
  if (c->lm_mid) (void)hipEventDestroy(c->lm_mid);
  if (c->src_in_ready) (void)hipEventDestroy(c->src_in_ready);
  if (c->tgt_prepared) (void)hipEventDestroy(c->tgt_prepared);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  delete c;
}

int rgc_set_params(rgc_ctx* c, const rgc_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  int rc = check_params(c, p);
  if (rc) return rc;
  const bool redo = p->voxel_res != c->prm.voxel_res || p->k_correspondences != c->prm.k_correspondences;
  if (redo && solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");  // (the clouds are prepared again below)
  // (away from RGC_DIRECT_RADIUS with its solved result waiting to be handed over: refused like rgc_set_neighbor_search)
  if (p->neighbor_method != c->prm.neighbor_method && radius_method(c) && solve_in_flight(c))
    return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (redo) HIPCHK(c, hipSetDevice(c->device));  // (the re-preparation launches kernels: like every entry point that does, whatever device the calling thread had current)
  if (p->voxel_res != c->prm.voxel_res) c->src_res_auto = 0.0;
  c->prm = *p;
  // The correspondences the last linearisation froze stay what rgc_compute_error uses (with their own offset count, corr_noff) unless the
  // clouds are prepared again: the reference's setters, setNeighborSearchMethod among them, leave voxel_correspondences_ alone.
  if (redo) drop_frozen(c);
  if (redo) {  // covariances / voxel map depend on these: recompute from the resident inputs
    if (c->tgt_owner) {
      // a BORROWED target (rgc_share_target) is the owner's, prepared under the owner's settings, and its input buffer is the owner's to
      // keep or free: nothing to recompute from here (tests/fuzz/fuzz_api.py: the re-preparation read an input the owner had long replaced --
      // a memory fault on the device).  The alias goes; share again once the owner holds a target under these settings.
      release_cloud(c->tgt);
      c->tgt.ready = false; c->tgt.n = 0; c->tgt.in = nullptr;
      c->tgt_owner = nullptr;
    }
    if (c->src.ready) { c->src.ready = false; if ((rc = prepare_cloud(c, c->src, false))) return rc; }
    if (c->tgt.ready) { c->tgt.ready = false; if ((rc = prepare_cloud(c, c->tgt, true))) return rc; }
  }
  return RGC_OK;
}

int rgc_get_params(const rgc_ctx* c, rgc_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  *p = c->prm;
  return RGC_OK;
}

// FastVGICPCuda::setNeighborSearchMethod(method, radius): fast_vgicp_cuda.hpp:60, impl/fast_vgicp_cuda_impl.hpp:58-61, fast_vgicp_cuda.cu:42-95
int rgc_set_neighbor_search(rgc_ctx* c, int method, double radius) {
  if (!c) return RGC_ERR_INVALID;
  if (method < RGC_DIRECT27 || method > RGC_DIRECT_RADIUS) return fail(c, RGC_ERR_INVALID, "rgc_set_neighbor_search: no neighbour method %d", method);
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (method == RGC_DIRECT_RADIUS) {
    if (!std::isfinite(radius) || radius < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_set_neighbor_search: RGC_DIRECT_RADIUS needs a finite radius >= 0");
    std::vector<int> offs;
    if (!neighbor_offsets_of(method, radius, offs))
      return fail(c, RGC_ERR_INVALID, "rgc_set_neighbor_search: radius %g has more than %d offsets", radius, kMaxNeighborOffsets);
    c->nbr_radius = radius;
    c->vr_offs_h.swap(offs);
    c->vr_offs_dirty = true;  // (uploaded by the next linearisation, in stream order)
  }
  // (the correspondences the last linearisation froze stay in force, with their own offset count: rgc_set_params' rule for a new method)
  c->prm.neighbor_method = method;
  return RGC_OK;
}

int rgc_get_neighbor_search(const rgc_ctx* c, int* method, double* radius) {
  if (!c || !method || !radius) return RGC_ERR_INVALID;
  *method = c->prm.neighbor_method;
  *radius = c->nbr_radius;
  return RGC_OK;
}

const char* rgc_last_error(const rgc_ctx* c) { return c ? c->err : "null context"; }

int rgc_set_target(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return c ? set_cloud(c, c->tgt, true, xyz, n, stride_bytes, false) : RGC_ERR_INVALID; }
int rgc_set_source(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return c ? set_cloud(c, c->src, false, xyz, n, stride_bytes, false) : RGC_ERR_INVALID; }
int rgc_set_target_device(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return c ? set_cloud(c, c->tgt, true, xyz, n, stride_bytes, true) : RGC_ERR_INVALID; }
int rgc_set_source_device(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return c ? set_cloud(c, c->src, false, xyz, n, stride_bytes, true) : RGC_ERR_INVALID; }

static int fetch_nvox(rgc_ctx* c);

// A second context registers scans to the SAME prepared target (a resident map) without preparing or copying it: its target
// becomes a non-owning alias of the owner's buffers.  What it is for: two contexts taking turns on a sequence whose map does not
// change from frame to frame -- the next scan is prepared on one while the current one is solved on the other (PipelinedVGICP).
int rgc_share_target(rgc_ctx* c, rgc_ctx* owner) {
  if (!c || !owner || c == owner) return RGC_ERR_INVALID;
  if (c->device != owner->device) return fail(c, RGC_ERR_INVALID, "rgc_share_target: the contexts are on different devices");
  if (c->lm_host || owner->lm_host) return fail(c, RGC_ERR_INVALID, "rgc_share_target is not available with RGC_LM_IMPL=host");
  if (!owner->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_share_target: the owner has no target");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_clouds(owner);  // a speculative grid the owner's target did not fit is resolved now (one synchronisation)
  if (rc) return fail(c, rc, "rgc_share_target: %s", owner->err);
  if (!owner->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_share_target: the owner has no target");
  if ((rc = fetch_nvox(owner))) return fail(c, rc, "rgc_share_target: %s", owner->err);
  HIPCHK(c, hipStreamSynchronize(owner->stream2));
  HIPCHK(c, hipStreamSynchronize(owner->stream));   // the target is complete in memory
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));       // nothing of this context still reads its old target
  Cloud& d = c->tgt;
  const Cloud& o = owner->tgt;
  release_cloud(d);
  const std::vector<DevBuf*> db = shared_bufs(d), ob = shared_bufs(owner->tgt);
  d.general = o.general;
  for (size_t k = 0; k < db.size(); k++) { db[k]->p = ob[k]->p; db[k]->cap = ob[k]->cap; db[k]->borrowed = ob[k]->p != nullptr; }
  d.in = o.in; d.stride_f = o.stride_f; d.n = o.n; d.grid = o.grid; d.grid = o.grid; d.nvox = o.nvox; d.deferred_seen = o.deferred_seen;
  d.spec_ok = false; d.spec_used = false; d.cnt_clean = 0; d.cnt_seen = nullptr; d.lazy = 0;
  d.ready = true;
  const int small[2] = {0, o.nvox};  // this context's copy of the target's guard (clear) and voxel count, which the solve reads
  static_assert(offsetof(rgck::SmallBlock, nvox) == offsetof(rgck::SmallBlock, guard) + sizeof(int), "guard and nvox in one copy");
  HIPCHK(c, hipMemcpyAsync(&c->d_small->map.guard, small, sizeof(small), hipMemcpyHostToDevice, c->stream));  // (not the blocking form: it goes through the NULL stream)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tgt_owner = owner;
  c->tgt_owner_gen = owner->tgt_generation;
  c->tgt_owner_uid = owner->uid;
  c->map.bound = false;
  drop_frozen(c);
  c->deferred_known = false;
  c->main_has_target_prep = false;
  c->stats.n_target = o.n; c->stats.target_cells = o.grid.ncell; c->stats.n_voxels = o.nvox;
  return RGC_OK;
}

// Two contexts taking turns on a DEPENDENT sequence (each frame's target is a function of the previous pose, RGC_odometer.cpp:1248-1256):
// the next scan can be prepared ahead -- it depends on no pose -- but enqueued beside the current frame's map preparation its small
// kernels share the chip with the 15 k-wave kNN launch the frame is waiting for (207 us instead of 155).  Held back until that
// preparation is done, they run under the current frame's SOLVE, a chain of short launches that leaves the chip mostly idle.
int rgc_set_target_lazy(rgc_ctx* c, int margin_cells) {
  if (!c) return RGC_ERR_INVALID;
  if (margin_cells < 0 || margin_cells > 16) return fail(c, RGC_ERR_INVALID, "rgc_set_target_lazy: margin_cells must be in [0, 16]");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  c->lazy_margin = margin_cells;  // (takes effect with the next target; one already set keeps the state it is in)
  return RGC_OK;
}

int rgc_set_regularization_method(rgc_ctx* c, int method) {
  if (!c) return RGC_ERR_INVALID;
  if (method < RGC_REG_NONE || method > RGC_REG_FROBENIUS) return fail(c, RGC_ERR_INVALID, "rgc_set_regularization_method: %d is not a RegularizationMethod", method);
  if (method != c->reg_method) {  // the covariances of the clouds set so far were computed under the other method (the reference computes them at align())
    if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
    c->src.ready = c->tgt.ready = false; drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  }
  c->reg_method = method;
  return RGC_OK;
}

int rgc_set_covariance_estimation(rgc_ctx* c, int method) {
  if (!c) return RGC_ERR_INVALID;
  if (method != RGC_COV_KNN && method != RGC_COV_RBF) return fail(c, RGC_ERR_INVALID, "rgc_set_covariance_estimation: %d is neither RGC_COV_KNN nor RGC_COV_RBF", method);
  if (method != c->cov_method) {  // the clouds' covariances were estimated the other way: the rule of rgc_set_regularization_method
    if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
    c->src.ready = c->tgt.ready = false; drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  }
  c->cov_method = method;
  return RGC_OK;
}

int rgc_get_covariance_estimation(const rgc_ctx* c, int* method) {
  if (!c || !method) return RGC_ERR_INVALID;
  *method = c->cov_method;
  return RGC_OK;
}

int rgc_set_rbf_kernel(rgc_ctx* c, double kernel_width, double max_dist) {
  if (!c) return RGC_ERR_INVALID;
  // the kernel computes with (float)kernel_width (covariance_estimation_rbf.cu:80): it must be a positive finite float as well
  if (!std::isfinite(kernel_width) || !(kernel_width > 0.0) || kernel_width > (double)FLT_MAX || !((float)kernel_width > 0.f))
    return fail(c, RGC_ERR_INVALID, "rgc_set_rbf_kernel: kernel_width must be finite and > 0");
  if (std::isnan(max_dist)) return fail(c, RGC_ERR_INVALID, "rgc_set_rbf_kernel: max_dist is not a number");
  if (max_dist <= 0.0) max_dist = 5.0 * kernel_width;  // fast_vgicp_cuda_impl.hpp:46-51
  if (c->cov_method == RGC_COV_RBF && (kernel_width != c->rbf_width || max_dist != c->rbf_max_dist)) {
    if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
    c->src.ready = c->tgt.ready = false; drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  }
  c->rbf_width = kernel_width;
  c->rbf_max_dist = max_dist;
  return RGC_OK;
}

int rgc_get_rbf_kernel(const rgc_ctx* c, double* kernel_width, double* max_dist) {
  if (!c || !kernel_width || !max_dist) return RGC_ERR_INVALID;
  *kernel_width = c->rbf_width;
  *max_dist = c->rbf_max_dist;
  return RGC_OK;
}

int rgc_set_voxel_accumulation_mode(rgc_ctx* c, int mode) {
  if (!c) return RGC_ERR_INVALID;
  if (mode < RGC_VOXEL_ADDITIVE || mode > RGC_VOXEL_MULTIPLICATIVE) return fail(c, RGC_ERR_INVALID, "rgc_set_voxel_accumulation_mode: %d is not a VoxelAccumulationMode", mode);
  const bool was = c->voxel_mode == RGC_VOXEL_MULTIPLICATIVE, is = mode == RGC_VOXEL_MULTIPLICATIVE;
  if (was != is) {  // (ADDITIVE <-> ADDITIVE_WEIGHTED changes nothing: one voxel class in the vendored FastVGICP, fast_vgicp_voxel.hpp:137-141)
    if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
    c->src.ready = c->tgt.ready = false; drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  }
  c->voxel_mode = mode;
  return RGC_OK;
}

int rgc_set_knn_reuse(rgc_ctx* c, int mode) {
  if (!c) return RGC_ERR_INVALID;
  if (mode < RGC_REUSE_NONE || mode > RGC_REUSE_LISTS) return fail(c, RGC_ERR_INVALID, "rgc_set_knn_reuse: mode must be RGC_REUSE_NONE, _SEEDS or _LISTS");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  const bool seeds = mode >= RGC_REUSE_SEEDS && RGC_KNN_SEEDS != 0, lists = seeds && mode >= RGC_REUSE_LISTS && RGC_KNN_CACHE != 0;
  Cloud& cl = c->tgt;
  if ((!lists && cl.nbr.p) || (!seeds && cl.seed.p)) {  // buffers this context no longer needs: nothing may still be reading them
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
  }
  if (!lists) {
    for (DevBuf* b : {&cl.nbr, &cl.pos_of, &cl.rank_of, &cl.qrank, &cl.map_copy, &cl.todo, &cl.cache_small}) release(*b);
    cl.cache_on = cl.cache_live = cl.cache_searched_lists = false;
    cl.rf.copy = nullptr; cl.rf.epoch = nullptr;
  }
  if (!seeds) {
    release(cl.seed);
    cl.seed_key = nullptr; cl.seed_n = 0;
    cl.seed_on = cl.seed_warm = false;
  }
  c->seeds_on = seeds;
  c->cache_on = lists;
  c->cache_dropped = false;
  return RGC_OK;
}

int rgc_get_knn_reuse(const rgc_ctx* c, int* mode) {
  if (!c || !mode) return RGC_ERR_INVALID;
  *mode = !c->seeds_on ? RGC_REUSE_NONE : (c->cache_on ? RGC_REUSE_LISTS : RGC_REUSE_SEEDS);
  return RGC_OK;
}

int rgc_hold_source_until_target_of(rgc_ctx* c, rgc_ctx* other) {
  if (!c || !other) return RGC_ERR_INVALID;
  // (the other context must be alive while its event is handed to the runtime: checked and used under the registry's lock)
  std::lock_guard<std::mutex> lk(g_live_mutex);
  if (!g_live.count(other)) return fail(c, RGC_ERR_INVALID, "rgc_hold_source_until_target_of: the other context has been destroyed");
  if (c->device != other->device) return fail(c, RGC_ERR_INVALID, "rgc_hold_source_until_target_of: the contexts are on different devices");
  HIPCHK(c, hipSetDevice(c->device));
  // the scan's stream waits for the end of other's latest target preparation (a wait on an event nobody recorded yet is no wait)
  HIPCHK(c, hipStreamWaitEvent(c->stream2, other->tgt_prepared, 0));
  c->src_hold_pending = true;  // (a pipelined sequence: the scan set next is not prepared beside this context's own map's search, cloud_covariances)
  return RGC_OK;
}

int rgc_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  return do_linearize(c, T, H, b, cost);
}

int rgc_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  return do_error(c, T, cost);
}

int rgc_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  if (!c->corr_valid) return fail(c, RGC_ERR_INVALID, "no linearisation yet");
  *n = c->stats.n_corr;
  return RGC_OK;
}

// The solve's launches, enqueued and not waited for: the one resident launch (k_lm_solve) where that route is taken (`open` only: it runs a
// solve from its opening to its posted result), otherwise one batch of blind LM steps (the first launch of a solve opens it), the fitness
// kernel behind them and the state's read-back.
static int lm_enqueue_batch(rgc_ctx* c, int batch, const rgck::LmInit* open, bool want_fitness) {
  const int n = c->src.n, noff = noff_of(c), nb_lm = rgck::linearize_blocks(n);
  hipStream_t s = c->solve_stream;  // see rgc_align_begin
  rgck::LmState* post = (c->post_on && c->d_post) ? c->d_post : nullptr;
  const int seq = want_fitness ? -c->lm_seq : c->lm_seq;  // what is posted: a finished state (> 0), or a finished state with its score (< 0)
  constexpr int kSpare = 3;
  // the stage-by-stage pass (events around the solve's regions) keeps the two apart: all steps, then the score
  const bool staged = profiled(c, RGC_K_LINEARIZE) || profiled(c, RGC_K_FITNESS);
  // The score is chained INTO the steps: the launch whose decision ends the solve scores the final pose and posts the result (k_lm_step).
  // No separate score launches, no blind steps between the deciding launch and the score.
  const bool fit_in_steps = want_fitness && !staged;
  if (open) c->lm_j = 0;
  // The whole solve as ONE resident launch (k_lm_solve) wherever it has no more workgroups than the device has CUs and the result is posted; the
  // chained launches otherwise: the stage-by-stage profiling pass, a scan of more rows than CUs, a context without mapped host memory, and
  // RGC_LM_IMPL=chained -- and for any solve whose resident launch gave up (rgc_align_end).
  c->lm_resident = open && !staged && !c->lm_chained && post && nb_lm <= c->cu_count && nb_lm <= rgck::kLmSolveMaxGroups;
  rgck::LmArea* area = c->lm_state.as<rgck::LmArea>();
  const bool lazy = c->tgt.lazy == 2;
  rgck::LmArgs a{};
  a.src = c->src.sorted(); a.nrm = c->src.normals(); a.tgt = c->tgt.sorted(); a.vm = c->tgt.voxels();
  a.noff = noff; a.corr[0] = corr_of(c); a.corr[1] = rgck::Corr{c->corr_v2.as<int>(), c->corr_M2.as<double>()};
  a.partials = c->partials.as<double>(); a.area = area; a.small = c->d_small; a.segs_t = c->tgt.segs.p; a.segs_s = c->src.segs.p;
  a.h_post = post; a.seq = seq; a.fit_partials = fit_in_steps ? c->fit_partials.as<double>() : nullptr;
  a.lazy_need = lazy ? c->tgt.need.as<const int>() : nullptr; a.lazy_stamp = c->tgt.need_stamp; a.lazy_counts = lazy ? c->tgt.segs.as<const int>() + 1 : nullptr;
  a.h_early = (fit_in_steps && post) ? c->d_early : nullptr;
  if (c->lm_resident) {
    rgck::lm_solve_resident(s, a, *open, c->lm_give_up_at);
    c->lm_j = 1;  // the finished state is image 0
    HIPCHK(c, hipEventRecord(c->lm_tail, s));
    c->lm_tail_stream = s;
    return RGC_OK;
  }
  auto step = [&](const rgck::LmInit* op, hipStream_t on) { rgck::lm_step(on, a, c->lm_j++, op); };
  auto score = [&]() {  // getFitnessScore at the final pose, chained blindly (on the image the last launch left)
    rgck::fitness_lm(s, a.src, rgck::lm_image(area, c->lm_j - 1), a.tgt, c->fit_partials.as<double>(), post, c->lm_seq);
  };
  hipStream_t tail = s;
  if (staged) {
    {
      ProfScope ps(c, RGC_K_LINEARIZE, (long long)n * batch, s);
      for (int k = 0; k < batch; k++) { step(open, s); open = nullptr; }
    }
    if (want_fitness) {
      ProfScope ps(c, RGC_K_FITNESS, n, s);
      score();
    }
  } else {
    // The launches a solve is EXPECTED to need go to the solve's stream; the spare ones -- enqueued blind in case it needs more: each costs
    // ~5 us of its stream's time even when it finds the solve finished -- go to the context's OTHER stream behind an event, where they
    // drain beside whatever the caller enqueues next on the solve's stream (the next frame's map preparation) instead of in front of it.
    // (Not a third stream: two contexts with three streams each outnumber the hardware queues, and streams that share a queue serialise --
    // the two-context sequence lost 130 us per frame that way.)
    const int spare = batch > kSpare + 1 ? kSpare : 0;
    hipStream_t other = s == c->stream ? c->stream2 : c->stream;
    for (int k = 0; k < batch - spare; k++) { step(open, s); open = nullptr; }
    if (spare > 0) {
      HIPCHK(c, hipEventRecord(c->lm_mid, s));
      HIPCHK(c, hipStreamWaitEvent(other, c->lm_mid, 0));
      for (int k = 0; k < spare; k++) step(nullptr, other);
      tail = other;
    }
  }
  // (a solve that POSTS its finished state needs no stream-ordered copy of it: the one case that reads the state otherwise -- a batch that
  // ends without a finished solve -- fetches it with a blocking copy once the stream has drained, rgc_align_end)
  if (!post) HIPCHK(c, hipMemcpyAsync(c->h_lm, rgck::lm_image(area, c->lm_j - 1), sizeof(rgck::LmState), hipMemcpyDeviceToHost, tail));
  HIPCHK(c, hipEventRecord(c->lm_tail, tail));
  c->lm_tail_stream = tail;
  return RGC_OK;
}

// The solve in two halves, so that a caller with two contexts can prepare the clouds of the next frame (on the other context)
// while this one's LM runs: rgc_align_begin enqueues the device-chained LM behind the clouds' preparation and returns;
// rgc_align_end waits for it (and enqueues further batches if the solve needs more than six outer iterations).
int rgc_align_begin(rgc_ctx* c, const float guess[16], int want_fitness) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (general_route(c) || radius_method(c)) {  // no asynchronous form on the general route or under RGC_DIRECT_RADIUS: the solve runs now, rgc_align_end hands its result over
    auto& g = c->gen_res;
    g.on = false;
    g.rc = rgc_align(c, guess, g.T, g.H, want_fitness ? &g.fitness : nullptr, &g.iterations, &g.converged, &g.lm_failed);
    if (g.rc) return g.rc;
    g.has_fit = want_fitness != 0;
    g.on = true;
    return RGC_OK;
  }
  if (c->lm_host) return fail(c, RGC_ERR_INVALID, "the host-driven LM loop (RGC_LM_IMPL=host) has no asynchronous form");
  HIPCHK(c, hipSetDevice(c->device));
  c->pend.active = false;
  // the guards of speculative grids come home with the LM state: no synchronisation here
  if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "source and target must be set first");
  { int rc = check_target_owner(c); if (rc) return rc; }
  if (c->tgt.lazy == 1) { int rc = lazy_build(c, guess); if (rc) return rc; }        // lazy target: built where this solve can look
  else if (c->tgt.lazy == 2) { int rc = complete_target(c); if (rc) return rc; }      // ... a second solve on the same target: all of it
  // The solve is a chain of short launches: it runs on the HIGH-PRIORITY stream -- the one the scan was prepared on, so it is already
  // behind that -- ordered after the map's preparation on the main stream by one event.  With a second context preparing the next
  // frame's map meanwhile (15 k waves that fill every CU), the dispatcher places the solve's ~100 workgroups as soon as slots free up
  // instead of behind that launch.
  int rc;
  bool join_late = false;
  if (c->solve_behind_map && c->main_has_target_prep && !map_prep_finished(c)) {
    // the map is still being prepared (a dependent sequence: it could only start when the previous pose was known): the solve goes
    // directly behind it on the main stream -- a dependency that resolves across streams costs ~10 us on this runtime, and the scan's
    // preparation, which the solve also waits for, has long finished
    c->solve_stream = c->stream;
    join_late = true;  // (join_source may wait on the host for an almost-ready scan: done last, right in front of the first launch)
  } else {
    c->solve_stream = c->stream2;
    HIPCHK(c, hipEventRecord(c->tgt_ready, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->tgt_ready, 0));
  }
  // rgc_align_end returns as soon as the device POSTS the finished state: the previous solve's spare steps, score launches and the copy
  // into h_lm may still be queued on the stream they were enqueued on.  A solve that goes to the other stream is ordered behind them
  // (they work on the same LM state images and rows); a wait on an event that has already fired costs nothing.
  if (c->lm_tail_stream && c->lm_tail_stream != c->solve_stream && hipEventQuery(c->lm_tail) != hipSuccess) {
    (void)hipGetLastError();
    HIPCHK(c, hipStreamWaitEvent(c->solve_stream, c->lm_tail, 0));
  }
  const rgc_params& P = c->prm;
  // device-chained LM: the loop of :65-75 / :125-172 runs as a state machine on the device (k_lm_step);
  // the host only enqueues slots and reads the state back once per batch.
  const int n = c->src.n, noff = noff_of(c);
  if ((rc = ensure_corr(c, n, noff, (rgck::kAccum + 2) * 2))) return rc;  // (two halves of kAccum + 2 doubles per workgroup: rgck::LmArgs)
  if ((rc = ensure(c, c->corr_v2, sizeof(int) * (size_t)n * noff))) return rc;
  if ((rc = ensure(c, c->corr_M2, sizeof(double) * 6 * (size_t)n * noff))) return rc;
  if (!c->lm_state.p) {
    if ((rc = ensure(c, c->lm_state, rgck::kLmAreaBytes))) return rc;
    // the score's ticket, the lazy target's miss flag and the resident solve's flags and give-up word start at 0
    HIPCHK(c, hipMemsetAsync(c->lm_state.p, 0, rgck::kLmAreaBytes, c->solve_stream));
  }
  if ((rc = ensure(c, c->fit_partials, sizeof(double) * (size_t)rgck::fitness_blocks(n) + 64))) return rc;
  rgck::LmInit in;
  for (int i = 0; i < 12; i++) in.x0[i] = (double)guess[i];
  in.x0[12] = in.x0[13] = in.x0[14] = 0.0;
  in.x0[15] = 1.0;
  in.rot_eps = P.rotation_eps; in.trans_eps = P.translation_eps; in.init_factor = P.lm_init_lambda_factor;
  in.max_outer = P.max_iterations; in.max_inner = P.lm_max_iterations;
  c->stats.n_linearize = c->stats.n_error = c->stats.outer_iterations = 0;
  // The launches are enqueued blind: enough for the outer iterations the PREVIOUS solve on this context took (consecutive frames of a
  // sequence need about the same number; a launch on a finished solve costs ~5 us of its stream's time, a read-back and a second batch
  // ~40), at least the six that cover a tracking frame, at most what max_iterations allows.
  // (a solve of o outer iterations without a rejected try needs o + 2 launches: the opening linearisation, one per try, and the one
  // whose decision ends it and scores the pose.  That many plus one stay on the solve's stream -- a launch too many there costs ~5 us in
  // front of the next frame, one too few a ~13 us hop to the other stream --, three more go aside as spares: lm_enqueue_batch)
  const int batch = std::max(2, std::min(std::max(9, c->lm_last_outer + 6), P.max_iterations + 2));
  if (c->lm_seq >= 0x3fffffff) {  // the solve numbers start over: neither a flag of the resident solve nor its give-up word may carry an old one (rgck::k_lm_solve)
    c->lm_seq = 0;
    HIPCHK(c, hipMemsetAsync(&c->lm_state.as<rgck::LmArea>()->give_up, 0, sizeof(rgck::LmArea) - offsetof(rgck::LmArea, give_up), c->solve_stream));
  }
  c->lm_seq++;
  if (join_late && (rc = join_source(c))) return rc;
  if ((rc = lm_enqueue_batch(c, batch, &in, want_fitness != 0))) return rc;
  c->pend.in = in;
  c->pend.batch = batch;
  memcpy(c->pend.guess, guess, sizeof(c->pend.guess));
  c->pend.want_fitness = want_fitness != 0;
  c->pend.active = true;
  return RGC_OK;
}

// ---- rgc_align_end, step by step ----
struct AlignOut { float* T; double* H; double* fitness; int *iterations, *converged, *lm_failed; };  // rgc_align_end's outputs, each nullable

// the general route solved in rgc_align_begin: its stored result is handed over
static int take_general_result(rgc_ctx* c, const AlignOut& out) {
  auto& g = c->gen_res;
  g.on = false;
  if (out.T) memcpy(out.T, g.T, sizeof(g.T));
  if (out.H) memcpy(out.H, g.H, sizeof(g.H));
  if (out.iterations) *out.iterations = g.iterations;
  if (out.converged) *out.converged = g.converged;
  if (out.lm_failed) *out.lm_failed = g.lm_failed;
  if (out.fitness) { if (g.has_fit) *out.fitness = g.fitness; else return do_fitness(c, g.T, out.fitness); }
  return RGC_OK;
}

// S <- the finished state of the pending solve, enqueueing whatever it still needs to finish
static int lm_wait_result(rgc_ctx* c, bool want_fitness, rgck::LmState& S) {
  int rc;
  for (int guard = 0;; guard++) {
    // The device posts a finished solve's state into mapped host memory and then the solve's number: the host spins on that word and
    // leaves as soon as it shows up -- the blind launches behind the deciding one and the stream's copy drain in the background.
    // A batch that ends without a finished solve shows up as a drained stream: then the copy has landed and more launches are enqueued.
    bool posted = false;
    if (c->post_on && c->d_post) {
      volatile int* gen = &c->h_post->gen;
      for (unsigned spin = 0;; spin++) {
        if (*gen == c->lm_seq) { posted = true; break; }
        if (spin & 31u) continue;  // the posted word is the usual way out: look at it often, at the event now and then
        const hipError_t q = hipEventQuery(c->lm_tail);  // (recorded behind the batch's last launch and its copy of the state, on whichever stream they went to)
        if (q == hipSuccess) { posted = *gen == c->lm_seq; break; }
        if (q != hipErrorNotReady) return fail(c, RGC_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        (void)hipGetLastError();
      }
      if (posted) {
        std::atomic_thread_fence(std::memory_order_acquire);
        memcpy(&S, c->h_post, sizeof(S));
      }
    }
    if (!posted && c->lm_resident) {
      // The resident launch has left without a result: a wait of one of its workgroups ran out (or RGC_LM_GIVE_UP_AT).  It touched nothing
      // but its own rows, flags and correspondence buffers -- the frame's counters are put back by the workgroup that FINISHES a solve -- so
      // the same solve, from its opening and with the same LmInit, goes out as chained launches: the same result, one frame's time later.
      HIPCHK(c, hipStreamSynchronize(c->lm_tail_stream));
      c->stats.lm_fallbacks++;
      c->lm_resident = false;
      const bool keep = c->lm_chained;
      c->lm_chained = true;
      // (workgroups that had reached the score before the others gave up have taken tickets nobody collected)
      HIPCHK(c, hipMemsetAsync(&c->lm_state.as<rgck::LmArea>()->ticket, 0, sizeof(rgck::LmArea::ticket), c->solve_stream));
      rc = lm_enqueue_batch(c, c->pend.batch, &c->pend.in, want_fitness);
      c->lm_chained = keep;
      if (rc) return rc;
      continue;
    }
    if (!posted) {
      HIPCHK(c, hipStreamSynchronize(c->lm_tail_stream));
      if (c->post_on && c->d_post) {  // (no copy was chained)
        // on the solve's own stream, never with the blocking hipMemcpy: that one goes through the NULL stream, whose hardware queue the
        // runtime creates at its first use -- 9 ms inside whichever frame first needed more launches than its batch held (the node's
        // "one slow frame" of rounds 3 and 4: frame 14 of the c2 stand-in)
        HIPCHK(c, hipMemcpyAsync(c->h_lm, rgck::lm_image(c->lm_state.as<rgck::LmArea>(), c->lm_j - 1), sizeof(rgck::LmState), hipMemcpyDeviceToHost,
                                 c->lm_tail_stream));
        HIPCHK(c, hipStreamSynchronize(c->lm_tail_stream));
      }
      memcpy(&S, c->h_lm, sizeof(S));
    }
    HIPCHK(c, hipGetLastError());
    if (S.done || guard >= 400) return RGC_OK;
    // a solve that is still running after six outer iterations usually runs many more (up to 25): batches of six, fewer read-backs
    if ((rc = lm_enqueue_batch(c, 6, nullptr, want_fitness))) return rc;
  }
}

// what the finished state carries home beside the pose: the valid correspondence buffer, the frame's counters, the sizes of the next launches
static void lm_adopt_result(rgc_ctx* c, const rgck::LmState& S) {
  const int n = c->src.n, noff = noff_of(c);
  if (S.cur) { std::swap(c->corr_v, c->corr_v2); std::swap(c->corr_M, c->corr_M2); }  // corr_v / corr_M = the valid buffer
  c->corr_noff = noff; c->corr_n = n; c->corr_valid = S.n_lin > 0;
  c->stats.n_corr = S.ncorr; c->stats.n_linearize = S.n_lin; c->stats.n_error = S.n_err;
  c->tgt.nvox = c->stats.n_voxels = S.nvox;
  c->stats.deferred_target = S.def_t; c->stats.deferred_source = S.def_s;
  c->tgt.deferred_seen = S.def_t; c->src.deferred_seen = S.def_s;
  c->deferred_known = true;
  if (c->tgt.lazy == 2) { c->tgt.lazy_nq_seen = S.lazy_nq; c->tgt.lazy_ncell_seen = S.lazy_ncell; }
  // (S.src_sq == 0: this scan's figure was consumed by an earlier solve on the same clouds -- the first step hands the counter back
  // zeroed -- and the steering it caused stands)
  if (S.src_sq > 0.f) c->stats.source_crowding = c->src.n > 0 ? (double)S.src_sq / (double)c->src.n : 0.0;
  c->lm_last_outer = S.outer;
  c->stats.outer_iterations = S.failed ? S.outer + 1 : S.outer;  // iterations started, like nr_iterations_ + 1
}

static void steer_scan_cell(rgc_ctx* c, const rgck::LmState& S) {
  // steer the next scan's cell size: halve above 500 points per own cell, double below 40 -- up to twice the voxel size, which is where a
  // 0.2 m leaf-filtered VLP-16 sweep (the odometer's source cloud) ends up: fewer of its far-field queries go to the cooperative
  // kernel (frame body 0.76 -> 0.73 ms); a raw VLP-16 sweep (117) stays at the voxel size (2837 scans/s against 2683 at twice that).
  // (With four lanes per query a crowded cell is
  // cheap and a fine grid's far field -- every sparse query deferred to the cooperative kernel -- is what costs: an HDL-64 sweep,
  // 1270 / 380 / 107 at 1 / 0.5 / 0.25 m, is fastest at 0.5 m (c3 529 -> 594 scans/s against the former threshold of 300, which took it
  // to 0.25 m); two fused 64-beam sweeps, 2420 / 720 / 201, still want 0.25 m (184 against 139 scans/s at 0.5 m).)
  if (S.src_sq > 0.f && c->src_res <= 0.0 && c->src.n > 0) {
    const double cur = c->src.grid.res, crowd = c->stats.source_crowding;
    double next = cur;
    if (crowd > 500.0 && cur > 0.26 * c->prm.voxel_res) next = cur * 0.5;
    else if (crowd < 40.0 && cur < 2.0 * c->prm.voxel_res) next = std::fmin(cur * 2.0, 2.0 * c->prm.voxel_res);  // a leaf-filtered sweep: 2 x voxel size
    c->src_res_auto = next;
  }
}

static int lm_write_outputs(rgc_ctx* c, const rgck::LmState& S, bool want_fitness, const AlignOut& out) {
  float fin[16];
  for (int i = 0; i < 16; i++) fin[i] = (float)S.x0[i];  // :77
  if (out.T) memcpy(out.T, fin, sizeof(fin));
  if (out.H) memcpy(out.H, S.Hfin, sizeof(double) * 36);
  if (out.iterations) *out.iterations = c->stats.outer_iterations;
  if (out.converged) *out.converged = S.conv != 0 ? 1 : 0;
  if (out.lm_failed) *out.lm_failed = S.failed != 0 ? 1 : 0;
  if (out.fitness) {
    if (want_fitness && S.has_fit) *out.fitness = S.fit_sum / (double)c->src.n;
    else return do_fitness(c, fin, out.fitness);
  }
  return RGC_OK;
}

int rgc_align_end(rgc_ctx* c, float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));  // (before the general route's score, too)
  const AlignOut out{final_T, final_H, fitness, iterations, converged, lm_failed};
  if (c->gen_res.on) return take_general_result(c, out);
  if (!c->pend.active) return fail(c, RGC_ERR_INVALID, "rgc_align_end without rgc_align_begin");
  c->pend.active = false;
  int rc;
  const bool want_fitness = c->pend.want_fitness;
  rgck::LmState& S = c->lm_res;  // (not h_lm itself: the stream's copy into it may still be in flight when a posted state is taken)
  if ((rc = lm_wait_result(c, want_fitness, S))) return rc;
  c->src_pending = false;  // the solve came after the scan's preparation and has finished (its spare launches may still drain: lm_tail)
  c->main_has_target_prep = false;  // (the solve came after the map's preparation)
  c->small_clean[0] = c->small_clean[1] = true;  // the solve re-initialised both blocks after capturing them (chained: its first step; resident: the workgroup that finished it)
  auto solve_again = [&]() {  // from the same guess (a copy: rgc_align_begin writes c->pend)
    float guess[16];
    memcpy(guess, c->pend.guess, sizeof(guess));
    return rgc_align(c, guess, final_T, final_H, fitness, iterations, converged, lm_failed);
  };
  {  // a cloud that did not fit its speculative grid: everything above ran on a parked cloud -- prepare it properly, solve again
    const int r = resolve_guards(c, S.pad & 0xff, (S.pad >> 8) & 0xff);
    if (r < 0) return r;
    if (r > 0) return solve_again();
  }
  if (c->tgt.lazy == 2 && S.pad2) {
    // lazy target: a look-up landed on an occupied voxel outside the part that was built (the pose moved further from the guess than the
    // margin covers).  The map is completed and the solve repeated from the same guess: the full build's result, bit for bit.
    c->stats.lazy_misses++;
    if ((rc = complete_target(c))) return rc;
    return solve_again();
  }
  lm_adopt_result(c, S);
  steer_scan_cell(c, S);
  return lm_write_outputs(c, S, want_fitness, out);
}

// lsq_registration_impl.hpp:53-79 (computeTransformation) + :125-172 (step_lm); SURVEY A.5
int rgc_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations,
              int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (!c->lm_host && !general_route(c) && !radius_method(c)) {
    const int rc0 = rgc_align_begin(c, guess, fitness != nullptr);
    return rc0 ? rc0 : rgc_align_end(c, final_T, final_H, fitness, iterations, converged, lm_failed);
  }
  // (the general covariance route solves here as well: the device-chained driver's step kernel takes the source's NORMAL; and RGC_DIRECT_RADIUS,
  // whose linearisation is a launch of its own over the offset table -- 19 to 485 look-ups per point: the hand-offs the device LM hides do not dominate)
  // ---- RGC_LM_IMPL=host: the shared host driver (rgc_api_lsq.hip) over the public fine-seam kernels, the first try of every outer
  // iteration on the device (do_linearize_try) -- a cross-check of the device-chained driver ----
  HIPCHK(c, hipSetDevice(c->device));
  int rc = need_inputs(c, /*validate=*/true);
  if (rc) return rc;
  c->stats.n_linearize = c->stats.n_error = c->stats.outer_iterations = 0;
  static const LmSystem sys = {nullptr, do_error, do_linearize_try, nullptr};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  c->stats.outer_iterations = r.iters;
  r.write(final_T, final_H, iterations, converged, lm_failed);
  if (fitness && (rc = do_fitness(c, r.fin, fitness))) return rc;
  return RGC_OK;
}

int rgc_fitness(rgc_ctx* c, const float T[16], double* fitness) {
  if (!c || !T || !fitness) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  return do_fitness(c, T, fitness);
}

int rgc_get_aligned_device(rgc_ctx* c, const float T[16], float* d_out, int stride_bytes) {
  if (!c || !T || !d_out) return RGC_ERR_INVALID;
  if (!c->src.ready) return fail(c, RGC_ERR_NO_INPUT, "source not set");
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "bad stride");
  { int rk = check_device_range(c, d_out, record_bytes(c->src.n, stride_bytes, false), "rgc_get_aligned_device: d_out"); if (rk) return rk; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = join_source(c);
  if (rc) return rc;
  rgck::transform_f32(c->stream, c->src.in, c->src.stride_f, c->src.n, posef_from(T), d_out, stride_bytes / 4);
  // the kernel reads the source's input buffer on the MAIN stream and nothing here waits for it: the next host source is copied into
  // that buffer on the scan's stream, which must queue behind this read (set_cloud)
  HIPCHK(c, hipEventRecord(c->src_read_done, c->stream));
  c->src_read_pending = true;
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

int rgc_get_aligned(rgc_ctx* c, const float T[16], float* out, int stride_bytes) {
  if (!c || !T || !out) return RGC_ERR_INVALID;
  if (!c->src.ready) return fail(c, RGC_ERR_NO_INPUT, "source not set");
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "bad stride");
  HIPCHK(c, hipSetDevice(c->device));
  const int n = c->src.n;
  int rc = join_source(c);
  if (rc) return rc;
  if ((rc = ensure(c, c->scratch, sizeof(float) * 3 * (size_t)n))) return rc;
  rgck::transform_f32(c->stream, c->src.in, c->src.stride_f, n, posef_from(T), c->scratch.as<float>(), 3);
  if (stride_bytes == 12) {
    HIPCHK(c, hipMemcpyAsync(out, c->scratch.p, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  } else {
    HIPCHK(c, hipMemcpy2DAsync(out, stride_bytes, c->scratch.p, 12, 12, n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RGC_OK;
}

static int get_covs(rgc_ctx* c, Cloud& cl, double* cov9, double* normals) {
  if (!cl.ready) return fail(c, RGC_ERR_NO_INPUT, "cloud not set");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_clouds(c);
  if (rc) return rc;
  if (!cl.ready) return fail(c, RGC_ERR_NO_INPUT, "cloud not set");
  const int n = cl.n;
  if ((rc = join_source(c))) return rc;
  if (cl.general) {  // the general route keeps a 3x3 per point, no normal
    if (normals) return fail(c, RGC_ERR_UNSUPPORTED, "normals exist only under RegularizationMethod PLANE with an additive voxel mode");
    if (!cov9) return RGC_OK;
    if ((rc = ensure(c, c->scratch, sizeof(double) * 9 * (size_t)n))) return rc;
    rgck::unsort6(c->stream, cl.c6.as<double>(), cl.P.as<float4>(), n, c->scratch.as<double>());
    HIPCHK(c, hipMemcpyAsync(cov9, c->scratch.p, sizeof(double) * 9 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RGC_OK;
  }
  if ((rc = ensure(c, c->scratch, sizeof(double) * 3 * (size_t)n))) return rc;
  rgck::unsort3(c->stream, cl.nx.as<double>(), cl.ny.as<double>(), cl.nz.as<double>(), cl.P.as<float4>(), n, c->scratch.as<double>());
  std::vector<double> tmp;
  double* dst = normals;
  if (!dst) { tmp.resize((size_t)n * 3); dst = tmp.data(); }
  HIPCHK(c, hipMemcpyAsync(dst, c->scratch.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (cov9) {
    for (int i = 0; i < n; i++) {  // C = I - 0.999 n n^T  (fast_gicp_impl.hpp:281,293)
      const double* v = dst + (size_t)i * 3;
      double* C = cov9 + (size_t)i * 9;
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) C[a * 3 + b] = (a == b ? 1.0 : 0.0) - 0.999 * v[a] * v[b];
    }
  }
  return RGC_OK;
}

int rgc_get_source_covariances(rgc_ctx* c, double* cov9, double* normals) { return c ? get_covs(c, c->src, cov9, normals) : RGC_ERR_INVALID; }
int rgc_get_target_covariances(rgc_ctx* c, double* cov9, double* normals) { return c ? get_covs(c, c->tgt, cov9, normals) : RGC_ERR_INVALID; }

// FastGICP::setSourceCovariances / setTargetCovariances (fast_gicp_impl.hpp:93-100): covariances given by the caller replace the ones
// computed from the 20 nearest neighbours.  This path keeps a covariance as its unit normal (C = I - 0.999 n n^T, the PLANE
// regularisation, fast_gicp_impl.hpp:280-293 -- the only form the reference's odometer produces): matrices of that form are
// accepted (to 1e-9), anything else is RGC_ERR_INVALID.  The target's voxel map is rebuilt from the new covariances.
// covariances in the caller's point order on the device (general route: 9 doubles per point, else the unit normal) into the cloud's sorted
// arrays, and the target's voxel map rebuilt from them
static void enqueue_given_covs(rgc_ctx* c, Cloud& cl, bool is_target, const double* d_cov) {
  if (cl.general) {
    rgck::sort6(c->stream, d_cov, cl.P.as<float4>(), cl.n, cl.c6.as<double>());
    if (is_target) rgck::voxel_build_general(c->stream, cl.sorted(), cl.c6.as<double>(), cl.voxels(), c->voxel_mode == RGC_VOXEL_MULTIPLICATIVE ? 1 : 0, nullptr);
  } else {
    rgck::sort3(c->stream, d_cov, cl.P.as<float4>(), cl.n, cl.nx.as<double>(), cl.ny.as<double>(), cl.nz.as<double>());
    if (is_target) rgck::voxel_build(c->stream, cl.sorted(), cl.normals(), cl.voxels());
  }
}
static int set_covs(rgc_ctx* c, Cloud& cl, bool is_target, const double* cov9, int n) {
  if (!cov9) return RGC_ERR_INVALID;
  if (!cl.ready) return fail(c, RGC_ERR_NO_INPUT, "cloud not set");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_clouds(c);
  if (rc) return rc;
  if (!cl.ready) return fail(c, RGC_ERR_NO_INPUT, "cloud not set");
  if (is_target && c->tgt_owner) return fail(c, RGC_ERR_INVALID, "the target is borrowed (rgc_share_target): its covariances belong to the owner");
  if (n != cl.n) return fail(c, RGC_ERR_INVALID, "%d covariances for a cloud of %d points", n, cl.n);
  if (cl.general) {  // the general route takes any symmetric 3x3 as it comes (fast_gicp_impl.hpp:93-100 does not look at them either)
    if ((rc = join_source(c))) return rc;
    if ((rc = ensure(c, c->scratch, sizeof(double) * 9 * (size_t)n))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->scratch.p, cov9, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    enqueue_given_covs(c, cl, is_target, c->scratch.as<double>());
    if (is_target) c->tgt_generation++;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the caller's array is read until here)
    HIPCHK(c, hipGetLastError());
    drop_frozen(c);
    cl.covs_user = true;
    return RGC_OK;
  }
  std::vector<double> nrm((size_t)n * 3);
  for (int i = 0; i < n; i++) {
    const double* C9 = cov9 + (size_t)i * 9;
    double M[9];
    for (int a = 0; a < 9; a++) M[a] = ((a % 4 == 0 ? 1.0 : 0.0) - C9[a]) / 0.999;   // n n^T
    const int d = (M[0] >= M[4] && M[0] >= M[8]) ? 0 : (M[4] >= M[8] ? 1 : 2);
    const double len = std::sqrt(M[4 * d]);
    double v[3] = {0, 0, 0};
    bool ok = len > 0.0 && std::isfinite(len);
    if (ok) {
      for (int a = 0; a < 3; a++) v[a] = M[3 * a + d] / len;
      for (int a = 0; a < 3 && ok; a++)
        for (int b = 0; b < 3; b++)
          if (!(std::fabs(M[3 * a + b] - v[a] * v[b]) <= 1.0e-9)) { ok = false; break; }
    }
    if (!ok) return fail(c, RGC_ERR_INVALID, "covariance %d is not of the plane-regularised form I - 0.999 n n^T: not supported", i);
    nrm[(size_t)i * 3] = v[0]; nrm[(size_t)i * 3 + 1] = v[1]; nrm[(size_t)i * 3 + 2] = v[2];
  }
  if ((rc = join_source(c))) return rc;
  if ((rc = ensure(c, c->scratch, sizeof(double) * 3 * (size_t)n))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->scratch.p, nrm.data(), sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  enqueue_given_covs(c, cl, is_target, c->scratch.as<double>());
  if (is_target) c->tgt_generation++;   // borrowers of this target must share again
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (the host vector goes out of scope)
  HIPCHK(c, hipGetLastError());
  drop_frozen(c);
  cl.covs_user = true;
  return RGC_OK;
}
int rgc_set_source_covariances(rgc_ctx* c, const double* cov9, int n) { return c ? set_covs(c, c->src, false, cov9, n) : RGC_ERR_INVALID; }
int rgc_set_target_covariances(rgc_ctx* c, const double* cov9, int n) { return c ? set_covs(c, c->tgt, true, cov9, n) : RGC_ERR_INVALID; }

// pcl::Registration / FastGICP::clearSource, clearTarget (fast_gicp_impl.hpp:60-69): the cloud and its covariances are dropped
int rgc_clear_source(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  c->src.ready = false; c->src.n = 0; c->src.spec_used = false; drop_frozen(c); c->deferred_known = false;
  return RGC_OK;
}
int rgc_clear_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  c->tgt.ready = false; c->tgt.n = 0; c->tgt.spec_used = false; drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  return RGC_OK;
}

// FastVGICP::swapSourceAndTarget (fast_vgicp_impl.hpp:46-53): the clouds change roles; the voxel map is rebuilt.  Each cloud is
// prepared again in its new role (the source's search grid is not the voxel grid): the covariances are the same function of the cloud.
int rgc_swap_source_and_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "source and target must be set first");
  if (c->tgt_owner) return fail(c, RGC_ERR_INVALID, "the target is borrowed (rgc_share_target): it cannot become the source");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_clouds(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // Covariances the CALLER set travel with their cloud (the reference swaps source_covs_ and target_covs_, fast_vgicp_impl.hpp:46-53):
  // taken out in the caller's point order here, put back into the new ordering behind the preparation (computed ones are simply
  // computed again: the same function of the cloud).
  struct Kept { bool on = false; double* p = nullptr; } kept[2];  // [0]: the old source's (-> new target), [1]: the old target's (-> new source)
  auto drop_kept = [&]() { for (auto& k : kept) if (k.p) { (void)hipFree(k.p); k.p = nullptr; } };
  {
    Cloud* from[2] = {&c->src, &c->tgt};
    for (int a = 0; a < 2; a++) {
      if (!from[a]->covs_user) continue;
      kept[a].on = true;
      if (hipMalloc((void**)&kept[a].p, sizeof(double) * (from[a]->general ? 9 : 3) * (size_t)from[a]->n) != hipSuccess) { drop_kept(); return fail(c, RGC_ERR_HIP, "hipMalloc failed (swap)"); }
      const Cloud& f = *from[a];
      if (f.general) rgck::unsort6(c->stream, f.c6.as<double>(), f.P.as<float4>(), f.n, kept[a].p);
      else rgck::unsort3(c->stream, f.nx.as<double>(), f.ny.as<double>(), f.nz.as<double>(), f.P.as<float4>(), f.n, kept[a].p);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { drop_kept(); return fail(c, RGC_ERR_HIP, "hipStreamSynchronize failed (swap)"); }
  }
  // A target bound to the resident map (rgc_map_commit) was set from the map's own filter output buffer, which the NEXT commit overwrites:
  // as the scan it would keep pointing there (tests/fuzz/fuzz_api.py: swapped back later, it was prepared from another cloud's
  // points).  It takes a copy of its own with it.
  if (c->map.target.p && c->tgt.in == c->map.target.as<const float>()) {
    const size_t bytes = (size_t)c->tgt.n * 16;
    if ((rc = ensure(c, c->tgt.in_copy, bytes))) { drop_kept(); return rc; }
    if (hipMemcpyAsync(c->tgt.in_copy.p, c->map.target.p, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); drop_kept(); return fail(c, RGC_ERR_HIP, "swap: copy of the map's target failed"); }
    c->tgt.in = c->tgt.in_copy.as<const float>();
    c->tgt.stride_f = 4;
  }
  std::swap(c->src.in_copy, c->tgt.in_copy);
  std::swap(c->src.in, c->tgt.in);
  std::swap(c->src.stride_f, c->tgt.stride_f);
  std::swap(c->src.n, c->tgt.n);
  c->src.ready = c->tgt.ready = false;
  drop_frozen(c); c->deferred_known = false; c->map.bound = false;
  if ((rc = prepare_cloud(c, c->tgt, true, /*force_bbox=*/true))) { drop_kept(); return rc; }
  if ((rc = prepare_cloud(c, c->src, false, /*force_bbox=*/true))) { drop_kept(); return rc; }
  if (kept[0].on || kept[1].on) {
    hipError_t e = hipStreamSynchronize(c->stream2);
    Cloud* to[2] = {&c->tgt, &c->src};  // the old source's covariances on the new target (normals, then its voxel map from them), the old target's on the new source
    for (int a = 0; a < 2 && e == hipSuccess; a++) {
      if (!kept[a].on) continue;
      enqueue_given_covs(c, *to[a], a == 0, kept[a].p);
      to[a]->covs_user = true;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    drop_kept();
    if (e != hipSuccess) return fail(c, RGC_ERR_HIP, "swap: %s", hipGetErrorString(e));
    c->src_pending = false;  // (both streams have drained)
  }
  c->stats.n_target = c->tgt.n; c->stats.target_cells = c->tgt.grid.ncell;
  c->stats.n_source = c->src.n; c->stats.source_cells = c->src.grid.ncell;
  return RGC_OK;
}

static int fetch_nvox(rgc_ctx* c) {
  if (c->tgt.nvox >= 0) return RGC_OK;
  HIPCHK(c, hipMemcpyAsync(&c->h_small->map.nvox, &c->d_small->map.nvox, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tgt.nvox = c->h_small->map.nvox;
  c->stats.n_voxels = c->tgt.nvox;
  return RGC_OK;
}

int rgc_get_voxels(rgc_ctx* c, int cap, int* coords, int* num, double* mean, double* cov9, int* count) {
  if (!c || !count) return RGC_ERR_INVALID;
  if (!c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "target not set");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = validate_clouds(c);
  if (rc) return rc;
  if (!c->tgt.ready) return fail(c, RGC_ERR_NO_INPUT, "target not set");
  if ((rc = fetch_nvox(c))) return rc;
  const int V = c->tgt.nvox;
  *count = V;
  const int m = V < cap ? V : cap;
  if (m <= 0) return RGC_OK;
  std::vector<double> rec((size_t)m * rgck::kVoxRec);
  std::vector<int> cell((size_t)m);
  HIPCHK(c, hipMemcpyAsync(rec.data(), c->tgt.vox.p, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cell.data(), c->tgt.vox_cell.p, sizeof(int) * cell.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const rgck::Grid& g = c->tgt.grid;
  for (int v = 0; v < m; v++) {
    const double* r = &rec[(size_t)v * rgck::kVoxRec];
    const int ci = cell[v];
    if (coords) rgck::cell_coords(g, ci, coords + v * 3);
    if (num) num[v] = (int)r[9];
    if (mean) { mean[v * 3] = r[0]; mean[v * 3 + 1] = r[1]; mean[v * 3 + 2] = r[2]; }
    if (cov9) {
      double* C = cov9 + (size_t)v * 9;
      C[0] = r[3]; C[1] = r[4]; C[2] = r[5];
      C[3] = r[4]; C[4] = r[6]; C[5] = r[7];
      C[6] = r[5]; C[7] = r[7]; C[8] = r[8];
    }
  }
  return RGC_OK;
}

int rgc_get_stats(rgc_ctx* c, rgc_stats* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));  // (a tripped guard or a lazy target is resolved below: kernels)
  { int rc = validate_clouds(c, /*whole_target=*/false); if (rc) return rc; }
  if (c->tgt.ready) { int rc = fetch_nvox(c); if (rc) return rc; }
  // queries the bulk kNN kernel handed to the cooperative kernel (first int of the deferred-list buffer)
  if (!c->deferred_known) c->stats.deferred_target = c->stats.deferred_source = 0;
  if (!c->deferred_known) {
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (c->tgt.ready && c->tgt.segs.p) HIPCHK(c, hipMemcpyAsync(&c->stats.deferred_target, c->tgt.segs.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (c->src.ready && c->src.segs.p) HIPCHK(c, hipMemcpyAsync(&c->stats.deferred_source, c->src.segs.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->stats.searched_target = c->tgt.ready ? c->tgt.n : 0;
  if (c->tgt.ready && c->tgt.searched_known >= 0 && !c->trace_cache) {
    c->stats.searched_target = c->tgt.searched_known;  // (fetched once per preparation)
  } else if (c->tgt.ready && c->tgt.cache_on && c->tgt.seed_warm && c->tgt.cache_small.p) {
    // the neighbour-list cache's list lengths and its epoch word (== the frame: everything was searched)
    int h[rgck::kTodoLists + 3];
    HIPCHK(c, hipMemcpyAsync(h, c->tgt.cache_small.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool redo = h[rgck::kTodoLists] == c->tgt.cache_frame || h[rgck::kTodoLists + 1 + ((c->tgt.cache_frame - 1) & 1)] == c->tgt.cache_frame - 1;
    if (c->trace_cache) {
      int mx = 0; long long sm = 0;
      for (int l = 0; l < rgck::kTodoLists; l++) { mx = std::max(mx, h[l]); sm += h[l]; }
      fprintf(stderr, "[rgc] cache: frame %d epoch %d overflow %d %d lists sum %lld max %d cap %d e2 %d slack %g searched_lists %d\n", c->tgt.cache_frame, h[rgck::kTodoLists],
              h[rgck::kTodoLists + 1], h[rgck::kTodoLists + 2], sm, mx, c->tgt.todo_cap, c->tgt.cache_e2, 4.0 * 1.7320508 * 1.1 * std::ldexp(1.0, c->tgt.cache_e2 - 24), (int)c->tgt.cache_searched_lists);
    }
    if (!redo && c->tgt.cache_searched_lists) {
      int sum = 0;
      for (int l = 0; l < rgck::kTodoLists; l++) sum += std::min(h[l], c->tgt.todo_cap);
      c->stats.searched_target = sum;
    }
    c->tgt.searched_known = c->stats.searched_target;
  }
  *out = c->stats;
  return RGC_OK;
}

#ifdef RGC_LAB_TURN
extern "C" RGC_API int rgc_lab_turn(rgc_ctx*, unsigned long long* out8) { rgck::lab_turn(out8); return RGC_OK; }
#endif
#if defined(RGC_LAB) || defined(RGC_LAB_BLK)
RGC_API int rgc_lab_blocks(rgc_ctx*, long long* out65536) { rgck::lab_blocks(out65536); return RGC_OK; }
#endif
#ifdef RGC_LAB
RGC_API int rgc_lab_lm_ts(rgc_ctx* c, unsigned long long* out16) { rgck::lab_lm_ts(out16, c->stream); return RGC_OK; }
RGC_API int rgc_lab_why(rgc_ctx*, int* out8) { rgck::lab_why(out8); return RGC_OK; }
RGC_API int rgc_lab_declines(rgc_ctx*, int* out16) { rgck::lab_declines(out16); return RGC_OK; }
RGC_API int rgc_lab_iters(rgc_ctx*, unsigned long long* out8) { rgck::lab_iters(out8); return RGC_OK; }
RGC_API int rgc_lab_wave_ts(rgc_ctx* c, long long* out16384) { (void)hipStreamSynchronize(c->stream); rgck::lab_wave_ts(out16384, c->stream2); return RGC_OK; }
// developer build only (-DRGC_LAB): the deferred-query list of a cloud as the bulk kNN kernel left it
// (a plain list only: a launch that resolved its deferred queries itself -- the scan's coop_stream, the map's k_knn_sp_vox -- leaves "empty"
// words where idx / thr would be; the count is right either way.  RGC_COOP_STREAM=0 / RGC_VOXEL_IMPL=separate give the lists.)
RGC_API int rgc_lab_deferred(rgc_ctx* c, int is_target, int* idx, float* thr, int cap, int* count) {
  Cloud& cl = is_target ? c->tgt : c->src;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int cnt = 0;
  HIPCHK(c, hipMemcpy(&cnt, cl.segs.p, sizeof(int), hipMemcpyDeviceToHost));
  *count = cnt;
  const int m = cnt < cap ? cnt : cap;
  HIPCHK(c, hipMemcpy(idx, cl.segs.as<const int>() + 16, sizeof(int) * m, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(thr, cl.segs.as<const int>() + 16 + cl.n, sizeof(float) * m, hipMemcpyDeviceToHost));
  return RGC_OK;
}
#endif

int rgc_device_alloc(rgc_ctx* c, size_t bytes, void** p) {
  if (!c || !p) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(p, bytes));
  return RGC_OK;
}
int rgc_device_free(rgc_ctx* c, void* p) {
  if (!c) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipFree(p));
  return RGC_OK;
}
int rgc_host_alloc(size_t bytes, void** p) {
  if (!p) return RGC_ERR_INVALID;
  *p = nullptr;
  return hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocPortable) == hipSuccess ? RGC_OK : RGC_ERR_HIP;
}
int rgc_host_free(void* p) {
  if (!p) return RGC_OK;
  return hipHostFree(p) == hipSuccess ? RGC_OK : RGC_ERR_HIP;
}

int rgc_upload(rgc_ctx* c, void* d, const void* h, size_t bytes) {
  if (!c || !d || !h) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  // behind a pending map preparation this copy is NOT covered by the mark the scan's stream waits for (rgc_set_source_device in rgc_hip.h):
  // remembered, so that a source set next is ordered behind it -- at the price of that one frame's overlap -- instead of racing it
  if (c->main_has_target_prep) c->main_late_producer = true;
  return RGC_OK;
}
int rgc_download(rgc_ctx* c, void* h, const void* d, size_t bytes) {
  if (!c || !d || !h) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RGC_OK;
}
int rgc_synchronize(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->main_has_target_prep = false;
  return RGC_OK;
}
void* rgc_stream(rgc_ctx* c) { return c ? (void*)c->stream : nullptr; }

int rgc_profile_enable(rgc_ctx* c, int on) {
  if (!c) return RGC_ERR_INVALID;
  c->prof_on = on != 0;
  return RGC_OK;
}
int rgc_profile_select(rgc_ctx* c, unsigned kind_mask) {
  if (!c) return RGC_ERR_INVALID;
  c->prof_mask = kind_mask;
  return RGC_OK;
}
int rgc_profile_reset(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  for (int i = 0; i < kProfKinds; i++) { c->prof_launches[i] = 0; c->prof_ms[i] = 0; c->prof_points[i] = 0; }
  return RGC_OK;
}
int rgc_profile_get(rgc_ctx* c, int kind, long long* launches, double* total_ms, long long* total_points) {
  if (!c || kind < 0 || kind >= kProfKinds) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  if (launches) *launches = c->prof_launches[kind];
  if (total_ms) *total_ms = c->prof_ms[kind];
  if (total_points) *total_points = c->prof_points[kind];
  return RGC_OK;
}
const char* rgc_profile_name(int kind) {
  static const char* names[kProfKinds] = {"grid_build", "knn_cov_target", "voxel_build", "linearize", "compute_error", "fitness",
                                          "knn_cov_source", "knn_coop_target", "knn_coop_source"};
  return (kind >= 0 && kind < kProfKinds) ? names[kind] : "?";
}

}  // extern "C"
