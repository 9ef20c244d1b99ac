// rgc_api_gicp.hip -- the three GICP variants on the context's own source and target: FastGICP (rgc_gicp_*, kernels in rgc_gicp.hip), FastGICPSingleThread
// (rgc_gicpst_*, rgc_gicp_st.hip: FastGICP with anchor-cached correspondences) and FastGICPMultiPoints (rgc_gicpmp_*, rgc_gicp_mp.hip).  Each keeps its
// frozen state in a record of its own (rgcapi::GicpRecord, GicpStRecord, GicpMpRecord: rgc_ctx.h; drop_frozen says what drops them).  The first two solve
// on the shared host LM driver (lm_solve, rgc_api_lsq.hip); MultiPoints has a plain Gauss-Newton loop of its own over the driver's scalar pieces.  What
// the three do alike on the host is written once, at the top.
#include "rgc_ctx.h"
#include "rgc_lm_decide.h"  // rgc_lm.h and the convergence test the device decides by (lsq_registration_impl.hpp:82-91)

using namespace rgcapi;

// a pose the GICP calls accept: finite in fp64 and after the cast to fp32 the search transforms with (fast_gicp_impl.hpp:119)
static bool gicp_pose_ok(const double T[16]) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(T[i]) || !std::isfinite((float)T[i])) return false;
  return true;
}

// a method's folded sums and their pinned mirror, 32 doubles each
static int ensure_sums(rgc_ctx* c, Sums& s) {
  if (!s.h_out) HIPCHK(c, hipHostMalloc((void**)&s.h_out, sizeof(double) * 32, hipHostMallocDefault));
  return ensure(c, s.out, sizeof(double) * 32);
}

// both clouds there, no solve in flight, the speculative grids' guards read, a lazy target completed, the source's preparation joined
static int gicp_need_inputs(rgc_ctx* c) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_INVALID, "rgc_gicp_*: source and target must be set first");
  int rc = need_inputs(c);
  if (rc == RGC_ERR_NO_INPUT) return fail(c, RGC_ERR_INVALID, "rgc_gicp_*: source and target must be set first");
  if (rc) return rc;
  return ensure_sums(c, c->gicp_sums);
}

// what every linearize, compute_error and align of the three opens with, behind its null checks: the pose (or the guess) finite, the device, the inputs
static int gicp_enter(rgc_ctx* c, bool finite, const char* who, const char* what) {
  if (!finite) return fail(c, RGC_ERR_INVALID, "%s: the %s is not finite", who, what);
  HIPCHK(c, hipSetDevice(c->device));
  return gicp_need_inputs(c);
}

// a record's kept results (valid, made for n source points) are those of the present clouds; made_by: the linearisation `who` needs, for the message
static int gicp_present(rgc_ctx* c, bool valid, int n, const char* who, const char* made_by) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!valid || !c->src.ready || !c->tgt.ready || n != c->src.n) return fail(c, RGC_ERR_INVALID, "%s needs a preceding %s", who, made_by);
  return RGC_OK;
}
static const char kGicpMadeBy[] = "rgc_gicp_linearize on the present clouds";
static const char kGicpStMadeBy[] = "rgc_gicpst_linearize on the present clouds";
static const char kGicpMpMadeBy[] = "rgc_gicpmp_linearize on the present clouds and settings";

// compute_error (fast_gicp_impl.hpp:214-237; fast_gicp_st_impl.hpp:122-125: linearize without H and b, which leaves the state alone, :81-85) over a
// frozen pair list and its Mahalanobis matrices
static int gicp_frozen_cost(rgc_ctx* c, const DevBuf& corr, const DevBuf& M, const double T[16], double* cost) {
  rgck::gicp_error(c->stream, c->src.sorted(), c->tgt.sorted(), corr.as<const int>(), M.as<const double>(), pose_from(T),
                   c->gicp_sums.partials.as<double>(), c->gicp_sums.out.as<double>());
  const int rc = read_sums(c, c->gicp_sums, 1);
  if (rc) return rc;
  *cost = c->gicp_sums.h_out[0];
  return RGC_OK;
}

// the copies to the caller behind an export launch on the context's stream, each output nullable; the launch checked
struct HostOut { void* dst; const void* src; size_t bytes; };
static int copy_out(rgc_ctx* c, std::initializer_list<HostOut> outs) {
  for (const HostOut& o : outs)
    if (o.dst && o.bytes) HIPCHK(c, hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// a finished solve handed over (each output nullable): the fitness score of the final pose as rgc_align gives it (NaN for a pose that is not finite)
static int gicp_finish(rgc_ctx* c, const LmResult& r, float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  r.write(final_T, final_H, iterations, converged, lm_failed);
  if (!fitness) return RGC_OK;
  if (!pose12_finite(r.fin)) { *fitness = (double)NAN; return RGC_OK; }
  return do_fitness(c, r.fin, fitness);
}

static rgck::GicpCov gicp_cov_of(const Cloud& cl) {
  if (cl.general) return rgck::GicpCov{cl.c6.as<const double>(), nullptr, nullptr, nullptr};
  return rgck::GicpCov{nullptr, cl.nx.as<const double>(), cl.ny.as<const double>(), cl.nz.as<const double>()};
}

extern "C" {

// ---- FastGICP: GICP on exact nearest-neighbour correspondences (include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237) on the context's own clouds ----
int rgc_gicp_set_max_correspondence_distance(rgc_ctx* c, double d_max) {
  if (!c) return RGC_ERR_INVALID;
  if (std::isnan(d_max) || d_max < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_gicp_set_max_correspondence_distance: the distance must be >= 0");
  c->gicp.dmax = d_max;
  return RGC_OK;
}

int rgc_gicp_get_max_correspondence_distance(const rgc_ctx* c, double* d_max) {
  if (!c || !d_max) return RGC_ERR_INVALID;
  *d_max = c->gicp.dmax;
  return RGC_OK;
}

// update_correspondences + linearize (fast_gicp_impl.hpp:115-211); the inputs have been checked (gicp_need_inputs)
static int gicp_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  rgcapi::GicpRecord& g = c->gicp;
  const int n = sc.n, nb = rgck::gicp_blocks(n);
  int rc;
  g.valid = false;
  if ((rc = ensure(c, g.corr, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.key, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.M, sizeof(double) * 6 * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_sums.partials, sizeof(double) * (rgck::kAccum + 1) * (size_t)nb))) return rc;
  float T32[16];
  for (int i = 0; i < 16; i++) T32[i] = (float)T[i];  // trans.cast<float>(), :119
  rgck::gicp_correspond(c->stream, sc.sorted(), posef_from(T32), tg.sorted(), g.dmax * g.dmax, g.corr.as<int>(), g.key.as<float>());
  rgck::gicp_terms(c->stream, sc.sorted(), tg.sorted(), g.corr.as<const int>(), gicp_cov_of(sc), gicp_cov_of(tg), pose_from(T), (H && b) ? 1 : 0,
                   g.M.as<double>(), c->gicp_sums.partials.as<double>(), c->gicp_sums.out.as<double>());
  if ((rc = read_system(c, c->gicp_sums, rgck::kAccum + 1, H, b, cost))) return rc;
  g.valid = true;
  g.n = n;
  g.kept = (int)c->gicp_sums.h_out[28];
  return RGC_OK;
}

static int gicp_do_error(rgc_ctx* c, const double T[16], double* cost) {
  const int rc = gicp_present(c, c->gicp.valid, c->gicp.n, "rgc_gicp_compute_error", kGicpMadeBy);
  return rc ? rc : gicp_frozen_cost(c, c->gicp.corr, c->gicp.M, T, cost);
}

int rgc_gicp_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  const int rc = gicp_enter(c, gicp_pose_ok(T), "rgc_gicp_linearize", "pose");
  return rc ? rc : gicp_do_linearize(c, T, H, b, cost);
}

int rgc_gicp_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  const int rc = gicp_enter(c, gicp_pose_ok(T), "rgc_gicp_compute_error", "pose");
  return rc ? rc : gicp_do_error(c, T, cost);
}

int rgc_gicp_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->gicp.valid) return fail(c, RGC_ERR_INVALID, "rgc_gicp_num_correspondences needs a preceding rgc_gicp_linearize on the present clouds");
  *n = c->gicp.kept;
  return RGC_OK;
}

int rgc_gicp_get_correspondences(rgc_ctx* c, int* idx, float* sq_dist) {
  if (!c) return RGC_ERR_INVALID;
  int rc = gicp_present(c, c->gicp.valid, c->gicp.n, "rgc_gicp_get_correspondences", kGicpMadeBy);
  if (rc) return rc;
  if (!idx && !sq_dist) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->src.n;
  if ((rc = check_target_owner(c))) return rc;
  if ((rc = ensure(c, c->scratch, (sizeof(int) + sizeof(float)) * n))) return rc;
  int* d_idx = c->scratch.as<int>();
  float* d_sq = (float*)(d_idx + n);
  HIPCHK(c, hipMemsetAsync(d_idx, 0xff, sizeof(int) * n, c->stream));
  HIPCHK(c, hipMemsetAsync(d_sq, 0, sizeof(float) * n, c->stream));
  rgck::gicp_export(c->stream, c->src.sorted(), c->tgt.sorted(), c->gicp.corr.as<const int>(), c->gicp.key.as<const float>(), d_idx, d_sq);
  return copy_out(c, {{idx, d_idx, sizeof(int) * n}, {sq_dist, d_sq, sizeof(float) * n}});
}

// computeTransformation (lm_solve) over the two calls above; the fitness score of the final pose as rgc_align gives it
int rgc_gicp_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  int rc = gicp_enter(c, pose12_finite(guess), "rgc_gicp_align", "guess");
  if (rc) return rc;
  static const LmSystem sys = {gicp_do_linearize, gicp_do_error, nullptr, gicp_pose_ok};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  return gicp_finish(c, r, final_T, final_H, fitness, iterations, converged, lm_failed);
}

// ---- FastGICPSingleThread: GICP with anchor-cached correspondences (include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125) on the context's own clouds ----
static rgck::GicpStState gicp_st_state(rgc_ctx* c) {
  rgcapi::GicpStRecord& g = c->gicp_st;
  return rgck::GicpStState{g.corr.as<int>(), g.key1.as<float>(), g.key2.as<float>(), g.anchor.as<float4>(), g.M.as<double>(), g.searched.as<int>(),
                           g.list.as<int>(), g.count.as<int>()};
}

// update_correspondences + linearize (fast_gicp_st_impl.hpp:25-120); the inputs have been checked (gicp_need_inputs).  Without a state of the
// present clouds every point is searched (is_first, :31); the host does not wait for the number searched: it comes back with the sums
static int gicp_st_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  rgcapi::GicpStRecord& g = c->gicp_st;
  const int n = sc.n, nb = rgck::gicp_blocks(n);
  const int first = (g.valid && g.n == n) ? 0 : 1;
  int rc;
  g.valid = false;
  if ((rc = ensure(c, g.corr, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.key1, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.key2, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.anchor, sizeof(float) * 4 * (size_t)n))) return rc;
  if ((rc = ensure(c, g.M, sizeof(double) * 6 * (size_t)n))) return rc;
  if ((rc = ensure(c, g.searched, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.list, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.count, sizeof(int) * 4))) return rc;
  if ((rc = ensure(c, c->gicp_sums.partials, sizeof(double) * rgck::kGicpStAcc * (size_t)nb))) return rc;
  float T32[16];
  for (int i = 0; i < 16; i++) T32[i] = (float)T[i];  // x.cast<float>(), :29
  const rgck::GicpStState st = gicp_st_state(c);
  if (first) HIPCHK(c, hipMemsetAsync(st.count, 0, sizeof(int), c->stream));  // (afterwards the term kernel leaves the counter at zero)
  rgck::gicpst_correspond(c->stream, sc.sorted(), posef_from(T32), tg.sorted(), c->gicp.dmax * c->gicp.dmax, first, st);
  rgck::gicpst_terms(c->stream, sc.sorted(), tg.sorted(), st, gicp_cov_of(sc), gicp_cov_of(tg), pose_from(T), (H && b) ? 1 : 0,
                     c->gicp_sums.partials.as<double>(), c->gicp_sums.out.as<double>());
  if ((rc = read_system(c, c->gicp_sums, rgck::kGicpStAcc, H, b, cost))) return rc;
  g.valid = true;
  g.n = n;
  g.kept = (int)c->gicp_sums.h_out[28];
  g.searched_n = (int)c->gicp_sums.h_out[29];
  return RGC_OK;
}

static int gicp_st_do_error(rgc_ctx* c, const double T[16], double* cost) {
  const int rc = gicp_present(c, c->gicp_st.valid, c->gicp_st.n, "rgc_gicpst_compute_error", kGicpStMadeBy);
  return rc ? rc : gicp_frozen_cost(c, c->gicp_st.corr, c->gicp_st.M, T, cost);
}

int rgc_gicpst_reset(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  c->gicp_st.valid = false;
  return RGC_OK;
}

int rgc_gicpst_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  const int rc = gicp_enter(c, gicp_pose_ok(T), "rgc_gicpst_linearize", "pose");
  return rc ? rc : gicp_st_do_linearize(c, T, H, b, cost);
}

int rgc_gicpst_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  const int rc = gicp_enter(c, gicp_pose_ok(T), "rgc_gicpst_compute_error", "pose");
  return rc ? rc : gicp_st_do_error(c, T, cost);
}

int rgc_gicpst_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  const int rc = gicp_present(c, c->gicp_st.valid, c->gicp_st.n, "rgc_gicpst_num_correspondences", kGicpStMadeBy);
  if (rc) return rc;
  *n = c->gicp_st.kept;
  return RGC_OK;
}

int rgc_gicpst_num_searched(rgc_ctx* c, int* n_searched) {
  if (!c || !n_searched) return RGC_ERR_INVALID;
  const int rc = gicp_present(c, c->gicp_st.valid, c->gicp_st.n, "rgc_gicpst_num_searched", kGicpStMadeBy);
  if (rc) return rc;
  *n_searched = c->gicp_st.searched_n;
  return RGC_OK;
}

int rgc_gicpst_get_correspondences(rgc_ctx* c, int* idx, float* sq_dist, float* second_sq_dist, int* searched) {
  if (!c) return RGC_ERR_INVALID;
  int rc = gicp_present(c, c->gicp_st.valid, c->gicp_st.n, "rgc_gicpst_get_correspondences", kGicpStMadeBy);
  if (rc) return rc;
  if (!idx && !sq_dist && !second_sq_dist && !searched) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->src.n;
  if ((rc = check_target_owner(c))) return rc;
  if ((rc = ensure(c, c->scratch, 16 * n))) return rc;
  int* d_idx = c->scratch.as<int>();
  float* d_sq = (float*)(d_idx + n);
  float* d_sq2 = d_sq + n;
  int* d_was = (int*)(d_sq2 + n);
  HIPCHK(c, hipMemsetAsync(d_idx, 0xff, sizeof(int) * n, c->stream));
  HIPCHK(c, hipMemsetAsync(d_sq, 0, 12 * n, c->stream));
  rgck::gicpst_export(c->stream, c->src.sorted(), c->tgt.sorted(), gicp_st_state(c), d_idx, d_sq, d_sq2, d_was);
  return copy_out(c, {{idx, d_idx, sizeof(int) * n}, {sq_dist, d_sq, sizeof(float) * n}, {second_sq_dist, d_sq2, sizeof(float) * n}, {searched, d_was, sizeof(int) * n}});
}

// computeTransformation (fast_gicp_st_impl.hpp:19-22): anchors_.clear(), then LsqRegistration's driver (lm_solve) over the two calls above
int rgc_gicpst_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  int rc = gicp_enter(c, pose12_finite(guess), "rgc_gicpst_align", "guess");
  if (rc) return rc;
  c->gicp_st.valid = false;  // :20
  static const LmSystem sys = {gicp_st_do_linearize, gicp_st_do_error, nullptr, gicp_pose_ok};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  return gicp_finish(c, r, final_T, final_H, fitness, iterations, converged, lm_failed);
}

// ---- FastGICPMultiPoints: GICP on radius-merged target distributions (include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:92-221) on the context's own clouds ----
void rgc_default_gicp_mp_params(rgc_gicp_mp_params* p) {
  if (!p) return;
  p->neighbor_search_radius = 0.5;   // fast_gicp_mp_impl.hpp:35
  p->max_iterations = 64;            // :29
  p->rotation_epsilon = 1e-5;        // :30
  p->transformation_epsilon = 1e-5;  // :31
}

// r2 as pcl::KdTreeFLANN::radiusSearch hands it to FLANN: the fp64 product rounded to fp32
static float gicp_mp_r2(double r) { return (float)(r * r); }

int rgc_gicpmp_set_params(rgc_ctx* c, const rgc_gicp_mp_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  const double r = p->neighbor_search_radius;
  if (!std::isfinite(r) || !(r > 0.0) || !std::isfinite(gicp_mp_r2(r)))
    return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_set_params: the radius must be finite and > 0, and its square a finite float");
  if (p->max_iterations < 1) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_set_params: max_iterations must be >= 1");
  if (!(p->rotation_epsilon > 0.0) || !(p->transformation_epsilon > 0.0)) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_set_params: the epsilons must be > 0");
  c->gicp_mp.prm = *p;
  c->gicp_mp.valid = false;
  return RGC_OK;
}

int rgc_gicpmp_get_params(const rgc_ctx* c, rgc_gicp_mp_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  *p = c->gicp_mp.prm;
  return RGC_OK;
}

// update_correspondences + loss_ls (fast_gicp_mp_impl.hpp:130-221) as the normal equations of its rows; the inputs have been checked
static int gicp_mp_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  rgcapi::GicpMpRecord& g = c->gicp_mp;
  const int n = sc.n, nb = rgck::gicp_mp_blocks(n);
  int rc;
  g.valid = false;
  if ((rc = ensure(c, g.merged, sizeof(double) * rgck::kGicpMpMerged * (size_t)n))) return rc;
  if ((rc = ensure(c, g.cand, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, g.sums.partials, sizeof(double) * rgck::kGicpMpAcc * (size_t)nb))) return rc;
  for (int i = 0; i < 16; i++) g.T32[i] = (float)T[i];  // trans (Matrix4f), :131-133
  const double r = g.prm.neighbor_search_radius;
  rgck::gicp_mp_merge(c->stream, sc.sorted(), posef_from(g.T32), tg.sorted(), gicp_cov_of(tg), gicp_mp_r2(r), r, g.merged.as<double>(), g.cand.as<int>());
  rgck::gicp_mp_terms(c->stream, sc.sorted(), g.merged.as<const double>(), gicp_cov_of(sc), pose_from(T), (H && b) ? 1 : 0, g.sums.partials.as<double>(),
                      g.sums.out.as<double>());
  if ((rc = read_system(c, g.sums, rgck::kGicpMpAcc, H, b, cost))) return rc;
  g.valid = true;
  g.n = n;
  g.points = (int)g.sums.h_out[28];
  g.pairs = (long long)g.sums.h_out[29];
  return RGC_OK;
}

int rgc_gicpmp_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  int rc = gicp_enter(c, gicp_pose_ok(T), "rgc_gicpmp_linearize", "pose");
  if (!rc) rc = ensure_sums(c, c->gicp_mp.sums);  // (this method folds into sums of its own)
  return rc ? rc : gicp_mp_do_linearize(c, T, H, b, cost);
}

int rgc_gicpmp_num_correspondences(rgc_ctx* c, int* n_points, long long* n_pairs) {
  if (!c) return RGC_ERR_INVALID;
  const int rc = gicp_present(c, c->gicp_mp.valid, c->gicp_mp.n, "rgc_gicpmp_num_correspondences", kGicpMpMadeBy);
  if (rc) return rc;
  if (n_points) *n_points = c->gicp_mp.points;
  if (n_pairs) *n_pairs = c->gicp_mp.pairs;
  return RGC_OK;
}

// what the gather looked at to find them: the candidates of all source points (every point of every grid row range the balls reach)
int rgc_gicpmp_num_candidates(rgc_ctx* c, long long* n_candidates) {
  if (!c || !n_candidates) return RGC_ERR_INVALID;
  const int rc = gicp_present(c, c->gicp_mp.valid, c->gicp_mp.n, "rgc_gicpmp_num_candidates", kGicpMpMadeBy);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int> cand((size_t)c->src.n);
  HIPCHK(c, hipMemcpyAsync(cand.data(), c->gicp_mp.cand.p, sizeof(int) * cand.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long long t = 0;
  for (int v : cand) t += v;
  *n_candidates = t;
  return RGC_OK;
}

int rgc_gicpmp_get_merged(rgc_ctx* c, int* count, double* sum_w, double* mean3, double* cov6) {
  if (!c) return RGC_ERR_INVALID;
  int rc = gicp_present(c, c->gicp_mp.valid, c->gicp_mp.n, "rgc_gicpmp_get_merged", kGicpMpMadeBy);
  if (rc) return rc;
  if (!count && !sum_w && !mean3 && !cov6) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->src.n;
  DevBuf& scratch = c->gicp_mp.scratch;
  if ((rc = ensure(c, scratch, (sizeof(double) * 10 + sizeof(int)) * n))) return rc;
  double* d_sw = scratch.as<double>();
  double* d_mean = d_sw + n;
  double* d_cov = d_mean + 3 * n;
  int* d_count = (int*)(d_cov + 6 * n);
  HIPCHK(c, hipMemsetAsync(scratch.p, 0, (sizeof(double) * 10 + sizeof(int)) * n, c->stream));
  rgck::gicp_mp_export(c->stream, c->src.sorted(), c->gicp_mp.merged.as<const double>(), d_count, d_sw, d_mean, d_cov);
  return copy_out(c, {{count, d_count, sizeof(int) * n}, {sum_w, d_sw, sizeof(double) * n}, {mean3, d_mean, sizeof(double) * 3 * n}, {cov6, d_cov, sizeof(double) * 6 * n}});
}

int rgc_gicpmp_get_neighbors(rgc_ctx* c, int* offsets, int* idx, float* sq_dist, int cap, long long* n_total) {
  if (!c || !n_total) return RGC_ERR_INVALID;
  rgcapi::GicpMpRecord& g = c->gicp_mp;
  int rc = gicp_present(c, g.valid, g.n, "rgc_gicpmp_get_neighbors", kGicpMpMadeBy);
  if (rc) return rc;
  *n_total = g.pairs;
  if (cap < 0 || (long long)cap < g.pairs) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_get_neighbors: cap is smaller than the %lld neighbours there are", g.pairs);
  if (!offsets && !idx && !sq_dist) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_target_owner(c))) return rc;
  // count (caller order) -> exclusive scan -> fill: [counts n + 1][offsets n + 1][block sums][idx total][keys total]
  const size_t n1 = (size_t)c->src.n + 1, nbs = n1 / 2048 + 2, total = (size_t)g.pairs;
  if ((rc = ensure(c, g.scratch, sizeof(int) * (2 * n1 + nbs + 2 * total)))) return rc;
  int* d_cnt = g.scratch.as<int>();
  int* d_off = d_cnt + n1;
  int* d_bs = d_off + n1;
  int* d_idx = d_bs + nbs;
  float* d_sq = (float*)(d_idx + total);
  HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * n1, c->stream));
  rgck::gicp_mp_export(c->stream, c->src.sorted(), g.merged.as<const double>(), d_cnt, nullptr, nullptr, nullptr);
  rgck::exclusive_scan(c->stream, d_cnt, d_off, (int)n1, d_bs);
  const double r = g.prm.neighbor_search_radius;
  if (total) rgck::gicp_mp_fill(c->stream, c->src.sorted(), posef_from(g.T32), c->tgt.sorted(), gicp_mp_r2(r), r, d_off, d_idx, d_sq);
  return copy_out(c, {{offsets, d_off, sizeof(int) * n1}, {idx, d_idx, sizeof(int) * total}, {sq_dist, d_sq, sizeof(float) * total}});  // (no neighbours: nothing of idx and sq_dist)
}

// computeTransformation (fast_gicp_mp_impl.hpp:80-115): plain Gauss-Newton.  The update is the one the Jacobian skew(R p + t) is derived for and every
// other driver here makes, T <- [so3_exp(d_r) | d_t] T (rgclm::lm_try at lambda = 0: the undamped solve of the host LM driver's 6x6 factorisation);
// the reference's own (:101-102) turns R alone.  Convergence (:118-127) is tested after the update.
int rgc_gicpmp_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  int rc = gicp_enter(c, pose12_finite(guess), "rgc_gicpmp_align", "guess");
  if (!rc) rc = ensure_sums(c, c->gicp_mp.sums);
  if (rc) return rc;
  const rgc_gicp_mp_params& P = c->gicp_mp.prm;
  LmResult r;
  r.open(guess);
  for (int it = 0; it < P.max_iterations; it++) {  // :92
    if (!gicp_pose_ok(r.x0)) { r.failed = true; break; }
    r.iters = it + 1;
    double H[36], b[6], y0, d[6], delta[16], xi[16];
    if ((rc = gicp_mp_do_linearize(c, r.x0, H, b, &y0))) return rc;  // :95-97
    if (c->gicp_mp.points == 0) { r.failed = true; break; }
    rgclm::lm_try(H, b, 0.0, r.x0, d, delta, xi);                   // :99-102
    bool finite = true;
    for (int i = 0; i < 6; i++) finite = finite && std::isfinite(d[i]);
    for (int i = 0; i < 12; i++) finite = finite && std::isfinite(xi[i]);
    if (!finite) { r.failed = true; break; }
    memcpy(r.x0, xi, sizeof(xi));
    memcpy(r.Hfin, H, sizeof(H));
    if (rgck::lm_is_converged(delta, P.rotation_epsilon, P.transformation_epsilon)) { r.conv = true; break; }  // :104-107
  }
  for (int i = 0; i < 16; i++) r.fin[i] = (float)r.x0[i];
  return gicp_finish(c, r, final_T, final_H, fitness, iterations, converged, failed);
}

}  // extern "C"
