// rgc_api_lsq.hip -- the host LM driver every registration method shares (LsqRegistration::computeTransformation and step_lm,
// lsq_registration_impl.hpp:53-79, 125-172) and the two methods that are nothing else on the host: NDT (rgc_ndt_*) and FastGICP (rgc_gicp_*).
// rgc_align's host-driven route (rgc_api.hip) runs on the same driver, and so does FastGICPSingleThread (rgc_gicpst_*, kernels in rgc_gicp_st.hip:
// FastGICP with anchor-cached correspondences).  The kernels are in rgc_ndt.hip and rgc_gicp.hip.  FastGICPMultiPoints
// (rgc_gicpmp_*, kernels in rgc_gicp_mp.hip) has a plain Gauss-Newton loop of its own over the driver's scalar pieces.
#include "rgc_ctx.h"
#include "rgc_lm_decide.h"  // rgc_lm.h and the convergence test the device decides by (lsq_registration_impl.hpp:82-91)

using namespace rgcapi;

// LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-79) + step_lm (:125-172); SURVEY A.5.  The scalar pieces (so3_exp, the
// LDLT solve, the 4x4 product) are rgc_lm.h's, shared with the device.
int rgcapi::lm_solve(rgc_ctx* c, const LmSystem& sys, const float guess[16], LmResult* r) {
  const rgc_params& P = c->prm;
  r->open(guess);
  double* x0 = r->x0;
  double lambda = -1.0;  // :56
  for (int it = 0; it < P.max_iterations && !r->conv; it++) {  // :65
    r->iters = it + 1;
    double H[36], b[6], y0, delta[16], d[6], xi[16], yi;
    int rc;
    if (sys.may_linearize && !sys.may_linearize(x0)) { r->failed = true; break; }  // (FastGICP: a step of an empty or singular system)
    if (sys.linearize_try) {  // :128 and the first try of :135-144 in one call; :130-132 with it (lambda0 = factor * max|H_ii|)
      if ((rc = sys.linearize_try(c, x0, lambda, H, b, &y0, d, xi, &lambda, &yi))) return rc;
      double R[9];  // that try's delta = [so3_exp(d[0:3]) | d[3:6]] (:136-143)
      rgclm::so3_exp_R(d, R);
      memset(delta, 0, sizeof(delta));
      for (int a = 0; a < 3; a++) { for (int e = 0; e < 3; e++) delta[a * 4 + e] = R[a * 3 + e]; delta[a * 4 + 3] = d[3 + a]; }
      delta[15] = 1.0;
    } else {
      if ((rc = sys.linearize(c, x0, H, b, &y0))) return rc;  // :128
      if (lambda < 0.0) {  // :130-132
        double m = 0;
        for (int a = 0; a < 6; a++) m = std::fmax(m, std::fabs(H[a * 7]));
        lambda = P.lm_init_lambda_factor * m;
      }
    }
    double nu = 2.0;
    bool ok = false;
    for (int k = 0; k < P.lm_max_iterations; k++) {  // :135
      if (k > 0 || !sys.linearize_try) {  // (every try but one that linearize_try has made)
        rgclm::lm_try(H, b, lambda, x0, d, delta, xi);  // :136-143
        if ((rc = sys.error(c, xi, &yi))) return rc;    // :144
      }
      double den = 0;
      for (int i = 0; i < 6; i++) den += d[i] * (lambda * d[i] - b[i]);
      const double rho = (y0 - yi) / den;  // :145
      if (rho < 0) {  // :155-163
        if (rgck::lm_is_converged(delta, P.rotation_eps, P.translation_eps)) { ok = true; break; }
        lambda = nu * lambda;
        nu = 2 * nu;
        continue;
      }
      memcpy(x0, xi, sizeof(xi));  // :165
      lambda = lambda * std::fmax(1.0 / 3.0, 1 - std::pow(2 * rho - 1, 3));  // :166
      memcpy(r->Hfin, H, sizeof(r->Hfin));  // :167
      ok = true;
      break;
    }
    if (!ok) { r->failed = true; break; }  // :69-72 "lm not converged!!"
    r->conv = rgck::lm_is_converged(delta, P.rotation_eps, P.translation_eps);  // :74
  }
  for (int i = 0; i < 16; i++) r->fin[i] = (float)x0[i];  // :77
  return RGC_OK;
}

// the k folded sums of a method (d_out, behind the launches on the context's stream) in its pinned buffer h_out, the launches checked
static int read_sums(rgc_ctx* c, double* h_out, const DevBuf& d_out, int k) {
  HIPCHK(c, hipMemcpyAsync(h_out, d_out.p, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// the offsets of a neighbour method in the reference's order (rgc_ctx.h): src/fast_gicp/cuda/ndt_cuda.cu:35-88, fast_vgicp_cuda.cu:42-95
bool rgcapi::neighbor_offsets_of(int method, double radius, std::vector<int>& o, int cap) {
  o.clear();
  if (method == RGC_NDT_DIRECT1) { o = {0, 0, 0}; return true; }
  if (method == RGC_NDT_DIRECT7) { o = {0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1}; return true; }
  if (method == RGC_NDT_DIRECT27) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) { o.push_back(i - 1); o.push_back(j - 1); o.push_back(k - 1); }
    return true;
  }
  if (radius > 16.0) return false;
  const int range = (int)std::ceil(radius);
  for (int i = -range; i <= range; i++)
    for (int j = -range; j <= range; j++)
      for (int k = -range; k <= range; k++)
        if (std::sqrt((double)(i * i + j * j + k * k)) <= radius + 1e-3) {
          if ((int)o.size() / 3 >= cap) return false;
          o.push_back(i); o.push_back(j); o.push_back(k);
        }
  return true;
}

extern "C" {

// ---- NDT registration (P2D / D2D) on a Gaussian voxel map: fast_gicp::NDTCuda (src/fast_gicp/cuda/ndt_cuda.cu, ndt_compute_derivatives.cu) ----
void rgc_default_ndt_params(rgc_ndt_params* p) {
  if (!p) return;
  p->resolution = 1.0;                     // src/fast_gicp/cuda/ndt_cuda.cu:15
  p->distance_mode = RGC_NDT_D2D;          // :21
  p->neighbor_method = RGC_NDT_DIRECT7;    // :22
  p->neighbor_radius = 0.0;
}

static void ndt_drop_terms(rgc_ctx* c) { c->ndt_corr_valid = false; c->ndt_terms = 0; }

int rgc_ndt_set_params(rgc_ctx* c, const rgc_ndt_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  if (!std::isfinite(p->resolution) || !(p->resolution > 0.0)) return fail(c, RGC_ERR_INVALID, "rgc_ndt_set_params: resolution must be finite and > 0");
  if (p->distance_mode != RGC_NDT_P2D && p->distance_mode != RGC_NDT_D2D) return fail(c, RGC_ERR_INVALID, "rgc_ndt_set_params: no distance mode %d", p->distance_mode);
  if (p->neighbor_method < RGC_NDT_DIRECT27 || p->neighbor_method > RGC_NDT_DIRECT_RADIUS) return fail(c, RGC_ERR_INVALID, "rgc_ndt_set_params: no neighbour method %d", p->neighbor_method);
  std::vector<int> offs;
  if (p->neighbor_method == RGC_NDT_DIRECT_RADIUS) {
    if (!std::isfinite(p->neighbor_radius) || p->neighbor_radius < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_ndt_set_params: DIRECT_RADIUS needs a finite radius >= 0");
  }
  if (!neighbor_offsets_of(p->neighbor_method, p->neighbor_radius, offs))
    return fail(c, RGC_ERR_INVALID, "rgc_ndt_set_params: radius %g has more than %d offsets", p->neighbor_radius, RGC_NDT_MAX_OFFSETS);
  if (p->resolution != c->ndt_prm.resolution || p->distance_mode != c->ndt_prm.distance_mode) ndt_drop_terms(c);
  c->ndt_prm = *p;
  c->ndt_offs_h.swap(offs);
  c->ndt_offs_dirty = true;
  return RGC_OK;
}

int rgc_ndt_get_params(const rgc_ctx* c, rgc_ndt_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  *p = c->ndt_prm;
  return RGC_OK;
}

// the offset table of a neighbour method as VGICP and NDT walk it: host code, no context (rgc_hip.h)
int rgc_neighbor_offsets(int method, double radius, int* xyz, int cap, int* n) {
  if (!n || cap < 0) return RGC_ERR_INVALID;  // (xyz == NULL: the size alone)
  if (method < RGC_DIRECT27 || method > RGC_DIRECT_RADIUS) return RGC_ERR_INVALID;
  if (method == RGC_DIRECT_RADIUS && (!std::isfinite(radius) || radius < 0.0)) return RGC_ERR_INVALID;
  std::vector<int> o;
  if (!neighbor_offsets_of(method, radius, o)) return RGC_ERR_INVALID;  // more than RGC_NDT_MAX_OFFSETS
  const int total = (int)o.size() / 3;
  if (xyz) memcpy(xyz, o.data(), sizeof(int) * 3 * (size_t)std::min(cap, total));
  *n = total;
  return RGC_OK;
}

// one body of the four setters: the points packed to 12 bytes each in the cloud's own buffer, in stream order on the context's stream
static int ndt_set_cloud(rgc_ctx* c, int which, const float* xyz, int n, int stride_bytes, bool on_device) {
  if (!c || !xyz) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "stride_bytes must be a multiple of 4 between 12 and 4096");
  if (n < 1) return fail(c, n < 0 ? RGC_ERR_INVALID : RGC_ERR_TOO_FEW_POINTS, "rgc_ndt_set_*: a cloud needs at least one point");
  if (n > (1 << 27)) return fail(c, RGC_ERR_INVALID, "cloud has %d points, the limit is 2^27", n);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (on_device && (rc = check_device_range(c, xyz, (size_t)n * stride_bytes - (stride_bytes - 12), which ? "rgc_ndt_set_source_device" : "rgc_ndt_set_target_device"))) return rc;
  Cloud& cl = c->ndt_cl[which];
  if ((rc = ensure(c, cl.in_copy, (size_t)n * 12))) return rc;
  HIPCHK(c, hipMemcpy2DAsync(cl.in_copy.p, 12, xyz, (size_t)stride_bytes, 12, (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  if (!on_device) HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller owns a host buffer for the duration of the call only
  cl.in = cl.in_copy.as<const float>();
  cl.stride_f = 3;
  cl.n = n;
  cl.ready = false;
  c->ndt_set[which] = true;
  c->ndt_built[which] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_set_target(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 0, xyz, n, stride_bytes, false); }
int rgc_ndt_set_source(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 1, xyz, n, stride_bytes, false); }
int rgc_ndt_set_target_device(rgc_ctx* c, const float* d_xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 0, d_xyz, n, stride_bytes, true); }
int rgc_ndt_set_source_device(rgc_ctx* c, const float* d_xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 1, d_xyz, n, stride_bytes, true); }

int rgc_ndt_clear_source(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  c->ndt_set[1] = c->ndt_built[1] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_clear_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  c->ndt_set[0] = c->ndt_built[0] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_swap_source_and_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  std::swap(c->ndt_cl[0], c->ndt_cl[1]);
  std::swap(c->ndt_set[0], c->ndt_set[1]);
  std::swap(c->ndt_built[0], c->ndt_built[1]);
  std::swap(c->ndt_built_res[0], c->ndt_built_res[1]);
  ndt_drop_terms(c);
  return RGC_OK;
}

static int ndt_scratch(rgc_ctx* c) {
  int rc;
  if ((rc = ensure(c, c->ndt_small, 64))) return rc;
  if ((rc = ensure(c, c->ndt_out, sizeof(double) * 32))) return rc;
  if (!c->ndt_h_out) HIPCHK(c, hipHostMalloc((void**)&c->ndt_h_out, sizeof(double) * 32, hipHostMallocDefault));
  if (!c->ndt_h_small) HIPCHK(c, hipHostMalloc((void**)&c->ndt_h_small, sizeof(int) * 8, hipHostMallocDefault));
  return RGC_OK;
}

// the voxel map of NDT cloud `which` at the current resolution, if it is not there yet: the VGICP target's table construction (bounding box,
// counting sort by voxel, points of a voxel in ascending index) and one segmented pass (rgck::ndt_voxels)
static int ndt_build(rgc_ctx* c, int which) {
  Cloud& cl = c->ndt_cl[which];
  const double res = c->ndt_prm.resolution;
  if (c->ndt_built[which] && c->ndt_built_res[which] == res) return RGC_OK;
  c->ndt_built[which] = false;
  int rc;
  if ((rc = ndt_scratch(c))) return rc;
  hipStream_t s = c->stream;
  int* dsm = c->ndt_small.as<int>();
  int* hsm = c->ndt_h_small;
  if ((rc = build_measured_grid(c, cl, res, dsm, hsm, true, which ? "NDT source" : "NDT target", which ? "NDT source: voxel grid" : "NDT target: voxel grid"))) return rc;
  HIPCHK(c, hipMemcpyAsync(hsm + 7, dsm + 7, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const int nvox = hsm[7];
  if (nvox < 1 || nvox > cl.n) return fail(c, RGC_ERR_HIP, "NDT voxel count %d out of range", nvox);
  if ((rc = ensure(c, cl.vox, sizeof(double) * rgck::kNdtRec * (size_t)nvox))) return rc;
  if ((rc = ensure(c, cl.vox_cell, sizeof(int) * (size_t)nvox))) return rc;
  rgck::ndt_voxels(s, cl.sorted(), cl.voxels());
  HIPCHK(c, hipGetLastError());
  cl.nvox = nvox;
  cl.ready = true;
  c->ndt_built[which] = true;
  c->ndt_built_res[which] = res;
  return RGC_OK;
}

static int ndt_need_inputs(rgc_ctx* c) {
  if (!c->ndt_set[0]) return fail(c, RGC_ERR_NO_INPUT, "NDT target not set");
  if (!c->ndt_set[1]) return fail(c, RGC_ERR_NO_INPUT, "NDT source not set");
  int rc;
  if ((rc = ndt_build(c, 0))) return rc;
  if (c->ndt_prm.distance_mode == RGC_NDT_D2D && (rc = ndt_build(c, 1))) return rc;
  return RGC_OK;
}

// find != 0: linearize at T (the term list and R_lin are made); else the cost at T over the frozen list.  out: 28 sums + the number of terms.
static int ndt_run_terms(rgc_ctx* c, const double T[16], bool find, bool want_H, double out[29]) {
  int rc;
  if ((rc = ndt_scratch(c))) return rc;
  const int d2d = find ? (c->ndt_prm.distance_mode == RGC_NDT_D2D) : c->ndt_corr_mode;
  const Cloud& tg = c->ndt_cl[0];
  const Cloud& sc = c->ndt_cl[1];
  const int n = find ? (d2d ? sc.nvox : sc.n) : c->ndt_corr_n;
  if (find) {
    if (c->ndt_offs_h.empty()) neighbor_offsets_of(c->ndt_prm.neighbor_method, c->ndt_prm.neighbor_radius, c->ndt_offs_h);
    if (c->ndt_offs_dirty) {
      if ((rc = ensure(c, c->ndt_offs, sizeof(int) * 3 * RGC_NDT_MAX_OFFSETS))) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));  // (a launch that reads the former list may still run)
      HIPCHK(c, hipMemcpy(c->ndt_offs.p, c->ndt_offs_h.data(), sizeof(int) * c->ndt_offs_h.size(), hipMemcpyHostToDevice));
      c->ndt_offs_dirty = false;
    }
    c->ndt_corr_valid = false;
    c->ndt_corr_noff = (int)c->ndt_offs_h.size() / 3;
    c->ndt_corr_n = n;
    c->ndt_corr_mode = d2d;
    memcpy(c->ndt_Tlin, T, sizeof(double) * 16);
    if ((rc = ensure(c, c->ndt_corr, sizeof(int) * (size_t)n * c->ndt_corr_noff))) return rc;
  }
  const int noff = c->ndt_corr_noff;
  const int nb = rgck::ndt_blocks(n);
  if ((rc = ensure(c, c->ndt_partials, sizeof(double) * rgck::kAccum * (size_t)nb))) return rc;
  if ((rc = ensure(c, c->ndt_ipartials, sizeof(int) * (size_t)nb))) return rc;
  rgck::ndt_terms(c->stream, d2d, find ? 1 : 0, sc.in, sc.stride_f, sc.vox.as<const double>(), n, pose_from(T), pose_from(c->ndt_Tlin), tg.grid,
                  tg.voxels(), c->ndt_offs.as<const int>(), noff, c->ndt_corr.as<int>(), want_H ? 1 : 0,
                  c->ndt_partials.as<double>(), c->ndt_ipartials.as<int>(), c->ndt_out.as<double>());
  if ((rc = read_sums(c, c->ndt_h_out, c->ndt_out, 29))) return rc;
  memcpy(out, c->ndt_h_out, sizeof(double) * 29);
  if (find) {
    c->ndt_corr_valid = true;
    c->ndt_terms = (int)out[28];
  }
  return RGC_OK;
}

static int ndt_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  int rc = ndt_need_inputs(c);
  if (rc) return rc;
  double out[29];
  const bool want = H && b;
  if ((rc = ndt_run_terms(c, T, true, want, out))) return rc;
  if (want) unpack_system(out, H, b);
  if (cost) *cost = out[27];
  return RGC_OK;
}

static int ndt_do_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c->ndt_set[0] || !c->ndt_set[1]) return fail(c, RGC_ERR_NO_INPUT, "NDT source or target not set");
  if (!c->ndt_corr_valid) return fail(c, RGC_ERR_INVALID, "rgc_ndt_compute_error needs a preceding rgc_ndt_linearize");
  double out[29];
  const int rc = ndt_run_terms(c, T, false, false, out);
  if (rc) return rc;
  *cost = out[27];
  return RGC_OK;
}

int rgc_ndt_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  if (!pose12_finite(T)) return fail(c, RGC_ERR_NONFINITE, "rgc_ndt_linearize: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  return ndt_do_linearize(c, T, H, b, cost);
}

int rgc_ndt_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  if (!pose12_finite(T)) return fail(c, RGC_ERR_NONFINITE, "rgc_ndt_compute_error: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  return ndt_do_error(c, T, cost);
}

int rgc_ndt_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  if (!c->ndt_corr_valid) return fail(c, RGC_ERR_INVALID, "rgc_ndt_num_correspondences needs a preceding rgc_ndt_linearize");
  *n = c->ndt_terms;
  return RGC_OK;
}

// computeTransformation (lm_solve) over the two calls above
int rgc_ndt_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], int* iterations, int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (!pose12_finite(guess)) return fail(c, RGC_ERR_NONFINITE, "rgc_ndt_align: the guess is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ndt_need_inputs(c);  // create_voxelmaps() (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:77)
  if (rc) return rc;
  static const LmSystem sys = {ndt_do_linearize, ndt_do_error, nullptr, nullptr};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  r.write(final_T, final_H, iterations, converged, lm_failed);
  return RGC_OK;
}

// the records of map `which` on the host (m of them); cells: their grid cells
static int ndt_fetch_voxels(rgc_ctx* c, int which, int cap, std::vector<double>& rec, std::vector<int>& cell, int* count) {
  if (which != 0 && which != 1) return fail(c, RGC_ERR_INVALID, "which: 0 target, 1 source");
  if (cap < 0) return fail(c, RGC_ERR_INVALID, "negative capacity");
  if (!c->ndt_set[which]) return fail(c, RGC_ERR_NO_INPUT, "NDT %s not set", which ? "source" : "target");
  int rc = ndt_build(c, which);
  if (rc) return rc;
  const Cloud& cl = c->ndt_cl[which];
  *count = cl.nvox;
  const int m = cl.nvox < cap ? cl.nvox : cap;
  rec.resize((size_t)m * rgck::kNdtRec);
  cell.resize((size_t)m);
  if (m <= 0) return RGC_OK;
  HIPCHK(c, hipMemcpyAsync(rec.data(), cl.vox.p, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cell.data(), cl.vox_cell.p, sizeof(int) * cell.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RGC_OK;
}

static void ndt_cov9(const double* r6, double* C) {
  C[0] = r6[0]; C[1] = r6[1]; C[2] = r6[2];
  C[3] = r6[1]; C[4] = r6[3]; C[5] = r6[4];
  C[6] = r6[2]; C[7] = r6[4]; C[8] = r6[5];
}

int rgc_ndt_get_voxels(rgc_ctx* c, int which, int cap, int* coords, int* num, double* mean, double* cov9, int* count) {
  if (!c || !count) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> rec;
  std::vector<int> cell;
  int total = 0;
  const int rc = ndt_fetch_voxels(c, which, cap, rec, cell, &total);
  if (rc) return rc;
  *count = total;
  const rgck::Grid& g = c->ndt_cl[which].grid;
  for (size_t v = 0; v < cell.size(); v++) {
    const double* r = &rec[v * rgck::kNdtRec];
    const int ci = cell[v];
    if (coords) rgck::cell_coords(g, ci, coords + v * 3);
    if (num) num[v] = (int)r[9];
    if (mean) { mean[v * 3] = r[0]; mean[v * 3 + 1] = r[1]; mean[v * 3 + 2] = r[2]; }
    if (cov9) ndt_cov9(r + 3, cov9 + v * 9);
  }
  return RGC_OK;
}

int rgc_ndt_get_raw_covariances(rgc_ctx* c, int which, int cap, double* cov9, int* count) {
  if (!c || !count) return RGC_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> rec;
  std::vector<int> cell;
  int total = 0;
  const int rc = ndt_fetch_voxels(c, which, cap, rec, cell, &total);
  if (rc) return rc;
  *count = total;
  if (cov9)
    for (size_t v = 0; v < cell.size(); v++) ndt_cov9(&rec[v * rgck::kNdtRec] + 16, cov9 + v * 9);
  return RGC_OK;
}

// ---- FastGICP: GICP on exact nearest-neighbour correspondences (include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237) on the context's own clouds ----
int rgc_gicp_set_max_correspondence_distance(rgc_ctx* c, double d_max) {
  if (!c) return RGC_ERR_INVALID;
  if (std::isnan(d_max) || d_max < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_gicp_set_max_correspondence_distance: the distance must be >= 0");
  c->gicp_dmax = d_max;
  return RGC_OK;
}

int rgc_gicp_get_max_correspondence_distance(const rgc_ctx* c, double* d_max) {
  if (!c || !d_max) return RGC_ERR_INVALID;
  *d_max = c->gicp_dmax;
  return RGC_OK;
}

// a pose the GICP calls accept: finite in fp64 and after the cast to fp32 the search transforms with (fast_gicp_impl.hpp:119)
static bool gicp_pose_ok(const double T[16]) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(T[i]) || !std::isfinite((float)T[i])) return false;
  return true;
}

// both clouds there, no solve in flight, the speculative grids' guards read, a lazy target completed, the source's preparation joined
static int gicp_need_inputs(rgc_ctx* c) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->src.ready || !c->tgt.ready) return fail(c, RGC_ERR_INVALID, "rgc_gicp_*: source and target must be set first");
  int rc = need_inputs(c);
  if (rc == RGC_ERR_NO_INPUT) return fail(c, RGC_ERR_INVALID, "rgc_gicp_*: source and target must be set first");
  if (rc) return rc;
  if (!c->gicp_h_out) HIPCHK(c, hipHostMalloc((void**)&c->gicp_h_out, sizeof(double) * 32, hipHostMallocDefault));
  return ensure(c, c->gicp_out, sizeof(double) * 32);
}

static rgck::GicpCov gicp_cov_of(const Cloud& cl) {
  if (cl.general) return rgck::GicpCov{cl.c6.as<const double>(), nullptr, nullptr, nullptr};
  return rgck::GicpCov{nullptr, cl.nx.as<const double>(), cl.ny.as<const double>(), cl.nz.as<const double>()};
}

// update_correspondences + linearize (fast_gicp_impl.hpp:115-211); the inputs have been checked (gicp_need_inputs)
static int gicp_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  const int n = sc.n, nb = rgck::gicp_blocks(n);
  int rc;
  c->gicp_valid = false;
  if ((rc = ensure(c, c->gicp_corr, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_key, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_M, sizeof(double) * 6 * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_partials, sizeof(double) * (rgck::kAccum + 1) * (size_t)nb))) return rc;
  float T32[16];
  for (int i = 0; i < 16; i++) T32[i] = (float)T[i];  // trans.cast<float>(), :119
  const int want = (H && b) ? 1 : 0;
  rgck::gicp_correspond(c->stream, sc.sorted(), posef_from(T32), tg.sorted(), c->gicp_dmax * c->gicp_dmax, c->gicp_corr.as<int>(), c->gicp_key.as<float>());
  rgck::gicp_terms(c->stream, sc.sorted(), tg.sorted(), c->gicp_corr.as<const int>(), gicp_cov_of(sc), gicp_cov_of(tg), pose_from(T), want,
                   c->gicp_M.as<double>(), c->gicp_partials.as<double>(), c->gicp_out.as<double>());
  if ((rc = read_sums(c, c->gicp_h_out, c->gicp_out, rgck::kAccum + 1))) return rc;
  const double* o = c->gicp_h_out;
  c->gicp_valid = true;
  c->gicp_n = n;
  c->gicp_kept = (int)o[28];
  if (want) unpack_system(o, H, b);
  if (cost) *cost = o[27];
  return RGC_OK;
}

// compute_error (fast_gicp_impl.hpp:214-237) over the frozen pairs and matrices
static int gicp_do_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c->gicp_valid || c->gicp_n != c->src.n) return fail(c, RGC_ERR_INVALID, "rgc_gicp_compute_error needs a preceding rgc_gicp_linearize on the present clouds");
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  rgck::gicp_error(c->stream, sc.sorted(), tg.sorted(), c->gicp_corr.as<const int>(), c->gicp_M.as<const double>(), pose_from(T),
                   c->gicp_partials.as<double>(), c->gicp_out.as<double>());
  const int rc = read_sums(c, c->gicp_h_out, c->gicp_out, 1);
  if (rc) return rc;
  *cost = c->gicp_h_out[0];
  return RGC_OK;
}

int rgc_gicp_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  if (!gicp_pose_ok(T)) return fail(c, RGC_ERR_INVALID, "rgc_gicp_linearize: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = gicp_need_inputs(c);
  return rc ? rc : gicp_do_linearize(c, T, H, b, cost);
}

int rgc_gicp_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  if (!gicp_pose_ok(T)) return fail(c, RGC_ERR_INVALID, "rgc_gicp_compute_error: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = gicp_need_inputs(c);
  return rc ? rc : gicp_do_error(c, T, cost);
}

int rgc_gicp_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->gicp_valid) return fail(c, RGC_ERR_INVALID, "rgc_gicp_num_correspondences needs a preceding rgc_gicp_linearize on the present clouds");
  *n = c->gicp_kept;
  return RGC_OK;
}

int rgc_gicp_get_correspondences(rgc_ctx* c, int* idx, float* sq_dist) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->gicp_valid || !c->src.ready || !c->tgt.ready || c->gicp_n != c->src.n)
    return fail(c, RGC_ERR_INVALID, "rgc_gicp_get_correspondences needs a preceding rgc_gicp_linearize on the present clouds");
  if (!idx && !sq_dist) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n = c->src.n;
  int rc = check_target_owner(c);
  if (rc) return rc;
  if ((rc = ensure(c, c->scratch, (sizeof(int) + sizeof(float)) * (size_t)n))) return rc;
  int* d_idx = c->scratch.as<int>();
  float* d_sq = (float*)(d_idx + n);
  HIPCHK(c, hipMemsetAsync(d_idx, 0xff, sizeof(int) * (size_t)n, c->stream));
  HIPCHK(c, hipMemsetAsync(d_sq, 0, sizeof(float) * (size_t)n, c->stream));
  rgck::gicp_export(c->stream, c->src.sorted(), c->tgt.sorted(), c->gicp_corr.as<const int>(), c->gicp_key.as<const float>(), d_idx, d_sq);
  if (idx) HIPCHK(c, hipMemcpyAsync(idx, d_idx, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (sq_dist) HIPCHK(c, hipMemcpyAsync(sq_dist, d_sq, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// the fitness score of a solve's final pose as rgc_align gives it (NaN for a pose that is not finite); fitness is nullable
static int gicp_final_fitness(rgc_ctx* c, const LmResult& r, double* fitness) {
  if (!fitness) return RGC_OK;
  if (!pose12_finite(r.fin)) { *fitness = (double)NAN; return RGC_OK; }
  return do_fitness(c, r.fin, fitness);
}

// computeTransformation (lm_solve) over the two calls above; the fitness score of the final pose as rgc_align gives it
int rgc_gicp_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (!pose12_finite(guess)) return fail(c, RGC_ERR_INVALID, "rgc_gicp_align: the guess is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = gicp_need_inputs(c);
  if (rc) return rc;
  static const LmSystem sys = {gicp_do_linearize, gicp_do_error, nullptr, gicp_pose_ok};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  r.write(final_T, final_H, iterations, converged, lm_failed);
  return gicp_final_fitness(c, r, fitness);
}

// ---- FastGICPSingleThread: GICP with anchor-cached correspondences (include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125) on the context's own clouds ----
static rgck::GicpStState gicp_st_state(rgc_ctx* c) {
  return rgck::GicpStState{c->gicp_st_corr.as<int>(), c->gicp_st_key1.as<float>(), c->gicp_st_key2.as<float>(), c->gicp_st_anchor.as<float4>(),
                           c->gicp_st_M.as<double>(), c->gicp_st_searched.as<int>(), c->gicp_st_list.as<int>(), c->gicp_st_count.as<int>()};
}

// update_correspondences + linearize (fast_gicp_st_impl.hpp:25-120); the inputs have been checked (gicp_need_inputs).  Without a state of the
// present clouds every point is searched (is_first, :31); the host does not wait for the number searched: it comes back with the sums
static int gicp_st_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  const int n = sc.n, nb = rgck::gicp_blocks(n);
  const int first = (c->gicp_st_valid && c->gicp_st_n == n) ? 0 : 1;
  int rc;
  c->gicp_st_valid = false;
  if ((rc = ensure(c, c->gicp_st_corr, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_key1, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_key2, sizeof(float) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_anchor, sizeof(float) * 4 * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_M, sizeof(double) * 6 * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_searched, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_list, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_st_count, sizeof(int) * 4))) return rc;
  if ((rc = ensure(c, c->gicp_partials, sizeof(double) * rgck::kGicpStAcc * (size_t)nb))) return rc;
  float T32[16];
  for (int i = 0; i < 16; i++) T32[i] = (float)T[i];  // x.cast<float>(), :29
  const int want = (H && b) ? 1 : 0;
  const rgck::GicpStState st = gicp_st_state(c);
  if (first) HIPCHK(c, hipMemsetAsync(st.count, 0, sizeof(int), c->stream));  // (afterwards the term kernel leaves the counter at zero)
  rgck::gicpst_correspond(c->stream, sc.sorted(), posef_from(T32), tg.sorted(), c->gicp_dmax * c->gicp_dmax, first, st);
  rgck::gicpst_terms(c->stream, sc.sorted(), tg.sorted(), st, gicp_cov_of(sc), gicp_cov_of(tg), pose_from(T), want, c->gicp_partials.as<double>(),
                     c->gicp_out.as<double>());
  if ((rc = read_sums(c, c->gicp_h_out, c->gicp_out, rgck::kGicpStAcc))) return rc;
  const double* o = c->gicp_h_out;
  c->gicp_st_valid = true;
  c->gicp_st_n = n;
  c->gicp_st_kept = (int)o[28];
  c->gicp_st_searched_n = (int)o[29];
  if (want) unpack_system(o, H, b);
  if (cost) *cost = o[27];
  return RGC_OK;
}

// compute_error (fast_gicp_st_impl.hpp:122-125: linearize without H and b, which leaves the state alone, :81-85) -- FastGICP's frozen cost over this state
static int gicp_st_do_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c->gicp_st_valid || c->gicp_st_n != c->src.n)
    return fail(c, RGC_ERR_INVALID, "rgc_gicpst_compute_error needs a preceding rgc_gicpst_linearize on the present clouds");
  rgck::gicp_error(c->stream, c->src.sorted(), c->tgt.sorted(), c->gicp_st_corr.as<const int>(), c->gicp_st_M.as<const double>(), pose_from(T),
                   c->gicp_partials.as<double>(), c->gicp_out.as<double>());
  const int rc = read_sums(c, c->gicp_h_out, c->gicp_out, 1);
  if (rc) return rc;
  *cost = c->gicp_h_out[0];
  return RGC_OK;
}

int rgc_gicpst_reset(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  c->gicp_st_valid = false;
  return RGC_OK;
}

int rgc_gicpst_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  if (!gicp_pose_ok(T)) return fail(c, RGC_ERR_INVALID, "rgc_gicpst_linearize: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = gicp_need_inputs(c);
  return rc ? rc : gicp_st_do_linearize(c, T, H, b, cost);
}

int rgc_gicpst_compute_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c || !T || !cost) return RGC_ERR_INVALID;
  if (!gicp_pose_ok(T)) return fail(c, RGC_ERR_INVALID, "rgc_gicpst_compute_error: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = gicp_need_inputs(c);
  return rc ? rc : gicp_st_do_error(c, T, cost);
}

// the state is there, and is that of the present clouds
static int gicp_st_need_state(rgc_ctx* c, const char* who) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->gicp_st_valid || !c->src.ready || !c->tgt.ready || c->gicp_st_n != c->src.n)
    return fail(c, RGC_ERR_INVALID, "%s needs a preceding rgc_gicpst_linearize on the present clouds", who);
  return RGC_OK;
}

int rgc_gicpst_num_correspondences(rgc_ctx* c, int* n) {
  if (!c || !n) return RGC_ERR_INVALID;
  const int rc = gicp_st_need_state(c, "rgc_gicpst_num_correspondences");
  if (rc) return rc;
  *n = c->gicp_st_kept;
  return RGC_OK;
}

int rgc_gicpst_num_searched(rgc_ctx* c, int* n_searched) {
  if (!c || !n_searched) return RGC_ERR_INVALID;
  const int rc = gicp_st_need_state(c, "rgc_gicpst_num_searched");
  if (rc) return rc;
  *n_searched = c->gicp_st_searched_n;
  return RGC_OK;
}

int rgc_gicpst_get_correspondences(rgc_ctx* c, int* idx, float* sq_dist, float* second_sq_dist, int* searched) {
  if (!c) return RGC_ERR_INVALID;
  int rc = gicp_st_need_state(c, "rgc_gicpst_get_correspondences");
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
  if (idx) HIPCHK(c, hipMemcpyAsync(idx, d_idx, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  if (sq_dist) HIPCHK(c, hipMemcpyAsync(sq_dist, d_sq, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  if (second_sq_dist) HIPCHK(c, hipMemcpyAsync(second_sq_dist, d_sq2, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  if (searched) HIPCHK(c, hipMemcpyAsync(searched, d_was, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// computeTransformation (fast_gicp_st_impl.hpp:19-22): anchors_.clear(), then LsqRegistration's driver (lm_solve) over the two calls above
int rgc_gicpst_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (!pose12_finite(guess)) return fail(c, RGC_ERR_INVALID, "rgc_gicpst_align: the guess is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = gicp_need_inputs(c);
  if (rc) return rc;
  c->gicp_st_valid = false;  // :20
  static const LmSystem sys = {gicp_st_do_linearize, gicp_st_do_error, nullptr, gicp_pose_ok};
  LmResult r;
  if ((rc = lm_solve(c, sys, guess, &r))) return rc;
  r.write(final_T, final_H, iterations, converged, lm_failed);
  return gicp_final_fitness(c, r, fitness);
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
  c->gicp_mp_prm = *p;
  c->gicp_mp_valid = false;
  return RGC_OK;
}

int rgc_gicpmp_get_params(const rgc_ctx* c, rgc_gicp_mp_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  *p = c->gicp_mp_prm;
  return RGC_OK;
}

static int gicp_mp_need_inputs(rgc_ctx* c) {
  const int rc = gicp_need_inputs(c);
  if (rc) return rc;
  if (!c->gicp_mp_h_out) HIPCHK(c, hipHostMalloc((void**)&c->gicp_mp_h_out, sizeof(double) * 32, hipHostMallocDefault));
  return ensure(c, c->gicp_mp_out, sizeof(double) * 32);
}

// update_correspondences + loss_ls (fast_gicp_mp_impl.hpp:130-221) as the normal equations of its rows; the inputs have been checked
static int gicp_mp_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const Cloud& sc = c->src;
  const Cloud& tg = c->tgt;
  const int n = sc.n, nb = rgck::gicp_mp_blocks(n);
  int rc;
  c->gicp_mp_valid = false;
  if ((rc = ensure(c, c->gicp_mp_merged, sizeof(double) * rgck::kGicpMpMerged * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_mp_cand, sizeof(int) * (size_t)n))) return rc;
  if ((rc = ensure(c, c->gicp_mp_partials, sizeof(double) * rgck::kGicpMpAcc * (size_t)nb))) return rc;
  for (int i = 0; i < 16; i++) c->gicp_mp_T32[i] = (float)T[i];  // trans (Matrix4f), :131-133
  const double r = c->gicp_mp_prm.neighbor_search_radius;
  const int want = (H && b) ? 1 : 0;
  rgck::gicp_mp_merge(c->stream, sc.sorted(), posef_from(c->gicp_mp_T32), tg.sorted(), gicp_cov_of(tg), gicp_mp_r2(r), r, c->gicp_mp_merged.as<double>(),
                      c->gicp_mp_cand.as<int>());
  rgck::gicp_mp_terms(c->stream, sc.sorted(), c->gicp_mp_merged.as<const double>(), gicp_cov_of(sc), pose_from(T), want, c->gicp_mp_partials.as<double>(),
                      c->gicp_mp_out.as<double>());
  if ((rc = read_sums(c, c->gicp_mp_h_out, c->gicp_mp_out, rgck::kGicpMpAcc))) return rc;
  const double* o = c->gicp_mp_h_out;
  c->gicp_mp_valid = true;
  c->gicp_mp_n = n;
  c->gicp_mp_points = (int)o[28];
  c->gicp_mp_pairs = (long long)o[29];
  if (want) unpack_system(o, H, b);
  if (cost) *cost = o[27];
  return RGC_OK;
}

int rgc_gicpmp_linearize(rgc_ctx* c, const double T[16], double H[36], double b[6], double* cost) {
  if (!c || !T) return RGC_ERR_INVALID;
  if (!gicp_pose_ok(T)) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_linearize: the pose is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = gicp_mp_need_inputs(c);
  return rc ? rc : gicp_mp_do_linearize(c, T, H, b, cost);
}

// the kept results are there, and are those of the present clouds
static int gicp_mp_need_results(rgc_ctx* c, const char* who) {
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->gicp_mp_valid || !c->src.ready || !c->tgt.ready || c->gicp_mp_n != c->src.n)
    return fail(c, RGC_ERR_INVALID, "%s needs a preceding rgc_gicpmp_linearize on the present clouds and settings", who);
  return RGC_OK;
}

int rgc_gicpmp_num_correspondences(rgc_ctx* c, int* n_points, long long* n_pairs) {
  if (!c) return RGC_ERR_INVALID;
  const int rc = gicp_mp_need_results(c, "rgc_gicpmp_num_correspondences");
  if (rc) return rc;
  if (n_points) *n_points = c->gicp_mp_points;
  if (n_pairs) *n_pairs = c->gicp_mp_pairs;
  return RGC_OK;
}

// what the gather looked at to find them: the candidates of all source points (every point of every grid row range the balls reach)
int rgc_gicpmp_num_candidates(rgc_ctx* c, long long* n_candidates) {
  if (!c || !n_candidates) return RGC_ERR_INVALID;
  const int rc = gicp_mp_need_results(c, "rgc_gicpmp_num_candidates");
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int> cand((size_t)c->src.n);
  HIPCHK(c, hipMemcpyAsync(cand.data(), c->gicp_mp_cand.p, sizeof(int) * cand.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long long t = 0;
  for (int v : cand) t += v;
  *n_candidates = t;
  return RGC_OK;
}

int rgc_gicpmp_get_merged(rgc_ctx* c, int* count, double* sum_w, double* mean3, double* cov6) {
  if (!c) return RGC_ERR_INVALID;
  int rc = gicp_mp_need_results(c, "rgc_gicpmp_get_merged");
  if (rc) return rc;
  if (!count && !sum_w && !mean3 && !cov6) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->src.n;
  if ((rc = ensure(c, c->gicp_mp_scratch, (sizeof(double) * 10 + sizeof(int)) * n))) return rc;
  double* d_sw = c->gicp_mp_scratch.as<double>();
  double* d_mean = d_sw + n;
  double* d_cov = d_mean + 3 * n;
  int* d_count = (int*)(d_cov + 6 * n);
  HIPCHK(c, hipMemsetAsync(c->gicp_mp_scratch.p, 0, (sizeof(double) * 10 + sizeof(int)) * n, c->stream));
  rgck::gicp_mp_export(c->stream, c->src.sorted(), c->gicp_mp_merged.as<const double>(), d_count, d_sw, d_mean, d_cov);
  if (count) HIPCHK(c, hipMemcpyAsync(count, d_count, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  if (sum_w) HIPCHK(c, hipMemcpyAsync(sum_w, d_sw, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  if (mean3) HIPCHK(c, hipMemcpyAsync(mean3, d_mean, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, c->stream));
  if (cov6) HIPCHK(c, hipMemcpyAsync(cov6, d_cov, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

int rgc_gicpmp_get_neighbors(rgc_ctx* c, int* offsets, int* idx, float* sq_dist, int cap, long long* n_total) {
  if (!c || !n_total) return RGC_ERR_INVALID;
  int rc = gicp_mp_need_results(c, "rgc_gicpmp_get_neighbors");
  if (rc) return rc;
  *n_total = c->gicp_mp_pairs;
  if (cap < 0 || (long long)cap < c->gicp_mp_pairs) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_get_neighbors: cap is smaller than the %lld neighbours there are", c->gicp_mp_pairs);
  if (!offsets && !idx && !sq_dist) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_target_owner(c))) return rc;
  // count (caller order) -> exclusive scan -> fill: [counts n + 1][offsets n + 1][block sums][idx total][keys total]
  const size_t n1 = (size_t)c->src.n + 1, nbs = n1 / 2048 + 2, total = (size_t)c->gicp_mp_pairs;
  if ((rc = ensure(c, c->gicp_mp_scratch, sizeof(int) * (2 * n1 + nbs + 2 * total)))) return rc;
  int* d_cnt = c->gicp_mp_scratch.as<int>();
  int* d_off = d_cnt + n1;
  int* d_bs = d_off + n1;
  int* d_idx = d_bs + nbs;
  float* d_sq = (float*)(d_idx + total);
  HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(int) * n1, c->stream));
  rgck::gicp_mp_export(c->stream, c->src.sorted(), c->gicp_mp_merged.as<const double>(), d_cnt, nullptr, nullptr, nullptr);
  rgck::exclusive_scan(c->stream, d_cnt, d_off, (int)n1, d_bs);
  const double r = c->gicp_mp_prm.neighbor_search_radius;
  if (total) rgck::gicp_mp_fill(c->stream, c->src.sorted(), posef_from(c->gicp_mp_T32), c->tgt.sorted(), gicp_mp_r2(r), r, d_off, d_idx, d_sq);
  if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, d_off, sizeof(int) * n1, hipMemcpyDeviceToHost, c->stream));
  if (idx && total) HIPCHK(c, hipMemcpyAsync(idx, d_idx, sizeof(int) * total, hipMemcpyDeviceToHost, c->stream));
  if (sq_dist && total) HIPCHK(c, hipMemcpyAsync(sq_dist, d_sq, sizeof(float) * total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// computeTransformation (fast_gicp_mp_impl.hpp:80-115): plain Gauss-Newton.  The update is the one the Jacobian skew(R p + t) is derived for and every
// other driver here makes, T <- [so3_exp(d_r) | d_t] T (rgclm::lm_try at lambda = 0: the undamped solve of the host LM driver's 6x6 factorisation);
// the reference's own (:101-102) turns R alone.  Convergence (:118-127) is tested after the update.
int rgc_gicpmp_align(rgc_ctx* c, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* failed) {
  if (!c || !guess) return RGC_ERR_INVALID;
  if (!pose12_finite(guess)) return fail(c, RGC_ERR_INVALID, "rgc_gicpmp_align: the guess is not finite");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = gicp_mp_need_inputs(c);
  if (rc) return rc;
  const rgc_gicp_mp_params& P = c->gicp_mp_prm;
  LmResult r;
  r.open(guess);
  for (int it = 0; it < P.max_iterations; it++) {  // :92
    if (!gicp_pose_ok(r.x0)) { r.failed = true; break; }
    r.iters = it + 1;
    double H[36], b[6], y0, d[6], delta[16], xi[16];
    if ((rc = gicp_mp_do_linearize(c, r.x0, H, b, &y0))) return rc;  // :95-97
    if (c->gicp_mp_points == 0) { r.failed = true; break; }
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
  r.write(final_T, final_H, iterations, converged, failed);
  return gicp_final_fitness(c, r, fitness);
}

}  // extern "C"
