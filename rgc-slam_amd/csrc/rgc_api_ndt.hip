// rgc_api_ndt.hip -- NDT registration (P2D / D2D) on a Gaussian voxel map (rgc_ndt_*): fast_gicp::NDTCuda (src/fast_gicp/cuda/ndt_cuda.cu,
// ndt_compute_derivatives.cu) on two clouds of the method's own (rgcapi::NdtRecord, rgc_ctx.h).  The solve is the shared host LM driver's
// (lm_solve, rgc_api_lsq.hip); the kernels are in rgc_ndt.hip.
#include "rgc_ctx.h"

using namespace rgcapi;

extern "C" {

// ---- NDT registration (P2D / D2D) on a Gaussian voxel map: fast_gicp::NDTCuda (src/fast_gicp/cuda/ndt_cuda.cu, ndt_compute_derivatives.cu) ----
void rgc_default_ndt_params(rgc_ndt_params* p) {
  if (!p) return;
  p->resolution = 1.0;                     // src/fast_gicp/cuda/ndt_cuda.cu:15
  p->distance_mode = RGC_NDT_D2D;          // :21
  p->neighbor_method = RGC_NDT_DIRECT7;    // :22
  p->neighbor_radius = 0.0;
}

static void ndt_drop_terms(rgc_ctx* c) { c->ndt.valid = false; c->ndt.terms = 0; }

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
  if (p->resolution != c->ndt.prm.resolution || p->distance_mode != c->ndt.prm.distance_mode) ndt_drop_terms(c);
  c->ndt.prm = *p;
  c->ndt.offs_h.swap(offs);
  c->ndt.offs_dirty = true;
  return RGC_OK;
}

int rgc_ndt_get_params(const rgc_ctx* c, rgc_ndt_params* p) {
  if (!c || !p) return RGC_ERR_INVALID;
  *p = c->ndt.prm;
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
  if (on_device && (rc = check_device_range(c, xyz, record_bytes(n, stride_bytes, false), which ? "rgc_ndt_set_source_device" : "rgc_ndt_set_target_device"))) return rc;
  Cloud& cl = c->ndt.cl[which];
  if ((rc = ensure(c, cl.in_copy, (size_t)n * 12))) return rc;
  HIPCHK(c, hipMemcpy2DAsync(cl.in_copy.p, 12, xyz, (size_t)stride_bytes, 12, (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  if (!on_device) HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller owns a host buffer for the duration of the call only
  cl.in = cl.in_copy.as<const float>();
  cl.stride_f = 3;
  cl.n = n;
  cl.ready = false;
  c->ndt.set[which] = true;
  c->ndt.built[which] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_set_target(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 0, xyz, n, stride_bytes, false); }
int rgc_ndt_set_source(rgc_ctx* c, const float* xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 1, xyz, n, stride_bytes, false); }
int rgc_ndt_set_target_device(rgc_ctx* c, const float* d_xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 0, d_xyz, n, stride_bytes, true); }
int rgc_ndt_set_source_device(rgc_ctx* c, const float* d_xyz, int n, int stride_bytes) { return ndt_set_cloud(c, 1, d_xyz, n, stride_bytes, true); }

int rgc_ndt_clear_source(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  c->ndt.set[1] = c->ndt.built[1] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_clear_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  c->ndt.set[0] = c->ndt.built[0] = false;
  ndt_drop_terms(c);
  return RGC_OK;
}
int rgc_ndt_swap_source_and_target(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  std::swap(c->ndt.cl[0], c->ndt.cl[1]);
  std::swap(c->ndt.set[0], c->ndt.set[1]);
  std::swap(c->ndt.built[0], c->ndt.built[1]);
  std::swap(c->ndt.built_res[0], c->ndt.built_res[1]);
  ndt_drop_terms(c);
  return RGC_OK;
}

static int ndt_scratch(rgc_ctx* c) {
  int rc;
  if ((rc = ensure(c, c->ndt.small, 64))) return rc;
  if ((rc = ensure(c, c->ndt.sums.out, sizeof(double) * 32))) return rc;
  if (!c->ndt.sums.h_out) HIPCHK(c, hipHostMalloc((void**)&c->ndt.sums.h_out, sizeof(double) * 32, hipHostMallocDefault));
  if (!c->ndt.h_small) HIPCHK(c, hipHostMalloc((void**)&c->ndt.h_small, sizeof(int) * 8, hipHostMallocDefault));
  return RGC_OK;
}

// the voxel map of NDT cloud `which` at the current resolution, if it is not there yet: the VGICP target's table construction (bounding box,
// counting sort by voxel, points of a voxel in ascending index) and one segmented pass (rgck::ndt_voxels)
static int ndt_build(rgc_ctx* c, int which) {
  Cloud& cl = c->ndt.cl[which];
  const double res = c->ndt.prm.resolution;
  if (c->ndt.built[which] && c->ndt.built_res[which] == res) return RGC_OK;
  c->ndt.built[which] = false;
  int rc;
  if ((rc = ndt_scratch(c))) return rc;
  hipStream_t s = c->stream;
  int* dsm = c->ndt.small.as<int>();
  int* hsm = c->ndt.h_small;
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
  c->ndt.built[which] = true;
  c->ndt.built_res[which] = res;
  return RGC_OK;
}

static int ndt_need_inputs(rgc_ctx* c) {
  if (!c->ndt.set[0]) return fail(c, RGC_ERR_NO_INPUT, "NDT target not set");
  if (!c->ndt.set[1]) return fail(c, RGC_ERR_NO_INPUT, "NDT source not set");
  int rc;
  if ((rc = ndt_build(c, 0))) return rc;
  if (c->ndt.prm.distance_mode == RGC_NDT_D2D && (rc = ndt_build(c, 1))) return rc;
  return RGC_OK;
}

// find: linearize at T (the term list and R_lin are made); else the cost at T over the frozen list.  H and b (nullable) and the cost out of the 28
// sums; the number of terms is kept when the list was made.
static int ndt_run_terms(rgc_ctx* c, const double T[16], bool find, double* H, double* b, double* cost) {
  int rc;
  if ((rc = ndt_scratch(c))) return rc;
  const int d2d = find ? (c->ndt.prm.distance_mode == RGC_NDT_D2D) : c->ndt.mode;
  const Cloud& tg = c->ndt.cl[0];
  const Cloud& sc = c->ndt.cl[1];
  const int n = find ? (d2d ? sc.nvox : sc.n) : c->ndt.n;
  if (find) {
    if (c->ndt.offs_h.empty()) neighbor_offsets_of(c->ndt.prm.neighbor_method, c->ndt.prm.neighbor_radius, c->ndt.offs_h);
    if (c->ndt.offs_dirty) {
      if ((rc = ensure(c, c->ndt.offs, sizeof(int) * 3 * RGC_NDT_MAX_OFFSETS))) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));  // (a launch that reads the former list may still run)
      HIPCHK(c, hipMemcpy(c->ndt.offs.p, c->ndt.offs_h.data(), sizeof(int) * c->ndt.offs_h.size(), hipMemcpyHostToDevice));
      c->ndt.offs_dirty = false;
    }
    c->ndt.valid = false;
    c->ndt.noff = (int)c->ndt.offs_h.size() / 3;
    c->ndt.n = n;
    c->ndt.mode = d2d;
    memcpy(c->ndt.Tlin, T, sizeof(double) * 16);
    if ((rc = ensure(c, c->ndt.corr, sizeof(int) * (size_t)n * c->ndt.noff))) return rc;
  }
  const int noff = c->ndt.noff;
  const int nb = rgck::ndt_blocks(n);
  if ((rc = ensure(c, c->ndt.sums.partials, sizeof(double) * rgck::kAccum * (size_t)nb))) return rc;
  if ((rc = ensure(c, c->ndt.ipartials, sizeof(int) * (size_t)nb))) return rc;
  rgck::ndt_terms(c->stream, d2d, find ? 1 : 0, sc.in, sc.stride_f, sc.vox.as<const double>(), n, pose_from(T), pose_from(c->ndt.Tlin), tg.grid,
                  tg.voxels(), c->ndt.offs.as<const int>(), noff, c->ndt.corr.as<int>(), (H && b) ? 1 : 0,
                  c->ndt.sums.partials.as<double>(), c->ndt.ipartials.as<int>(), c->ndt.sums.out.as<double>());
  if ((rc = read_system(c, c->ndt.sums, 29, H, b, cost))) return rc;
  if (find) {
    c->ndt.valid = true;
    c->ndt.terms = (int)c->ndt.sums.h_out[28];
  }
  return RGC_OK;
}

static int ndt_do_linearize(rgc_ctx* c, const double T[16], double* H, double* b, double* cost) {
  const int rc = ndt_need_inputs(c);
  return rc ? rc : ndt_run_terms(c, T, true, H, b, cost);
}

static int ndt_do_error(rgc_ctx* c, const double T[16], double* cost) {
  if (!c->ndt.set[0] || !c->ndt.set[1]) return fail(c, RGC_ERR_NO_INPUT, "NDT source or target not set");
  if (!c->ndt.valid) return fail(c, RGC_ERR_INVALID, "rgc_ndt_compute_error needs a preceding rgc_ndt_linearize");
  return ndt_run_terms(c, T, false, nullptr, nullptr, cost);
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
  if (!c->ndt.valid) return fail(c, RGC_ERR_INVALID, "rgc_ndt_num_correspondences needs a preceding rgc_ndt_linearize");
  *n = c->ndt.terms;
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
  if (!c->ndt.set[which]) return fail(c, RGC_ERR_NO_INPUT, "NDT %s not set", which ? "source" : "target");
  int rc = ndt_build(c, which);
  if (rc) return rc;
  const Cloud& cl = c->ndt.cl[which];
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
  const rgck::Grid& g = c->ndt.cl[which].grid;
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

}  // extern "C"
