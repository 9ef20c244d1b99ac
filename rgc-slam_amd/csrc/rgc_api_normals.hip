// rgc_api_normals.hip -- host side of surface normal estimation (rgc_normal_*): pcl::NormalEstimation of a cloud against a surface cloud (or itself) on a
// grid of the call's own (rgc_ctx::normal_cl, built by build_search_grid like the search index's: the same automatic cell rule).  The kernels are
// rgc_normals.hip's; the semantics are stated in include/rgc_hip.h.  One chain per call -- the queries' finiteness check, the surface's grid, the fused
// estimate straight into the caller's device buffers (or scratch for a host caller) -- and ONE read-back behind it (the read-out words); what can refuse
// a call (the arguments, the grid build's flag word, the queries' flag) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kNormalMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it
constexpr size_t kFlagAt = 32;             // rgc_ctx::normal_h: the 8 ints of the grid's measurement, the queries' non-finite flag ...
constexpr size_t kStatsAt = 64;            // ... and (normal_small too) what the kernels post (rgck::NormalStats)
constexpr size_t kSmallBytes = 4096;
static_assert(kStatsAt + sizeof(rgck::NormalStats) <= kSmallBytes, "the read-out words fit");

rgck::NormalStats* dev_stats(rgc_ctx* c) { return reinterpret_cast<rgck::NormalStats*>(c->normal_small.as<unsigned char>() + kStatsAt); }
const rgck::NormalStats* host_stats(rgc_ctx* c) { return reinterpret_cast<const rgck::NormalStats*>(c->normal_h + kStatsAt); }

}  // namespace

int rgcapi::stage_cloud(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, DevBuf& stage, const char* what, const float** d, int* stride_f) {
  int rc;
  if (on_device) {
    if ((rc = check_device_range(c, p, (size_t)n * stride_bytes - (stride_bytes - 12), what))) return rc;
    *d = p;
    *stride_f = stride_bytes / 4;
    return RGC_OK;
  }
  if ((rc = ensure(c, stage, (size_t)n * 12))) return rc;
  HIPCHK(c, hipMemcpy2DAsync(stage.p, 12, p, (size_t)stride_bytes, 12, (size_t)n, hipMemcpyHostToDevice, c->stream));
  *d = stage.as<const float>();
  *stride_f = 3;
  return RGC_OK;
}

extern "C" {

void rgc_default_normal_params(rgc_normal_params* p) {
  if (!p) return;
  *p = rgc_normal_params{};
  p->flip = 1;
}

int rgc_normal_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  if (!std::isfinite(cell) || cell < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_normal_set_cell: cell must be finite and >= 0");
  c->normal_cell = cell;
  return RGC_OK;
}

int rgc_normal_get_info(rgc_ctx* c, rgc_normal_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->normal_info;
  return RGC_OK;
}

int rgc_normal_estimate(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, const float* surface, int n_surface, int surface_stride_bytes, int on_device,
                        const rgc_normal_params* params, float* out_normal4, double* out_cov6, double* out_centroid, int* out_count, int* n_valid) {
  if (!c || !params || !n_valid || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  const rgc_normal_params& p = *params;
  const bool by_k = p.k != 0, by_radius = !(p.radius == 0.0);
  if (by_k == by_radius) return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: exactly one of k and radius selects the neighbourhood");
  if (by_k && (p.k < 3 || p.k > RGC_NORMAL_MAX_K)) return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: k in 3..%d", RGC_NORMAL_MAX_K);
  const float r2 = (float)(p.radius * p.radius);
  if (by_radius && !(std::isfinite(p.radius) && p.radius > 0.0 && std::isfinite(r2) && r2 > 0.f))
    return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: the radius must be finite and > 0, float(r r) finite and > 0");
  if (!std::isfinite(p.viewpoint[0]) || !std::isfinite(p.viewpoint[1]) || !std::isfinite(p.viewpoint[2]) || (p.flip != 0 && p.flip != 1))
    return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: the viewpoint must be finite, flip 0 or 1");
  if (!stride_ok(stride_bytes) || (surface && (n_surface <= 0 || !stride_ok(surface_stride_bytes))))
    return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: strides are multiples of 4 between 12 and 4096, a surface cloud has at least one point");
  if (n > kNormalMaxPoints || (surface && n_surface > kNormalMaxPoints)) return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: a cloud has more than 2^27 points");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_normal_estimate: a solve is in flight");
  *n_valid = 0;
  c->normal_info = rgc_normal_info{};
  c->normal_info.route = by_k ? RGC_NORMAL_ROUTE_K : RGC_NORMAL_ROUTE_RADIUS;
  if (n == 0) return RGC_OK;
  const int ns = surface ? n_surface : n;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->normal_small, kSmallBytes))) return rc;
  if (!c->normal_h) HIPCHK(c, hipHostMalloc((void**)&c->normal_h, kSmallBytes, hipHostMallocDefault));
  hipStream_t s = c->stream;
  const float *dq = nullptr, *dsurf = nullptr;
  int qs = 0, ss = 0;
  if ((rc = stage_cloud(c, xyzc, n, stride_bytes, on_device, c->normal_q, "the query cloud", &dq, &qs))) return rc;
  if (surface) {
    if ((rc = stage_cloud(c, surface, ns, surface_stride_bytes, on_device, c->normal_surf, "the surface cloud", &dsurf, &ss))) return rc;
  } else {
    dsurf = dq;
    ss = qs;
  }
  const size_t nn = (size_t)n;
  rgck::NormalOut out{};
  if ((rc = place_output(c, out_normal4, 16 * nn, on_device, c->normal_n4, "out_normal4", &out.n4))) return rc;
  if ((rc = place_output(c, out_cov6, 48 * nn, on_device, c->normal_cov, "out_cov6", &out.cov6))) return rc;
  if ((rc = place_output(c, out_centroid, 24 * nn, on_device, c->normal_cen, "out_centroid", &out.cen))) return rc;
  if ((rc = place_output(c, out_count, 4 * nn, on_device, c->normal_cnt, "out_count", &out.cnt))) return rc;
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::NormalStats), s));
  int* const h_flag = reinterpret_cast<int*>(c->normal_h + kFlagAt);
  *h_flag = 0;
  if (surface) {  // (a cloud that is its own surface is checked by its grid build)
    rgck::normal_check(s, dq, qs, n, &dev_stats(c)->nonfinite);
    HIPCHK(c, hipMemcpyAsync(h_flag, &dev_stats(c)->nonfinite, sizeof(int), hipMemcpyDeviceToHost, s));  // (home with the grid's measurement)
  }
  Cloud& cl = c->normal_cl;
  cl.in = dsurf;
  cl.stride_f = ss;
  cl.n = ns;
  cl.ready = false;
  double cell = c->normal_cell;
  rc = build_search_grid(c, cl, &cell, c->normal_small.as<int>(), reinterpret_cast<int*>(c->normal_h), "rgc_normal_estimate", "the surface cloud", "the normals' grid");
  cl.in = nullptr;  // (the caller's buffer is not kept beyond the call)
  if (rc) return rc;
  if (*h_flag) return fail(c, RGC_ERR_NONFINITE, "rgc_normal_estimate: a query has a non-finite coordinate");
  const rgck::NormalSign sg{p.viewpoint[0], p.viewpoint[1], p.viewpoint[2], p.flip};
  // a cloud that is its own surface is walked in the grid's sorted order (a null query array): measured to pay, EXPERIMENTS.md "Normal estimation"
#ifdef RGC_LAB_NORMAL_INPUT_ORDER  // developer build: the self-surface case in input order too, what scripts/bench_normals.py compares with
  const float* const walk = dq;
#else
  const float* const walk = surface ? dq : nullptr;
#endif
  if (by_k) rgck::normal_knn(s, walk, qs, n, dsurf, ss, cl.sorted(), p.k, sg, out, dev_stats(c));
  else rgck::normal_radius(s, walk, qs, n, cl.sorted(), r2, p.radius, sg, out, dev_stats(c));
  HIPCHK(c, hipMemcpyAsync(c->normal_h + kStatsAt, dev_stats(c), sizeof(rgck::NormalStats), hipMemcpyDeviceToHost, s));
  if (!on_device) {
    if (out_normal4) HIPCHK(c, hipMemcpyAsync(out_normal4, out.n4, 16 * nn, hipMemcpyDeviceToHost, s));
    if (out_cov6) HIPCHK(c, hipMemcpyAsync(out_cov6, out.cov6, 48 * nn, hipMemcpyDeviceToHost, s));
    if (out_centroid) HIPCHK(c, hipMemcpyAsync(out_centroid, out.cen, 24 * nn, hipMemcpyDeviceToHost, s));
    if (out_count) HIPCHK(c, hipMemcpyAsync(out_count, out.cnt, 4 * nn, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const rgck::NormalStats& st = *host_stats(c);
  unsigned long long candidates = 0, grown = 0, valid = 0;
  for (int j = 0; j < rgck::kNormalSlots; j++) {
    candidates += st.words[j][0];
    grown += st.words[j][1];
    valid += st.words[j][2];
  }
  rgc_normal_info& info = c->normal_info;
  info.n = n;
  info.n_surface = ns;
  info.n_valid = (int)valid;
  info.cell = cell;
  info.cells = cl.grid.ncell;
  info.candidates = (long long)candidates;
  info.grown = (int)grown;
  *n_valid = (int)valid;
  return RGC_OK;
}

}  // extern "C"
