// rgc_api_normals.hip -- host side of surface normal estimation (rgc_normal_*): pcl::NormalEstimation of a cloud against a surface cloud (or itself) on a
// grid of the call's own (rgcapi::NormalRecord, built by index_cloud like the search index's: the same automatic cell rule).  The kernels are
// rgc_normals.hip's; the semantics are stated in include/rgc_hip.h.  One chain per call -- the queries' finiteness check, the surface's grid, the fused
// estimate straight into the caller's device buffers (or scratch for a host caller) -- and ONE read-back behind it (the read-out words); what can refuse
// a call (the arguments, the grid build's flag word, the queries' flag) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kNormalMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it

rgck::NormalStats* dev_stats(rgc_ctx* c) { return stats<rgck::NormalStats>(c->normal.f); }  // (the frame's own word is the queries' non-finite flag)

}  // namespace

extern "C" {

void rgc_default_normal_params(rgc_normal_params* p) {
  if (!p) return;
  *p = rgc_normal_params{};
  p->flip = 1;
}

int rgc_normal_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  return set_cell_of(c, &c->normal.f.cell, cell, "rgc_normal_set_cell");
}

int rgc_normal_get_info(rgc_ctx* c, rgc_normal_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->normal.info;
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
  c->normal.info = rgc_normal_info{};
  c->normal.info.route = by_k ? RGC_NORMAL_ROUTE_K : RGC_NORMAL_ROUTE_RADIUS;
  if (n == 0) return RGC_OK;
  const int ns = surface ? n_surface : n;
  HIPCHK(c, hipSetDevice(c->device));
  rgcapi::NormalRecord& r = c->normal;
  int rc;
  if ((rc = frame_open(c, r.f))) return rc;
  hipStream_t s = c->stream;
  const float *dq = nullptr, *dsurf = nullptr;
  int qs = 0, ss = 0;
  if ((rc = stage_cloud(c, xyzc, n, stride_bytes, on_device, r.q, "the query cloud", &dq, &qs))) return rc;
  if (surface) {
    if ((rc = stage_cloud(c, surface, ns, surface_stride_bytes, on_device, r.surf, "the surface cloud", &dsurf, &ss))) return rc;
  } else {
    dsurf = dq;
    ss = qs;
  }
  const size_t nn = (size_t)n;
  rgck::NormalOut out{};
  if ((rc = place_output(c, out_normal4, 16 * nn, on_device, r.n4, "out_normal4", &out.n4))) return rc;
  if ((rc = place_output(c, out_cov6, 48 * nn, on_device, r.cov, "out_cov6", &out.cov6))) return rc;
  if ((rc = place_output(c, out_centroid, 24 * nn, on_device, r.cen, "out_centroid", &out.cen))) return rc;
  if ((rc = place_output(c, out_count, 4 * nn, on_device, r.cnt, "out_count", &out.cnt))) return rc;
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::NormalStats), s));
  int* const h_flag = host_words(r.f);
  *h_flag = 0;
  if (surface) {  // (a cloud that is its own surface is checked by its grid build)
    rgck::normal_check(s, dq, qs, n, &dev_stats(c)->nonfinite);
    HIPCHK(c, hipMemcpyAsync(h_flag, &dev_stats(c)->nonfinite, sizeof(int), hipMemcpyDeviceToHost, s));  // (home with the grid's measurement)
  }
  const Cloud& cl = r.f.cl;
  double cell = 0.0;
  if ((rc = index_cloud(c, r.f, dsurf, ss, ns, "rgc_normal_estimate", "the surface cloud", "the normals' grid", &cell))) return rc;
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
  HIPCHK(c, hipMemcpyAsync(r.f.h + kFrameStatsAt, dev_stats(c), sizeof(rgck::NormalStats), hipMemcpyDeviceToHost, s));
  if (!on_device) {
    if ((rc = copy_out(c, out_normal4, out.n4, 16 * nn, 0))) return rc;
    if ((rc = copy_out(c, out_cov6, out.cov6, 48 * nn, 0))) return rc;
    if ((rc = copy_out(c, out_centroid, out.cen, 24 * nn, 0))) return rc;
    if ((rc = copy_out(c, out_count, out.cnt, 4 * nn, 0))) return rc;
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const rgck::NormalStats& st = *host_stats<rgck::NormalStats>(r.f);
  rgc_normal_info& info = r.info;
  info.n = n;
  info.n_surface = ns;
  info.n_valid = (int)sum_words(st.words, 2);
  info.cell = cell;
  info.cells = cl.grid.ncell;
  info.candidates = (long long)sum_words(st.words, 0);
  info.grown = (int)sum_words(st.words, 1);
  *n_valid = info.n_valid;
  return RGC_OK;
}

}  // extern "C"
