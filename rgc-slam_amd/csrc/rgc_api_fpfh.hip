// rgc_api_fpfh.hip -- host side of the FPFH descriptors (rgc_fpfh_*): pcl::FPFHEstimation of a cloud against a surface cloud (or itself) and that
// surface's normals, on a grid of the call's own (rgcapi::FpfhRecord, built by index_cloud like the normals': the same automatic cell rule).  The
// kernels are rgc_fpfh.hip's; the semantics are stated in include/rgc_hip.h.  One chain per call -- the finiteness check and the normals' float4 form, the
// surface's grid, (a separate surface: the marks, their scan, the list,) the SPFH pass, the combine pass straight into the caller's device buffers (or
// scratch for a host caller) -- and ONE read-back behind it (the read-out words and the list's length); what can refuse a call (the arguments, the grid
// build's flag word, the queries' flag) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kFpfhMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it

rgck::FpfhStats* dev_stats(rgc_ctx* c) { return stats<rgck::FpfhStats>(c->fpfh.f); }  // (the frame's own words: the queries' non-finite flag, the number of listed surface points)

}  // namespace

extern "C" {

void rgc_default_fpfh_params(rgc_fpfh_params* p) {
  if (p) *p = rgc_fpfh_params{};
}

int rgc_fpfh_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  return set_cell_of(c, &c->fpfh.f.cell, cell, "rgc_fpfh_set_cell");
}

int rgc_fpfh_get_info(rgc_ctx* c, rgc_fpfh_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->fpfh.info;
  return RGC_OK;
}

int rgc_fpfh_estimate(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, const float* surface, int n_surface, int surface_stride_bytes, const float* normals,
                      int normal_stride_bytes, int on_device, const rgc_fpfh_params* params, float* out_fpfh, unsigned* out_spfh, int* out_spfh_count, int* out_count,
                      int* n_valid) {
  if (!c || !params || !n_valid || n < 0 || (n > 0 && (!xyzc || !normals))) return RGC_ERR_INVALID;
  const double radius = params->radius;
  const float r2 = (float)(radius * radius);
  if (!(std::isfinite(radius) && radius > 0.0 && std::isfinite(r2) && r2 > 0.f))
    return fail(c, RGC_ERR_INVALID, "rgc_fpfh_estimate: the radius must be finite and > 0, float(r r) finite and > 0");
  if (!stride_ok(stride_bytes) || !stride_ok(normal_stride_bytes) || (surface && (n_surface <= 0 || !stride_ok(surface_stride_bytes))))
    return fail(c, RGC_ERR_INVALID, "rgc_fpfh_estimate: strides are multiples of 4 between 12 and 4096, a surface cloud has at least one point");
  if (n > kFpfhMaxPoints || (surface && n_surface > kFpfhMaxPoints)) return fail(c, RGC_ERR_INVALID, "rgc_fpfh_estimate: a cloud has more than 2^27 points");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_fpfh_estimate: a solve is in flight");
  *n_valid = 0;
  c->fpfh.info = rgc_fpfh_info{};
  if (n == 0) return RGC_OK;
  const int ns = surface ? n_surface : n;
  HIPCHK(c, hipSetDevice(c->device));
  rgcapi::FpfhRecord& r = c->fpfh;
  int rc;
  if ((rc = frame_open(c, r.f))) return rc;
  hipStream_t s = c->stream;
  const float *dq = nullptr, *dsurf = nullptr, *dnrm = nullptr;
  int qs = 0, ss = 0, nrs = 0;
  if ((rc = stage_cloud(c, xyzc, n, stride_bytes, on_device, r.q, "the query cloud", &dq, &qs))) return rc;
  if (surface) {
    if ((rc = stage_cloud(c, surface, ns, surface_stride_bytes, on_device, r.surf, "the surface cloud", &dsurf, &ss))) return rc;
  } else {
    dsurf = dq;
    ss = qs;
  }
  if ((rc = stage_cloud(c, normals, ns, normal_stride_bytes, on_device, r.nrm, "the normals", &dnrm, &nrs))) return rc;
  const size_t nn = (size_t)n, nsz = (size_t)ns;
  float* d_out = nullptr;
  unsigned* d_spfh = nullptr;
  int *d_m = nullptr, *d_cnt = nullptr;
  if ((rc = place_output(c, out_fpfh, 4 * RGC_FPFH_BINS * nn, on_device, r.out, "out_fpfh", &d_out))) return rc;
  if ((rc = place_output(c, out_count, 4 * nn, on_device, r.cnt, "out_count", &d_cnt))) return rc;
  // the first pass' counts and row sizes are the second pass' input: the caller's buffers where asked for (device), else scratch
  if ((rc = place_output(c, out_spfh, 4 * RGC_FPFH_BINS * nsz, on_device, r.spfh, "out_spfh", &d_spfh, true))) return rc;
  if ((rc = place_output(c, out_spfh_count, 4 * nsz, on_device, r.m, "out_spfh_count", &d_m, true))) return rc;
  if ((rc = ensure(c, r.n4, 16 * nsz))) return rc;
  if (surface) {
    if ((rc = ensure(c, r.flag, sizeof(int) * (nsz + 1)))) return rc;
    if ((rc = ensure(c, r.off, sizeof(int) * (nsz + 1)))) return rc;
    if ((rc = ensure(c, r.bs, sizeof(int) * ((nsz + 1) / 2048 + 2)))) return rc;
    if ((rc = ensure(c, r.list, sizeof(int) * nsz))) return rc;
  }
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::FpfhStats), s));
  int* const h_flag = host_words(r.f);
  int* const h_list = h_flag + 1;
  *h_flag = 0;
  *h_list = ns;
  float4* const n4 = r.n4.as<float4>();
  // (a cloud that is its own surface is checked by its grid build: a null query array)
  rgck::fpfh_check(s, surface ? dq : nullptr, qs, n, dnrm, nrs, ns, n4, &dev_stats(c)->nonfinite);
  if (surface) HIPCHK(c, hipMemcpyAsync(h_flag, &dev_stats(c)->nonfinite, sizeof(int), hipMemcpyDeviceToHost, s));  // (home with the grid's measurement)
  const Cloud& cl = r.f.cl;
  double cell = 0.0;
  if ((rc = index_cloud(c, r.f, dsurf, ss, ns, "rgc_fpfh_estimate", "the surface cloud", "the descriptors' grid", &cell))) return rc;
  if (*h_flag) return fail(c, RGC_ERR_NONFINITE, "rgc_fpfh_estimate: a query has a non-finite coordinate");
  const rgck::SortedCloud sc = cl.sorted();
  if (surface) {  // only the SPFHs some query's row holds: the marks, their scan, the list; the rest reads as "not computed"
    int* const flag = r.flag.as<int>();
    int* const off = r.off.as<int>();
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int) * (nsz + 1), s));
    HIPCHK(c, hipMemsetAsync(d_spfh, 0, 4 * RGC_FPFH_BINS * nsz, s));
    HIPCHK(c, hipMemsetAsync(d_m, 0xff, 4 * nsz, s));
    rgck::fpfh_mark(s, dq, qs, n, sc, r2, radius, flag, dev_stats(c));
    rgck::exclusive_scan(s, flag, off, ns + 1, r.bs.as<int>());
    rgck::fpfh_list(s, flag, off, ns, r.list.as<int>());
    HIPCHK(c, hipMemcpyAsync(h_list, off + ns, sizeof(int), hipMemcpyDeviceToHost, s));
    rgck::fpfh_spfh(s, sc, r.list.as<const int>(), off + ns, n4, r2, radius, d_spfh, d_m, dev_stats(c));
  } else {
    rgck::fpfh_spfh(s, sc, nullptr, nullptr, n4, r2, radius, d_spfh, d_m, dev_stats(c));
  }
  rgck::fpfh_combine(s, surface ? dq : nullptr, qs, n, sc, d_spfh, d_m, r2, radius, d_out, d_cnt, dev_stats(c));
  HIPCHK(c, hipMemcpyAsync(r.f.h + kFrameStatsAt, dev_stats(c), sizeof(rgck::FpfhStats), hipMemcpyDeviceToHost, s));
  if (!on_device) {
    if ((rc = copy_out(c, out_fpfh, d_out, 4 * RGC_FPFH_BINS * nn, 0))) return rc;
    if ((rc = copy_out(c, out_count, d_cnt, 4 * nn, 0))) return rc;
    if ((rc = copy_out(c, out_spfh, d_spfh, 4 * RGC_FPFH_BINS * nsz, 0))) return rc;
    if ((rc = copy_out(c, out_spfh_count, d_m, 4 * nsz, 0))) return rc;
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const rgck::FpfhStats& st = *host_stats<rgck::FpfhStats>(r.f);
  rgc_fpfh_info& info = r.info;
  info.n = n;
  info.n_surface = ns;
  info.n_valid = (int)sum_words(st.words, 2);
  info.n_spfh = *h_list;
  info.cell = cell;
  info.cells = cl.grid.ncell;
  info.pairs = (long long)sum_words(st.words, 1);
  info.candidates = (long long)sum_words(st.words, 0);
  *n_valid = info.n_valid;
  return RGC_OK;
}

}  // extern "C"
