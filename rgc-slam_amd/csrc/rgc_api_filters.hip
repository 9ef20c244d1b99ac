// rgc_api_filters.hip -- host side of the outlier filters (rgc_outlier_*): pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval of a cloud against
// itself on a grid of the filters' own (rgcapi::OutlierRecord, built by index_cloud like the search index's: the same automatic cell rule).  The
// kernels are rgc_filters.hip's; the semantics are stated in include/rgc_hip.h.  One chain per call -- the per-point value (mean distance or count) at
// the original index, SOR's statistics on the device, the flags in input order, their scan, the records -- and ONE read-back behind it (the read-out
// words and the number kept); what can refuse a call (the arguments, the grid build's flag word) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kFilterMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it

rgck::OutlierStats* dev_stats(rgc_ctx* c) { return stats<rgck::OutlierStats>(c->outlier.f); }  // (the frame's own word is the number kept)

struct FilterCall {  // what the two filters share: the staged cloud and where the outputs go on the device
  const float* d_in = nullptr;
  int stride_f = 0;
  float* d_out = nullptr;
  int* d_index = nullptr;
  void* d_val = nullptr;  // n floats (SOR) or ints (ROR): the caller's device buffer, or scratch
};

// the checks both filters make (after their own), the cloud on the device, its grid built, the outputs' places.  val: out_mean_dist / out_count
int filter_open(rgc_ctx* c, const char* who, const float* xyzc, int n, int stride_bytes, int on_device, float* out_xyzc, int* out_index, void* val, FilterCall* f) {
  if (n > kFilterMaxPoints) return fail(c, RGC_ERR_INVALID, "%s: cloud has %d points, the limit is 2^27", who, n);
  HIPCHK(c, hipSetDevice(c->device));
  rgcapi::OutlierRecord& r = c->outlier;
  const size_t nn = (size_t)n;
  int rc;
  if ((rc = frame_open(c, r.f))) return rc;
  if ((rc = stage_records(c, xyzc, n, stride_bytes, on_device, out_xyzc != nullptr, r.in, "input cloud", &f->d_in))) return rc;
  if ((rc = place_output(c, out_xyzc, 16 * nn, on_device, r.sel.out, "out_xyzc", &f->d_out))) return rc;
  if ((rc = place_output(c, out_index, sizeof(int) * nn, on_device, r.sel.idx, "out_index", &f->d_index))) return rc;
  if ((rc = place_output(c, val, 4 * nn, on_device, r.val, "the per-point output", &f->d_val, true))) return rc;
  f->stride_f = stride_bytes / 4;
  if ((rc = selection_scratch(c, r.sel, n))) return rc;
  double cell = 0.0;
  if ((rc = index_cloud(c, r.f, f->d_in, f->stride_f, n, who, "the cloud", "the filter's grid", &cell))) return rc;
  r.info.cell = cell;
  r.info.cells = r.f.cl.grid.ncell;
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::OutlierStats), c->stream));
  return RGC_OK;
}

// the decision in input order, its scan, the records; then the one read-back and a host caller's results
int filter_close(rgc_ctx* c, const FilterCall& f, int n, int on_device, const float* d_mean, const int* d_cnt, int min_nb, int negative, float* out_xyzc, int* out_index,
                 void* val, int* n_out) {
  rgcapi::OutlierRecord& r = c->outlier;
  int rc;
  rgck::outlier_flag(c->stream, d_mean, d_cnt, n, dev_stats(c), min_nb, negative, r.sel.flag.as<int>());
  const EmitTo to{f.d_out, f.d_index, out_xyzc, out_index};
  const EmitHome home{r.f.h + kFrameStatsAt, dev_stats(c), sizeof(rgck::OutlierStats), host_words(r.f)};
  if ((rc = emit_selected(c, r.sel, f.d_in, f.stride_f, n, on_device, to, home))) return rc;
  const int kept = *host_words(r.f);
  if (!on_device) {
    if ((rc = copy_out(c, val, f.d_val, 4 * (size_t)n, 0))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  const rgck::OutlierStats& st = *host_stats<rgck::OutlierStats>(r.f);
  r.info.n = n;
  r.info.n_out = kept;
  r.info.candidates = (long long)sum_words(st.words, 0);
  r.info.grown = (int)sum_words(st.words, 1);
  *n_out = kept;
  return RGC_OK;
}

}  // namespace

extern "C" {

int rgc_outlier_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  return set_cell_of(c, &c->outlier.f.cell, cell, "rgc_outlier_set_cell");
}

int rgc_outlier_get_info(rgc_ctx* c, rgc_outlier_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->outlier.info;
  return RGC_OK;
}

int rgc_outlier_statistical(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, int on_device, int mean_k, double std_mul, int negative, float* out_xyzc,
                            int* out_index, float* out_mean_dist, int* n_out) {
  if (!c || !n_out || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  if (mean_k < 1 || mean_k > RGC_OUTLIER_MAX_MEAN_K) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: mean_k in 1..%d", RGC_OUTLIER_MAX_MEAN_K);
  if (!std::isfinite(std_mul) || !stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: std_mul must be finite, stride_bytes a multiple of 4 between 12 and 4096");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: a solve is in flight");
  *n_out = 0;
  c->outlier.info = rgc_outlier_info{};
  if (n == 0) return RGC_OK;
  if (n < 2 || n <= mean_k) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: %d points, mean_k = %d neighbours need more than that (and at least 2)", n, mean_k);
  FilterCall f;
  int rc;
  if ((rc = filter_open(c, "rgc_outlier_statistical", xyzc, n, stride_bytes, on_device, out_xyzc, out_index, out_mean_dist, &f))) return rc;
  if ((rc = ensure(c, c->outlier.partials, sizeof(double) * 2 * (size_t)rgck::outlier_stat_rows(n)))) return rc;
  float* d = static_cast<float*>(f.d_val);
  rgck::sor_meandist(c->stream, c->outlier.f.cl.sorted(), mean_k, d, dev_stats(c));
  rgck::sor_stats(c->stream, d, n, std_mul, c->outlier.partials.as<double>(), dev_stats(c));
  if ((rc = filter_close(c, f, n, on_device, d, nullptr, 0, negative, out_xyzc, out_index, out_mean_dist, n_out))) return rc;
  const rgck::OutlierStats& st = *host_stats<rgck::OutlierStats>(c->outlier.f);
  c->outlier.info.mean = st.mean;
  c->outlier.info.stddev = st.stddev;
  c->outlier.info.threshold = st.threshold;
  return RGC_OK;
}

int rgc_outlier_radius(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, int on_device, double radius, int min_neighbors, int negative, float* out_xyzc,
                       int* out_index, int* out_count, int* n_out) {
  if (!c || !n_out || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  const float r2 = (float)(radius * radius);
  if (!std::isfinite(radius) || radius <= 0.0 || !std::isfinite(r2)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_radius: the radius must be finite and > 0, float(r r) finite");
  if (min_neighbors < 0 || !stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_radius: min_neighbors >= 0, stride_bytes a multiple of 4 between 12 and 4096");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_radius: a solve is in flight");
  *n_out = 0;
  c->outlier.info = rgc_outlier_info{};
  if (n == 0) return RGC_OK;
  FilterCall f;
  int rc;
  if ((rc = filter_open(c, "rgc_outlier_radius", xyzc, n, stride_bytes, on_device, out_xyzc, out_index, out_count, &f))) return rc;
  int* cnt = static_cast<int*>(f.d_val);
  rgck::ror_count(c->stream, c->outlier.f.cl.sorted(), r2, radius, min_neighbors, out_count != nullptr, cnt, dev_stats(c));
  return filter_close(c, f, n, on_device, nullptr, cnt, min_neighbors, negative, out_xyzc, out_index, out_count, n_out);
}

}  // extern "C"
