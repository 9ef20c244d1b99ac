// rgc_api_filters.hip -- host side of the outlier filters (rgc_outlier_*): pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval of a cloud against
// itself on a grid of the filters' own (rgc_ctx::filter_cl, built by build_search_grid like the search index's: the same automatic cell rule).  The
// kernels are rgc_filters.hip's; the semantics are stated in include/rgc_hip.h.  One chain per call -- the per-point value (mean distance or count) at
// the original index, SOR's statistics on the device, the flags in input order, their scan, the records -- and ONE read-back behind it (the read-out
// words and the number kept); what can refuse a call (the arguments, the grid build's flag word) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kFilterMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it
constexpr size_t kKeptAt = 32;             // rgc_ctx::filter_small / filter_h: the 8 ints of the grid's measurement, the number kept (the scan's last offset) ...
constexpr size_t kStatsAt = 64;            // ... and what the kernels post (rgck::OutlierStats: the statistics, the read-out words' slots)
constexpr size_t kSmallBytes = 4096;
static_assert(kStatsAt + sizeof(rgck::OutlierStats) <= kSmallBytes, "the read-out words fit");

rgck::OutlierStats* dev_stats(rgc_ctx* c) { return reinterpret_cast<rgck::OutlierStats*>(c->filter_small.as<unsigned char>() + kStatsAt); }
const rgck::OutlierStats* host_stats(rgc_ctx* c) { return reinterpret_cast<const rgck::OutlierStats*>(c->filter_h + kStatsAt); }

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
  int rc;
  if ((rc = ensure(c, c->filter_small, kSmallBytes))) return rc;
  if (!c->filter_h) HIPCHK(c, hipHostMalloc((void**)&c->filter_h, kSmallBytes, hipHostMallocDefault));
  const size_t nn = (size_t)n;
  if (on_device) {
    if ((rc = check_device_range(c, xyzc, nn * stride_bytes - (stride_bytes - 12), "input cloud"))) return rc;
    if (out_xyzc && (rc = check_device_range(c, out_xyzc, 16 * nn, "out_xyzc"))) return rc;
    if (out_index && (rc = check_device_range(c, out_index, sizeof(int) * nn, "out_index"))) return rc;
    if (val && (rc = check_device_range(c, val, 4 * nn, "the per-point output"))) return rc;
    f->d_in = xyzc;
    f->d_out = out_xyzc;
    f->d_index = out_index;
  } else {
    if ((rc = ensure(c, c->filter_in, nn * stride_bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->filter_in.p, xyzc, nn * stride_bytes, hipMemcpyHostToDevice, c->stream));
    f->d_in = c->filter_in.as<const float>();
    if (out_xyzc) {
      if ((rc = ensure(c, c->filter_out, 16 * nn))) return rc;
      f->d_out = c->filter_out.as<float>();
    }
    if (out_index) {
      if ((rc = ensure(c, c->filter_idx, sizeof(int) * nn))) return rc;
      f->d_index = c->filter_idx.as<int>();
    }
  }
  f->stride_f = stride_bytes / 4;
  f->d_val = on_device ? val : nullptr;
  if (!f->d_val) {
    if ((rc = ensure(c, c->filter_val, 4 * nn))) return rc;
    f->d_val = c->filter_val.p;
  }
  if ((rc = ensure(c, c->filter_flag, sizeof(int) * (nn + 1)))) return rc;
  if ((rc = ensure(c, c->filter_off, sizeof(int) * (nn + 1)))) return rc;
  if ((rc = ensure(c, c->filter_bs, sizeof(int) * ((nn + 1) / 2048 + 2)))) return rc;
  Cloud& cl = c->filter_cl;
  cl.in = f->d_in;
  cl.stride_f = f->stride_f;
  cl.n = n;
  cl.ready = false;
  double cell = c->outlier_cell;
  rc = build_search_grid(c, cl, &cell, c->filter_small.as<int>(), reinterpret_cast<int*>(c->filter_h), who, "the cloud", "the filter's grid");
  cl.in = nullptr;  // (the caller's buffer is not kept beyond the call)
  if (rc) return rc;
  c->outlier_info.cell = cell;
  c->outlier_info.cells = cl.grid.ncell;
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::OutlierStats), c->stream));
  return RGC_OK;
}

// the decision in input order, its scan, the records; then the one read-back and a host caller's results
int filter_close(rgc_ctx* c, const FilterCall& f, int n, int on_device, const float* d_mean, const int* d_cnt, int min_nb, int negative, float* out_xyzc, int* out_index,
                 void* val, int* n_out) {
  hipStream_t s = c->stream;
  int* flag = c->filter_flag.as<int>();
  int* off = c->filter_off.as<int>();
  rgck::outlier_flag(s, d_mean, d_cnt, n, dev_stats(c), min_nb, negative, flag);
  rgck::exclusive_scan(s, flag, off, n + 1, c->filter_bs.as<int>());
  rgck::outlier_emit(s, f.d_in, f.stride_f, n, flag, off, f.d_out, f.d_index);
  HIPCHK(c, hipMemcpyAsync(c->filter_h + kStatsAt, dev_stats(c), sizeof(rgck::OutlierStats), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(c->filter_h + kKeptAt, off + n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const int kept = *reinterpret_cast<const int*>(c->filter_h + kKeptAt);
  if (!on_device) {
    if (out_xyzc && kept) HIPCHK(c, hipMemcpyAsync(out_xyzc, f.d_out, 16 * (size_t)kept, hipMemcpyDeviceToHost, s));
    if (out_index && kept) HIPCHK(c, hipMemcpyAsync(out_index, f.d_index, sizeof(int) * (size_t)kept, hipMemcpyDeviceToHost, s));
    if (val) HIPCHK(c, hipMemcpyAsync(val, f.d_val, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  const rgck::OutlierStats& st = *host_stats(c);
  unsigned long long candidates = 0, grown = 0;
  for (int j = 0; j < rgck::kOutlierSlots; j++) {
    candidates += st.words[j][0];
    grown += st.words[j][1];
  }
  c->outlier_info.n = n;
  c->outlier_info.n_out = kept;
  c->outlier_info.candidates = (long long)candidates;
  c->outlier_info.grown = (int)grown;
  *n_out = kept;
  return RGC_OK;
}

}  // namespace

extern "C" {

int rgc_outlier_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  if (!std::isfinite(cell) || cell < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_outlier_set_cell: cell must be finite and >= 0");
  c->outlier_cell = cell;
  return RGC_OK;
}

int rgc_outlier_get_info(rgc_ctx* c, rgc_outlier_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->outlier_info;
  return RGC_OK;
}

int rgc_outlier_statistical(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, int on_device, int mean_k, double std_mul, int negative, float* out_xyzc,
                            int* out_index, float* out_mean_dist, int* n_out) {
  if (!c || !n_out || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  if (mean_k < 1 || mean_k > RGC_OUTLIER_MAX_MEAN_K) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: mean_k in 1..%d", RGC_OUTLIER_MAX_MEAN_K);
  if (!std::isfinite(std_mul) || !stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: std_mul must be finite, stride_bytes a multiple of 4 between 12 and 4096");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: a solve is in flight");
  *n_out = 0;
  c->outlier_info = rgc_outlier_info{};
  if (n == 0) return RGC_OK;
  if (n < 2 || n <= mean_k) return fail(c, RGC_ERR_INVALID, "rgc_outlier_statistical: %d points, mean_k = %d neighbours need more than that (and at least 2)", n, mean_k);
  FilterCall f;
  int rc;
  if ((rc = filter_open(c, "rgc_outlier_statistical", xyzc, n, stride_bytes, on_device, out_xyzc, out_index, out_mean_dist, &f))) return rc;
  if ((rc = ensure(c, c->filter_partials, sizeof(double) * 2 * (size_t)rgck::outlier_stat_rows(n)))) return rc;
  float* d = static_cast<float*>(f.d_val);
  rgck::sor_meandist(c->stream, c->filter_cl.sorted(), mean_k, d, dev_stats(c));
  rgck::sor_stats(c->stream, d, n, std_mul, c->filter_partials.as<double>(), dev_stats(c));
  if ((rc = filter_close(c, f, n, on_device, d, nullptr, 0, negative, out_xyzc, out_index, out_mean_dist, n_out))) return rc;
  const rgck::OutlierStats& st = *host_stats(c);
  c->outlier_info.mean = st.mean;
  c->outlier_info.stddev = st.stddev;
  c->outlier_info.threshold = st.threshold;
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
  c->outlier_info = rgc_outlier_info{};
  if (n == 0) return RGC_OK;
  FilterCall f;
  int rc;
  if ((rc = filter_open(c, "rgc_outlier_radius", xyzc, n, stride_bytes, on_device, out_xyzc, out_index, out_count, &f))) return rc;
  int* cnt = static_cast<int*>(f.d_val);
  rgck::ror_count(c->stream, c->filter_cl.sorted(), r2, radius, min_neighbors, out_count != nullptr, cnt, dev_stats(c));
  return filter_close(c, f, n, on_device, nullptr, cnt, min_neighbors, negative, out_xyzc, out_index, out_count, n_out);
}

}  // extern "C"
