// rgc_api_search.hip -- host side of the search index (rgc_search_*): pcl::KdTreeFLANN::nearestKSearch / radiusSearch for batches of queries against
// a cloud of the context's own (rgcapi::SearchRecord: the grid only, built by build_measured_grid like the feature maps and the NDT clouds).  The
// kernels are rgc_search.hip's; the semantics are stated in include/rgc_hip.h.  Every query call computes into the context's scratch, reads the
// read-out words back (one small copy: the refusals and rgc_search_get_info need them) and only then copies rows to the caller -- a refused call
// writes nothing.
//   Behind the grid build: the call frame the cloud operations share (rgc_ctx.h: the search index, the outlier filters, clusters, plane, normals, FPFH).
#include "rgc_ctx.h"

#include <algorithm>

using namespace rgcapi;

namespace {

constexpr int kSearchMaxPoints = 1 << 27;  // offsets, counts and point_at's 32-bit byte offsets rely on it

rgck::SearchStats* dev_stats(rgc_ctx* c) { return stats<rgck::SearchStats>(c->search.f); }
const rgck::SearchStats* host_stats(rgc_ctx* c) { return rgcapi::host_stats<rgck::SearchStats>(c->search.f); }

void search_drop(rgc_ctx* c) {
  c->search.set = false;
  c->search.f.cl.n = 0;
  c->search.f.cl.in = nullptr;
  c->search.f.cl.ready = false;
  c->search.info = rgc_search_info{};
}

// the cloud's box in cells of `res` (rgck::bbox: the grid build's measurement and its flag word): hsm[0..2] lowest, hsm[3..5] highest cell
int search_measure(rgc_ctx* c, const char* who, const Cloud& cl, double res, int* dsm, int* hsm) {
  const int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
  memcpy(hsm, init, sizeof(init));
  HIPCHK(c, hipMemcpyAsync(dsm, hsm, 7 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  rgck::bbox(c->stream, cl.in, cl.stride_f, cl.n, res, dsm, dsm + 6);
  HIPCHK(c, hipMemcpyAsync(hsm, dsm, 7 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  if (hsm[6]) return fail(c, RGC_ERR_NONFINITE, "%s: the cloud contains non-finite or absurd coordinates", who);
  return RGC_OK;
}

// cell = 0 (rgc_hip.h): the power of two nearest cbrt(4 V / n), V = the product of the box's extents as measured in `unit`-sized cells
double auto_cell(const int hsm[8], double unit, int n, long long max_cells) {
  double ext[3], V = 1.0;
  for (int a = 0; a < 3; a++) {
    ext[a] = ((double)hsm[3 + a] - (double)hsm[a] + 1.0) * unit;
    V *= ext[a];
  }
  double cell = std::exp2(std::round(std::log2(std::cbrt(4.0 * V / (double)n))));
  cell = std::min(std::max(cell, std::exp2(-8.0)), std::exp2(16.0));
  const double most = std::min((double)std::max(4ll * n, 4096ll), (double)max_cells);
  for (int i = 0; i < 64; i++) {
    double cells = 1.0;
    for (int a = 0; a < 3; a++) cells *= std::floor(ext[a] / cell) + 2.0;  // (an upper bound of the axis' cells)
    if (cells <= most) break;
    cell *= 2.0;
  }
  return cell;
}

// what every query call checks first, and the queries on the device: *dq / *qstride_f
int search_queries(rgc_ctx* c, const char* who, const float* queries, int nq, int stride_bytes, int on_device, const float** dq, int* qstride_f) {
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "%s: stride_bytes must be a multiple of 4 between 12 and 4096", who);
  if (nq > kSearchMaxPoints) return fail(c, RGC_ERR_INVALID, "%s: %d queries, the limit is 2^27", who, nq);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = frame_open(c, c->search.f))) return rc;
  return stage_cloud(c, queries, nq, stride_bytes, on_device, c->search.q, "search queries", dq, qstride_f);
}

int stats_zero(rgc_ctx* c) {
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::SearchStats), c->stream));
  return RGC_OK;
}
// the read-out words on the host; the stream is idle afterwards
int stats_fetch(rgc_ctx* c) {
  HIPCHK(c, hipMemcpyAsync(c->search.f.h + kFrameStatsAt, dev_stats(c), sizeof(rgck::SearchStats), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}
void info_of_call(rgc_ctx* c) {
  const rgck::SearchStats& st = *host_stats(c);
  c->search.info.candidates = (long long)st.candidates;
  c->search.info.grown = (int)st.grown;
  c->search.info.rows_sorted_long = (int)st.rows_long;
}

}  // namespace

// The measured grid of a cloud that is searched by the rows of its cells (the search index, and through index_cloud every other cloud operation): the
// flag word is read before anything is indexed; *cell > 0 is the cell size as given (RGC_ERR_GRID_TOO_LARGE beyond max_cells), 0 selects it by the rule
// include/rgc_hip.h states (and *cell returns it).  dsm / hsm: eight scratch ints on the device / the host; who: the entry point, name / grid_name: the
// cloud, in the error messages
static int build_search_grid(rgc_ctx* c, Cloud& cl, double* cell_io, int* dsm, int* hsm, const char* who, const char* name, const char* grid_name) {
  int rc;
  double cell = *cell_io;
  const int n = cl.n;
  if ((rc = search_measure(c, who, cl, 1.0, dsm, hsm))) return rc;
  double far = 0.0, cells_est = 1.0;
  for (int a = 0; a < 3; a++) far = std::max(far, std::max(std::fabs((double)hsm[a]), std::fabs((double)hsm[3 + a])) + 2.0);
  if (cell == 0.0) {
    bool small = true;
    for (int a = 0; a < 3; a++) small = small && hsm[3 + a] - hsm[a] + 1 <= 8;
    double unit = 1.0;
    if (small) {
      unit = 1.0 / 16.0;
      if ((rc = search_measure(c, who, cl, unit, dsm, hsm))) return rc;
    }
    cell = auto_cell(hsm, unit, n, c->prm.max_cells);
  } else {
    // a cell coordinate must fit an int, and the grid the context's max_cells (build_measured_grid counts the cells exactly)
    for (int a = 0; a < 3; a++) cells_est *= std::max(1.0, ((double)hsm[3 + a] - (double)hsm[a] - 1.0) / cell);
    if (far / cell >= 1073741824.0 || cells_est > (double)c->prm.max_cells) return fail(c, RGC_ERR_GRID_TOO_LARGE, "%s exceeds max_cells", grid_name);
  }
  *cell_io = cell;
  return build_measured_grid(c, cl, cell, dsm, hsm, false, name, grid_name);
}

// ---- the cloud operations' call frame (declared in rgc_ctx.h) ----
int rgcapi::frame_open(rgc_ctx* c, OpFrame& f) {
  int rc;
  if ((rc = ensure(c, f.small, kFrameBytes))) return rc;
  if (!f.h) HIPCHK(c, hipHostMalloc((void**)&f.h, kFrameBytes, hipHostMallocDefault));
  return RGC_OK;
}

int rgcapi::index_cloud(rgc_ctx* c, OpFrame& f, const float* d, int stride_f, int n, const char* who, const char* name, const char* grid_name, double* cell) {
  Cloud& cl = f.cl;
  cl.in = d;
  cl.stride_f = stride_f;
  cl.n = n;
  cl.ready = false;
  *cell = f.cell;
  const int rc = build_search_grid(c, cl, cell, f.small.as<int>(), reinterpret_cast<int*>(f.h), who, name, grid_name);
  cl.in = nullptr;  // (the caller's buffer is not kept beyond the call)
  return rc;
}

int rgcapi::stage_cloud(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, DevBuf& stage, const char* what, const float** d, int* stride_f) {
  int rc;
  if (on_device) {
    if ((rc = check_device_range(c, p, record_bytes(n, stride_bytes, false), what))) return rc;
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

int rgcapi::stage_records(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, bool fourth, DevBuf& stage, const char* what, const float** d) {
  int rc;
  const size_t bytes = record_bytes(n, stride_bytes, fourth);
  if (on_device) {
    if ((rc = check_device_range(c, p, bytes, what))) return rc;
    *d = p;
    return RGC_OK;
  }
  if ((rc = ensure(c, stage, bytes))) return rc;
  HIPCHK(c, hipMemcpyAsync(stage.p, p, bytes, hipMemcpyHostToDevice, c->stream));
  *d = stage.as<const float>();
  return RGC_OK;
}

int rgcapi::copy_out(rgc_ctx* c, void* dst, const void* src, size_t bytes, int on_device) {
  if (dst && bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  return RGC_OK;
}

int rgcapi::write_empty_offsets(rgc_ctx* c, int* offsets, int on_device) {
  if (offsets && on_device) {
    HIPCHK(c, hipMemsetAsync(offsets, 0, sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else if (offsets) {
    offsets[0] = 0;
  }
  return RGC_OK;
}

int rgcapi::selection_scratch(rgc_ctx* c, Selection& sel, int n) {
  const size_t n1 = (size_t)n + 1;
  int rc;
  if ((rc = ensure(c, sel.flag, sizeof(int) * n1))) return rc;
  if ((rc = ensure(c, sel.off, sizeof(int) * n1))) return rc;
  return ensure(c, sel.bs, sizeof(int) * (n1 / 2048 + 2));
}

int rgcapi::emit_selected(rgc_ctx* c, Selection& sel, const float* d_in, int stride_f, int n, int on_device, const EmitTo& to, const EmitHome& home) {
  hipStream_t s = c->stream;
  const int* flag = sel.flag.as<const int>();
  int* off = sel.off.as<int>();
  rgck::exclusive_scan(s, flag, off, n + 1, sel.bs.as<int>());
  rgck::outlier_emit(s, d_in, stride_f, n, flag, off, to.d_out, to.d_index);
  if (home.h) HIPCHK(c, hipMemcpyAsync(home.h, home.d, home.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(home.h_kept, off + n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (on_device) return RGC_OK;
  const size_t kept = (size_t)*home.h_kept;
  int rc;
  if ((rc = copy_out(c, to.out_xyzc, to.d_out, 16 * kept, 0))) return rc;
  return copy_out(c, to.out_index, to.d_index, sizeof(int) * kept, 0);
}

int rgcapi::set_cell_of(rgc_ctx* c, double* knob, double cell, const char* who) {
  if (!std::isfinite(cell) || cell < 0.0) return fail(c, RGC_ERR_INVALID, "%s: cell must be finite and >= 0", who);
  *knob = cell;
  return RGC_OK;
}

extern "C" {

int rgc_search_sort_window(void) { return rgck::search_sort_window(); }

int rgc_search_set_cloud(rgc_ctx* c, const float* xyz, int n, int stride_bytes, int on_device, double cell) {
  if (!c || !xyz) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_search_set_cloud: a solve is in flight");
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "stride_bytes must be a multiple of 4 between 12 and 4096");
  if (n < 1) return fail(c, n < 0 ? RGC_ERR_INVALID : RGC_ERR_TOO_FEW_POINTS, "rgc_search_set_cloud: a cloud needs at least one point");
  if (n > kSearchMaxPoints) return fail(c, RGC_ERR_INVALID, "cloud has %d points, the limit is 2^27", n);
  if (!std::isfinite(cell) || cell < 0.0) return fail(c, RGC_ERR_INVALID, "rgc_search_set_cloud: cell must be finite and >= 0");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (on_device && (rc = check_device_range(c, xyz, record_bytes(n, stride_bytes, false), "rgc_search_set_cloud"))) return rc;
  if ((rc = frame_open(c, c->search.f))) return rc;
  search_drop(c);  // whatever happens below, the previous index is gone
  Cloud& cl = c->search.f.cl;
  if (on_device) {  // (looked up above, before the previous index was dropped)
    cl.in = xyz;
    cl.stride_f = stride_bytes / 4;
  } else if ((rc = stage_cloud(c, xyz, n, stride_bytes, 0, cl.in_copy, "rgc_search_set_cloud", &cl.in, &cl.stride_f))) {
    return rc;
  }
  cl.n = n;
  int* dsm = c->search.f.small.as<int>();
  int* hsm = reinterpret_cast<int*>(c->search.f.h);
  if ((rc = build_search_grid(c, cl, &cell, dsm, hsm, "rgc_search_set_cloud", "search cloud", "search grid"))) {
    search_drop(c);
    return rc;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's buffer has been read: it need not outlive the call
  HIPCHK(c, hipGetLastError());
  cl.in = nullptr;
  cl.ready = true;
  c->search.set = true;
  c->search.info.n = n;
  c->search.info.cell = cell;
  c->search.info.cells = cl.grid.ncell;
  return RGC_OK;
}

int rgc_search_clear(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_search_clear: a solve is in flight");
  search_drop(c);
  return RGC_OK;
}

int rgc_search_get_info(rgc_ctx* c, rgc_search_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->search.info;
  return RGC_OK;
}

int rgc_search_knn(rgc_ctx* c, const float* queries, int nq, int stride_bytes, int on_device, int k, int* idx, float* sq_dist) {
  if (!c) return RGC_ERR_INVALID;
  rgcapi::SearchRecord& r = c->search;
  if (nq < 0 || k < 1 || k > RGC_SEARCH_MAX_K) return fail(c, RGC_ERR_INVALID, "rgc_search_knn: nq >= 0 and k in 1..%d", RGC_SEARCH_MAX_K);
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_search_knn: a solve is in flight");
  if (!r.set) return fail(c, RGC_ERR_NO_INPUT, "rgc_search_knn: no cloud indexed (rgc_search_set_cloud)");
  r.info.candidates = 0;
  r.info.grown = r.info.rows_sorted_long = 0;
  if (nq == 0) return RGC_OK;
  if (!queries || !idx) return fail(c, RGC_ERR_INVALID, "rgc_search_knn: queries and idx must not be NULL");
  const float* dq = nullptr;
  int qs = 0, rc;
  if ((rc = search_queries(c, "rgc_search_knn", queries, nq, stride_bytes, on_device, &dq, &qs))) return rc;
  const size_t cells = (size_t)nq * k;
  if (on_device) {
    if ((rc = check_device_range(c, idx, sizeof(int) * cells, "rgc_search_knn: idx"))) return rc;
    if ((rc = check_device_range(c, sq_dist, sizeof(float) * cells, "rgc_search_knn: sq_dist"))) return rc;
  }
  if ((rc = ensure(c, r.row_idx, sizeof(int) * cells))) return rc;
  if ((rc = ensure(c, r.row_sq, sizeof(float) * cells))) return rc;
  if ((rc = ensure(c, r.cnt, sizeof(int) * ((size_t)nq + 1)))) return rc;
  if ((rc = stats_zero(c))) return rc;
  rgck::search_knn(c->stream, dq, qs, nq, r.f.cl.sorted(), k, 0, INFINITY, 0.0, r.row_idx.as<int>(), r.row_sq.as<float>(), r.cnt.as<int>(),
                   dev_stats(c));
  if ((rc = stats_fetch(c))) return rc;
  if (host_stats(c)->nonfinite) return fail(c, RGC_ERR_NONFINITE, "rgc_search_knn: a query has a non-finite coordinate");
  if ((rc = copy_out(c, idx, r.row_idx.p, sizeof(int) * cells, on_device))) return rc;
  if ((rc = copy_out(c, sq_dist, r.row_sq.p, sizeof(float) * cells, on_device))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  info_of_call(c);
  return RGC_OK;
}

int rgc_search_radius(rgc_ctx* c, const float* queries, int nq, int stride_bytes, int on_device, double radius, int max_nn, int sorted, int* offsets, int* idx,
                      float* sq_dist, long long cap, long long* n_total) {
  if (!c || !n_total) return RGC_ERR_INVALID;
  rgcapi::SearchRecord& r = c->search;
  if (nq < 0 || max_nn < 0 || max_nn > RGC_SEARCH_MAX_K || cap < 0) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: nq >= 0, max_nn in 0..%d, cap >= 0", RGC_SEARCH_MAX_K);
  const float r2 = (float)(radius * radius);
  if (!std::isfinite(radius) || radius <= 0.0 || !std::isfinite(r2)) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: the radius must be finite and > 0, float(r r) finite");
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: a solve is in flight");
  if (!r.set) return fail(c, RGC_ERR_NO_INPUT, "rgc_search_radius: no cloud indexed (rgc_search_set_cloud)");
  r.info.candidates = 0;
  r.info.grown = r.info.rows_sorted_long = 0;
  *n_total = 0;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (nq == 0) {
    if (offsets && on_device && (rc = check_device_range(c, offsets, sizeof(int), "rgc_search_radius: offsets"))) return rc;
    return write_empty_offsets(c, offsets, on_device);
  }
  if (!queries) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: queries must not be NULL");
  const float* dq = nullptr;
  int qs = 0;
  if ((rc = search_queries(c, "rgc_search_radius", queries, nq, stride_bytes, on_device, &dq, &qs))) return rc;
  const size_t n1 = (size_t)nq + 1;
  if ((rc = ensure(c, r.cnt, sizeof(int) * n1))) return rc;
  if ((rc = ensure(c, r.off, sizeof(int) * n1))) return rc;
  if ((rc = ensure(c, r.bs, sizeof(int) * (n1 / 2048 + 2)))) return rc;
  int* d_cnt = r.cnt.as<int>();
  int* d_off = r.off.as<int>();
  hipStream_t s = c->stream;
  const rgck::SortedCloud cl = r.f.cl.sorted();
  if ((rc = stats_zero(c))) return rc;
  HIPCHK(c, hipMemsetAsync(d_cnt + nq, 0, sizeof(int), s));
  if (max_nn > 0) {  // the max_nn smallest members: the top-k kernel with the member test; rows sorted by construction
    const size_t cells = (size_t)nq * max_nn;
    if ((rc = ensure(c, r.row_idx, sizeof(int) * cells))) return rc;
    if ((rc = ensure(c, r.row_sq, sizeof(float) * cells))) return rc;
    rgck::search_knn(s, dq, qs, nq, cl, max_nn, 1, r2, radius, r.row_idx.as<int>(), r.row_sq.as<float>(), d_cnt, dev_stats(c));
  } else {
    rgck::search_count(s, dq, qs, nq, cl, r2, radius, d_cnt, dev_stats(c));
  }
  rgck::exclusive_scan(s, d_cnt, d_off, (int)n1, r.bs.as<int>());
  if ((rc = stats_fetch(c))) return rc;
  const rgck::SearchStats st = *host_stats(c);
  if (st.nonfinite) return fail(c, RGC_ERR_NONFINITE, "rgc_search_radius: a query has a non-finite coordinate");
  const long long total = (long long)st.members;
  *n_total = total;
  if (total > (long long)INT_MAX) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: %lld neighbours, the 32-bit offsets take 2^31 - 1", total);
  if (cap < total) return fail(c, RGC_ERR_INVALID, "rgc_search_radius: cap is smaller than the %lld neighbours there are", total);
  if (on_device) {
    if ((rc = check_device_range(c, offsets, sizeof(int) * n1, "rgc_search_radius: offsets"))) return rc;
    if ((rc = check_device_range(c, idx, sizeof(int) * (size_t)total, "rgc_search_radius: idx"))) return rc;
    if ((rc = check_device_range(c, sq_dist, sizeof(float) * (size_t)total, "rgc_search_radius: sq_dist"))) return rc;
  }
  if (total > 0) {
    if ((rc = ensure(c, r.idx, sizeof(int) * (size_t)total))) return rc;
    if ((rc = ensure(c, r.sq, sizeof(float) * (size_t)total))) return rc;
    if (max_nn > 0) {
      rgck::search_compact(s, r.row_idx.as<const int>(), r.row_sq.as<const float>(), d_cnt, d_off, nq, max_nn, r.idx.as<int>(), r.sq.as<float>());
    } else {
      const bool long_rows = sorted && st.longest > rgck::kSearchSortWindow;
      if ((rc = ensure(c, r.ent, sizeof(unsigned long long) * (size_t)total))) return rc;
      if (long_rows && (rc = ensure(c, r.tmp, sizeof(unsigned long long) * (size_t)total))) return rc;
      unsigned long long* ent = r.ent.as<unsigned long long>();
      rgck::search_fill(s, dq, qs, nq, cl, r2, radius, d_off, ent);
      if (sorted) rgck::search_sort_rows(s, d_off, nq, st.longest, ent, long_rows ? r.tmp.as<unsigned long long>() : nullptr, dev_stats(c));
      rgck::search_unpack(s, ent, total, r.idx.as<int>(), r.sq.as<float>());
    }
  }
  if ((rc = copy_out(c, offsets, d_off, sizeof(int) * n1, on_device))) return rc;
  if ((rc = copy_out(c, idx, r.idx.p, sizeof(int) * (size_t)total, on_device))) return rc;
  if ((rc = copy_out(c, sq_dist, r.sq.p, sizeof(float) * (size_t)total, on_device))) return rc;
  if ((rc = stats_fetch(c))) return rc;
  info_of_call(c);
  return RGC_OK;
}

}  // extern "C"
