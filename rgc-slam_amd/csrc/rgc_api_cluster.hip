// rgc_api_cluster.hip -- host side of Euclidean cluster extraction (rgc_cluster_*): pcl::EuclideanClusterExtraction of a cloud on a grid of the call's own
// (rgcapi::ClusterRecord, built by index_cloud like the search index's and the outlier filters': the same automatic cell rule).  The kernels are
// rgc_cluster.hip's; the semantics are stated in include/rgc_hip.h.
//   Host round trips of a call: index_cloud's grid build's own (it measures the box before it sizes the grid, as for every cloud searched by rows);
// then ONE mid-chain read-back -- the error word, the read-out words, the number of kept clusters and of clustered points: the host needs them to size
// the two sorts' passes -- and the wait at the end (with a host caller's downloads in front of it).  What can refuse a call (the arguments, the grid
// build's flag word, the error word) does so before anything is written to the caller.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

constexpr int kClusterMaxPoints = 1 << 27;  // point_at's 32-bit byte offsets rely on it

// the int arrays of a call, slices of ClusterRecord::work (a slice: n + 1 ints, rounded up to 16 bytes)
enum Slice {
  kParent = 0, kLead, kSize,     // the union-find and the census, on SORTED positions; dead behind cluster_assign: the sorts' first three arrays
  kComp, kCsize, kFlagP, kFlagL, kOffP, kOffL,  // at the ORIGINAL index
  kPair4,                        // the sorts' fourth array
  kRankAt, kSizes,               // a leader's rank at its original index; the sizes in rank order
  kLabels, kOffsets,             // a host caller's results (its indices are read from where the second sort leaves them)
  kSlices
};

rgck::ClusterStats* dev_stats(rgc_ctx* c) { return stats<rgck::ClusterStats>(c->cluster.f); }  // (the frame's own words are the two counts: the scans' last offsets)
int bit_length(unsigned v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

}  // namespace

extern "C" {

int rgc_cluster_set_cell(rgc_ctx* c, double cell) {
  if (!c) return RGC_ERR_INVALID;
  return set_cell_of(c, &c->cluster.f.cell, cell, "rgc_cluster_set_cell");
}

int rgc_cluster_get_info(rgc_ctx* c, rgc_cluster_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->cluster.info;
  return RGC_OK;
}

int rgc_cluster_extract(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, int on_device, double tolerance, int min_size, int max_size, int* labels, int* offsets,
                        int* indices, int* n_clusters) {
  const char* who = "rgc_cluster_extract";
  if (!c || !n_clusters || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  const float r2 = (float)(tolerance * tolerance);
  if (!std::isfinite(tolerance) || tolerance <= 0.0 || !std::isfinite(r2)) return fail(c, RGC_ERR_INVALID, "%s: the tolerance must be finite and > 0, float(t t) finite", who);
  if (min_size < 1 || max_size < min_size) return fail(c, RGC_ERR_INVALID, "%s: 1 <= min_size <= max_size", who);
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "%s: stride_bytes must be a multiple of 4 between 12 and 4096", who);
  if (n > kClusterMaxPoints) return fail(c, RGC_ERR_INVALID, "%s: cloud has %d points, the limit is 2^27", who, n);
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "%s: a solve is in flight", who);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t nn = (size_t)n;
  int rc;
  if (on_device) {
    if (n && (rc = check_device_range(c, xyzc, record_bytes(n, stride_bytes, false), "input cloud"))) return rc;
    if (labels && n && (rc = check_device_range(c, labels, sizeof(int) * nn, "labels"))) return rc;
    if (offsets && (rc = check_device_range(c, offsets, sizeof(int) * (nn + 1), "offsets"))) return rc;
    if (indices && n && (rc = check_device_range(c, indices, sizeof(int) * nn, "indices"))) return rc;
  }
  *n_clusters = 0;
  c->cluster.info = rgc_cluster_info{};
  if (n == 0) return write_empty_offsets(c, offsets, on_device);
  rgcapi::ClusterRecord& r = c->cluster;
  if ((rc = frame_open(c, r.f))) return rc;
  const float* d_in = xyzc;  // (a device caller's cloud was looked up above)
  if (!on_device && (rc = stage_records(c, xyzc, n, stride_bytes, 0, false, r.in, "input cloud", &d_in))) return rc;
  const size_t slice = (nn + 1 + 3) & ~(size_t)3;
  const int tiles = rgck::cluster_radix_tiles(n);
  const size_t hist_n = (size_t)rgck::kClusterRadixDigits * tiles + 1, hist_slice = (hist_n + 3) & ~(size_t)3;
  if ((rc = ensure(c, r.work, sizeof(int) * slice * kSlices))) return rc;
  if ((rc = ensure(c, r.hist, sizeof(int) * hist_slice * 2))) return rc;
  if ((rc = ensure(c, r.bs, sizeof(int) * (std::max(nn + 1, hist_n) / 2048 + 2)))) return rc;
  int* const work = r.work.as<int>();
  auto at = [&](Slice k) { return work + slice * (size_t)k; };
  int* const hist = r.hist.as<int>();
  int* const bs = r.bs.as<int>();
  const Cloud& cl = r.f.cl;
  double cell = 0.0;
  if ((rc = index_cloud(c, r.f, d_in, stride_bytes / 4, n, who, "the cloud", "the clustering's grid", &cell))) return rc;
  HIPCHK(c, hipMemsetAsync(dev_stats(c), 0, sizeof(rgck::ClusterStats), s));
  // the components, their leaders and sizes, the kept leaders in input order
  const rgck::SortedCloud sc = cl.sorted();
  rgck::cluster_link(s, sc, r2, tolerance, at(kParent), at(kLead), at(kSize), dev_stats(c));
  rgck::cluster_assign(s, sc, at(kParent), at(kLead), at(kSize), min_size, max_size, at(kComp), at(kCsize), at(kFlagP), at(kFlagL), dev_stats(c));
  rgck::exclusive_scan(s, at(kFlagL), at(kOffL), n + 1, bs);
  rgck::exclusive_scan(s, at(kFlagP), at(kOffP), n + 1, bs);
  int* key[2] = {at(kParent), at(kSize)};
  int* val[2] = {at(kLead), at(kPair4)};
  rgck::cluster_emit(s, n, at(kFlagL), at(kOffL), at(kCsize), key[0], val[0]);
  // the one read-back
  int* const h_counts = host_words(r.f);
  HIPCHK(c, hipMemcpyAsync(r.f.h + kFrameStatsAt, dev_stats(c), sizeof(rgck::ClusterStats), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(h_counts, at(kOffL) + n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(h_counts + 1, at(kOffP) + n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  const rgck::ClusterStats& st = *host_stats<rgck::ClusterStats>(r.f);
  if (st.err) return fail(c, RGC_ERR_HIP, "%s: a union-find loop ran past its iteration cap (error word %d): nothing was written", who, st.err);
  const int m = h_counts[0], mp = h_counts[1];
  if (labels || offsets || indices) {
    // the leaders by n - size, stable over ascending leaders: size descending, leader ascending
    const int cur = rgck::cluster_radix_sort(s, m, bit_length((unsigned)(n - 1)), key, val, hist, hist + hist_slice, bs);
    rgck::cluster_rank(s, n, m, key[cur], val[cur], at(kRankAt), at(kSizes));
    int* const d_offsets = on_device ? offsets : at(kOffsets);
    if (offsets) rgck::exclusive_scan(s, at(kSizes), d_offsets, m + 1, bs);
    int* const d_labels = on_device ? labels : at(kLabels);
    // (the rank table is read before the second sort takes the arrays of the first: the stream orders them)
    rgck::cluster_labels(s, n, at(kFlagP), at(kOffP), at(kComp), at(kRankAt), labels ? d_labels : nullptr, indices ? key[0] : nullptr, indices ? val[0] : nullptr);
    if (indices && mp) {
      // the kept points, ascending in input index, by their cluster's rank: the rows
      const int curp = rgck::cluster_radix_sort(s, mp, m > 1 ? bit_length((unsigned)(m - 1)) : 0, key, val, hist, hist + hist_slice, bs);
      if ((rc = copy_out(c, indices, val[curp], sizeof(int) * (size_t)mp, on_device))) return rc;
    }
    if (!on_device) {
      if ((rc = copy_out(c, labels, d_labels, sizeof(int) * nn, 0))) return rc;
      if ((rc = copy_out(c, offsets, d_offsets, sizeof(int) * ((size_t)m + 1), 0))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
  }
  r.info.n = n;
  r.info.n_components = (int)sum_words(st.words, 1);
  r.info.n_clusters = m;
  r.info.n_clustered = mp;
  r.info.largest = (int)max_words(st.words, 2);
  r.info.cell = cell;
  r.info.cells = cl.grid.ncell;
  r.info.candidates = (long long)sum_words(st.words, 0);
  *n_clusters = m;
  return RGC_OK;
}

}  // extern "C"
