// segmentation_hip.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_cluster_*): Euclidean cluster extraction on the GPU.  It stands
// in for pcl::EuclideanClusterExtraction<PointT> WITHOUT requiring PCL at build time, with its member names:
//
//   rgc::EuclideanClusterExtractionHip ec(0);            // its own context on device 0, or (ctx) in an existing one (not owned)
//   ec.setInputCloud(cloud);                             // any cloud with ->points of x,y,z-first points of at least 12 bytes
//   ec.setClusterTolerance(0.5); ec.setMinClusterSize(10); ec.setMaxClusterSize(25000);
//   std::vector<std::vector<int>> clusters;              // (pcl::PointIndices::indices, one vector per cluster)
//   ec.extract(clusters);                                // size descending, then smallest member ascending; members ascending
//   ec.labels();                                         // per point: the rank of its cluster, -1 in none
//
// The semantics (the fp32 key, the strict tolerance, the size limits, the order) are stated in include/rgc_hip.h.  A refused call throws
// std::runtime_error carrying rgc_last_error(), a refused setter one naming the range it accepts.  No CPU fallback.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

class EuclideanClusterExtractionHip {
public:
  explicit EuclideanClusterExtractionHip(int hip_device = 0) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
  }
  explicit EuclideanClusterExtractionHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: null context");
  }
  ~EuclideanClusterExtractionHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  EuclideanClusterExtractionHip(const EuclideanClusterExtractionHip&) = delete;
  EuclideanClusterExtractionHip& operator=(const EuclideanClusterExtractionHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    xyz_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    n_ = (int)cloud->points.size();
    stride_ = (int)sizeof(cloud->points[0]);
    on_device_ = 0;
    extracted_ = false;
  }
  void setInputCloudDevice(const float* d_xyz, int n, int stride_bytes) { xyz_ = d_xyz; n_ = n; stride_ = stride_bytes; on_device_ = 1; extracted_ = false; }
  void setClusterTolerance(double tolerance) {
    const float r2 = (float)(tolerance * tolerance);
    if (!std::isfinite(tolerance) || tolerance <= 0.0 || !std::isfinite(r2))
      throw std::runtime_error("rgc::EuclideanClusterExtractionHip: the tolerance must be finite and > 0, float(t t) finite");
    tolerance_ = tolerance;
  }
  double getClusterTolerance() const { return tolerance_; }
  void setMinClusterSize(int min_size) {
    if (min_size < 1) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: min_size >= 1");
    min_ = min_size;
  }
  int getMinClusterSize() const { return min_; }
  void setMaxClusterSize(int max_size) {
    if (max_size < 1) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: max_size >= 1");
    max_ = max_size;
  }
  int getMaxClusterSize() const { return max_; }
  // the grid's cell size, for tests and tuning (0 = chosen from the cloud's box and size); no output depends on it
  void setCell(double cell) { check(rgc_cluster_set_cell(ctx_, cell), "rgc_cluster_set_cell"); }

  // pcl::EuclideanClusterExtraction::extract (host clouds): clusters[r] = the members of the cluster of rank r, ascending
  void extract(std::vector<std::vector<int>>& clusters) {
    if (on_device_) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: a device cloud is extracted with the device-pointer overload");
    std::vector<int> offsets((size_t)n_ + 1, 0), indices((size_t)n_, 0);
    labels_.assign((size_t)n_, -1);
    int m = 0;
    check(rgc_cluster_extract(ctx_, xyz_, n_, stride_, 0, tolerance_, min_, max_, labels_.data(), offsets.data(), indices.data(), &m), "rgc_cluster_extract");
    clusters.assign((size_t)m, std::vector<int>());
    for (int r = 0; r < m; r++) clusters[(size_t)r].assign(indices.begin() + offsets[(size_t)r], indices.begin() + offsets[(size_t)r + 1]);
    extracted_ = true;
  }
  // device clouds: labels (n ints), offsets (n + 1) and indices (n) into device memory of the context's GPU, each nullable; returns the clusters kept
  int extract(int* d_labels, int* d_offsets, int* d_indices) {
    if (!on_device_) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: the device-pointer overload needs setInputCloudDevice");
    int m = 0;
    check(rgc_cluster_extract(ctx_, xyz_, n_, stride_, 1, tolerance_, min_, max_, d_labels, d_offsets, d_indices, &m), "rgc_cluster_extract");
    return m;
  }
  // per point, of the last extract() of a host cloud: the rank of its cluster, -1 for a point in no kept cluster
  const std::vector<int>& labels() const {
    if (!extracted_) throw std::runtime_error("rgc::EuclideanClusterExtractionHip: extract() has not run on this cloud");
    return labels_;
  }
  rgc_cluster_info info() const {
    rgc_cluster_info s;
    check(rgc_cluster_get_info(ctx_, &s), "rgc_cluster_get_info");
    return s;
  }

private:
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  const float* xyz_ = nullptr;
  int n_ = 0, stride_ = 16, on_device_ = 0;
  double tolerance_ = 0.0;  // PCL's defaults: a tolerance must be set before extract()
  int min_ = 1, max_ = INT_MAX;
  bool extracted_ = false;
  std::vector<int> labels_;
};

}  // namespace rgc
