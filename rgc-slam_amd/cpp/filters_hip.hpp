// filters_hip.hpp -- header-only C++ adaptors over the C-ABI (include/rgc_hip.h, rgc_outlier_*): the two outlier filters on the GPU.  They stand in for
// pcl::StatisticalOutlierRemoval<PointT> and pcl::RadiusOutlierRemoval<PointT> WITHOUT requiring PCL at build time, with their member names:
//
//   rgc::StatisticalOutlierRemovalHip sor(0);            // its own context on device 0, or (ctx) in an existing one (not owned)
//   sor.setInputCloud(cloud);                            // any cloud with ->points of x,y,z-first points of at least 12 bytes
//   sor.setMeanK(50); sor.setStddevMulThresh(1.0);
//   sor.filter(out);                                     // out.points: the kept points, in input order (copies of the input's points)
//   sor.filter(indices);                                 // or their indices; getRemovedIndices() after either
//
//   rgc::RadiusOutlierRemovalHip ror(0); ror.setRadiusSearch(0.5); ror.setMinNeighborsInRadius(5); ...
//
// The semantics (the fp32 key, the mean distance, the statistics, the strict radius) are stated in include/rgc_hip.h.  A refused call throws
// std::runtime_error carrying rgc_last_error(), a refused setter one naming the range it accepts.  No CPU fallback.
#pragma once
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

class OutlierFilterHip {
public:
  OutlierFilterHip(const OutlierFilterHip&) = delete;
  OutlierFilterHip& operator=(const OutlierFilterHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    xyz_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    n_ = (int)cloud->points.size();
    stride_ = (int)sizeof(cloud->points[0]);
    on_device_ = 0;
    filtered_ = false;
  }
  void setInputCloudDevice(const float* d_xyz, int n, int stride_bytes) { xyz_ = d_xyz; n_ = n; stride_ = stride_bytes; on_device_ = 1; filtered_ = false; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  // the grid's cell size, for tests and tuning (0 = chosen from the cloud's box and size); no output depends on it
  void setCell(double cell) { check(rgc_outlier_set_cell(ctx_, cell), "rgc_outlier_set_cell"); }

  // pcl::FilterIndices::filter(indices): the kept points' input indices, ascending (host clouds)
  void filter(std::vector<int>& indices) {
    need_host();
    indices.assign((size_t)n_, 0);
    int kept = 0;
    check(run(nullptr, indices.data(), &kept), name());
    indices.resize((size_t)kept);
    kept_ = indices;
    filtered_ = true;
  }
  // pcl::Filter::filter(output): output.points = copies of the kept input points, in input order
  template <typename CloudT> void filter(CloudT& output) {
    std::vector<int> indices;
    const void* base = xyz_;
    filter(indices);
    output.points.clear();
    output.points.reserve(indices.size());
    typedef typename std::remove_reference<decltype(output.points[0])>::type PointT;
    for (int i : indices) output.points.push_back(*reinterpret_cast<const PointT*>(static_cast<const char*>(base) + (size_t)i * (size_t)stride_));
  }
  // device clouds: 16-byte records and indices into device memory of the context's GPU (each nullable, room for n); returns the number kept
  int filterDevice(float* d_out_xyzc, int* d_out_index) {
    if (!on_device_) throw std::runtime_error("rgc outlier filter: filterDevice needs setInputCloudDevice");
    int kept = 0;
    check(run(d_out_xyzc, d_out_index, &kept), name());
    return kept;
  }
  // pcl::FilterIndices::getRemovedIndices (extract_removed_indices_ is always on here): of the last filter() of a host cloud
  std::vector<int> getRemovedIndices() const {
    if (!filtered_) throw std::runtime_error("rgc outlier filter: filter() has not run on this cloud");
    std::vector<int> removed;
    size_t j = 0;
    for (int i = 0; i < n_; i++) {
      if (j < kept_.size() && kept_[j] == i) j++;
      else removed.push_back(i);
    }
    return removed;
  }
  rgc_outlier_info info() const {
    rgc_outlier_info s;
    check(rgc_outlier_get_info(ctx_, &s), "rgc_outlier_get_info");
    return s;
  }

protected:
  explicit OutlierFilterHip(int hip_device) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
  }
  explicit OutlierFilterHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc outlier filter: null context");
  }
  ~OutlierFilterHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  virtual int run(float* out_xyzc, int* out_index, int* kept) = 0;
  virtual const char* name() const = 0;
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  void need_host() const {
    if (on_device_) throw std::runtime_error("rgc outlier filter: a device cloud is filtered with filterDevice");
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  const float* xyz_ = nullptr;
  int n_ = 0, stride_ = 16, on_device_ = 0;
  bool negative_ = false, filtered_ = false;
  std::vector<int> kept_;
};

class StatisticalOutlierRemovalHip : public OutlierFilterHip {
public:
  explicit StatisticalOutlierRemovalHip(int hip_device = 0) : OutlierFilterHip(hip_device) {}
  explicit StatisticalOutlierRemovalHip(rgc_ctx* ctx) : OutlierFilterHip(ctx) {}
  void setMeanK(int mean_k) {
    if (mean_k < 1 || mean_k > RGC_OUTLIER_MAX_MEAN_K) throw std::runtime_error("rgc::StatisticalOutlierRemovalHip: mean_k in 1.." + std::to_string(RGC_OUTLIER_MAX_MEAN_K));
    mean_k_ = mean_k;
  }
  int getMeanK() const { return mean_k_; }
  void setStddevMulThresh(double std_mul) {
    if (!std::isfinite(std_mul)) throw std::runtime_error("rgc::StatisticalOutlierRemovalHip: std_mul must be finite");
    std_mul_ = std_mul;
  }
  double getStddevMulThresh() const { return std_mul_; }
  // every point's mean distance to its mean_k nearest neighbours (host clouds); the filter's statistics are info()'s
  std::vector<float> meanDistances() {
    need_host();
    std::vector<float> d((size_t)n_, 0.f);
    int kept = 0;
    check(rgc_outlier_statistical(ctx_, xyz_, n_, stride_, 0, mean_k_, std_mul_, negative_ ? 1 : 0, nullptr, nullptr, d.data(), &kept), name());
    return d;
  }

private:
  int run(float* out_xyzc, int* out_index, int* kept) override {
    return rgc_outlier_statistical(ctx_, xyz_, n_, stride_, on_device_, mean_k_, std_mul_, negative_ ? 1 : 0, out_xyzc, out_index, nullptr, kept);
  }
  const char* name() const override { return "rgc_outlier_statistical"; }
  int mean_k_ = 1;        // PCL's defaults
  double std_mul_ = 0.0;
};

class RadiusOutlierRemovalHip : public OutlierFilterHip {
public:
  explicit RadiusOutlierRemovalHip(int hip_device = 0) : OutlierFilterHip(hip_device) {}
  explicit RadiusOutlierRemovalHip(rgc_ctx* ctx) : OutlierFilterHip(ctx) {}
  void setRadiusSearch(double radius) {
    const float r2 = (float)(radius * radius);
    if (!std::isfinite(radius) || radius <= 0.0 || !std::isfinite(r2)) throw std::runtime_error("rgc::RadiusOutlierRemovalHip: the radius must be finite and > 0, float(r r) finite");
    radius_ = radius;
  }
  double getRadiusSearch() const { return radius_; }
  void setMinNeighborsInRadius(int min_neighbors) {
    if (min_neighbors < 0) throw std::runtime_error("rgc::RadiusOutlierRemovalHip: min_neighbors >= 0");
    min_nb_ = min_neighbors;
  }
  int getMinNeighborsInRadius() const { return min_nb_; }
  // the points within the radius of every point, itself included (host clouds): the exact counts, no walk stops early
  std::vector<int> counts() {
    need_host();
    std::vector<int> c((size_t)n_, 0);
    int kept = 0;
    check(rgc_outlier_radius(ctx_, xyz_, n_, stride_, 0, radius_, min_nb_, negative_ ? 1 : 0, nullptr, nullptr, c.data(), &kept), name());
    return c;
  }

private:
  int run(float* out_xyzc, int* out_index, int* kept) override {
    return rgc_outlier_radius(ctx_, xyz_, n_, stride_, on_device_, radius_, min_nb_, negative_ ? 1 : 0, out_xyzc, out_index, nullptr, kept);
  }
  const char* name() const override { return "rgc_outlier_radius"; }
  double radius_ = 0.0;   // PCL's defaults: a radius must be set before filter()
  int min_nb_ = 1;
};

}  // namespace rgc
