// kdtree_hip.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_search_*): exact k nearest neighbours and radius search on the GPU.
// Stands in for pcl::KdTreeFLANN<PointT> as the reference's nodes call it (rgc_slam/src/RGC_mapping.cpp:1097,1537,
// rgc_slam/include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:133) WITHOUT requiring PCL at build time, with its member names:
//
//   rgc::KdTreeHip tree(0);                               // its own context on device 0, or KdTreeHip(ctx) in an existing one (not owned)
//   tree.setInputCloud(map);                              // any cloud with ->points / ->size() of x,y,z-first points
//   tree.nearestKSearch(point, 5, k_indices, k_sqr_distances);                // one point with .x .y .z: a one-row call of the batch
//   tree.radiusSearch(point, 1.0, k_indices, k_sqr_distances, max_nn);
//   tree.nearestKSearch(scan, 5, indices, sqr_distances);                     // every point of a cloud: rows of k, -1 / +inf behind min(k, n)
//   tree.radiusSearch(scan, 1.0, offsets, indices, sqr_distances, max_nn);    // CSR rows
//
// Rows are ascending (key, index) unless setSortedResults(false).  What PCL's nearestKSearch does for k > n (it shrinks k) the single-point form
// does too: the vectors are resized to the entries found.  Errors throw std::runtime_error carrying rgc_last_error().  No CPU fallback.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

class KdTreeHip {
public:
  explicit KdTreeHip(int hip_device = 0, bool sorted = true) : own_(true), sorted_(sorted) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
  }
  explicit KdTreeHip(rgc_ctx* ctx, bool sorted = true) : ctx_(ctx), own_(false), sorted_(sorted) {
    if (!ctx) throw std::runtime_error("rgc::KdTreeHip: null context");
  }
  ~KdTreeHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  KdTreeHip(const KdTreeHip&) = delete;
  KdTreeHip& operator=(const KdTreeHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  void setSortedResults(bool sorted) { sorted_ = sorted; }  // pcl::KdTree::setSortedResults: the order inside a radius row
  bool getSortedResults() const { return sorted_; }

  // cell: the grid's cell size, 0 = chosen from the cloud's box and size (results never depend on it)
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud, double cell = 0.0) {
    check(rgc_search_set_cloud(ctx_, &cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0]), 0, cell), "rgc_search_set_cloud");
  }
  void setInputCloudDevice(const float* d_xyz, int n, int stride_bytes, double cell = 0.0) {
    check(rgc_search_set_cloud(ctx_, d_xyz, n, stride_bytes, 1, cell), "rgc_search_set_cloud");
  }
  void clear() { check(rgc_search_clear(ctx_), "rgc_search_clear"); }
  rgc_search_info info() const {
    rgc_search_info s;
    check(rgc_search_get_info(ctx_, &s), "rgc_search_get_info");
    return s;
  }

  // ---- batches (host memory): nq points of stride_bytes, x, y, z first ----
  void nearestKSearch(const float* xyz, int nq, int stride_bytes, int k, std::vector<int>& indices, std::vector<float>& sqr_distances) {
    const size_t cells = (size_t)(nq > 0 ? nq : 0) * (size_t)(k > 0 ? k : 0);
    indices.assign(cells, -1);
    sqr_distances.assign(cells, 0.f);
    check(rgc_search_knn(ctx_, xyz, nq, stride_bytes, 0, k, indices.data(), sqr_distances.data()), "rgc_search_knn");
  }
  // rows in CSR form: indices[offsets[i] .. offsets[i + 1]); returns the total
  long long radiusSearch(const float* xyz, int nq, int stride_bytes, double radius, std::vector<int>& offsets, std::vector<int>& indices,
                         std::vector<float>& sqr_distances, unsigned int max_nn = 0) {
    long long total = 0;
    const int rc = rgc_search_radius(ctx_, xyz, nq, stride_bytes, 0, radius, (int)max_nn, sorted_ ? 1 : 0, nullptr, nullptr, nullptr, 0, &total);
    if (rc != RGC_OK && !(rc == RGC_ERR_INVALID && total > 0)) check(rc, "rgc_search_radius");  // (cap 0 < total: the sizing call)
    offsets.assign((size_t)(nq > 0 ? nq : 0) + 1, 0);
    indices.assign((size_t)total, -1);
    sqr_distances.assign((size_t)total, 0.f);
    check(rgc_search_radius(ctx_, xyz, nq, stride_bytes, 0, radius, (int)max_nn, sorted_ ? 1 : 0, offsets.data(), indices.data(), sqr_distances.data(), total, &total),
          "rgc_search_radius");
    return total;
  }
  // (the trailing return types tell a cloud pointer, ->points, from a point, .x)
  template <typename CloudPtr>
  auto nearestKSearch(const CloudPtr& cloud, int k, std::vector<int>& indices, std::vector<float>& sqr_distances) -> decltype((void)cloud->points.size(), void()) {
    nearestKSearch(&cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0]), k, indices, sqr_distances);
  }
  template <typename CloudPtr>
  auto radiusSearch(const CloudPtr& cloud, double radius, std::vector<int>& offsets, std::vector<int>& indices, std::vector<float>& sqr_distances, unsigned int max_nn = 0)
      -> decltype((void)cloud->points.size(), (long long)0) {
    return radiusSearch(&cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0]), radius, offsets, indices, sqr_distances, max_nn);
  }

  // ---- pcl::KdTreeFLANN's single-point members: one-row calls of the batch; both return the number of neighbours found ----
  template <typename PointT>
  auto nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) -> decltype((void)point.x, int()) {
    const float q[3] = {point.x, point.y, point.z};
    nearestKSearch(q, 1, (int)sizeof(q), k, k_indices, k_sqr_distances);
    size_t found = 0;
    while (found < k_indices.size() && k_indices[found] >= 0) found++;
    k_indices.resize(found);
    k_sqr_distances.resize(found);
    return (int)found;
  }
  template <typename PointT>
  auto radiusSearch(const PointT& point, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, unsigned int max_nn = 0)
      -> decltype((void)point.x, int()) {
    const float q[3] = {point.x, point.y, point.z};
    std::vector<int> offsets;
    return (int)radiusSearch(q, 1, (int)sizeof(q), radius, offsets, k_indices, k_sqr_distances, max_nn);
  }

private:
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  bool sorted_;
};

}  // namespace rgc
