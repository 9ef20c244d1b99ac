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
// and for pcl::SACSegmentation<PointT> (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC) with the pcl::ExtractIndices step behind it
// (rgc_plane_*):
//
//   rgc::SACSegmentationHip seg(0);
//   seg.setInputCloud(cloud); seg.setModelType(rgc::SACMODEL_PLANE); seg.setMethodType(rgc::SAC_RANSAC);
//   seg.setDistanceThreshold(0.2); seg.setMaxIterations(50); seg.setSeed(1);
//   std::vector<int> inliers; std::vector<float> coefficients;   // (pcl::PointIndices::indices, pcl::ModelCoefficients::values)
//   seg.segment(inliers, coefficients);
//   seg.setNegative(true); seg.filter(rest);             // the ground-removed cloud as x, y, z, c records in input order
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

enum { SACMODEL_PLANE = 0, SACMODEL_PERPENDICULAR_PLANE = 11 };  // PCL's values (model_types.h)
enum { SAC_RANSAC = 0 };                                         // method_types.h; the other methods are not built

class SACSegmentationHip {
public:
  explicit SACSegmentationHip(int hip_device = 0) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
    rgc_default_plane_params(&prm_);
  }
  explicit SACSegmentationHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::SACSegmentationHip: null context");
    rgc_default_plane_params(&prm_);
  }
  ~SACSegmentationHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  SACSegmentationHip(const SACSegmentationHip&) = delete;
  SACSegmentationHip& operator=(const SACSegmentationHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    xyz_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    n_ = (int)cloud->points.size();
    stride_ = (int)sizeof(cloud->points[0]);
    on_device_ = 0;
  }
  void setInputCloudDevice(const float* d_xyz, int n, int stride_bytes) { xyz_ = d_xyz; n_ = n; stride_ = stride_bytes; on_device_ = 1; }
  void setModelType(int model) {
    if (model != SACMODEL_PLANE && model != SACMODEL_PERPENDICULAR_PLANE) throw std::runtime_error("rgc::SACSegmentationHip: SACMODEL_PLANE or SACMODEL_PERPENDICULAR_PLANE");
    prm_.model_type = model == SACMODEL_PLANE ? RGC_PLANE_PLANE : RGC_PLANE_PERPENDICULAR;
  }
  int getModelType() const { return prm_.model_type == RGC_PLANE_PLANE ? SACMODEL_PLANE : SACMODEL_PERPENDICULAR_PLANE; }
  void setMethodType(int method) {
    if (method != SAC_RANSAC) throw std::runtime_error("rgc::SACSegmentationHip: only SAC_RANSAC is built");
  }
  int getMethodType() const { return SAC_RANSAC; }
  void setDistanceThreshold(double threshold) {
    const float t = (float)threshold;
    if (!std::isfinite(threshold) || !std::isfinite(t) || !(t > 0.f)) throw std::runtime_error("rgc::SACSegmentationHip: the distance threshold must be finite and > 0 (as a float too)");
    prm_.distance_threshold = threshold;
  }
  double getDistanceThreshold() const { return prm_.distance_threshold; }
  void setMaxIterations(int max_iterations) {
    if (max_iterations < 1) throw std::runtime_error("rgc::SACSegmentationHip: max_iterations >= 1");
    prm_.max_iterations = max_iterations;
  }
  int getMaxIterations() const { return prm_.max_iterations; }
  void setProbability(double probability) {
    if (!(probability > 0.0 && probability < 1.0)) throw std::runtime_error("rgc::SACSegmentationHip: probability in (0, 1)");
    prm_.probability = probability;
  }
  double getProbability() const { return prm_.probability; }
  void setOptimizeCoefficients(bool optimize) { prm_.optimize = optimize ? 1 : 0; }
  bool getOptimizeCoefficients() const { return prm_.optimize != 0; }
  void setAxis(double ax, double ay, double az) {
    const double len = std::sqrt((ax * ax + ay * ay) + az * az);
    if (!std::isfinite(len) || !(len > 0.0)) throw std::runtime_error("rgc::SACSegmentationHip: the axis must be finite and not zero");
    prm_.axis[0] = ax; prm_.axis[1] = ay; prm_.axis[2] = az;
  }
  void setEpsAngle(double eps_angle) {
    if (!(eps_angle >= 0.0 && eps_angle <= 1.5707963267948966)) throw std::runtime_error("rgc::SACSegmentationHip: eps_angle in [0, pi / 2] radians");
    prm_.eps_angle = eps_angle;
  }
  double getEpsAngle() const { return prm_.eps_angle; }
  // the seed of the generated hypothesis stream (rgc_plane_sample); PCL draws with rand()
  void setSeed(unsigned long long seed) { prm_.seed = seed; }
  // the hypothesis stream as triples of point indices in place of the generator (empty: the generator again)
  void setSamples(const std::vector<int>& triples) {
    if (triples.size() % 3) throw std::runtime_error("rgc::SACSegmentationHip: samples are triples of indices");
    samples_ = triples;
    use_samples_ = !triples.empty();
  }
  void setNegative(bool negative) { negative_ = negative; }
  // positions scored per launch, for tests and tuning (0 = automatic); no output depends on it
  void setBatch(int batch) { check(rgc_plane_set_batch(ctx_, batch), "rgc_plane_set_batch"); }

  // pcl::SACSegmentation::segment (host clouds): the inliers ascending, the coefficients a, b, c, d (empty when no model was found, as PCL leaves them)
  void segment(std::vector<int>& inliers, std::vector<float>& coefficients) {
    if (on_device_) throw std::runtime_error("rgc::SACSegmentationHip: a device cloud is segmented with the device-pointer overload");
    inliers.assign((size_t)n_, 0);
    int m = 0;
    double coeff[4];
    check(run(0, coeff, nullptr, inliers.data(), &m), "rgc_plane_segment");
    inliers.resize((size_t)m);
    const rgc_plane_info s = info();
    coefficients.clear();
    if (s.best_position >= 0) coefficients.assign({(float)coeff[0], (float)coeff[1], (float)coeff[2], (float)coeff[3]});
  }
  // pcl::ExtractIndices::filter behind it (host clouds): the inliers' x, y, z, c records in input order, or with setNegative(true) everything else
  void filter(std::vector<float>& xyzc) {
    if (on_device_) throw std::runtime_error("rgc::SACSegmentationHip: a device cloud is segmented with the device-pointer overload");
    xyzc.assign(4 * (size_t)n_, 0.f);
    int m = 0;
    double coeff[4];
    check(run(negative_ ? 1 : 0, coeff, xyzc.data(), nullptr, &m), "rgc_plane_segment");
    xyzc.resize(4 * (size_t)m);
  }
  // device clouds: records (n x 16 bytes) and indices (n ints) into device memory of the context's GPU, each nullable; returns the points written
  int segment(double coeff[4], float* d_xyzc, int* d_index) {
    if (!on_device_) throw std::runtime_error("rgc::SACSegmentationHip: the device-pointer overload needs setInputCloudDevice");
    int m = 0;
    check(run(negative_ ? 1 : 0, coeff, d_xyzc, d_index, &m), "rgc_plane_segment");
    return m;
  }
  rgc_plane_info info() const {
    rgc_plane_info s;
    check(rgc_plane_get_info(ctx_, &s), "rgc_plane_get_info");
    return s;
  }

private:
  int run(int negative, double* coeff, float* out, int* index, int* m) {
    return rgc_plane_segment(ctx_, xyz_, n_, stride_, on_device_, &prm_, use_samples_ ? samples_.data() : nullptr, use_samples_ ? (int)(samples_.size() / 3) : 0, negative, coeff, out,
                             index, nullptr, m);
  }
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  const float* xyz_ = nullptr;
  int n_ = 0, stride_ = 16, on_device_ = 0;
  rgc_plane_params prm_;
  std::vector<int> samples_;
  bool use_samples_ = false, negative_ = false;
};

}  // namespace rgc
