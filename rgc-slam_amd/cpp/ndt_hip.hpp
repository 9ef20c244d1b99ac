// ndt_hip.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_ndt_*): NDT registration (P2D / D2D) on a Gaussian voxel map.
// Stands in for fast_gicp::NDTCuda<PointSource, PointTarget> (rgc_slam/include/fast_gicp/ndt/ndt_cuda.hpp:27-60, impl/ndt_cuda_impl.hpp:10-90) WITHOUT
// requiring PCL/Eigen at build time, shaped like fast_vgicp_hip.hpp:
//
//   rgc::NDTHip ndt(0);                                   // its own context on device 0, or NDTHip(ctx) in an existing one (not owned)
//   ndt.setResolution(1.0); ndt.setDistanceMode(RGC_NDT_D2D); ndt.setNeighborSearchMethod(RGC_NDT_DIRECT7);
//   ndt.setInputTarget(map); ndt.setInputSource(scan);    // any cloud with ->points / ->size() of x,y,z-first points
//   ndt.align(guess);  ndt.getFinalTransformation();  ndt.hasConverged();
//
// Errors throw std::runtime_error carrying rgc_last_error().  No CPU fallback.
#pragma once
#include <array>
#include <cstddef>
#include <stdexcept>
#include <string>

#include "../../include/rgc_hip.h"

namespace rgc {

class NDTHip {
public:
  typedef std::array<float, 16> Matrix4f;    // row-major
  typedef std::array<double, 16> Matrix4d;   // row-major
  typedef std::array<double, 36> Matrix6d;
  typedef std::array<double, 6> Vector6d;

  explicit NDTHip(int hip_device = 0, const rgc_params* params = nullptr) : own_(true) {
    const int rc = rgc_create(hip_device, params, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
    init();
  }
  explicit NDTHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::NDTHip: null context");
    init();
  }
  ~NDTHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  NDTHip(const NDTHip&) = delete;
  NDTHip& operator=(const NDTHip&) = delete;

  rgc_ctx* context() const { return ctx_; }

  void setDistanceMode(int mode) { rgc_ndt_params p = prm_; p.distance_mode = mode; apply(p); }
  void setResolution(double resolution) { rgc_ndt_params p = prm_; p.resolution = resolution; apply(p); }
  void setNeighborSearchMethod(int method, double radius = -1.0) {
    rgc_ndt_params p = prm_;
    p.neighbor_method = method;
    if (method == RGC_NDT_DIRECT_RADIUS) p.neighbor_radius = radius;
    apply(p);
  }

  template <typename CloudPtr> void setInputTarget(const CloudPtr& cloud) {
    check(rgc_ndt_set_target(ctx_, &cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0])), "rgc_ndt_set_target");
  }
  template <typename CloudPtr> void setInputSource(const CloudPtr& cloud) {
    check(rgc_ndt_set_source(ctx_, &cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0])), "rgc_ndt_set_source");
  }
  void setInputTargetDevice(const float* d_xyz, int n, int stride_bytes) { check(rgc_ndt_set_target_device(ctx_, d_xyz, n, stride_bytes), "rgc_ndt_set_target_device"); }
  void setInputSourceDevice(const float* d_xyz, int n, int stride_bytes) { check(rgc_ndt_set_source_device(ctx_, d_xyz, n, stride_bytes), "rgc_ndt_set_source_device"); }
  void clearSource() { check(rgc_ndt_clear_source(ctx_), "rgc_ndt_clear_source"); }
  void clearTarget() { check(rgc_ndt_clear_target(ctx_), "rgc_ndt_clear_target"); }
  void swapSourceAndTarget() { check(rgc_ndt_swap_source_and_target(ctx_), "rgc_ndt_swap_source_and_target"); }

  double linearize(const Matrix4d& T, Matrix6d* H = nullptr, Vector6d* b = nullptr) {
    double cost = 0.0;
    check(rgc_ndt_linearize(ctx_, T.data(), H && b ? H->data() : nullptr, H && b ? b->data() : nullptr, &cost), "rgc_ndt_linearize");
    return cost;
  }
  double compute_error(const Matrix4d& T) {
    double cost = 0.0;
    check(rgc_ndt_compute_error(ctx_, T.data(), &cost), "rgc_ndt_compute_error");
    return cost;
  }

  void align(const Matrix4f& guess) {
    check(rgc_ndt_align(ctx_, guess.data(), final_.data(), hessian_.data(), &iterations_, &converged_, &lm_failed_), "rgc_ndt_align");
  }
  void align() {
    const Matrix4f I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    align(I);
  }
  const Matrix4f& getFinalTransformation() const { return final_; }
  const Matrix6d& getFinalHessian() const { return hessian_; }
  bool hasConverged() const { return converged_ != 0; }
  bool lmFailed() const { return lm_failed_ != 0; }
  int iterations() const { return iterations_; }

private:
  void init() {
    rgc_default_ndt_params(&prm_);
    apply(prm_);
    final_ = Matrix4f{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    hessian_.fill(0.0);
  }
  void apply(const rgc_ndt_params& p) {
    check(rgc_ndt_set_params(ctx_, &p), "rgc_ndt_set_params");
    prm_ = p;
  }
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + rgc_last_error(ctx_));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_ = false;
  rgc_ndt_params prm_;
  Matrix4f final_;
  Matrix6d hessian_;
  int iterations_ = 0, converged_ = 0, lm_failed_ = 0;
};

}  // namespace rgc
