// features_hip.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_normal_*): surface normal estimation on the GPU.  It stands in for
// pcl::NormalEstimation<PointInT, PointOutT> WITHOUT requiring PCL at build time, with its member names:
//
//   rgc::NormalEstimationHip ne(0);                      // its own context on device 0, or (ctx) in an existing one (not owned)
//   ne.setInputCloud(cloud);                             // any cloud with ->points of x,y,z-first points of at least 12 bytes
//   ne.setSearchSurface(dense);                          // optional: the cloud the neighbours come from
//   ne.setKSearch(10);                                   // or ne.setRadiusSearch(0.5): exactly one of the two
//   ne.setViewPoint(0.f, 0.f, 0.f);
//   ne.compute(normals);                                 // std::vector<float>, 4 per point: nx, ny, nz, curvature (NaN: fewer than three neighbours)
//
// The semantics (the fp32 key, the total order, the strict radius, the fp64 moments about the query, the sign rule) are stated in include/rgc_hip.h.  A
// refused call throws std::runtime_error carrying rgc_last_error(), a refused setter one naming the range it accepts.  No CPU fallback.
// rgc::FPFHEstimationHip (rgc_fpfh_*, pcl::FPFHEstimation), further down, consumes those normals.
#pragma once
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

class NormalEstimationHip {
public:
  explicit NormalEstimationHip(int hip_device = 0) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
    rgc_default_normal_params(&p_);
  }
  explicit NormalEstimationHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::NormalEstimationHip: null context");
    rgc_default_normal_params(&p_);
  }
  ~NormalEstimationHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  NormalEstimationHip(const NormalEstimationHip&) = delete;
  NormalEstimationHip& operator=(const NormalEstimationHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    xyz_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    n_ = (int)cloud->points.size();
    stride_ = (int)sizeof(cloud->points[0]);
    on_device_ = 0;
  }
  // pcl::Feature::setSearchSurface: the cloud the neighbours come from (an empty pointer-like or an empty cloud: the input cloud itself)
  template <typename CloudPtr> void setSearchSurface(const CloudPtr& cloud) {
    surf_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    ns_ = (int)cloud->points.size();
    sstride_ = (int)sizeof(cloud->points[0]);
  }
  void clearSearchSurface() { surf_ = nullptr; ns_ = 0; sstride_ = 0; }
  // both clouds in device memory of the context's GPU (d_surface nullable), the outputs of computeDevice too
  void setInputCloudDevice(const float* d_xyz, int n, int stride_bytes, const float* d_surface = nullptr, int n_surface = 0, int surface_stride_bytes = 0) {
    xyz_ = d_xyz; n_ = n; stride_ = stride_bytes; on_device_ = 1;
    surf_ = d_surface; ns_ = n_surface; sstride_ = surface_stride_bytes;
  }
  // 3 .. RGC_NORMAL_MAX_K selects the k route (and clears a radius), 0 deselects it
  void setKSearch(int k) {
    if (k != 0 && (k < 3 || k > RGC_NORMAL_MAX_K)) throw std::runtime_error("rgc::NormalEstimationHip: k in 3.." + std::to_string(RGC_NORMAL_MAX_K) + " (0: not this route)");
    p_.k = k;
    if (k) p_.radius = 0.0;
  }
  int getKSearch() const { return p_.k; }
  // > 0 selects the radius route (and clears k), 0 deselects it
  void setRadiusSearch(double radius) {
    const float r2 = (float)(radius * radius);
    if (radius != 0.0 && !(std::isfinite(radius) && radius > 0.0 && std::isfinite(r2) && r2 > 0.f))
      throw std::runtime_error("rgc::NormalEstimationHip: the radius must be finite and > 0, float(r r) finite and > 0");
    p_.radius = radius;
    if (radius != 0.0) p_.k = 0;
  }
  double getRadiusSearch() const { return p_.radius; }
  void setViewPoint(float vpx, float vpy, float vpz) {
    if (!std::isfinite(vpx) || !std::isfinite(vpy) || !std::isfinite(vpz)) throw std::runtime_error("rgc::NormalEstimationHip: the viewpoint must be finite");
    p_.viewpoint[0] = vpx; p_.viewpoint[1] = vpy; p_.viewpoint[2] = vpz;
  }
  void getViewPoint(float& vpx, float& vpy, float& vpz) const { vpx = p_.viewpoint[0]; vpy = p_.viewpoint[1]; vpz = p_.viewpoint[2]; }
  // true (PCL): flipNormalTowardsViewpoint; false: the component of largest magnitude is made positive
  void setFlip(bool flip) { p_.flip = flip ? 1 : 0; }
  // the grid's cell size, for tests and tuning (0 = chosen from the surface cloud's box and size)
  void setCell(double cell) { check(rgc_normal_set_cell(ctx_, cell), "rgc_normal_set_cell"); }

  // pcl::Feature::compute: 4 floats per input point -- nx, ny, nz, curvature; returns the number of valid rows (host clouds)
  int compute(std::vector<float>& normal4) { return compute(normal4, nullptr, nullptr, nullptr); }
  // ... and, each nullable, the covariances {xx,xy,xz,yy,yz,zz} (6 per point), the centroids (3 per point), the members used
  int compute(std::vector<float>& normal4, std::vector<double>* cov6, std::vector<double>* centroid, std::vector<int>* count) {
    if (on_device_) throw std::runtime_error("rgc::NormalEstimationHip: a device cloud is computed with computeDevice");
    normal4.assign((size_t)n_ * 4, 0.f);
    if (cov6) cov6->assign((size_t)n_ * 6, 0.0);
    if (centroid) centroid->assign((size_t)n_ * 3, 0.0);
    if (count) count->assign((size_t)n_, 0);
    int valid = 0;
    check(rgc_normal_estimate(ctx_, xyz_, n_, stride_, surf_, ns_, sstride_, 0, &p_, normal4.data(), cov6 ? cov6->data() : nullptr, centroid ? centroid->data() : nullptr,
                              count ? count->data() : nullptr, &valid),
          "rgc_normal_estimate");
    return valid;
  }
  // device clouds: the outputs into device memory of the context's GPU (each nullable, room for n rows); returns the number of valid rows
  int computeDevice(float* d_normal4, double* d_cov6 = nullptr, double* d_centroid = nullptr, int* d_count = nullptr) {
    if (!on_device_) throw std::runtime_error("rgc::NormalEstimationHip: computeDevice needs setInputCloudDevice");
    int valid = 0;
    check(rgc_normal_estimate(ctx_, xyz_, n_, stride_, surf_, ns_, sstride_, 1, &p_, d_normal4, d_cov6, d_centroid, d_count, &valid), "rgc_normal_estimate");
    return valid;
  }
  rgc_normal_info info() const {
    rgc_normal_info s;
    check(rgc_normal_get_info(ctx_, &s), "rgc_normal_get_info");
    return s;
  }

private:
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  rgc_normal_params p_;
  const float* xyz_ = nullptr;
  const float* surf_ = nullptr;
  int n_ = 0, stride_ = 16, ns_ = 0, sstride_ = 0, on_device_ = 0;
};

// pcl::FPFHEstimation<PointInT, PointNT, pcl::FPFHSignature33> over rgc_fpfh_*: 33 floats per input point from the normals of the search surface.
//
//   rgc::FPFHEstimationHip fe(ne.context());             // in the context the normals were computed in, or (0): its own on device 0
//   fe.setInputCloud(keypoints);
//   fe.setSearchSurface(dense);                          // optional
//   fe.setInputNormals(normals);                         // a cloud with ->points of normal_x, normal_y, normal_z-first points (pcl::Normal), or
//   fe.setInputNormals(n4.data(), rows, 16);             //   NormalEstimationHip::compute's rows as they are
//   fe.setRadiusSearch(0.5);
//   fe.compute(fpfh);                                    // std::vector<float>, 33 per point (NaN: no member)
class FPFHEstimationHip {
public:
  explicit FPFHEstimationHip(int hip_device = 0) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
    rgc_default_fpfh_params(&p_);
  }
  explicit FPFHEstimationHip(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::FPFHEstimationHip: null context");
    rgc_default_fpfh_params(&p_);
  }
  ~FPFHEstimationHip() { if (own_ && ctx_) rgc_destroy(ctx_); }
  FPFHEstimationHip(const FPFHEstimationHip&) = delete;
  FPFHEstimationHip& operator=(const FPFHEstimationHip&) = delete;

  rgc_ctx* context() const { return ctx_; }
  template <typename CloudPtr> void setInputCloud(const CloudPtr& cloud) {
    xyz_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    n_ = (int)cloud->points.size();
    stride_ = (int)sizeof(cloud->points[0]);
    on_device_ = 0;
  }
  template <typename CloudPtr> void setSearchSurface(const CloudPtr& cloud) {
    surf_ = cloud->points.empty() ? nullptr : &cloud->points[0].x;
    ns_ = (int)cloud->points.size();
    sstride_ = (int)sizeof(cloud->points[0]);
  }
  void clearSearchSurface() { surf_ = nullptr; ns_ = 0; sstride_ = 0; }
  // one normal per SURFACE point (per input point without a search surface), used as given
  template <typename NormalsPtr> void setInputNormals(const NormalsPtr& normals) {
    nrm_ = normals->points.empty() ? nullptr : &normals->points[0].normal_x;
    nn_ = (int)normals->points.size();
    nstride_ = (int)sizeof(normals->points[0]);
  }
  void setInputNormals(const float* normals, int rows, int stride_bytes) { nrm_ = normals; nn_ = rows; nstride_ = stride_bytes; }
  // the clouds and the normals in device memory of the context's GPU (d_surface nullable), the outputs of computeDevice too
  void setInputDevice(const float* d_xyz, int n, int stride_bytes, const float* d_normals, int normal_stride_bytes, const float* d_surface = nullptr, int n_surface = 0,
                      int surface_stride_bytes = 0) {
    xyz_ = d_xyz; n_ = n; stride_ = stride_bytes; on_device_ = 1;
    surf_ = d_surface; ns_ = n_surface; sstride_ = surface_stride_bytes;
    nrm_ = d_normals; nn_ = d_surface ? n_surface : n; nstride_ = normal_stride_bytes;
  }
  void setRadiusSearch(double radius) {
    const float r2 = (float)(radius * radius);
    if (!(std::isfinite(radius) && radius > 0.0 && std::isfinite(r2) && r2 > 0.f))
      throw std::runtime_error("rgc::FPFHEstimationHip: the radius must be finite and > 0, float(r r) finite and > 0");
    p_.radius = radius;
  }
  double getRadiusSearch() const { return p_.radius; }
  void setCell(double cell) { check(rgc_fpfh_set_cell(ctx_, cell), "rgc_fpfh_set_cell"); }

  // pcl::Feature::compute: 33 floats per input point; returns the number of queries with a member (host clouds)
  int compute(std::vector<float>& fpfh) { return compute(fpfh, nullptr, nullptr, nullptr); }
  // ... and, each nullable, the first pass' counts (33 per surface point) and row sizes (-1: not computed), the queries' row sizes
  int compute(std::vector<float>& fpfh, std::vector<unsigned>* spfh, std::vector<int>* spfh_count, std::vector<int>* count) {
    if (on_device_) throw std::runtime_error("rgc::FPFHEstimationHip: device clouds are computed with computeDevice");
    const size_t rows = surf_ ? (size_t)ns_ : (size_t)n_;
    if ((size_t)nn_ != rows) throw std::runtime_error("rgc::FPFHEstimationHip: one normal per surface point (setInputNormals)");
    fpfh.assign((size_t)n_ * RGC_FPFH_BINS, 0.f);
    if (spfh) spfh->assign(rows * RGC_FPFH_BINS, 0u);
    if (spfh_count) spfh_count->assign(rows, 0);
    if (count) count->assign((size_t)n_, 0);
    int valid = 0;
    check(rgc_fpfh_estimate(ctx_, xyz_, n_, stride_, surf_, ns_, sstride_, nrm_, nstride_, 0, &p_, fpfh.data(), spfh ? spfh->data() : nullptr,
                            spfh_count ? spfh_count->data() : nullptr, count ? count->data() : nullptr, &valid),
          "rgc_fpfh_estimate");
    return valid;
  }
  int computeDevice(float* d_fpfh, unsigned* d_spfh = nullptr, int* d_spfh_count = nullptr, int* d_count = nullptr) {
    if (!on_device_) throw std::runtime_error("rgc::FPFHEstimationHip: computeDevice needs setInputDevice");
    int valid = 0;
    check(rgc_fpfh_estimate(ctx_, xyz_, n_, stride_, surf_, ns_, sstride_, nrm_, nstride_, 1, &p_, d_fpfh, d_spfh, d_spfh_count, d_count, &valid), "rgc_fpfh_estimate");
    return valid;
  }
  rgc_fpfh_info info() const {
    rgc_fpfh_info s;
    check(rgc_fpfh_get_info(ctx_, &s), "rgc_fpfh_get_info");
    return s;
  }

private:
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? rgc_last_error(ctx_) : rgc_status_string(rc)));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_;
  rgc_fpfh_params p_;
  const float* xyz_ = nullptr;
  const float* surf_ = nullptr;
  const float* nrm_ = nullptr;
  int n_ = 0, stride_ = 16, ns_ = 0, sstride_ = 0, nn_ = 0, nstride_ = 16, on_device_ = 0;
};

}  // namespace rgc
