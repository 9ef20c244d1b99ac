// fast_gicp_hip.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_gicp_*): GICP on exact nearest-neighbour correspondences.
// Stands in for fast_gicp::FastGICP<PointSource, PointTarget> (rgc_slam/include/fast_gicp/gicp/fast_gicp.hpp:25-87, impl/fast_gicp_impl.hpp:103-237) WITHOUT
// requiring PCL/Eigen at build time, shaped like ndt_hip.hpp:
//
//   rgc::FastGICPHip gicp(0);                              // its own context on device 0, or FastGICPHip(vgicp.context()) on the clouds of a FastVGICPHip (not owned)
//   gicp.setCorrespondenceRandomness(20); gicp.setMaxCorrespondenceDistance(1.0);
//   gicp.setInputTarget(map); gicp.setInputSource(scan);   // any cloud with ->points / ->size() of x,y,z-first points
//   gicp.align(guess);  gicp.getFinalTransformation();  gicp.hasConverged();
//
// The clouds and covariances are the context's own (rgc_set_source / rgc_set_target): what a FastVGICPHip on the same context has set is what
// GICP registers.  Errors throw std::runtime_error carrying rgc_last_error().  No CPU fallback.
#pragma once
#include <array>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

// What the adaptors below share: the context (owned, or another adaptor's), the clouds and covariances handed to it, the results of the last align().
class GICPHipBase {
public:
  typedef std::array<float, 16> Matrix4f;    // row-major
  typedef std::array<double, 16> Matrix4d;   // row-major
  typedef std::array<double, 36> Matrix6d;
  typedef std::array<double, 6> Vector6d;

  virtual ~GICPHipBase() { if (own_ && ctx_) rgc_destroy(ctx_); }
  GICPHipBase(const GICPHipBase&) = delete;
  GICPHipBase& operator=(const GICPHipBase&) = delete;

  rgc_ctx* context() const { return ctx_; }

  void setCorrespondenceRandomness(int k) { rgc_params p = params(); p.k_correspondences = k; check(rgc_set_params(ctx_, &p), "rgc_set_params"); }
  void setRegularizationMethod(int method) { check(rgc_set_regularization_method(ctx_, method), "rgc_set_regularization_method"); }

  template <typename CloudPtr> void setInputTarget(const CloudPtr& cloud) {
    check(rgc_set_target(ctx_, &cloud->points[0].x, (int)cloud->points.size(), (int)sizeof(cloud->points[0])), "rgc_set_target");
  }
  template <typename CloudPtr> void setInputSource(const CloudPtr& cloud) {
    n_source_ = (int)cloud->points.size();
    check(rgc_set_source(ctx_, &cloud->points[0].x, n_source_, (int)sizeof(cloud->points[0])), "rgc_set_source");
  }
  void setInputTargetDevice(const float* d_xyz, int n, int stride_bytes) { check(rgc_set_target_device(ctx_, d_xyz, n, stride_bytes), "rgc_set_target_device"); }
  void setInputSourceDevice(const float* d_xyz, int n, int stride_bytes) {
    n_source_ = n;
    check(rgc_set_source_device(ctx_, d_xyz, n, stride_bytes), "rgc_set_source_device");
  }
  // row-major 3x3 per point (the upper-left block of the reference's Matrix4d)
  void setSourceCovariances(const std::vector<double>& cov9) { check(rgc_set_source_covariances(ctx_, cov9.data(), (int)(cov9.size() / 9)), "rgc_set_source_covariances"); }
  void setTargetCovariances(const std::vector<double>& cov9) { check(rgc_set_target_covariances(ctx_, cov9.data(), (int)(cov9.size() / 9)), "rgc_set_target_covariances"); }
  void clearSource() { n_source_ = 0; check(rgc_clear_source(ctx_), "rgc_clear_source"); }
  void clearTarget() { check(rgc_clear_target(ctx_), "rgc_clear_target"); }

  const Matrix4f& getFinalTransformation() const { return final_; }
  const Matrix6d& getFinalHessian() const { return hessian_; }
  double getFitnessScore() const { return fitness_; }
  bool hasConverged() const { return converged_ != 0; }
  int iterations() const { return iterations_; }

protected:
  GICPHipBase(int hip_device, const rgc_params* params) : own_(true) {
    const int rc = rgc_create(hip_device, params, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
    init();
  }
  GICPHipBase(rgc_ctx* ctx, const char* who) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error(std::string(who) + ": null context");
    init();
  }
  void init() {
    final_ = Matrix4f{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    hessian_.fill(0.0);
  }
  rgc_params params() const {
    rgc_params p;
    check(rgc_get_params(ctx_, &p), "rgc_get_params");
    return p;
  }
  void check(int rc, const char* what) const {
    if (rc != RGC_OK) throw std::runtime_error(std::string(what) + ": " + rgc_last_error(ctx_));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_ = false;
  int n_source_ = 0;
  Matrix4f final_;
  Matrix6d hessian_;
  double fitness_ = 0.0;
  int iterations_ = 0, converged_ = 0, failed_ = 0;   // failed_: the solve gave up (lmFailed() / failed())
};

class FastGICPHip : public GICPHipBase {
public:
  explicit FastGICPHip(int hip_device = 0, const rgc_params* params = nullptr) : GICPHipBase(hip_device, params) {}
  explicit FastGICPHip(rgc_ctx* ctx) : GICPHipBase(ctx, "rgc::FastGICPHip") {}

  void setMaximumIterations(int n) { rgc_params p = params(); p.max_iterations = n; check(rgc_set_params(ctx_, &p), "rgc_set_params"); }
  void setTransformationEpsilon(double e) { rgc_params p = params(); p.translation_eps = e; check(rgc_set_params(ctx_, &p), "rgc_set_params"); }
  void setRotationEpsilon(double e) { rgc_params p = params(); p.rotation_eps = e; check(rgc_set_params(ctx_, &p), "rgc_set_params"); }
  void setMaxCorrespondenceDistance(double d) { check(rgc_gicp_set_max_correspondence_distance(ctx_, d), "rgc_gicp_set_max_correspondence_distance"); }
  double getMaxCorrespondenceDistance() const {
    double d = 0.0;
    check(rgc_gicp_get_max_correspondence_distance(ctx_, &d), "rgc_gicp_get_max_correspondence_distance");
    return d;
  }
  void swapSourceAndTarget() {
    check(rgc_swap_source_and_target(ctx_), "rgc_swap_source_and_target");
    rgc_stats st;
    check(rgc_get_stats(ctx_, &st), "rgc_get_stats");
    n_source_ = st.n_source;
  }

  // (virtual where FastGICPSingleThreadHip below overrides, as the reference class overrides FastGICP: fast_gicp_st.hpp:53-60)
  virtual double linearize(const Matrix4d& T, Matrix6d* H = nullptr, Vector6d* b = nullptr) {
    double cost = 0.0;
    check(rgc_gicp_linearize(ctx_, T.data(), H && b ? H->data() : nullptr, H && b ? b->data() : nullptr, &cost), "rgc_gicp_linearize");
    return cost;
  }
  virtual double compute_error(const Matrix4d& T) {
    double cost = 0.0;
    check(rgc_gicp_compute_error(ctx_, T.data(), &cost), "rgc_gicp_compute_error");
    return cost;
  }
  virtual int numCorrespondences() {
    int n = 0;
    check(rgc_gicp_num_correspondences(ctx_, &n), "rgc_gicp_num_correspondences");
    return n;
  }
  // the pairs of the last linearize in the source's order: idx -1 where rejected, sq_dist the key even there
  virtual void getCorrespondences(std::vector<int>& idx, std::vector<float>& sq_dist) {
    idx.assign((size_t)n_source_, -1);
    sq_dist.assign((size_t)n_source_, 0.f);
    check(rgc_gicp_get_correspondences(ctx_, idx.data(), sq_dist.data()), "rgc_gicp_get_correspondences");
  }

  virtual void align(const Matrix4f& guess) {
    check(rgc_gicp_align(ctx_, guess.data(), final_.data(), hessian_.data(), &fitness_, &iterations_, &converged_, &failed_), "rgc_gicp_align");
  }
  void align() {
    const Matrix4f I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    align(I);
  }
  bool lmFailed() const { return failed_ != 0; }
};

// Stands in for fast_gicp::FastGICPSingleThread<PointSource, PointTarget> (rgc_slam/include/fast_gicp/gicp/fast_gicp_st.hpp:20-65,
// impl/fast_gicp_st_impl.hpp:19-125) over rgc_gicpst_*, and derives from FastGICPHip as that class derives from FastGICP: the clouds, the covariances and
// the settings are FastGICP's; linearize, compute_error, align and the read-outs are overridden.  A source point keeps an anchor and is searched again
// only when the triangle inequality cannot prove its nearest neighbour unchanged; a point that is not searched keeps its pair and its Mahalanobis
// matrix.  align() drops the anchors first (:19-22); reset() drops them between linearisations.
//
//   rgc::FastGICPSingleThreadHip st(0);                    // or FastGICPSingleThreadHip(other.context()) on the clouds of another adaptor (not owned)
//   st.setInputTarget(map); st.setInputSource(scan);
//   st.align(guess);  st.getFinalTransformation();  st.numSearched();
class FastGICPSingleThreadHip : public FastGICPHip {
public:
  explicit FastGICPSingleThreadHip(int hip_device = 0, const rgc_params* params = nullptr) : FastGICPHip(hip_device, params) {}
  explicit FastGICPSingleThreadHip(rgc_ctx* ctx) : FastGICPHip(ctx) {}

  void reset() { check(rgc_gicpst_reset(ctx_), "rgc_gicpst_reset"); }
  double linearize(const Matrix4d& T, Matrix6d* H = nullptr, Vector6d* b = nullptr) override {
    double cost = 0.0;
    check(rgc_gicpst_linearize(ctx_, T.data(), H && b ? H->data() : nullptr, H && b ? b->data() : nullptr, &cost), "rgc_gicpst_linearize");
    return cost;
  }
  double compute_error(const Matrix4d& T) override {
    double cost = 0.0;
    check(rgc_gicpst_compute_error(ctx_, T.data(), &cost), "rgc_gicpst_compute_error");
    return cost;
  }
  int numCorrespondences() override {
    int n = 0;
    check(rgc_gicpst_num_correspondences(ctx_, &n), "rgc_gicpst_num_correspondences");
    return n;
  }
  int numSearched() {   // source points the last linearize searched
    int n = 0;
    check(rgc_gicpst_num_searched(ctx_, &n), "rgc_gicpst_num_searched");
    return n;
  }
  void getCorrespondences(std::vector<int>& idx, std::vector<float>& sq_dist) override {
    idx.assign((size_t)n_source_, -1);
    sq_dist.assign((size_t)n_source_, 0.f);
    check(rgc_gicpst_get_correspondences(ctx_, idx.data(), sq_dist.data(), nullptr, nullptr), "rgc_gicpst_get_correspondences");
  }
  // the state after the last linearize in the source's order: idx -1 where not kept, the keys to the nearest and the second nearest at the point's
  // anchor, searched 1 where the last linearize searched the point
  void getCorrespondences(std::vector<int>& idx, std::vector<float>& sq_dist, std::vector<float>& second_sq_dist, std::vector<int>& searched) {
    idx.assign((size_t)n_source_, -1);
    sq_dist.assign((size_t)n_source_, 0.f);
    second_sq_dist.assign((size_t)n_source_, 0.f);
    searched.assign((size_t)n_source_, 0);
    check(rgc_gicpst_get_correspondences(ctx_, idx.data(), sq_dist.data(), second_sq_dist.data(), searched.data()), "rgc_gicpst_get_correspondences");
  }
  using FastGICPHip::align;
  void align(const Matrix4f& guess) override {
    check(rgc_gicpst_align(ctx_, guess.data(), final_.data(), hessian_.data(), &fitness_, &iterations_, &converged_, &failed_), "rgc_gicpst_align");
  }
};

// Stands in for fast_gicp::FastGICPMultiPoints<PointSource, PointTarget> (rgc_slam/include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp:40-53,
// fast_gicp_mp_impl.hpp:92-221) over rgc_gicpmp_*: every source point against the distance-weighted merge of every target Gaussian within the search
// radius, plain Gauss-Newton.  The reference's public names, the pcl::Registration calls FastGICPHip has, and the setter the reference forgot
// (setNeighborSearchRadius).  setRotationEpsilon / setTransformationEpsilon / setMaximumIterations set THIS method's limits (1e-5, 1e-5, 64).
//
//   rgc::FastGICPMultiPointsHip mp(0);                      // or FastGICPMultiPointsHip(other.context()) on the clouds of another adaptor (not owned)
//   mp.setNeighborSearchRadius(0.5); mp.setInputTarget(map); mp.setInputSource(scan);
//   mp.align(guess);  mp.getFinalTransformation();  mp.hasConverged();
class FastGICPMultiPointsHip : public GICPHipBase {
public:
  explicit FastGICPMultiPointsHip(int hip_device = 0, const rgc_params* params = nullptr) : GICPHipBase(hip_device, params) {}
  explicit FastGICPMultiPointsHip(rgc_ctx* ctx) : GICPHipBase(ctx, "rgc::FastGICPMultiPointsHip") {}

  void setNumThreads(int) {}                 // CPU threads (fast_gicp_mp_impl.hpp:47-55): nothing to set on the GPU
  void setNeighborSearchRadius(double r) { rgc_gicp_mp_params p = mp_params(); p.neighbor_search_radius = r; check(rgc_gicpmp_set_params(ctx_, &p), "rgc_gicpmp_set_params"); }
  double getNeighborSearchRadius() const { return mp_params().neighbor_search_radius; }
  void setRotationEpsilon(double e) { rgc_gicp_mp_params p = mp_params(); p.rotation_epsilon = e; check(rgc_gicpmp_set_params(ctx_, &p), "rgc_gicpmp_set_params"); }
  void setTransformationEpsilon(double e) { rgc_gicp_mp_params p = mp_params(); p.transformation_epsilon = e; check(rgc_gicpmp_set_params(ctx_, &p), "rgc_gicpmp_set_params"); }
  void setMaximumIterations(int n) { rgc_gicp_mp_params p = mp_params(); p.max_iterations = n; check(rgc_gicpmp_set_params(ctx_, &p), "rgc_gicpmp_set_params"); }

  double linearize(const Matrix4d& T, Matrix6d* H = nullptr, Vector6d* b = nullptr) {
    double cost = 0.0;
    check(rgc_gicpmp_linearize(ctx_, T.data(), H && b ? H->data() : nullptr, H && b ? b->data() : nullptr, &cost), "rgc_gicpmp_linearize");
    return cost;
  }
  // of the last linearize: the source points with a neighbour / the neighbours of all of them
  int numCorrespondences() {
    int n = 0;
    check(rgc_gicpmp_num_correspondences(ctx_, &n, nullptr), "rgc_gicpmp_num_correspondences");
    return n;
  }
  long long numPairs() {
    long long m = 0;
    check(rgc_gicpmp_num_correspondences(ctx_, nullptr, &m), "rgc_gicpmp_num_correspondences");
    return m;
  }
  long long numCandidates() {   // target points the gather looked at over all source points
    long long m = 0;
    check(rgc_gicpmp_num_candidates(ctx_, &m), "rgc_gicpmp_num_candidates");
    return m;
  }
  // the merge of the last linearize in the source's order: |N_i|, sw, mean_B (3 per point), cov_B (6 per point: xx xy xz yy yz zz)
  void merged(std::vector<int>& count, std::vector<double>& sum_w, std::vector<double>& mean3, std::vector<double>& cov6) {
    count.assign((size_t)n_source_, 0);
    sum_w.assign((size_t)n_source_, 0.0);
    mean3.assign((size_t)n_source_ * 3, 0.0);
    cov6.assign((size_t)n_source_ * 6, 0.0);
    check(rgc_gicpmp_get_merged(ctx_, count.data(), sum_w.data(), mean3.data(), cov6.data()), "rgc_gicpmp_get_merged");
  }
  // the rows N_i in CSR form: row i = idx[offsets[i] .. offsets[i + 1]), original target indices, and their fp32 keys
  void neighbors(std::vector<int>& offsets, std::vector<int>& idx, std::vector<float>& sq_dist) {
    const long long total = numPairs();
    if (total > 2147483647LL) throw std::runtime_error("rgc::FastGICPMultiPointsHip::neighbors: more than 2^31 - 1 neighbours");
    offsets.assign((size_t)n_source_ + 1, 0);
    idx.assign((size_t)total, -1);
    sq_dist.assign((size_t)total, 0.f);
    long long n_total = 0;
    check(rgc_gicpmp_get_neighbors(ctx_, offsets.data(), idx.data(), sq_dist.data(), (int)total, &n_total), "rgc_gicpmp_get_neighbors");
  }

  void align(const Matrix4f& guess) {
    check(rgc_gicpmp_align(ctx_, guess.data(), final_.data(), hessian_.data(), &fitness_, &iterations_, &converged_, &failed_), "rgc_gicpmp_align");
  }
  void align() {
    const Matrix4f I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    align(I);
  }
  bool failed() const { return failed_ != 0; }

private:
  rgc_gicp_mp_params mp_params() const {
    rgc_gicp_mp_params p;
    check(rgc_gicpmp_get_params(ctx_, &p), "rgc_gicpmp_get_params");
    return p;
  }
};

}  // namespace rgc
