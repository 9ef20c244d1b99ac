// keyframe_store.hpp -- header-only C++ adaptor over the C-ABI (include/rgc_hip.h, rgc_kf_*): the mapping node's keyframe store kept on
// the device.  Stands in for cornerCloudKeyFrames / surfCloudKeyFrames / scanCloudKeyFrames + cloudKeyPoses6D and for the three loops that
// assemble a cloud from them with transformPointCloud per keyframe, `+=` and a pcl::VoxelGrid
// (rgc_slam/src/RGC_mapping.cpp:1503-1616, 2180-2216, 2508-2537), WITHOUT requiring PCL/Eigen at build time:
//
//   rgc::KeyframeStore store(ctx);                         // in the context that consumes its clouds (FastVGICPHip::context()), or its own
//   store.push(keyFrameNum, pose6D, corner, surf, scan);   // any cloud with ->points / ->size() of 16-byte-or-wider x,y,z,c points
//   store.setPoses(ids, poses);                            // correctKeyFramePoseGraph (:1618-1686)
//   rgc::DeviceCloud target = store.assembleDevice(ids, rgc::KeyframeStore::CORNER | rgc::KeyframeStore::SURF, 0.4f);
//   rgc_icp_align_device(ctx, source.data(), source.size(), target.data(), target.size(), 16, &icp_params, T, &result);
//   loops.push_back(rgc::makeLoop(latestPose, loopPose, T, latestId, loopId));            // the loop edge of :2086-2107
//   rgc_pgo_report rep = store.optimizePoseGraph(ids, loops);                             // PoseGraphOptimize4DoF (:2303-2466): the poses are corrected
//   rgc::LoopDetection d = store.detectLoop();            // detectLoopClosure (:2141-2225): which pair, which history keyframes
//   std::vector<int> near = store.selectSurrounding(x, y, z, 15.f, 0.3f), all = store.selectGlobal(0.5f);   // (:1525-1548, 2493-2505)
//
// Errors throw std::runtime_error carrying rgc_last_error().  No CPU fallback.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rgc_hip.h"

namespace rgc {

// n points {x, y, z, c} in device memory of a context; frees them with the object
class DeviceCloud {
public:
  DeviceCloud() = default;
  DeviceCloud(rgc_ctx* ctx, float* d, int n, int n_raw) : ctx_(ctx), d_(d), n_(n), n_raw_(n_raw) {}
  ~DeviceCloud() { reset(); }
  DeviceCloud(const DeviceCloud&) = delete;
  DeviceCloud& operator=(const DeviceCloud&) = delete;
  DeviceCloud(DeviceCloud&& o) noexcept : ctx_(o.ctx_), d_(o.d_), n_(o.n_), n_raw_(o.n_raw_) { o.d_ = nullptr; o.n_ = o.n_raw_ = 0; }
  DeviceCloud& operator=(DeviceCloud&& o) noexcept {
    if (this != &o) { reset(); ctx_ = o.ctx_; d_ = o.d_; n_ = o.n_; n_raw_ = o.n_raw_; o.d_ = nullptr; o.n_ = o.n_raw_ = 0; }
    return *this;
  }
  const float* data() const { return d_; }
  int size() const { return n_; }          // points after the leaf filter (or of the concatenation)
  int rawSize() const { return n_raw_; }   // points before it
  std::vector<float> download() const {
    std::vector<float> h((std::size_t)n_ * 4);
    if (n_ > 0 && rgc_download(ctx_, h.data(), d_, h.size() * sizeof(float)) != RGC_OK) throw std::runtime_error(std::string("rgc_download: ") + rgc_last_error(ctx_));
    return h;
  }

private:
  void reset() { if (d_) (void)rgc_device_free(ctx_, d_); d_ = nullptr; }
  rgc_ctx* ctx_ = nullptr;
  float* d_ = nullptr;
  int n_ = 0, n_raw_ = 0;
};

// the loop edge a loop-closure ICP gives (rgc_pgo_make_loop): the two key poses as they were when it ran, its final transformation (row-major 4x4)
inline rgc_pgo_loop makeLoop(const rgc_kf_pose& latest_pose, const rgc_kf_pose& loop_pose, const float T_drift[16], int key_curr, int key_loop) {
  rgc_pgo_loop l;
  if (rgc_pgo_make_loop(&latest_pose, &loop_pose, T_drift, key_curr, key_loop, &l) != RGC_OK) throw std::runtime_error("rgc::makeLoop: a pose or the drift is not finite");
  return l;
}

// pcl::UniformSampling on the device (rgc_uniform_sampling): per occupied leaf the point of the host cloud nearest the leaf's centre, leaves in ascending
// leaf index; n x 4 floats {x, y, z, c} and, when asked for, the winners' input indices
inline std::vector<float> uniformSampling(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, float leaf, std::vector<int>* index = nullptr) {
  std::vector<float> out((std::size_t)(n > 0 ? n : 1) * 4);
  if (index) index->assign((std::size_t)(n > 0 ? n : 1), 0);
  int n_out = 0;
  const int rc = rgc_uniform_sampling(ctx, xyzc, n, stride_bytes, leaf, out.data(), index ? index->data() : nullptr, &n_out, 0);
  if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_uniform_sampling: ") + rgc_status_string(rc) + ": " + rgc_last_error(ctx));
  out.resize((std::size_t)n_out * 4);
  if (index) index->resize((std::size_t)n_out);
  return out;
}

// what rgc::KeyframeStore::detectLoop returns: the candidate and the history keyframes (the ICP target's ids, in order)
struct LoopDetection {
  rgc_kf_loop_candidate candidate;
  std::vector<int> history_ids;
};

class KeyframeStore {
public:
  enum Kind : unsigned { CORNER = 1u << RGC_KF_CORNER, SURF = 1u << RGC_KF_SURF, SCAN = 1u << RGC_KF_SCAN };

  // a store in an existing context (not owned: it must outlive the store) ...
  explicit KeyframeStore(rgc_ctx* ctx) : ctx_(ctx), own_(false) {
    if (!ctx) throw std::runtime_error("rgc::KeyframeStore: null context");
  }
  // ... or in a context of its own
  explicit KeyframeStore(int hip_device = 0) : own_(true) {
    const int rc = rgc_create(hip_device, nullptr, &ctx_);
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_create: ") + rgc_status_string(rc));
  }
  ~KeyframeStore() { if (own_) rgc_destroy(ctx_); }
  KeyframeStore(const KeyframeStore&) = delete;
  KeyframeStore& operator=(const KeyframeStore&) = delete;

  rgc_ctx* context() { return ctx_; }
  void reset() { chk(rgc_kf_reset(ctx_)); }

  // body-frame clouds, host memory (on_device = false) or device memory of the context; a kind may be empty (nullptr, 0)
  void push(int id, const rgc_kf_pose& pose, const float* corner, int n_corner, const float* surf, int n_surf, const float* scan, int n_scan,
            int stride_bytes, bool on_device = false) {
    chk(rgc_kf_push(ctx_, id, &pose, corner, n_corner, surf, n_surf, scan, n_scan, stride_bytes, on_device ? 1 : 0));
  }
  // pcl-style clouds: anything with ->points[i].x and ->points.size(), all three of one point type; a null pointer is an empty kind
  template <class CloudPtr>
  void push(int id, const rgc_kf_pose& pose, const CloudPtr& corner, const CloudPtr& surf, const CloudPtr& scan) {
    push(id, pose, first(corner), count(corner), first(surf), count(surf), first(scan), count(scan), (int)sizeof(corner->points[0]));
  }
  // PointXYZIRPYT-like poses (x, y, z, roll, pitch, yaw members)
  template <class Pose6D>
  static rgc_kf_pose pose(const Pose6D& p) { return rgc_kf_pose{(float)p.x, (float)p.y, (float)p.z, (float)p.roll, (float)p.pitch, (float)p.yaw}; }

  void setPoses(const std::vector<int>& ids, const std::vector<rgc_kf_pose>& poses) {
    if (ids.size() != poses.size()) throw std::runtime_error("rgc::KeyframeStore::setPoses: one pose per id");
    chk(rgc_kf_set_poses(ctx_, ids.data(), poses.data(), (int)ids.size()));
  }
  rgc_kf_info info() { rgc_kf_info i; chk(rgc_kf_get_info(ctx_, &i)); return i; }

  // travelled distance / accumulated |yaw change| up to each keyframe, fixed at its push (:1887-1908); either output nullable
  void travel(const std::vector<int>& ids, std::vector<float>* distance, std::vector<float>* angle = nullptr) {
    if (distance) distance->assign(ids.size(), 0.f);
    if (angle) angle->assign(ids.size(), 0.f);
    chk(rgc_kf_get_travel(ctx_, ids.data(), (int)ids.size(), distance && !ids.empty() ? distance->data() : nullptr, angle && !ids.empty() ? angle->data() : nullptr));
  }
  // extractSurroundingKeyFramesAndMap's selection (:1525-1548): the key poses strictly within `radius` of the centre, thinned by UniformSampling at leaf
  // `density`; ids in ascending leaf index.  n_in_radius (nullable): poses inside the radius
  std::vector<int> selectSurrounding(float x, float y, float z, float radius = 15.f, float density = 0.3f, int* n_in_radius = nullptr) {
    const float c[3] = {x, y, z};
    std::vector<int> out((std::size_t)info().n_keyframes + 1);
    int n_in = 0, n_out = 0;
    chk(rgc_kf_select_surrounding(ctx_, c, radius, density, out.data(), (int)out.size(), &n_in, &n_out));
    out.resize((std::size_t)n_out);
    if (n_in_radius) *n_in_radius = n_in;
    return out;
  }
  // publishGlobalMap's selection (:2493-2505): UniformSampling of every key position
  std::vector<int> selectGlobal(float pose_density = 0.5f) {
    std::vector<int> out((std::size_t)info().n_keyframes + 1);
    int n_out = 0;
    chk(rgc_kf_select_global(ctx_, pose_density, out.data(), (int)out.size(), &n_out));
    out.resize((std::size_t)n_out);
    return out;
  }
  // detectLoopClosure (:2141-2225) for the last keyframe pushed; params nullable: rgc_default_kf_loop_params
  LoopDetection detectLoop(const rgc_kf_loop_params* params = nullptr) {
    rgc_kf_loop_params p;
    rgc_default_kf_loop_params(&p);
    if (params) p = *params;
    LoopDetection d;
    d.history_ids.resize((std::size_t)info().n_keyframes + 1);
    int n_history = 0;
    chk(rgc_kf_detect_loop(ctx_, &p, &d.candidate, d.history_ids.data(), (int)d.history_ids.size(), &n_history));
    d.history_ids.resize((std::size_t)n_history);
    return d;
  }

  // PoseGraphOptimize4DoF (:2303-2466) over the keyframes `ids` in that order; apply: the store's poses are corrected (all or nothing);
  // corrected (nullable): the ids.size() corrected poses either way; params (nullable): Ceres' iteration cap and initial radius
  rgc_pgo_report optimizePoseGraph(const std::vector<int>& ids, const std::vector<rgc_pgo_loop>& loops, bool apply = true,
                                   std::vector<rgc_kf_pose>* corrected = nullptr, const rgc_pgo_params* params = nullptr) {
    rgc_pgo_report rep;
    if (corrected) corrected->resize(ids.size());
    chk(rgc_pgo_optimize(ctx_, ids.data(), (int)ids.size(), loops.empty() ? nullptr : loops.data(), (int)loops.size(), params, apply ? 1 : 0,
                         corrected && !ids.empty() ? corrected->data() : nullptr, &rep));
    return rep;
  }

  // the selection's point count before the filter (nothing runs on the device)
  int rawSize(const std::vector<int>& ids, unsigned kind_mask) {
    int n_raw = 0, n_out = 0;
    const int rc = rgc_kf_assemble(ctx_, ids.data(), (int)ids.size(), kind_mask, 0.f, nullptr, 0, 0, &n_raw, &n_out);
    if (rc != RGC_OK && n_raw == 0) chk(rc);
    return n_raw;
  }
  // n x 4 floats on the host
  std::vector<float> assemble(const std::vector<int>& ids, unsigned kind_mask, float leaf = 0.f) {
    const int cap = rawSize(ids, kind_mask);
    std::vector<float> out((std::size_t)cap * 4);
    int n_raw = 0, n_out = 0;
    chk(rgc_kf_assemble(ctx_, ids.data(), (int)ids.size(), kind_mask, leaf, cap ? out.data() : nullptr, cap, 0, &n_raw, &n_out));
    out.resize((std::size_t)n_out * 4);
    return out;
  }
  // the same cloud left on the device, for rgc_icp_align_device / rgc_mapreg_set_maps_device / rgc_set_target_device on this context
  DeviceCloud assembleDevice(const std::vector<int>& ids, unsigned kind_mask, float leaf = 0.f) {
    const int cap = rawSize(ids, kind_mask);
    void* d = nullptr;
    chk(rgc_device_alloc(ctx_, (std::size_t)(cap > 0 ? cap : 1) * 16, &d));
    int n_raw = 0, n_out = 0;
    const int rc = rgc_kf_assemble(ctx_, ids.data(), (int)ids.size(), kind_mask, leaf, (float*)d, cap, 1, &n_raw, &n_out);
    if (rc != RGC_OK) { (void)rgc_device_free(ctx_, d); chk(rc); }
    return DeviceCloud(ctx_, (float*)d, n_out, n_raw);
  }

private:
  template <class CloudPtr>
  static const float* first(const CloudPtr& c) { return c && !c->points.empty() ? &c->points[0].x : nullptr; }
  template <class CloudPtr>
  static int count(const CloudPtr& c) { return c ? (int)c->points.size() : 0; }
  void chk(int rc) {
    if (rc != RGC_OK) throw std::runtime_error(std::string("rgc_hip: ") + rgc_status_string(rc) + ": " + rgc_last_error(ctx_));
  }
  rgc_ctx* ctx_ = nullptr;
  bool own_ = false;
};

}  // namespace rgc
