// rgc_api_keyframes.hip -- host side of f5, rgc_kf_*: the mapping node's keyframe store with batched sub-map assembly (src/RGC_mapping.cpp:1503-1616,
// 2180-2216, 2508-2537) and its selections.  The kernels are in rgc_keyframes.hip.
#include "rgc_ctx.h"

void rgc_host_key_pose_quat(float roll, float pitch, float yaw, double q_xyzw[4]);  // rgc_host.cpp: the reference's key pose -> quaternion chain (f5)

using namespace rgcapi;

// ---- the selections: which keyframes to assemble (extractSurroundingKeyFramesAndMap :1525-1548, detectLoopClosure :2141-2225, publishGlobalMap
// :2493-2505).  One gate launch over the device mirror of the key positions, then UniformSampling's chain or a 64-bit minimum. ----
static int kf_mirror(rgc_ctx* c) {   // the mirror holds the store's current revision on return
  const size_t n = c->kfs.recs.size();
  if (c->kfs.mirror_rev == c->kfs.rev && c->kfs.pos.p) return RGC_OK;
  int rc;
  if ((rc = ensure(c, c->kfs.pos, 16 * n)) || (rc = ensure(c, c->kfs.travel, 4 * n)) || (rc = ensure(c, c->kfs.ids, 4 * n))) return rc;
  std::vector<float> hp(4 * n), ht(n);
  std::vector<int> hi(n);
  for (size_t p = 0; p < n; p++) {
    const KeyframeRecord::KfRec& r = c->kfs.recs[p];
    const int pi = (int)p;
    hp[4 * p] = r.pose.x; hp[4 * p + 1] = r.pose.y; hp[4 * p + 2] = r.pose.z;
    memcpy(&hp[4 * p + 3], &pi, 4);   // the position's bits: the fourth float is only ever copied
    ht[p] = r.travel;
    hi[p] = r.id;
  }
  HIPCHK(c, hipMemcpyAsync(c->kfs.pos.p, hp.data(), 16 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->kfs.travel.p, ht.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->kfs.ids.p, hi.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->kfs.mirror_rev = c->kfs.rev;
  return RGC_OK;
}
// the gate of every selection: r2 = (float)((double)radius * (double)radius), inside when dist2 < r2 (strict)
static float kf_gate_r2(float radius) { return (float)((double)radius * (double)radius); }
// gate launch over the mirror; small4 <- {number inside, 0, the loop search's minimum (two words)}.  flags: the in-radius flags are kept for a compaction
static int kf_run_gate(rgc_ctx* c, const float q[3], float r2, int loop, float travel_last, float thr, int min_id, bool flags, unsigned small4[4]) {
  const int n = (int)c->kfs.recs.size();
  int rc;
  if ((rc = ensure(c, c->kfs.small, 16))) return rc;
  if (flags && (rc = ensure(c, c->kfs.flag, 4 * (size_t)n))) return rc;
  const unsigned init[4] = {0u, 0u, ~0u, ~0u};
  HIPCHK(c, hipMemcpyAsync(c->kfs.small.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  rgck::kf_gate(c->stream, c->kfs.pos.as<const float4>(), c->kfs.travel.as<const float>(), c->kfs.ids.as<const int>(), n, q, r2, loop, travel_last, thr, min_id,
                flags ? c->kfs.flag.as<int>() : nullptr, c->kfs.small.as<unsigned>());
  HIPCHK(c, hipMemcpyAsync(small4, c->kfs.small.p, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}
// UniformSampling of m device points {x, y, z, position} at leaf `density`; the winners' ids in ascending leaf index
static int kf_sample_ids(rgc_ctx* c, const float* d_pts, int m, float density, int* out_ids, int cap, int* n_out, const char* who) {
  int rc;
  if ((rc = ensure(c, c->kfs.sel_out, 16 * (size_t)m))) return rc;
  int no = 0;
  if ((rc = voxelgrid_routed(c, d_pts, m, 16, density, c->kfs.sel_out.as<float>(), &no, 1, rgck::kVgModePick))) return rc;
  *n_out = no;
  if (no > cap) return fail(c, RGC_ERR_INVALID, "%s: %d keyframes selected, room for %d", who, no, cap);
  std::vector<float> h(4 * (size_t)no);
  if (no) HIPCHK(c, hipMemcpyAsync(h.data(), c->kfs.sel_out.p, 16 * (size_t)no, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < no; j++) {
    int p;
    memcpy(&p, &h[4 * (size_t)j + 3], 4);
    if (p < 0 || p >= (int)c->kfs.recs.size()) return fail(c, RGC_ERR_HIP, "%s: the sampling returned position %d of %d", who, p, (int)c->kfs.recs.size());
    out_ids[j] = c->kfs.recs[p].id;
  }
  return RGC_OK;
}

extern "C" {

static bool kf_pose_finite(const rgc_kf_pose& p) {
  return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::isfinite(p.roll) && std::isfinite(p.pitch) && std::isfinite(p.yaw);
}

int rgc_kf_reset(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (!c->kfs.recs.empty()) c->kfs.rev++;
  c->kfs.recs.clear();
  c->kfs.index.clear();
  for (int k = 0; k < RGC_KF_KINDS; k++) c->kfs.n[k] = 0;
  return RGC_OK;
}

int rgc_kf_push(rgc_ctx* c, int id, const rgc_kf_pose* pose, const float* corner, int n_corner, const float* surf, int n_surf, const float* scan,
                int n_scan, int stride_bytes, int on_device) {
  if (!c || !pose || n_corner < 0 || n_surf < 0 || n_scan < 0) return RGC_ERR_INVALID;
  if ((n_corner && !corner) || (n_surf && !surf) || (n_scan && !scan)) return fail(c, RGC_ERR_INVALID, "rgc_kf_push: a cloud with points and no pointer");
  if (!stride4_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "a keyframe point is x,y,z,c: stride_bytes >= 16");
  if (!kf_pose_finite(*pose)) return fail(c, RGC_ERR_NONFINITE, "rgc_kf_push: the key pose is not finite");
  if (c->kfs.index.count(id)) return fail(c, RGC_ERR_INVALID, "rgc_kf_push: keyframe %d is in the store already", id);
  const float* src[RGC_KF_KINDS] = {corner, surf, scan};
  const int n[RGC_KF_KINDS] = {n_corner, n_surf, n_scan};
  for (int k = 0; k < RGC_KF_KINDS; k++)
    if ((unsigned long long)c->kfs.n[k] + (unsigned long long)n[k] > (1ull << 27)) return fail(c, RGC_ERR_INVALID, "the keyframe store would exceed 2^27 points of kind %d", k);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  for (int k = 0; k < RGC_KF_KINDS; k++) {
    if (!n[k]) continue;
    if (on_device && (rc = check_device_range(c, src[k], record_bytes(n[k], stride_bytes, true), "rgc_kf_push: cloud"))) return rc;
    if ((rc = grow_store(c, c->kfs.store[k], c->kfs.n[k], c->kfs.n[k] + n[k], true))) return rc;
  }
  KeyframeRecord::KfRec rec{};
  rec.id = id;
  rec.pose = *pose;
  rgc_host_key_pose_quat(pose->roll, pose->pitch, pose->yaw, rec.q);
  // travel_distance / travel_angle (:1887-1908), fp32, against the pose stored NOW for the previous position (cloudKeyPoses6D->back(), corrected or
  // not); never recomputed afterwards
  if (!c->kfs.recs.empty()) {
    const KeyframeRecord::KfRec& last = c->kfs.recs.back();
    const float dx = pose->x - last.pose.x, dy = pose->y - last.pose.y, dz = pose->z - last.pose.z;
    rec.travel = last.travel + sqrtf((dx * dx + dy * dy) + dz * dz);
    float rad_delta = pose->yaw - last.pose.yaw;
    if (rad_delta > M_PI) rad_delta = rad_delta - M_PI * 2;    // (float op double: in double, stored as float, :1904-1905)
    if (rad_delta < -M_PI) rad_delta = rad_delta + M_PI * 2;
    rec.travel_angle = last.travel_angle + fabsf(rad_delta);
  }
  bool copied = false;
  for (int k = 0; k < RGC_KF_KINDS; k++) {
    rec.off[k] = c->kfs.n[k];
    rec.n[k] = n[k];
    if (!n[k]) continue;
    char* dst = c->kfs.store[k].as<char>() + c->kfs.n[k] * 16;
    const hipMemcpyKind dir = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (stride_bytes == 16) HIPCHK(c, hipMemcpyAsync(dst, src[k], (size_t)n[k] * 16, dir, c->stream));
    else HIPCHK(c, hipMemcpy2DAsync(dst, 16, src[k], (size_t)stride_bytes, 16, (size_t)n[k], dir, c->stream));
    copied = true;
  }
  if (copied && !on_device) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's host buffers are the caller's again on return
  for (int k = 0; k < RGC_KF_KINDS; k++) c->kfs.n[k] += n[k];
  c->kfs.index[id] = (int)c->kfs.recs.size();
  c->kfs.recs.push_back(rec);
  c->kfs.rev++;
  return RGC_OK;
}

int rgc_kf_set_poses(rgc_ctx* c, const int* ids, const rgc_kf_pose* poses, int n) {
  if (!c || n < 0 || (n && (!ids || !poses))) return RGC_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!c->kfs.index.count(ids[i])) return fail(c, RGC_ERR_INVALID, "rgc_kf_set_poses: keyframe %d is not in the store", ids[i]);
    if (!kf_pose_finite(poses[i])) return fail(c, RGC_ERR_NONFINITE, "rgc_kf_set_poses: the pose of keyframe %d is not finite", ids[i]);
  }
  for (int i = 0; i < n; i++) {
    KeyframeRecord::KfRec& r = c->kfs.recs[c->kfs.index[ids[i]]];
    r.pose = poses[i];
    rgc_host_key_pose_quat(poses[i].roll, poses[i].pitch, poses[i].yaw, r.q);
  }
  if (n) c->kfs.rev++;
  return RGC_OK;
}

int rgc_kf_get_info(rgc_ctx* c, rgc_kf_info* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  out->n_keyframes = (int)c->kfs.recs.size();
  for (int k = 0; k < RGC_KF_KINDS; k++) out->n_points[k] = (long long)c->kfs.n[k];
  out->revision = c->kfs.rev;
  return RGC_OK;
}

int rgc_kf_get_travel(rgc_ctx* c, const int* ids, int n, float* distance, float* angle) {
  if (!c || n < 0 || (n && !ids)) return RGC_ERR_INVALID;
  for (int i = 0; i < n; i++)
    if (!c->kfs.index.count(ids[i])) return fail(c, RGC_ERR_INVALID, "rgc_kf_get_travel: keyframe %d is not in the store", ids[i]);
  for (int i = 0; i < n; i++) {
    const KeyframeRecord::KfRec& r = c->kfs.recs[c->kfs.index[ids[i]]];
    if (distance) distance[i] = r.travel;
    if (angle) angle[i] = r.travel_angle;
  }
  return RGC_OK;
}

int rgc_kf_select_surrounding(rgc_ctx* c, const float center[3], float radius, float density, int* out_ids, int cap, int* n_in_radius, int* n_out) {
  if (!c || !center || !n_in_radius || !n_out || cap < 0 || (cap && !out_ids)) return RGC_ERR_INVALID;
  *n_in_radius = *n_out = 0;
  if (!std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2]) || !std::isfinite(radius) || !std::isfinite(density) || !(radius > 0.f) ||
      !(density > 0.f))
    return fail(c, RGC_ERR_INVALID, "rgc_kf_select_surrounding: the centre, radius > 0 and density > 0 must be finite");
  const int n = (int)c->kfs.recs.size();
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = kf_mirror(c))) return rc;
  unsigned small4[4];
  if ((rc = kf_run_gate(c, center, kf_gate_r2(radius), 0, 0.f, 0.f, 0, true, small4))) return rc;
  const int m = (int)small4[0];
  *n_in_radius = m;
  if (m == 0) { c->vg.route = rgc_vg_route{}; return RGC_OK; }
  if ((rc = ensure(c, c->kfs.scan, 4 * (size_t)n)) || (rc = ensure(c, c->kfs.bsum, 4 * ((size_t)n / 2048 + 2))) || (rc = ensure(c, c->kfs.sel, 16 * (size_t)m))) return rc;
  rgck::exclusive_scan(c->stream, c->kfs.flag.as<const int>(), c->kfs.scan.as<int>(), n, c->kfs.bsum.as<int>());
  rgck::kf_compact(c->stream, c->kfs.pos.as<const float4>(), c->kfs.flag.as<const int>(), c->kfs.scan.as<const int>(), n, c->kfs.sel.as<float4>());
  HIPCHK(c, hipGetLastError());
  return kf_sample_ids(c, c->kfs.sel.as<const float>(), m, density, out_ids, cap, n_out, "rgc_kf_select_surrounding");
}

int rgc_kf_select_global(rgc_ctx* c, float pose_density, int* out_ids, int cap, int* n_out) {
  if (!c || !n_out || cap < 0 || (cap && !out_ids)) return RGC_ERR_INVALID;
  *n_out = 0;
  if (!std::isfinite(pose_density) || !(pose_density > 0.f)) return fail(c, RGC_ERR_INVALID, "rgc_kf_select_global: the density must be finite and > 0");
  const int n = (int)c->kfs.recs.size();
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = kf_mirror(c))) return rc;
  return kf_sample_ids(c, c->kfs.pos.as<const float>(), n, pose_density, out_ids, cap, n_out, "rgc_kf_select_global");
}

void rgc_default_kf_loop_params(rgc_kf_loop_params* p) {
  if (!p) return;
  p->history_search_radius = 5.0f;    // historyKeyframeSearchRadius, :155
  p->drift_factor = 0.02f;            // DRIFT_FACTOR, :159
  p->distance_by_loop = 0.0f;         // DistanceByLoop, :158 (the caller's state, :2130-2135)
  p->loop_keyframe_dis_diff = 20.0f;  // loopKeyframeDisDiff, :160
  p->history_search_num = 50;         // historyKeyframeSearchNum, :157
  p->min_key_id = 10;                 // :2166
}

int rgc_kf_detect_loop(rgc_ctx* c, const rgc_kf_loop_params* prm, rgc_kf_loop_candidate* out, int* history_ids, int cap, int* n_history) {
  if (!c || !prm || !out || !n_history || cap < 0 || (cap && !history_ids)) return RGC_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->latest_id = out->closest_id = -1;
  *n_history = 0;
  if (!std::isfinite(prm->history_search_radius) || !std::isfinite(prm->drift_factor) || !std::isfinite(prm->distance_by_loop) ||
      !std::isfinite(prm->loop_keyframe_dis_diff) || prm->history_search_num < 0)
    return fail(c, RGC_ERR_INVALID, "rgc_kf_detect_loop: the parameters must be finite, history_search_num >= 0");
  const int n = (int)c->kfs.recs.size();
  if (n == 0) return RGC_OK;
  const int L = n - 1;
  const KeyframeRecord::KfRec& last = c->kfs.recs[L];
  // poseGraphSearchRadius (:2148) in fp32; the search takes its square, the travel threshold its signed value (:2164)
  const float R = prm->history_search_radius + (last.travel - prm->distance_by_loop) * prm->drift_factor;
  const float thr = prm->loop_keyframe_dis_diff + R;
  if (!std::isfinite(R) || !std::isfinite(thr)) return fail(c, RGC_ERR_INVALID, "rgc_kf_detect_loop: the search radius is not finite");
  out->latest_id = last.id;
  out->latest_pose = last.pose;
  out->search_radius = R;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = kf_mirror(c))) return rc;
  const float q[3] = {last.pose.x, last.pose.y, last.pose.z};
  unsigned small4[4];
  if ((rc = kf_run_gate(c, q, kf_gate_r2(R), 1, last.travel, thr, prm->min_key_id, false, small4))) return rc;
  out->n_in_radius = (int)small4[0];
  if (small4[2] == ~0u && small4[3] == ~0u) return RGC_OK;   // nothing qualifies
  const int pc = (int)small4[2];                                // (little endian: the low word is the position)
  if (pc < 0 || pc >= n) return fail(c, RGC_ERR_HIP, "rgc_kf_detect_loop: the search returned position %d of %d", pc, n);
  const KeyframeRecord::KfRec& cl = c->kfs.recs[pc];
  out->closest_id = cl.id;
  out->closest_pose = cl.pose;
  if (cl.id == last.id) return RGC_OK;
  // the history window (:2195-2216): positions either side of the closest one, before the latest, ids in [0, latest id)
  int nh = 0;
  long long pts = 0;
  for (int pass = 0; pass < 2; pass++) {
    nh = 0;
    for (long long i = -(long long)prm->history_search_num; i <= (long long)prm->history_search_num; i++) {
      const long long p = (long long)pc + i;
      if (p < 0 || p >= L) continue;
      const KeyframeRecord::KfRec& r = c->kfs.recs[(size_t)p];
      if (r.id < 0 || r.id >= last.id) continue;
      if (pass == 0) pts += (long long)r.n[0] + (long long)r.n[1];
      else history_ids[nh] = r.id;
      nh++;
    }
    if (pass == 0) {
      *n_history = nh;
      if (nh > cap) return fail(c, RGC_ERR_INVALID, "rgc_kf_detect_loop: %d history keyframes, room for %d", nh, cap);
    }
  }
  out->found = pts > 0 ? 1 : 0;    // an empty nearHistoryKeyFrameCloud: no loop (:2218)
  return RGC_OK;
}

int rgc_kf_assemble(rgc_ctx* c, const int* ids, int n_ids, unsigned kind_mask, float leaf, float* out_xyzc, int cap, int on_device, int* n_raw,
                    int* n_out) {
  if (!c || !n_raw || !n_out || n_ids < 0 || cap < 0 || (n_ids && !ids) || (cap && !out_xyzc)) return RGC_ERR_INVALID;
  *n_raw = *n_out = 0;
  if (kind_mask == 0 || kind_mask >= (1u << RGC_KF_KINDS)) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: kind_mask must name one to three of the kinds (1..7)");
  if (!std::isfinite(leaf)) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: the leaf size is not finite");
  if (on_device && (((uintptr_t)out_xyzc) & 15)) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: a device output must be 16-byte aligned");
  // the selection: one segment per (id, kind) that holds points, in the order given and in ascending kind order; counts first, nothing is touched
  unsigned long long total = 0, blocks = 0;
  size_t nseg = 0;
  for (int i = 0; i < n_ids; i++) {
    const auto it = c->kfs.index.find(ids[i]);
    if (it == c->kfs.index.end()) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: keyframe %d is not in the store", ids[i]);
    const KeyframeRecord::KfRec& r = c->kfs.recs[it->second];
    for (int k = 0; k < RGC_KF_KINDS; k++)
      if (((kind_mask >> k) & 1u) && r.n[k]) {
        total += (unsigned long long)r.n[k];
        blocks += ((unsigned long long)r.n[k] + rgck::kKfBlock - 1) / rgck::kKfBlock;
        nseg++;
      }
  }
  if (total > (1ull << 27)) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: the selection has %llu points, the limit is 2^27", total);
  const int nr = (int)total;
  *n_raw = nr;
  const bool filter = leaf > 0.f;
  if (!filter) {
    *n_out = nr;
    if (nr > cap) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: %d points, room for %d", nr, cap);
  }
  if (nr == 0) {
    if (filter) c->vg.route = rgc_vg_route{};
    return RGC_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int rc;
  if (on_device && (rc = check_device_range(c, out_xyzc, (size_t)std::min(cap, nr) * 16, "rgc_kf_assemble: out_xyzc"))) return rc;
  // where the concatenation is written: the caller's device buffer when it is the result, else a buffer of the store (the leaf filter's input,
  // or the staging of a host result)
  float4* d_raw = (float4*)out_xyzc;
  if (filter || !on_device) {
    if ((rc = ensure(c, c->kfs.raw, (size_t)nr * 16))) return rc;
    d_raw = c->kfs.raw.as<float4>();
  }
  // the segment table through pinned staging: [nseg segments][nseg + 1 first workgroups]
  const size_t seg_bytes = nseg * sizeof(rgck::KfSegment), tab_bytes = seg_bytes + (nseg + 1) * sizeof(int);
  if (c->kfs.upload_pending) { HIPCHK(c, hipEventSynchronize(c->kfs.uploaded)); c->kfs.upload_pending = false; }
  if ((rc = ensure_pinned(c, c->kfs.h_table, tab_bytes, tab_bytes + tab_bytes / 2 + 4096))) return rc;
  if ((rc = ensure(c, c->kfs.table, tab_bytes))) return rc;
  rgck::KfSegment* hs = (rgck::KfSegment*)c->kfs.h_table.p;
  int* hb = (int*)(c->kfs.h_table.p + seg_bytes);
  size_t si = 0;
  int out0 = 0, b0 = 0;
  for (int i = 0; i < n_ids; i++) {
    const KeyframeRecord::KfRec& r = c->kfs.recs[c->kfs.index.find(ids[i])->second];
    for (int k = 0; k < RGC_KF_KINDS; k++) {
      if (!((kind_mask >> k) & 1u) || !r.n[k]) continue;
      rgck::KfSegment& S = hs[si];
      S.src = c->kfs.store[k].as<const float4>() + r.off[k];
      S.n = r.n[k];
      S.out0 = out0;
      S.q = rgck::Quat{r.q[0], r.q[1], r.q[2], r.q[3]};
      S.t[0] = (double)r.pose.x; S.t[1] = (double)r.pose.y; S.t[2] = (double)r.pose.z;   // Eigen::Vector3d t_temp(x, y, z), :2575
      hb[si] = b0;
      out0 += r.n[k];
      b0 += (r.n[k] + rgck::kKfBlock - 1) / rgck::kKfBlock;
      si++;
    }
  }
  hb[nseg] = b0;
  HIPCHK(c, hipMemcpyAsync(c->kfs.table.p, c->kfs.h_table.p, tab_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->kfs.uploaded, s));
  c->kfs.upload_pending = true;
  if (c->main_has_target_prep && map_prep_finished(c)) c->main_has_target_prep = false;  // it has drained
  rgck::kf_assemble(s, c->kfs.table.as<const rgck::KfSegment>(), (const int*)(c->kfs.table.as<const char>() + seg_bytes), (int)nseg, (int)blocks, d_raw);
  HIPCHK(c, hipGetLastError());
  if (!filter) {
    if (!on_device) HIPCHK(c, hipMemcpyAsync(out_xyzc, d_raw, (size_t)nr * 16, hipMemcpyDeviceToHost, s));
    // device memory: stream-ordered like rgc_transform_cloud, with the same exception (a pending map preparation, see rgc_deskew)
    if (!on_device || c->main_has_target_prep) HIPCHK(c, hipStreamSynchronize(s));
    return RGC_OK;
  }
  // downSizeFilter*.setInputCloud(assembled); filter (:1608-1614, 2530-2537): the library's leaf filter, device to device -- into the caller's
  // buffer when it has room for the unfiltered count (the filter may write that many), else into the store's own and copied once the count is known
  const bool direct = on_device && cap >= nr;
  float* d_f = out_xyzc;
  if (!direct) {
    if ((rc = ensure(c, c->kfs.filt, (size_t)nr * 16))) return rc;
    d_f = c->kfs.filt.as<float>();
  }
  int no = 0;
  if ((rc = voxelgrid_routed(c, (const float*)d_raw, nr, 16, leaf, d_f, &no, 1))) return rc;
  *n_out = no;
  if (direct) return RGC_OK;
  if (no > cap) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: %d points after the filter, room for %d", no, cap);
  if (no > 0) HIPCHK(c, hipMemcpyAsync(out_xyzc, d_f, (size_t)no * 16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (!on_device) HIPCHK(c, hipStreamSynchronize(s));
  return RGC_OK;
}

}  // extern "C"
