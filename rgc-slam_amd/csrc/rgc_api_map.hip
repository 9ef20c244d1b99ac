// rgc_api_map.hip -- host side of f2, rgc_map_*: the rolling local map resident on the device (replaces the keyframe deque + per-frame re-framing +
// re-upload of src/RGC_odometer.cpp:1218-1256, 985-991, 1007).
#include "rgc_ctx.h"

using namespace rgcapi;

extern "C" {

int rgc_map_reset(rgc_ctx* c, const double origin[3]) {
  if (!c) return RGC_ERR_INVALID;
  c->map.kf.clear();
  c->map.n = 0;
  c->map.dirty = true;
  c->map.ntarget = 0;
  if (c->map.bound) { c->tgt.ready = false; c->tgt.n = 0; drop_frozen(c); c->map.bound = false; }
  for (int a = 0; a < 3; a++) c->map.origin[a] = origin ? origin[a] : 0.0;
  c->map.rev++;
  return RGC_OK;
}

int rgc_map_insert(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, const double q[4], const double t[3], int on_device, int* keyframe_id) {
  if (!c || !xyzi || !q || !t || n <= 0) return RGC_ERR_INVALID;
  if (!stride4_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "a keyframe is x,y,z,intensity: stride_bytes >= 16");
  if (c->map.n + (size_t)n > ((size_t)1 << 27)) return fail(c, RGC_ERR_INVALID, "the map would exceed 2^27 points");
  HIPCHK(c, hipSetDevice(c->device));
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  if ((rc = grow_store(c, c->map.store[c->map.cur], c->map.n, c->map.n + n, true))) return rc;
  // (the other buffer -- where the first eviction or re-basing compacts to -- grows with it: a first hipMalloc of that size is 9 ms in
  // whichever frame it falls)
  if ((rc = grow_store(c, c->map.store[c->map.cur ^ 1], c->map.n, c->map.n + n, false))) return rc;
  // surroundingCloud.push_back(transformPointCloud(FullPointsLessFlat, q_w_curr, t_w_curr)) (:1237), relative to the origin
  const double tr[3] = {t[0] - c->map.origin[0], t[1] - c->map.origin[1], t[2] - c->map.origin[2]};
  rgck::transform_q(c->stream, d_in, stride_bytes / 4, n, rgck::Quat{q[0], q[1], q[2], q[3]}, tr, c->map.store[c->map.cur].as<float>() + 4 * c->map.n, 4);
  if (!on_device) HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging is re-used by the next staged call
  HIPCHK(c, hipGetLastError());
  RollingMapRecord::MapKf kf{c->map.next_id++, c->map.n, n, {t[0], t[1], t[2]}};
  c->map.kf.push_back(kf);
  c->map.n += n;
  c->map.dirty = true;
  c->map.rev++;
  if (keyframe_id) *keyframe_id = kf.id;
  return RGC_OK;
}

int rgc_map_evict(rgc_ctx* c, int max_keyframes, const double center[3], double radius, int* n_evicted) {
  if (!c) return RGC_ERR_INVALID;
  if (n_evicted) *n_evicted = 0;
  std::vector<RollingMapRecord::MapKf> keep;
  for (const auto& k : c->map.kf) {
    bool far = false;
    if (center && radius > 0 && &k != &c->map.kf.back()) {  // the newest keyframe always stays: an empty map cannot be committed
      const double dx = k.t[0] - center[0], dy = k.t[1] - center[1], dz = k.t[2] - center[2];
      far = std::sqrt(dx * dx + dy * dy + dz * dz) > radius;
    }
    if (!far) keep.push_back(k);
  }
  if (max_keyframes > 0 && (int)keep.size() > max_keyframes) keep.erase(keep.begin(), keep.end() - max_keyframes);  // pop_front, :1242-1247
  const int gone = (int)c->map.kf.size() - (int)keep.size();
  if (!gone) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  size_t total = 0;
  for (const auto& k : keep) total += k.n;
  const int other = c->map.cur ^ 1;
  int rc = grow_store(c, c->map.store[other], c->map.n, std::max(total, (size_t)1), false);
  if (rc) return rc;
  size_t off = 0;
  for (size_t i = 0; i < keep.size();) {  // runs of surviving neighbours move with one copy
    size_t j = i, run = 0;
    const size_t base = keep[i].off;
    while (j < keep.size() && keep[j].off == base + run) { run += keep[j].n; j++; }
    HIPCHK(c, hipMemcpyAsync(c->map.store[other].as<char>() + off * 16, c->map.store[c->map.cur].as<const char>() + base * 16, run * 16,
                             hipMemcpyDeviceToDevice, c->stream));
    for (size_t k = i; k < j; k++) keep[k].off = off + (keep[k].off - base);
    off += run;
    i = j;
  }
  c->map.cur = other;
  c->map.kf.swap(keep);
  c->map.n = total;
  c->map.dirty = true;
  c->map.rev++;
  if (n_evicted) *n_evicted = gone;
  return RGC_OK;
}

int rgc_map_rebase(rgc_ctx* c, const double new_origin[3]) {
  if (!c || !new_origin) return RGC_ERR_INVALID;
  const double d[3] = {c->map.origin[0] - new_origin[0], c->map.origin[1] - new_origin[1], c->map.origin[2] - new_origin[2]};
  if (c->map.n) {
    HIPCHK(c, hipSetDevice(c->device));
    const int other = c->map.cur ^ 1;
    int rc = grow_store(c, c->map.store[other], c->map.n, c->map.n, false);
    if (rc) return rc;
    rgck::transform_q(c->stream, c->map.store[c->map.cur].as<const float>(), 4, (int)c->map.n, rgck::Quat{0, 0, 0, 1}, d, c->map.store[other].as<float>(), 4);
    HIPCHK(c, hipGetLastError());
    c->map.cur = other;
  }
  for (int a = 0; a < 3; a++) c->map.origin[a] = new_origin[a];
  c->map.dirty = true;
  c->map.rev++;
  if (c->map.bound) {  // the committed target is in the OLD origin's coordinates: an align before the next rgc_map_commit must fail, not drift
    c->tgt.ready = false;
    drop_frozen(c);
  }
  return RGC_OK;
}

int rgc_map_commit(rgc_ctx* c, float leaf, int* n_target) {
  if (!c || !(leaf > 0.f)) return RGC_ERR_INVALID;
  if (c->map.bound && !c->map.dirty && leaf == c->map.leaf && c->tgt.ready) {  // nothing changed: the resident target stands
    if (n_target) *n_target = c->map.ntarget;
    return RGC_OK;
  }
  // (before anything is written: the filter below writes the buffer the resident target was set from -- a commit refused behind it would
  // leave a set target whose input has been overwritten, and rgc_map_download(1) returning another cloud; tests/fuzz/fuzz_api.py)
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->map.n) return fail(c, RGC_ERR_NO_INPUT, "the map holds no keyframe");
  int rc = ensure(c, c->map.target, c->map.n * 16);
  if (rc) return rc;
  int nt = 0;
  // downSizeFilter2.setInputCloud(laserCloudsubmap); filter (:985-991) -- on the resident store, nothing crosses PCIe
  if (c->map.bound) {  // from here on the buffer no longer holds the cloud the bound target was set from: whatever fails below, that target goes
    c->map.bound = false;
    c->tgt.ready = false; c->tgt.n = 0; drop_frozen(c);
  }
  if ((rc = rgc_voxelgrid(c, c->map.store[c->map.cur].as<const float>(), (int)c->map.n, 16, leaf, c->map.target.as<float>(), &nt, 1))) return rc;
  // setInputTarget (:1007): grid, exact-kNN covariances, Gaussian voxel map
  if ((rc = set_cloud(c, c->tgt, true, c->map.target.as<const float>(), nt, 16, true))) return rc;
  c->map.bound = true;
  c->map.dirty = false;
  c->map.leaf = leaf;
  c->map.ntarget = nt;
  if (n_target) *n_target = nt;
  return RGC_OK;
}

int rgc_map_get_info(rgc_ctx* c, rgc_map_info* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  out->n_keyframes = (int)c->map.kf.size();
  out->n_points = (long long)c->map.n;
  out->n_target = c->map.bound && !c->map.dirty ? c->map.ntarget : -1;
  out->revision = c->map.rev;
  out->oldest_id = c->map.kf.empty() ? -1 : c->map.kf.front().id;
  out->newest_id = c->map.kf.empty() ? -1 : c->map.kf.back().id;
  for (int a = 0; a < 3; a++) out->origin[a] = c->map.origin[a];
  return RGC_OK;
}

int rgc_map_download(rgc_ctx* c, int which, float* out_xyzi, int cap, int* n) {
  if (!c || !n || cap < 0 || (cap && !out_xyzi)) return RGC_ERR_INVALID;
  const void* src = nullptr;
  int have = 0;
  if (which == 0) { src = c->map.store[c->map.cur].p; have = (int)c->map.n; }
  else if (which == 1) {
    if (!c->map.bound || c->map.dirty) return fail(c, RGC_ERR_NO_INPUT, "rgc_map_commit first");
    src = c->map.target.p; have = c->map.ntarget;
  } else return RGC_ERR_INVALID;
  *n = have;
  const int m = std::min(have, cap);
  if (m > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out_xyzi, src, (size_t)m * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return RGC_OK;
}
}  // extern "C"
