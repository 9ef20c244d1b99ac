// rgc_api_pre.hip -- host side of the stages around the registration: B2 de-skew, B3 leaf filter, B9 re-framing (rgc_deskew,
// rgc_transform_cloud, rgc_set_target_reframed, rgc_align_end_reframe, rgc_voxelgrid*, rgc_uniform_sampling) and the staging of a host
// caller's cloud (stage_in).  The kernels are in rgc_pre.hip.
#include "rgc_ctx.h"

using namespace rgcapi;

// ---- B2 / B3 / B9: the stages either side of the operator in the odometer's frame body ----
int rgcapi::stage_in(rgc_ctx* c, const float* p, int n, int stride_bytes, int on_device, const float** d_in) {
  if (n > (1 << 27)) return fail(c, RGC_ERR_INVALID, "cloud has %d points, the limit is 2^27", n);  // (every entry point that takes a cloud: one limit)
  if (on_device) {
    if (n > 0) { const int rk = check_device_range(c, p, record_bytes(n, stride_bytes, false), "input cloud"); if (rk) return rk; }
    *d_in = p;
    return RGC_OK;
  }
  const size_t bytes = (size_t)n * stride_bytes;
  int rc = ensure(c, c->vg.in, bytes);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->vg.in.p, p, bytes, hipMemcpyHostToDevice, c->stream));
  *d_in = c->vg.in.as<const float>();
  return RGC_OK;
}

extern "C" {

int rgc_deskew(rgc_ctx* c, float* xyzi, int n, int stride_bytes, const double q[4], const double t[3], int on_device) {
  if (!c || !xyzi || !q || !t || n < 0) return RGC_ERR_INVALID;
  if (!stride4_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "de-skew needs x,y,z,intensity: stride_bytes >= 16");
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  // q_last_curr.inverse() = conjugate / squaredNorm (Eigen), RGC_odometer.cpp:1444
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (!(n2 > 0)) return fail(c, RGC_ERR_INVALID, "zero quaternion");
  rgck::Quat qi{-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2};
  if (c->main_has_target_prep && map_prep_finished(c)) c->main_has_target_prep = false;  // it has drained
  rgck::deskew(c->stream, (float*)d_in, stride_bytes / 4, n, qi, t);
  if (!on_device) HIPCHK(c, hipMemcpyAsync(xyzi, d_in, (size_t)n * stride_bytes, hipMemcpyDeviceToHost, c->stream));
  // device memory: in place and stream-ordered, whatever reads the sweep next on the main stream is enqueued behind it -- unless a map
  // preparation is still pending there: rgc_set_source_device orders the scan's stream after a mark recorded BEFORE that preparation
  // (see prepare_cloud), which this kernel would then lie behind
  if (!on_device || c->main_has_target_prep) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

int rgc_transform_cloud(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, const double q[4], const double t[3], float* out_xyzi,
                        int on_device) {
  if (!c || !xyzi || !q || !t || !out_xyzi || n < 0) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "bad stride");
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  float* d_out = out_xyzi;
  if (!on_device) {
    if ((rc = ensure(c, c->vg.out, sizeof(float) * 4 * (size_t)n))) return rc;
    d_out = c->vg.out.as<float>();
  }
  rgck::transform_q(c->stream, d_in, stride_bytes / 4, n, rgck::Quat{q[0], q[1], q[2], q[3]}, t, d_out, 4);
  if (!on_device) HIPCHK(c, hipMemcpyAsync(out_xyzi, d_out, sizeof(float) * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  // device memory: stream-ordered like rgc_deskew; the one exception is the same as there (a pending map preparation, see rgc_deskew)
  if (!on_device || c->main_has_target_prep) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// B9 followed by setInputTarget, in one call and without a host round trip: the sub-map (device memory, fixed between calls) re-expressed
// by (q, t) into d_scratch and handed to the registration as its new target (RGC_odometer.cpp:1248-1256, 998, 1007).  The output's
// bounding box follows from the input's -- measured once per input buffer (whole 1 m cells, k_bbox) -- and the transform: its eight
// corners through q * p + t in fp64, a millimetre added for the fp32 rounding of the stored points.  rgc_set_target_device takes its grid
// from that box: no bounding-box kernel, no read-back, and no speculative-grid miss when the re-framed map's box swings with the yaw.
// the argument checks of rgc_set_target_reframed (also made by rgc_align_end_reframe BEFORE it consumes the solve)
static int reframe_args_ok(rgc_ctx* c, const float* d_xyzi, int n, int stride_bytes, const float* d_scratch) {
  if (!d_xyzi || !d_scratch || n <= 0) return fail(c, RGC_ERR_INVALID, "rgc_set_target_reframed: null buffer or no points");
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "bad stride");
  if (n > (1 << 27)) return fail(c, RGC_ERR_INVALID, "cloud has %d points, the limit is 2^27 (32-bit byte offsets into the sorted array)", n);
  if (n < min_cloud_points(c)) return fail(c, RGC_ERR_TOO_FEW_POINTS, "target cloud has %d points, need >= k = %d", n, c->prm.k_correspondences);
  // the re-framed cloud is WRITTEN to d_scratch while d_xyzi is read: they must not overlap (and one buffer has one bounding-box hint)
  const char* a0 = (const char*)d_xyzi; const char* a1 = a0 + (size_t)n * stride_bytes;
  const char* b0 = (const char*)d_scratch; const char* b1 = b0 + (size_t)n * 16;
  if (a0 < b1 && b0 < a1) return fail(c, RGC_ERR_INVALID, "rgc_set_target_reframed: d_scratch overlaps d_xyzi");
  { int rk = check_device_range(c, d_xyzi, record_bytes(n, stride_bytes, false), "rgc_set_target_reframed: d_xyzi"); if (rk) return rk; }
  { int rk = check_device_range(c, d_scratch, (size_t)n * 16, "rgc_set_target_reframed: d_scratch"); if (rk) return rk; }
  return RGC_OK;
}

int rgc_set_target_reframed(rgc_ctx* c, const float* d_xyzi, int n, int stride_bytes, const double q[4], const double t[3], float* d_scratch) {
  if (!c || !q || !t) return RGC_ERR_INVALID;
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  {
    const int rc = reframe_args_ok(c, d_xyzi, n, stride_bytes, d_scratch);
    if (rc) return rc;
  }
  // a pose that is not a pose -- the NaN a diverged solve hands on through rgc_align_end_reframe, a zero quaternion -- has no box to derive a
  // grid from (the float -> int conversions behind it are undefined: tests/fuzz/fuzz_api.py saw a 40-petabyte allocation request)
  {
    const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(std::isfinite(qq) && qq > 1.0e-12 && qq < 1.0e12 && std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]) &&
          std::fabs(t[0]) <= 1.0e8 && std::fabs(t[1]) <= 1.0e8 && std::fabs(t[2]) <= 1.0e8))
      return fail(c, RGC_ERR_NONFINITE, "rgc_set_target_reframed: the pose (q, t) is not finite");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const float* xyzi = d_xyzi;
  const float* d_in = d_xyzi;
  float* out_xyzi = d_scratch;
  const int on_device = 1;
  if (on_device && c->spec_on) {
    // the output's bounding box from the input's: measured once per input buffer (whole cells of 1 m, k_bbox), then the eight
    // corners through q * p + t in fp64, a millimetre added for the fp32 rounding of the stored points
    const rgc_ctx::BoxHint* hin = find_hint(c, xyzi, n);
    if (!hin) {
      rgck::SmallBlock* dsm = &c->d_small->hint;
      rgck::SmallBlock* hsm = &c->h_small->hint;
      const int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
      memcpy(hsm, init, sizeof(init));
      HIPCHK(c, hipMemcpyAsync(dsm, hsm, sizeof(init), hipMemcpyHostToDevice, c->stream));
      rgck::bbox(c->stream, d_in, stride_bytes / 4, n, 1.0, dsm->lo, &dsm->guard);
      HIPCHK(c, hipMemcpyAsync(hsm, dsm, offsetof(rgck::SmallBlock, nvox), hipMemcpyDeviceToHost, c->stream));  // (box and guard)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (!hsm->guard) {
        const double lo[3] = {hsm->lo[0] + 0.5, hsm->lo[1] + 0.5, hsm->lo[2] + 0.5}, hi[3] = {hsm->hi[0] + 1.5, hsm->hi[1] + 1.5, hsm->hi[2] + 1.5};
        put_hint(c, xyzi, n, lo, hi);
        hin = find_hint(c, xyzi, n);
      }
    }
    if (hin) {
      const double x = q[0], y = q[1], z = q[2], w = q[3];
      const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                           2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
      double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
      for (int k = 0; k < 8; k++) {
        const double p[3] = {(k & 1) ? hin->hi[0] : hin->lo[0], (k & 2) ? hin->hi[1] : hin->lo[1], (k & 4) ? hin->hi[2] : hin->lo[2]};
        for (int a = 0; a < 3; a++) {
          const double v = R[3 * a] * p[0] + R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2] + t[a];
          lo[a] = std::min(lo[a], v - 1.0e-3);
          hi[a] = std::max(hi[a], v + 1.0e-3);
        }
      }
      // how large the re-framed box can get as the vehicle turns: under any yaw its x / y extents stay within the horizontal diagonal of
      // the map's own box; pitch and roll of a ground vehicle tilt it by a few cells.  The cell arrays are sized for that ONCE.
      const double dxy = std::hypot(hin->hi[0] - hin->lo[0], hin->hi[1] - hin->lo[1]);
      put_hint(c, out_xyzi, n, lo, hi, dxy, (hi[2] - lo[2]) + 0.08 * dxy);
    }
  }
  // (the re-framing itself is left to the preparation: its counting pass writes d_scratch on the way, prepare_cloud)
  const rgck::Reframe rf{d_in, stride_bytes / 4, rgck::Quat{q[0], q[1], q[2], q[3]}, {t[0], t[1], t[2]}};
  HIPCHK(c, hipGetLastError());
  return set_cloud(c, c->tgt, true, d_scratch, n, 16, true, &rf);
}

int rgc_align_end_reframe(rgc_ctx* c, rgc_ctx* next, double Tw[16], const float* d_map, int n, int stride_bytes, float* d_scratch,
                          float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged, int* lm_failed) {
  if (!c || !next || !Tw) return RGC_ERR_INVALID;
  // Everything that could make the second half (the next frame's target) fail for the caller's arguments is checked BEFORE the solve is
  // consumed: a non-OK return then means "nothing happened" (the solve is still pending, Tw untouched) -- or, past this point, a HIP /
  // allocation failure inside the preparation, with the solve's outputs and Tw already valid (the message says which call failed).
  if (next != c) {
    if (!ctx_alive(next)) return fail(c, RGC_ERR_INVALID, "rgc_align_end_reframe: the next context is not alive");
    if (solve_in_flight(next)) return fail(c, RGC_ERR_INVALID, "rgc_align_end_reframe: a solve is in flight on the next context");
  }
  if (!c->pend.active && !c->gen_res.on) return fail(c, RGC_ERR_INVALID, "rgc_align_end without rgc_align_begin");
  {
    const int rc0 = reframe_args_ok(next, d_map, n, stride_bytes, d_scratch);
    if (rc0) { if (next != c) fail(c, rc0, "rgc_align_end_reframe: %s", next->err); return rc0; }
  }
  // world_T * T in fp64, rows in ascending k (the composition of :1201-1203 on matrices), and world -> body of the new pose: R^T and
  // -R^T t; the unit quaternion of R^T by Shepperd's branches (:1250-1255)
  auto compose = [](const double* Tw_in, const float* T, double* W, double* q, double* t) {
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++) {
        double v = 0.0;
        for (int k = 0; k < 4; k++) v += Tw_in[a * 4 + k] * (double)T[k * 4 + b];
        W[a * 4 + b] = v;
      }
    const double Rt[3][3] = {{W[0], W[4], W[8]}, {W[1], W[5], W[9]}, {W[2], W[6], W[10]}};
    const double tr = Rt[0][0] + Rt[1][1] + Rt[2][2];
    if (tr > 0) {
      const double s4 = 2.0 * std::sqrt(tr + 1.0);
      q[0] = (Rt[2][1] - Rt[1][2]) / s4; q[1] = (Rt[0][2] - Rt[2][0]) / s4; q[2] = (Rt[1][0] - Rt[0][1]) / s4; q[3] = 0.25 * s4;
    } else {
      const int i = (Rt[0][0] >= Rt[1][1] && Rt[0][0] >= Rt[2][2]) ? 0 : (Rt[1][1] >= Rt[2][2] ? 1 : 2);
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      const double s4 = 2.0 * std::sqrt(1.0 + Rt[i][i] - Rt[j][j] - Rt[k][k]);
      q[3] = (Rt[k][j] - Rt[j][k]) / s4;
      q[i] = 0.25 * s4;
      q[j] = (Rt[j][i] + Rt[i][j]) / s4;
      q[k] = (Rt[k][i] + Rt[i][k]) / s4;
    }
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int a = 0; a < 4; a++) q[a] /= nrm;
    const double tx = W[3], ty = W[7], tz = W[11];
    t[0] = -(Rt[0][0] * tx + Rt[0][1] * ty + Rt[0][2] * tz);
    t[1] = -(Rt[1][0] * tx + Rt[1][1] * ty + Rt[1][2] * tz);
    t[2] = -(Rt[2][0] * tx + Rt[2][1] * ty + Rt[2][2] * tz);
  };
  // The POSE of a solve whose score is chained to it arrives before the score does (LmEarly: the deciding launch posts it, then scores it,
  // ~25 us at the headline size).  On two contexts taking turns the next frame's target needs nothing else: it is enqueued on `next` while
  // this context's last launch still computes the score, whose arrival the call then waits for like rgc_align_end.  Not on one context
  // (the score reads the buffers the next preparation writes), not when a guard tripped or a lazy target missed (the solve is repeated).
  float Te[16];
  double We[16], qe[4], te[3];
  bool early_done = false;
  int rc_next = RGC_OK;
  if (next != c && RGC_EARLY_POSE && c->post_on && c->d_post && c->d_early && c->pend.active && c->pend.want_fitness && !c->lm_host && !c->gen_res.on) {
    volatile int* eg = &c->h_early->gen;
    volatile int* fg = &c->h_post->gen;
    bool early = false;
    for (unsigned spin = 0;; spin++) {
      if (*eg == c->lm_seq) { early = true; break; }
      if (*fg == c->lm_seq) break;
      if (spin & 31u) continue;
      const hipError_t qy = hipEventQuery(c->lm_tail);
      if (qy == hipSuccess) { early = *eg == c->lm_seq; break; }
      if (qy != hipErrorNotReady) break;   // (rgc_align_end below reports it)
      (void)hipGetLastError();
    }
    if (early) {
      std::atomic_thread_fence(std::memory_order_acquire);
      rgck::LmEarly E;
      memcpy(&E, c->h_early, sizeof(E));
      if (E.pad == 0 && E.pad2 == 0) {
        for (int i = 0; i < 16; i++) Te[i] = (float)E.x0[i];  // final_transformation_ = x0.cast<float>(), :77
        compose(Tw, Te, We, qe, te);
        rc_next = rgc_set_target_reframed(next, d_map, n, stride_bytes, qe, te, d_scratch);
        if (rc_next) fail(c, rc_next, "rgc_align_end_reframe: %s", next->err);
        early_done = true;
      }
    }
  }
  float T[16];
  char next_err[sizeof(c->err)];
  if (rc_next) memcpy(next_err, c->err, sizeof(next_err));
  int rc = rgc_align_end(c, T, final_H, fitness, iterations, converged, lm_failed);
  if (rc) return rc;
  if (final_T) memcpy(final_T, T, sizeof(T));
  if (early_done && memcmp(T, Te, sizeof(T)) == 0) {  // (always, unless the solve had to be repeated behind the early pose's back)
    memcpy(Tw, We, sizeof(We));
    if (rc_next) memcpy(c->err, next_err, sizeof(next_err));
    return rc_next;
  }
  double W[16], q[4], t[3];
  compose(Tw, T, W, q, t);
  memcpy(Tw, W, sizeof(W));
  rc = rgc_set_target_reframed(next, d_map, n, stride_bytes, q, t, d_scratch);
  if (rc && next != c) fail(c, rc, "rgc_align_end_reframe: %s", next->err);
  return rc;
}

}  // extern "C"

// The rows chain of the leaf filter on box g (rgc_pre.hip); one read-back: *flags (bits as rgck::vg_rows documents) and *n_out.
// h_result (nullable): the chain is only ENQUEUED -- its three result ints go to h_result (pinned), c->vg.done is recorded behind the
// copy, and the caller picks them up later (rgc_voxelgrid_begin / _end); flags / n_out are not written then.
static int voxelgrid_rows(rgc_ctx* c, const float* d_in, int stride_f, int n, float inv, const rgck::LeafGrid& g, int edge, bool dense, float* d_out,
                          int* flags, int* n_out, rgc_vg_route* rt, int* h_result = nullptr, int mode = rgck::kVgModeCentroid, float leaf = 0.f,
                          int* d_index = nullptr) {
  hipStream_t s = c->stream;
  int* const d_res = c->d_small->leaf_rows.res;        // rgck::vg_rows' res[3]; res[1], the live flag word, is the block's guard
  const int* const h_res = c->h_small->leaf_rows.res;
  Cloud& cl = c->vg.aux;
  int rc;
  // the sort's buckets: leaves for a dense cloud, whole grid rows for a sweep, and for a LARGE cloud in a box too big for leaf buckets
  // segments of a row, as many as keep the table near 4 n entries (the ranking pass is quadratic in a bucket's population: a ground-level
  // row of a 1.3 M-point keyframe store holds thousands of points)
  int seg_shift = dense ? 0 : 31;
  if (!dense) {
    const double rows = (double)g.div[1] * (double)g.div[2], nseg_max = 4.0 * (double)n / rows;
    if (nseg_max >= 2.0) {
      seg_shift = 3;
      while (seg_shift < 30 && (double)(((long long)g.div[0] + (1ll << seg_shift) - 1) >> seg_shift) > nseg_max) seg_shift++;
    }
  }
  const size_t nr1 = (size_t)g.div[1] * (size_t)g.div[2] * (size_t)rgck::vg_segments(g, seg_shift) + 1;   // buckets
  if ((rc = ensure(c, cl.cell_of, sizeof(int) * n))) return rc;                                                    // row of every point
  if ((rc = ensure(c, cl.slot_of, sizeof(int) * n))) return rc;                                                    // leaf x of every point
  if ((rc = ensure(c, c->vg.pos, sizeof(int) * n))) return rc;                                                     // arrival slot, then output number
  if ((rc = ensure(c, c->vg.order, sizeof(int) * n))) return rc;
  if ((rc = ensure(c, c->vg.tmp, sizeof(long long) * n))) return rc;
  if ((rc = ensure(c, c->vg.leaf, sizeof(long long) * n))) return rc;
  if ((rc = ensure(c, cl.cnt, sizeof(int) * nr1))) return rc;
  if ((rc = ensure(c, cl.start, sizeof(int) * nr1))) return rc;
  const size_t row_bs = sizeof(long long) * (nr1 / 2048 + 2);
  if ((rc = ensure(c, cl.block_sums, row_bs + sizeof(int) * ((size_t)n / 2048 + 2)))) return rc;
  if (cl.cnt.p != cl.cnt_seen) { cl.cnt_clean = 0; cl.cnt_seen = cl.cnt.p; }
  if (cl.cnt_clean < nr1) {  // afterwards the scan leaves the counters it consumed at zero: no fill per call
    const size_t fill = std::min(cl.cnt.cap, (sizeof(int) * nr1 + 255) & ~(size_t)255);
    HIPCHK(c, hipMemsetAsync(cl.cnt.p, 0, fill, s));
  }
  cl.cnt_clean = std::max(cl.cnt_clean, nr1);  // (what lies beyond this call's rows was not touched: the scan's and the map's filter take turns)
  if (!c->vg.flags_clean) HIPCHK(c, hipMemsetAsync(&c->d_small->leaf.guard, 0, sizeof(int), s));
  c->vg.flags_clean = false;
  const bool packed = rgck::vg_rows(s, d_in, stride_f, n, inv, g, edge, seg_shift, cl.cell_of.as<int>(), cl.slot_of.as<int>(), c->vg.pos.as<int>(), cl.cnt.as<int>(),
                                    cl.start.as<int>(), cl.block_sums.p, c->vg.tmp.as<unsigned long long>(), c->vg.order.as<int>(), c->vg.leaf.as<unsigned long long>(),
                                    (int*)(cl.block_sums.as<char>() + row_bs), d_out, d_res, mode, leaf, d_index);
  rt->chain = 1; rt->leaf_buckets = dense ? 1 : 0; rt->seg_shift = seg_shift; rt->nseg = rgck::vg_segments(g, seg_shift); rt->packed = packed ? 1 : 0;
  rt->edge = edge; rt->flags = 0;
  for (int a = 0; a < 3; a++) { rt->minb[a] = g.minb[a]; rt->div[a] = g.div[a]; }
  if (h_result) {  // (the finished chain leaves the flag word zeroed: the next chain on this stream finds it so)
    HIPCHK(c, hipMemcpyAsync(h_result, d_res, sizeof(rgck::LeafRows::res), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->vg.done, s));
    c->vg.flags_clean = true;
    return RGC_OK;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_small->leaf_rows.res, d_res, sizeof(rgck::LeafRows::res), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->vg.flags_clean = true;
  *flags = h_res[0];
  *n_out = h_res[2];
  rt->flags = h_res[0];
  return RGC_OK;
}
static bool vg_rows_fit(const rgck::LeafGrid& g, int n) {  // sparse enough for the sort over rows (else: over the leaves)
  const double ncell = (double)g.div[0] * (double)g.div[1] * (double)g.div[2], nrows = (double)g.div[1] * (double)g.div[2];
  return ncell <= 2147483647.0 && ncell > 64.0 * (double)n && nrows <= 64.0e6;
}

// rt: what rgc_voxelgrid_route reports, filled as the call goes (voxelgrid_routed adds status and n_out)
static int voxelgrid_run(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, float leaf, float* out_xyzi, int* n_out, int on_device, rgc_vg_route& rt,
                         int mode, int* out_index) {
  hipStream_t s = c->stream;
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  const int stride_f = stride_bytes / 4;
  const float inv = 1.0f / leaf;  // inverse_leaf_size_
  rgck::SmallBlock* dsm = &c->d_small->leaf;
  rgck::SmallBlock* hsm = &c->h_small->leaf;
  float* d_out = out_xyzi;
  if (!on_device) {
    if ((rc = ensure(c, c->vg.out, sizeof(float) * 4 * (size_t)n))) return rc;
    d_out = c->vg.out.as<float>();
  }
  // UniformSampling (mode = kVgModePick): the winners' input indices beside the points, staged like them for a host caller
  int* d_index = mode == rgck::kVgModePick ? out_index : nullptr;
  if (d_index && !on_device) {
    if ((rc = ensure(c, c->vg.us_index, sizeof(int) * (size_t)n))) return rc;
    d_index = c->vg.us_index.as<int>();
  }
  // leaves added on every side of a measured box when the next cloud of this leaf size is filtered on it: 32 for a sweep (its rows are
  // what is counted and scanned), 8 for a dense cloud (its leaves are: a wider box is a longer scan)
  constexpr int kPadSparse = 32, kPadDense = 8;
  auto padded = [](const rgck::LeafGrid& g, int pad) {
    rgck::LeafGrid p = g;
    for (int a = 0; a < 3; a++) { p.minb[a] -= pad; p.div[a] += 2 * pad; }
    return p;
  };
  LeafFilterRecord::VgBox* box = nullptr;
  for (auto& b : c->vg.box) if (b.leaf == leaf) box = &b;
  bool done = false;
  rt.kept_box = !box ? 0 : box->valid ? 2 : 3;
  if (box && box->valid) {
    // the box of an earlier cloud: no bounding-box pass, no read-back before the filter (the frames of a sequence span the same volume)
    const rgck::LeafGrid ps = padded(box->g, kPadSparse), pd = padded(box->g, kPadDense);
    const bool sparse = vg_rows_fit(ps, n);
    const double dcell = (double)pd.div[0] * (double)pd.div[1] * (double)pd.div[2];
    if (sparse || dcell <= (double)c->prm.max_cells) {
      int flags = 0, no = 0;
      rt.kept_box = 1;
      rt.path = RGC_VG_PATH_KEPT;
      if ((rc = voxelgrid_rows(c, d_in, stride_f, n, inv, sparse ? ps : pd, (sparse ? kPadSparse : kPadDense) / 2, !sparse, d_out, &flags, &no, &rt, nullptr, mode, leaf, d_index))) return rc;
      rt.kept_flags = flags;
      if (flags & 1) return fail(c, RGC_ERR_NONFINITE, "cloud contains non-finite coordinates (PCL skips them; remove NaNs first)");
      if (flags & 6) { box->valid = false; rt.box_invalidated = 1; }  // outside: measure and repeat now; near a face: measure at the next call
      if (!(flags & 2)) { *n_out = no; done = true; hint_from_leaf_grid(c, out_xyzi, no, sparse ? ps : pd, leaf); }
    }
  }
  if (!done) {
    rt.repeated = rt.path == RGC_VG_PATH_KEPT ? 1 : 0;
    rt.path = RGC_VG_PATH_MEASURED;
    rt.chain = rt.leaf_buckets = rt.seg_shift = rt.nseg = rt.packed = rt.edge = rt.flags = 0;  // (of the chain on the kept box)
    int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
    memcpy(hsm, init, sizeof(init));
    c->vg.flags_clean = false;
    HIPCHK(c, hipMemcpyAsync(dsm, hsm, sizeof(init), hipMemcpyHostToDevice, s));
    rgck::vg_bbox(s, d_in, stride_f, n, inv, dsm->lo, &dsm->guard);
    HIPCHK(c, hipMemcpyAsync(hsm, dsm, offsetof(rgck::SmallBlock, nvox), hipMemcpyDeviceToHost, s));  // (box and guard)
    HIPCHK(c, hipStreamSynchronize(s));
    if (hsm->guard) return fail(c, RGC_ERR_NONFINITE, "cloud contains non-finite coordinates (PCL skips them; remove NaNs first)");
    c->vg.flags_clean = true;
    rgck::LeafGrid g{};
    double ncell = 1.0;
    for (int a = 0; a < 3; a++) { g.minb[a] = hsm->lo[a]; g.div[a] = hsm->hi[a] - hsm->lo[a] + 1; ncell *= (double)g.div[a]; }
    for (int a = 0; a < 3; a++) { rt.minb[a] = g.minb[a]; rt.div[a] = g.div[a]; }
    {  // keep the measured box for the next cloud of this leaf size
      if (!box) { box = &c->vg.box[c->vg.box_next]; c->vg.box_next = (c->vg.box_next + 1) % 4; box->leaf = leaf; }
      bool ok = ncell <= 2.0e9;
      for (int a = 0; a < 3; a++) if (g.minb[a] < -1000000000 || g.div[a] > 1000000000) ok = false;
      box->g = g;
      box->valid = ok;
    }
    if (ncell > 2147483647.0) {
      // PCL: "Leaf size is too small for the input dataset. Integer indices would overflow." -> output = input
      rt.path = RGC_VG_PATH_UNFILTERED;
      if (mode == rgck::kVgModePick) rgck::us_copy(s, d_in, stride_f, n, d_out, d_index);
      else rgck::transform_q(s, d_in, stride_f, n, rgck::Quat{0, 0, 0, 1}, (const double[3]){0, 0, 0}, d_out, 4);
      *n_out = n;
      HIPCHK(c, hipStreamSynchronize(s));
    } else if (vg_rows_fit(g, n)) {
      int flags = 0;
      if ((rc = voxelgrid_rows(c, d_in, stride_f, n, inv, g, 0, false, d_out, &flags, n_out, &rt, nullptr, mode, leaf, d_index))) return rc;
      hint_from_leaf_grid(c, out_xyzi, *n_out, g, leaf);
    } else {
      // a dense cloud: the same chain with the leaves themselves as the sort's buckets
      if (ncell > (double)c->prm.max_cells) return fail(c, RGC_ERR_GRID_TOO_LARGE, "leaf grid %d x %d x %d exceeds max_cells", g.div[0], g.div[1], g.div[2]);
      int flags = 0;
      if ((rc = voxelgrid_rows(c, d_in, stride_f, n, inv, g, 0, true, d_out, &flags, n_out, &rt, nullptr, mode, leaf, d_index))) return rc;
      hint_from_leaf_grid(c, out_xyzi, *n_out, g, leaf);
    }
  }
  if (!on_device) {
    HIPCHK(c, hipMemcpyAsync(out_xyzi, d_out, sizeof(float) * 4 * (size_t)*n_out, hipMemcpyDeviceToHost, s));
    if (d_index) HIPCHK(c, hipMemcpyAsync(out_index, d_index, sizeof(int) * (size_t)*n_out, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

int rgcapi::voxelgrid_routed(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, float leaf, float* out_xyzi, int* n_out, int on_device, int mode,
                             int* out_index, int rc) {
  rgc_vg_route rt{};
  rt.n = n;
  auto run = [&]() -> int { HIPCHK(c, hipSetDevice(c->device)); return voxelgrid_run(c, xyzi, n, stride_bytes, leaf, out_xyzi, n_out, on_device, rt, mode, out_index); };
  if (n > 0 && !rc) rc = run();
  rt.status = rc;
  rt.n_out = *n_out;
  c->vg.route = rt;
  return rc;
}

extern "C" {

int rgc_voxelgrid(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, float leaf, float* out_xyzi, int* n_out, int on_device) {
  if (!c || !xyzi || !out_xyzi || !n_out || n < 0) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes) || !(leaf > 0.f) || !std::isfinite(leaf)) return fail(c, RGC_ERR_INVALID, "bad stride or leaf size");
  *n_out = 0;
  return voxelgrid_routed(c, xyzi, n, stride_bytes, leaf, out_xyzi, n_out, on_device);
}

// pcl::UniformSampling: rgc_voxelgrid's chain with another last launch (rgck::k_us_rows_pick) -- the same routes, the same refusals
int rgc_uniform_sampling(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, float leaf, float* out_xyzc, int* out_index, int* n_out, int on_device) {
  if (!c || !xyzc || !out_xyzc || !n_out || n < 0) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes) || !(leaf > 0.f) || !std::isfinite(leaf)) return fail(c, RGC_ERR_INVALID, "bad stride or leaf size");
  *n_out = 0;
  int rc = RGC_OK;
  if (n > 0 && on_device && out_index) rc = check_device_range(c, out_index, sizeof(int) * (size_t)n, "rgc_uniform_sampling: out_index");
  return voxelgrid_routed(c, xyzc, n, stride_bytes, leaf, out_xyzc, n_out, on_device, rgck::kVgModePick, out_index, rc);
}

int rgc_voxelgrid_route(rgc_ctx* c, rgc_vg_route* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  *out = c->vg.route;
  return RGC_OK;
}

// rgc_voxelgrid for a DEVICE cloud in two halves.  begin enqueues the filter on the box kept from the previous cloud of this leaf size and
// returns; end waits for it, looks at its flags and returns the point count -- repeating the filter through rgc_voxelgrid when the kept box
// did not hold the cloud (the input must therefore stay untouched in between).  Without a kept box begin is the whole rgc_voxelgrid.
// What it is for: the odometer's sub-map filter (RGC_odometer.cpp:985-991) depends on the pose of the PREVIOUS frame only, so a caller
// can start it when that frame ends and collect the result after the next sweep's own filter -- its 55 us of kernels and the read-back
// of its count are off the frame's critical path.  Other rgc_voxelgrid calls may run in between (they come later in stream order and
// use other result words); only ONE begin may be open per context.
int rgc_voxelgrid_begin(rgc_ctx* c, const float* d_xyzi, int n, int stride_bytes, float leaf, float* d_out) {
  if (!c || !d_xyzi || !d_out || n < 0 || n > (1 << 27)) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes) || !(leaf > 0.f) || !std::isfinite(leaf)) return fail(c, RGC_ERR_INVALID, "bad stride or leaf size");
  if (c->vg.pend.active) return fail(c, RGC_ERR_INVALID, "rgc_voxelgrid_begin: the previous one has not been ended");
  if (n > 0) { int rk = check_device_range(c, d_xyzi, record_bytes(n, stride_bytes, false), "rgc_voxelgrid_begin: d_xyzi"); if (rk) return rk; rk = check_device_range(c, d_out, (size_t)n * 16, "rgc_voxelgrid_begin: d_out"); if (rk) return rk; }
  HIPCHK(c, hipSetDevice(c->device));
  LeafFilterRecord::VgPending& pd_ = c->vg.pend;
  pd_ = LeafFilterRecord::VgPending{};
  pd_.d_in = d_xyzi; pd_.n = n; pd_.stride_bytes = stride_bytes; pd_.leaf = leaf; pd_.d_out = d_out;
  LeafFilterRecord::VgBox* box = nullptr;
  for (auto& b : c->vg.box) if (b.leaf == leaf) box = &b;
  bool enqueued = false;
  if (n > 0 && box && box->valid) {
    constexpr int kPadSparse = 32, kPadDense = 8;   // as in rgc_voxelgrid
    rgck::LeafGrid ps = box->g, pdg = box->g;
    for (int a = 0; a < 3; a++) { ps.minb[a] -= kPadSparse; ps.div[a] += 2 * kPadSparse; pdg.minb[a] -= kPadDense; pdg.div[a] += 2 * kPadDense; }
    const bool sparse = vg_rows_fit(ps, n);
    const double dcell = (double)pdg.div[0] * (double)pdg.div[1] * (double)pdg.div[2];
    if (sparse || dcell <= (double)c->prm.max_cells) {
      pd_.route.n = n;
      pd_.route.kept_box = 1;
      pd_.route.path = RGC_VG_PATH_KEPT;
      int rc = voxelgrid_rows(c, d_xyzi, stride_bytes / 4, n, 1.0f / leaf, sparse ? ps : pdg, (sparse ? kPadSparse : kPadDense) / 2, !sparse, d_out, nullptr,
                              nullptr, &pd_.route, c->vg.h_res);
      if (rc) return rc;
      pd_.g = sparse ? ps : pdg;
      enqueued = true;
    }
  }
  if (!enqueued) {  // no box to trust yet: the whole filter now
    const rgc_vg_route last = c->vg.route;
    int rc = rgc_voxelgrid(c, d_xyzi, n, stride_bytes, leaf, d_out, &pd_.n_out, 1);
    if (rc) return rc;
    pd_.route = c->vg.route;  // reported when this filter is ended; until then the context shows the filter before it
    c->vg.route = last;
    pd_.ready = true;
  }
  pd_.active = true;
  return RGC_OK;
}

int rgc_voxelgrid_end(rgc_ctx* c, int* n_out) {
  if (!c || !n_out) return RGC_ERR_INVALID;
  LeafFilterRecord::VgPending& pd_ = c->vg.pend;
  if (!pd_.active) return fail(c, RGC_ERR_INVALID, "rgc_voxelgrid_end without rgc_voxelgrid_begin");
  pd_.active = false;
  if (pd_.ready) { *n_out = pd_.n_out; c->vg.route = pd_.route; return RGC_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->vg.done));
  const int flags = c->vg.h_res[0], no = c->vg.h_res[2];
  rgc_vg_route& rt = pd_.route;
  rt.flags = rt.kept_flags = flags;
  if (flags & 1) { rt.status = RGC_ERR_NONFINITE; c->vg.route = rt; return fail(c, RGC_ERR_NONFINITE, "cloud contains non-finite coordinates (PCL skips them; remove NaNs first)"); }
  LeafFilterRecord::VgBox* box = nullptr;
  for (auto& b : c->vg.box) if (b.leaf == pd_.leaf) box = &b;
  if (box && (flags & 6)) { box->valid = false; rt.box_invalidated = 1; }  // outside: measure and repeat now; near a face: measure at the next call
  if (!(flags & 2)) { *n_out = no; rt.n_out = no; c->vg.route = rt; hint_from_leaf_grid(c, pd_.d_out, no, pd_.g, pd_.leaf); return RGC_OK; }
  const int rc = rgc_voxelgrid(c, pd_.d_in, pd_.n, pd_.stride_bytes, pd_.leaf, pd_.d_out, n_out, 1);  // (the kept box is invalid now: measured)
  c->vg.route.repeated = 1;
  c->vg.route.kept_box = 1;
  c->vg.route.kept_flags = flags;
  c->vg.route.box_invalidated = rt.box_invalidated;
  return rc;
}

}  // extern "C"
