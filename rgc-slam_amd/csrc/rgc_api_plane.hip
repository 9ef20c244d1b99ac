// rgc_api_plane.hip -- host side of RANSAC plane segmentation (rgc_plane_*): pcl::SACSegmentation (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE,
// SAC_RANSAC, setOptimizeCoefficients) and the pcl::ExtractIndices step behind it.  The kernels are rgc_plane.hip's; the semantics are stated in
// include/rgc_hip.h.  No grid is built: every hypothesis is scored against every point.
//   The hypothesis stream is scored a BATCH of positions at a time -- k_pl_models, k_pl_score, ONE small read-back (the non-finite word, the models,
// the counts) -- and PCL's sequential loop is replayed on the host over those counts, position by position, exactly as if each had been scored alone:
// what lies behind the stop is ignored, so no output bit depends on the batch size.  At most one host round trip per batch, never one per hypothesis.
// Then one chain -- the best model's upload, the refinement's fixed-order sums and eigenvector, the flags, their scan, the records -- and one read-back
// behind it.  What can refuse a call (the arguments, a caller's samples, the non-finite word of the first walk) does so before anything is written.
#include "rgc_ctx.h"
#include "rgc_plane.h"

#include <limits>

using namespace rgcapi;

namespace {

constexpr int kPlaneMaxPoints = 1 << 27;
constexpr double kPi = 3.14159265358979323846;
// a batch on the device and in the pinned mirror: 16 bytes for the non-finite word, B models, B counts; behind the largest batch the mirror holds the
// final rgck::PlaneFit and the number written
constexpr size_t kModelsAt = 16;
constexpr size_t kFitAt = 24576, kKeptAt = kFitAt + 512, kPinnedBytes = 32768;
static_assert(kModelsAt + 20 * (size_t)rgck::kPlaneMaxBatch <= kFitAt && sizeof(rgck::PlaneFit) <= 512, "the mirror's layout");
static_assert(RGC_PLANE_MAX_BATCH == rgck::kPlaneMaxBatch, "one limit");

size_t batch_bytes(int B) { return kModelsAt + 20 * (size_t)B; }

}  // namespace

extern "C" {

void rgc_default_plane_params(rgc_plane_params* p) {
  if (!p) return;
  *p = rgc_plane_params{};
  p->distance_threshold = 0.0;  // PCL's: it must be set
  p->probability = 0.99;
  p->eps_angle = 0.0;
  p->axis[0] = p->axis[1] = 0.0;
  p->axis[2] = 1.0;
  p->seed = 0;
  p->max_iterations = 50;
  p->optimize = 1;
  p->model_type = RGC_PLANE_PLANE;
}

int rgc_plane_sample(unsigned long long seed, unsigned long long t, int n, int* ijk) {
  if (n < 3 || !ijk) return RGC_ERR_INVALID;
  rgck::plane_sample(seed, t, n, ijk[0], ijk[1], ijk[2]);
  return RGC_OK;
}

int rgc_plane_set_batch(rgc_ctx* c, int batch) {
  if (!c) return RGC_ERR_INVALID;
  if (batch < 0 || batch > RGC_PLANE_MAX_BATCH) return fail(c, RGC_ERR_INVALID, "rgc_plane_set_batch: batch in 0..%d (0 = automatic)", RGC_PLANE_MAX_BATCH);
  c->plane.batch = batch;
  return RGC_OK;
}

int rgc_plane_get_info(rgc_ctx* c, rgc_plane_info* info) {
  if (!c || !info) return RGC_ERR_INVALID;
  *info = c->plane.info;
  return RGC_OK;
}

int rgc_plane_segment(rgc_ctx* c, const float* xyzc, int n, int stride_bytes, int on_device, const rgc_plane_params* prm, const int* samples, int n_samples,
                      int negative, double* coeff, float* out_xyzc, int* out_index, int* out_counts, int* n_out) {
  const char* who = "rgc_plane_segment";
  if (!c || !prm || !coeff || !n_out || n < 0 || (n > 0 && !xyzc)) return RGC_ERR_INVALID;
  const float thr = (float)prm->distance_threshold;
  if (n > 0 && n < 3) return fail(c, RGC_ERR_INVALID, "%s: a plane needs 3 points, the cloud has %d", who, n);
  if (n > kPlaneMaxPoints) return fail(c, RGC_ERR_INVALID, "%s: cloud has %d points, the limit is 2^27", who, n);
  if (!std::isfinite(prm->distance_threshold) || !std::isfinite(thr) || !(thr > 0.f)) return fail(c, RGC_ERR_INVALID, "%s: the distance threshold must be finite and > 0 (as a float too)", who);
  if (!(prm->probability > 0.0 && prm->probability < 1.0)) return fail(c, RGC_ERR_INVALID, "%s: probability in (0, 1)", who);
  if (prm->max_iterations < 1) return fail(c, RGC_ERR_INVALID, "%s: max_iterations >= 1", who);
  if (prm->model_type != RGC_PLANE_PLANE && prm->model_type != RGC_PLANE_PERPENDICULAR) return fail(c, RGC_ERR_INVALID, "%s: model_type 0 (plane) or 1 (perpendicular plane)", who);
  rgck::PlaneStream st{};
  if (prm->model_type == RGC_PLANE_PERPENDICULAR) {
    const double ax = prm->axis[0], ay = prm->axis[1], az = prm->axis[2];
    const double len = std::sqrt((ax * ax + ay * ay) + az * az);
    if (!(prm->eps_angle >= 0.0 && prm->eps_angle <= kPi / 2)) return fail(c, RGC_ERR_INVALID, "%s: eps_angle in [0, pi / 2]", who);
    if (!std::isfinite(len) || !(len > 0.0)) return fail(c, RGC_ERR_INVALID, "%s: the axis must be finite and not zero", who);
    st.use_axis = 1;
    st.axis[0] = ax / len; st.axis[1] = ay / len; st.axis[2] = az / len;
    st.cos_eps = std::cos(prm->eps_angle);
  }
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "%s: stride_bytes must be a multiple of 4 between 12 and 4096", who);
  if (n_samples < 0) return fail(c, RGC_ERR_INVALID, "%s: n_samples >= 0", who);
  if (samples && n > 0)
    for (long long t = 0; t < n_samples; t++) {
      const int i0 = samples[3 * t], i1 = samples[3 * t + 1], i2 = samples[3 * t + 2];
      if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n || i1 >= n || i2 >= n || i0 == i1 || i0 == i2 || i1 == i2)
        return fail(c, RGC_ERR_INVALID, "%s: samples[%lld] = (%d, %d, %d): three distinct indices below %d", who, t, i0, i1, i2, n);
    }
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "%s: a solve is in flight", who);
  c->plane.info = rgc_plane_info{};
  c->plane.info.best_count = -1;
  c->plane.info.best_position = -1;
  if (n == 0) {
    for (int a = 0; a < 4; a++) coeff[a] = 0.0;
    *n_out = 0;
    return RGC_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t nn = (size_t)n;
  rgcapi::PlaneRecord& r = c->plane;
  int rc;
  const float* d_in = nullptr;
  float* d_out = nullptr;
  int* d_index = nullptr;
  if ((rc = stage_records(c, xyzc, n, stride_bytes, on_device, out_xyzc != nullptr, r.in, "input cloud", &d_in))) return rc;
  if ((rc = place_output(c, out_xyzc, 16 * nn, on_device, r.sel.out, "out_xyzc", &d_out))) return rc;
  if ((rc = place_output(c, out_index, sizeof(int) * nn, on_device, r.sel.idx, "out_index", &d_index))) return rc;
  const int stride_f = stride_bytes / 4;
  const long long T = samples ? (long long)n_samples : 10ll * prm->max_iterations;  // the stream's end
  const int B = r.batch > 0 ? r.batch : std::min(prm->max_iterations, 64);
  if ((rc = ensure(c, r.bat, batch_bytes(B)))) return rc;
  if ((rc = ensure(c, r.fit, sizeof(rgck::PlaneFit)))) return rc;
  if ((rc = selection_scratch(c, r.sel, n))) return rc;
  if (prm->optimize && (rc = ensure(c, r.rows, sizeof(double) * rgck::kPlaneRowCols * (size_t)rgck::plane_moment_rows(n)))) return rc;
  if (!r.h) HIPCHK(c, hipHostMalloc((void**)&r.h, kPinnedBytes, hipHostMallocDefault));
  if (samples && n_samples > 0) {
    if ((rc = ensure(c, r.samples, sizeof(int) * 3 * (size_t)n_samples))) return rc;
    HIPCHK(c, hipMemcpyAsync(r.samples.p, samples, sizeof(int) * 3 * (size_t)n_samples, hipMemcpyHostToDevice, s));
    st.samples = r.samples.as<const int>();
  }
  st.seed = prm->seed;
  unsigned char* const dbat = r.bat.as<unsigned char>();
  const rgck::PlaneBatch bat{reinterpret_cast<int*>(dbat), reinterpret_cast<float4*>(dbat + kModelsAt), reinterpret_cast<int*>(dbat + kModelsAt + 16 * (size_t)B)};
  const int* const h_nonfinite = reinterpret_cast<const int*>(r.h);
  const float4* const h_models = reinterpret_cast<const float4*>(r.h + kModelsAt);
  const int* const h_counts = reinterpret_cast<const int*>(r.h + kModelsAt + 16 * (size_t)B);
  HIPCHK(c, hipMemsetAsync(dbat, 0, kModelsAt, s));

  // ---- the decision: PCL's sequential loop, replayed over each batch's counts ----
  const double log_fail = std::log(1.0 - prm->probability);
  long long t0 = 0, best_position = -1, skipped = 0;
  int best = -1, iterations = 0, launches = 0;
  double k = 1.0;
  float4 best_model = make_float4(0.f, 0.f, 0.f, 0.f);
  bool stop = T == 0;
  if (stop) {  // an empty stream: the cloud is walked all the same, for the non-finite word
    rgck::plane_score(s, d_in, stride_f, n, thr, 0, 1, bat);
    HIPCHK(c, hipMemcpyAsync(r.h, dbat, kModelsAt, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (h_nonfinite[0]) return fail(c, RGC_ERR_NONFINITE, "%s: the cloud has a non-finite coordinate", who);
  }
  while (!stop) {
    const int b = (int)std::min<long long>(B, T - t0);
    st.t0 = (unsigned long long)t0;
    st.batch = b;
    rgck::plane_models(s, d_in, stride_f, n, st, bat);
    rgck::plane_score(s, d_in, stride_f, n, thr, b, launches == 0, bat);
    HIPCHK(c, hipMemcpyAsync(r.h, dbat, batch_bytes(B), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (launches == 0 && h_nonfinite[0]) return fail(c, RGC_ERR_NONFINITE, "%s: the cloud has a non-finite coordinate", who);
    launches++;
    for (int j = 0; j < b && !stop; j++) {
      const int count = h_counts[j];
      if (out_counts) out_counts[t0 + j] = count;
      if (count < 0) {
        skipped++;
      } else {
        if (count > best) {
          best = count;
          best_position = t0 + j;
          best_model = h_models[j];
          const double w = (double)best / (double)n;
          double q = 1.0 - (w * w) * w;
          q = std::min(std::max(q, DBL_EPSILON), 1.0 - DBL_EPSILON);
          k = log_fail / std::log(q);
        }
        iterations++;
        if ((double)iterations >= k || iterations == prm->max_iterations) stop = true;
      }
      if (t0 + j + 1 == T) stop = true;
      if (stop) c->plane.info.positions = t0 + j + 1;
    }
    t0 += b;
  }

  // ---- the best model's inliers, the refinement, the records ----
  rgck::PlaneFit* const h_fit = reinterpret_cast<rgck::PlaneFit*>(r.h + kFitAt);
  rgck::PlaneFit* const d_fit = r.fit.as<rgck::PlaneFit>();
  *h_fit = rgck::PlaneFit{};
  const float qnan = std::numeric_limits<float>::quiet_NaN();
  h_fit->model = best_position >= 0 ? best_model : make_float4(qnan, qnan, qnan, qnan);  // no model: no point is an inlier
  HIPCHK(c, hipMemcpyAsync(d_fit, h_fit, sizeof(rgck::PlaneFit), hipMemcpyHostToDevice, s));
  if (prm->optimize && best >= 3) rgck::plane_refine(s, d_in, stride_f, n, thr, r.rows.as<double>(), d_fit);
  rgck::plane_flag(s, d_in, stride_f, n, thr, d_fit, negative, r.sel.flag.as<int>());
  int* const h_kept = reinterpret_cast<int*>(r.h + kKeptAt);
  const EmitTo to{d_out, d_index, out_xyzc, out_index};
  const EmitHome home{h_fit, d_fit, sizeof(rgck::PlaneFit), h_kept};
  if ((rc = emit_selected(c, r.sel, d_in, stride_f, n, on_device, to, home))) return rc;
  if (!on_device) HIPCHK(c, hipStreamSynchronize(s));
  const int kept = *h_kept;
  const bool found = best_position >= 0;
  const float4 m = h_fit->model;
  coeff[0] = found ? (double)m.x : 0.0; coeff[1] = found ? (double)m.y : 0.0; coeff[2] = found ? (double)m.z : 0.0; coeff[3] = found ? (double)m.w : 0.0;
  rgc_plane_info& info = c->plane.info;
  info.n = n;
  info.n_inliers = negative ? n - kept : kept;
  info.iterations = iterations;
  info.best_count = best;
  info.batch = B;
  info.launches = launches;
  info.refined = h_fit->refined;
  info.skipped = skipped;
  info.best_position = best_position;
  info.k = k;
  info.ransac_coeff[0] = found ? (double)best_model.x : 0.0; info.ransac_coeff[1] = found ? (double)best_model.y : 0.0;
  info.ransac_coeff[2] = found ? (double)best_model.z : 0.0; info.ransac_coeff[3] = found ? (double)best_model.w : 0.0;
  *n_out = kept;
  return RGC_OK;
}

}  // extern "C"
