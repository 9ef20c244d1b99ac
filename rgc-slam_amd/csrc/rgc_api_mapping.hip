// rgc_api_mapping.hip -- host side of the mapping node's entry points: f1 feature registration (rgc_mapreg_*), f2 rolling local map
// (rgc_map_*), f3 PointCloud2 (rgc_pc2_*), f4 loop-closure ICP (rgc_icp_*), f5 keyframe store (rgc_kf_*).
#include "rgc_ctx.h"

void rgc_host_key_pose_quat(float roll, float pitch, float yaw, double q_xyzw[4]);  // rgc_host.cpp: the reference's key pose -> quaternion chain (f5)

using namespace rgcapi;

namespace {

// ---- f1: grid of a feature map (bbox -> counting sort; no covariances) and the host side of the robust LM ----------------
// grid cell of a feature map = the largest 5th-neighbour distance that still yields a factor (1 m for edges :1098, sqrt(2) m for
// planes :1200): the 3x3x3 block of cells then proves every accepted neighbourhood, and holds as few candidates as possible
constexpr double kMapregCell[2] = {1.0, 1.4143};

int prepare_map_grid(rgc_ctx* c, Cloud& cl, double cell) {
  int rc, hsm[8];
  if ((rc = ensure(c, c->mr_small, 64))) return rc;
  if ((rc = build_measured_grid(c, cl, cell, c->mr_small.as<int>(), hsm, false, "feature map", "feature-map grid"))) return rc;
  HIPCHK(c, hipGetLastError());
  cl.ready = true;
  return RGC_OK;
}

// Cholesky solve of a symmetric positive definite n x n, n <= 12 (the damped normal equations of the two poses: block
// diagonal unless the IMU block couples the rotations)
bool chol_solve(const double* A, const double* rhs, double* x, int n) {
  double L[144] = {0}, y[12];
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i * n + j];
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      if (i == j) { if (!(s > 0)) return false; L[i * n + i] = std::sqrt(s); }
      else L[i * n + j] = s / L[j * n + j];
    }
  for (int i = 0; i < n; i++) { double s = rhs[i]; for (int k = 0; k < i; k++) s -= L[i * n + k] * y[k]; y[i] = s / L[i * n + i]; }
  for (int i = n - 1; i >= 0; i--) { double s = y[i]; for (int k = i + 1; k < n; k++) s -= L[k * n + i] * x[k]; x[i] = s / L[i * n + i]; }
  return true;
}

void quat_plus(const double q[4], const double d[3], double out[4]) {  // EigenQuaternionParameterization::Plus [3P-memory]
  const double nd = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  double dq[4];
  if (nd > 0.0) { const double s = std::sin(nd) / nd; dq[0] = s * d[0]; dq[1] = s * d[1]; dq[2] = s * d[2]; dq[3] = std::cos(nd); }
  else { dq[0] = d[0]; dq[1] = d[1]; dq[2] = d[2]; dq[3] = 1.0; }
  const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = q[0], by = q[1], bz = q[2], bw = q[3];
  out[0] = aw * bx + ax * bw + ay * bz - az * by;
  out[1] = aw * by - ax * bz + ay * bw + az * bx;
  out[2] = aw * bz + ax * by - ay * bx + az * bw;
  out[3] = aw * bw - ax * bx - ay * by - az * bz;
}

void quat_rot_h(const double q[4], const double p[3], double out[3]) {  // Eigen: quaternion * vector (x,y,z,w)
  const double tx = 2 * (q[1] * p[2] - q[2] * p[1]), ty = 2 * (q[2] * p[0] - q[0] * p[2]), tz = 2 * (q[0] * p[1] - q[1] * p[0]);
  out[0] = p[0] + q[3] * tx + (q[1] * tz - q[2] * ty);
  out[1] = p[1] + q[3] * ty + (q[2] * tx - q[0] * tz);
  out[2] = p[2] + q[3] * tz + (q[0] * ty - q[1] * tx);
}
void quat_mul_h(const double a[4], const double b[4], double o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
// Ground_DeltaFactor_goable::operator() (lidarFactor.hpp:357-391)
void ground_residual(const rgc_mapreg_ground* G, const double q[4], const double t[3], double r[3]) {
  const double lqc[4] = {-G->last_q[0], -G->last_q[1], -G->last_q[2], G->last_q[3]};
  double q_lc[4], dt[3] = {t[0] - G->last_t[0], t[1] - G->last_t[1], t[2] - G->last_t[2]}, t_lc[3], gn[3], delta_t[3];
  quat_mul_h(lqc, q, q_lc);
  quat_rot_h(lqc, dt, t_lc);
  quat_rot_h(q_lc, G->cur_norm, gn);
  quat_rot_h(G->q_history, t_lc, delta_t);
  const double dist_cur = G->cur_distance + delta_t[2];
  r[0] = (G->last_distance - dist_cur) / (G->p_var / 1000);
  r[1] = std::fabs(G->last_v1[0] * gn[0] + G->last_v1[1] * gn[1] + G->last_v1[2] * gn[2]) / (G->p_var * 10);
  r[2] = std::fabs(G->last_v2[0] * gn[0] + G->last_v2[1] * gn[1] + G->last_v2[2] * gn[2]) / (G->p_var * 10);
}
// the ground block of one pose added on the host (three scalars: not worth a launch).  NULL loss; the Jacobian on the local
// parameterisation by central differences (step 1e-6; Ceres differentiates abs() as sign(), which this matches away from 0).
void ground_terms(const rgc_mapreg_ground* G, const double q[4], const double t[3], bool want_H, double S28[28]) {
  if (!G) return;
  double r[3];
  ground_residual(G, q, t, r);
  S28[27] += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (!want_H) return;
  double J[18];
  const double h = 1e-6;
  for (int a = 0; a < 6; a++) {
    double rp[3], rm[3], qq[4], tt[3], d[3] = {0, 0, 0};
    for (int sgn = 0; sgn < 2; sgn++) {
      const double e = sgn ? -h : h;
      memcpy(qq, q, sizeof(qq)); memcpy(tt, t, sizeof(tt));
      if (a < 3) { d[0] = d[1] = d[2] = 0; d[a] = e; quat_plus(q, d, qq); } else tt[a - 3] += e;
      ground_residual(G, qq, tt, sgn ? rm : rp);
    }
    for (int k = 0; k < 3; k++) J[k * 6 + a] = (rp[k] - rm[k]) / (2 * h);
  }
  int u = 0;
  for (int a = 0; a < 6; a++)
    for (int e = a; e < 6; e++) {
      double v = 0;
      for (int k = 0; k < 3; k++) v += J[k * 6 + a] * J[k * 6 + e];
      S28[u++] += v;
    }
  for (int a = 0; a < 6; a++) {
    double v = 0;
    for (int k = 0; k < 3; k++) v += J[k * 6 + a] * r[k];
    S28[21 + a] += v;
  }
}

// Quaternion2EulerAngle (lidarFactor.hpp:405-433) on x,y,z,w: pitch and roll only
void pitch_roll(const double q[4], double* pitch, double* roll) {
  const double sinp = 2 * (q[3] * q[1] - q[0] * q[2]);
  *pitch = sinp >= 1 ? M_PI / 2 : (sinp <= -1 ? -M_PI / 2 : std::asin(sinp));
  *roll = std::atan2(2 * (q[3] * q[0] + q[1] * q[2]), 1 - 2 * (q[0] * q[0] + q[1] * q[1]));
}
// RelativeRFactor on (q_last, q_cur) (lidarFactor.hpp:174-226; QuaternionInverse = conjugate, :124-130) followed by the
// PitchRollFactor of the current and of the last pose (:434-468): 3 + 2 + 2 residuals
void imu_residual(const rgc_mapreg_imu* I, const double q_cur[4], const double q_last[4], double r[7]) {
  const double li[4] = {-q_last[0], -q_last[1], -q_last[2], q_last[3]};
  const double di[4] = {-I->delta_q[0], -I->delta_q[1], -I->delta_q[2], I->delta_q[3]};
  double q_ij[4], e[4], p, ro;
  quat_mul_h(li, q_cur, q_ij);
  quat_mul_h(di, q_ij, e);
  for (int a = 0; a < 3; a++) r[a] = 2 * e[a] / I->imu_cov;
  pitch_roll(q_cur, &p, &ro);
  r[3] = 2 * (p - I->pitch_cur) / I->pr_var;
  r[4] = 2 * (ro - I->roll_cur) / I->pr_var;
  pitch_roll(q_last, &p, &ro);
  r[5] = 2 * (p - I->pitch_last) / I->pr_var;
  r[6] = 2 * (ro - I->roll_last) / I->pr_var;
}
// the IMU block (RGC_mapping.cpp:1285-1312) added on the host: seven scalars over the two rotations, NULL loss, Jacobian
// on the local parameterisation by central differences (step 1e-6) like the ground block.  H is the full 12 x 12.
void imu_terms(const rgc_mapreg_imu* I, const double x[14], bool want_H, double H[144], double g[12], double* cost) {
  if (!I) return;
  double r[7];
  imu_residual(I, x, x + 7, r);
  for (int k = 0; k < 7; k++) *cost += 0.5 * r[k] * r[k];
  if (!want_H) return;
  double J[7][12] = {};
  const double h = 1e-6;
  for (int b = 0; b < 2; b++)
    for (int a = 0; a < 3; a++) {  // the translations do not enter
      double rp[7], rm[7];
      for (int sgn = 0; sgn < 2; sgn++) {
        double qc[4], ql[4], d[3] = {0, 0, 0};
        memcpy(qc, x, sizeof(qc)); memcpy(ql, x + 7, sizeof(ql));
        d[a] = sgn ? -h : h;
        quat_plus(x + 7 * b, d, b ? ql : qc);
        imu_residual(I, qc, ql, sgn ? rm : rp);
      }
      for (int k = 0; k < 7; k++) J[k][6 * b + a] = (rp[k] - rm[k]) / (2 * h);
    }
  for (int a = 0; a < 12; a++) {
    for (int e = 0; e < 12; e++) {
      double v = 0;
      for (int k = 0; k < 7; k++) v += J[k][a] * J[k][e];
      H[a * 12 + e] += v;
    }
    double v = 0;
    for (int k = 0; k < 7; k++) v += J[k][a] * r[k];
    g[a] += v;
  }
}

// the robustified normal equations of both poses at x (14 doubles): H 12 x 12 (two 6 x 6 pose blocks, plus the IMU block's
// coupling of the rotations), g 12, the cost.  Feature sets 0/1 = corner/surf of the current pose, 2/3 = of the last pose;
// the kernels return 21 H + 6 g + cost per pose.
struct MapregSystem { double H[144], g[12], cost; };
int mapreg_eval(rgc_ctx* c, const int nfeat[4], const double x[14], bool want_H, const rgc_mapreg_ground* const ground[2],
                const rgc_mapreg_imu* imu, MapregSystem* out) {
  const float* feat[4];
  const double* fac[4];
  for (int s = 0; s < 4; s++) { feat[s] = c->mr_feat[s].as<const float>(); fac[s] = c->mr_fac[s].as<const double>(); }
  rgck::mapreg_terms(c->stream, feat, fac, nfeat, x, 0.1, want_H ? 1 : 0, c->mr_partials.as<double>(), c->d_out);
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double) * 56, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  double S[2][28];
  memcpy(S, c->h_out, sizeof(S));
  for (int b = 0; b < 2; b++) ground_terms(ground[b], x + 7 * b, x + 7 * b + 4, want_H, S[b]);
  memset(out->H, 0, sizeof(out->H));
  memset(out->g, 0, sizeof(out->g));
  for (int b = 0; b < 2 && want_H; b++) {
    int u = 0;
    for (int a = 0; a < 6; a++)
      for (int e = a; e < 6; e++, u++) out->H[(6 * b + a) * 12 + 6 * b + e] = out->H[(6 * b + e) * 12 + 6 * b + a] = S[b][u];
    for (int a = 0; a < 6; a++) out->g[6 * b + a] = S[b][21 + a];
  }
  out->cost = S[0][27] + S[1][27];
  imu_terms(imu, x, want_H, out->H, out->g, &out->cost);
  return RGC_OK;
}

}  // namespace

extern "C" {

// ---- f1: scan-to-map FEATURE registration of the mapping node (RGC_mapping.cpp:1069-1358) --------------------------------
// rgc_mapreg_set_maps / rgc_mapreg_set_maps_device: one body; on_device: the maps are read where they lie instead of being uploaded first
static int mapreg_set_maps_impl(rgc_ctx* c, const float* corner_map, int n_corner, const float* surf_map, int n_surf, int stride_bytes, bool on_device) {
  if (!c || !corner_map || !surf_map) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (n_corner < 5 || n_surf < 5) return fail(c, RGC_ERR_TOO_FEW_POINTS, "feature maps need at least 5 points each (5-NN)");
  if (n_corner > (1 << 27) || n_surf > (1 << 27)) return fail(c, RGC_ERR_INVALID, "feature map larger than 2^27 points");
  HIPCHK(c, hipSetDevice(c->device));
  const float* src[2] = {corner_map, surf_map};
  const int n[2] = {n_corner, n_surf};
  for (int m = 0; m < 2; m++) {
    Cloud& cl = c->mr_map[m];
    cl.ready = false;
    const size_t bytes = (size_t)n[m] * stride_bytes;
    int rc;
    if (on_device) {
      if ((rc = check_device_range(c, src[m], bytes - (stride_bytes - 12), "rgc_mapreg_set_maps_device: feature map"))) return rc;
      cl.in = src[m];
    } else {
      if ((rc = ensure(c, cl.in_copy, bytes))) return rc;
      HIPCHK(c, hipMemcpyAsync(cl.in_copy.p, src[m], bytes - (stride_bytes - 12), hipMemcpyHostToDevice, c->stream));
      cl.in = cl.in_copy.as<const float>();
    }
    cl.stride_f = stride_bytes / 4;
    cl.n = n[m];
    if ((rc = prepare_map_grid(c, cl, kMapregCell[m]))) return rc;
  }
  return RGC_OK;
}
int rgc_mapreg_set_maps(rgc_ctx* c, const float* corner_map, int n_corner, const float* surf_map, int n_surf, int stride_bytes) {
  return mapreg_set_maps_impl(c, corner_map, n_corner, surf_map, n_surf, stride_bytes, false);
}
int rgc_mapreg_set_maps_device(rgc_ctx* c, const float* d_corner, int n_corner, const float* d_surf, int n_surf, int stride_bytes) {
  return mapreg_set_maps_impl(c, d_corner, n_corner, d_surf, n_surf, stride_bytes, true);
}

static int mapreg_upload_features(rgc_ctx* c, int slot, const float* feat, int n) {
  int rc;
  if ((rc = ensure(c, c->mr_feat[slot], sizeof(float) * 4 * (size_t)(n > 0 ? n : 1)))) return rc;
  if ((rc = ensure(c, c->mr_fac[slot], sizeof(double) * 8 * (size_t)(n > 0 ? n : 1)))) return rc;
  if (n > 0) HIPCHK(c, hipMemcpyAsync(c->mr_feat[slot].p, feat, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  return RGC_OK;
}

int rgc_mapreg_associate(rgc_ctx* c, int kind, const float* feat_xyzw, int n, const double q_xyzw[4], const double t[3], double* factors8,
                         int* n_valid) {
  if (!c || !feat_xyzw || !q_xyzw || !t || n < 0 || n > (1 << 27) || (kind != 0 && kind != 1)) return RGC_ERR_INVALID;
  if (!c->mr_map[kind].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = mapreg_upload_features(c, kind, feat_xyzw, n);
  if (rc) return rc;
  const Cloud& m = c->mr_map[kind];
  const rgck::MapregAssoc one{c->mr_feat[kind].as<const float>(), n, kind == 0 ? 1 : 0, rgck::Quat{q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3]},
                              {t[0], t[1], t[2]}, m.P.as<const float4>(), m.start.as<const int>(), m.grid, c->mr_fac[kind].as<double>(), nullptr};
  rgck::mapreg_associate(c->stream, &one, 1);
  std::vector<double> tmp;
  double* dst = factors8;
  if (!dst) { tmp.resize((size_t)8 * (n > 0 ? n : 1)); dst = tmp.data(); }
  if (n > 0) HIPCHK(c, hipMemcpyAsync(dst, c->mr_fac[kind].p, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  if (n_valid) {
    int cnt = 0;
    for (int i = 0; i < n; i++) cnt += dst[(size_t)8 * i + 7] != 0.0;
    *n_valid = cnt;
  }
  return RGC_OK;
}

int rgc_mapreg_optimize(rgc_ctx* c, const float* corner_cur, int n_ccur, const float* surf_cur, int n_scur, const float* corner_last,
                        int n_clast, const float* surf_last, int n_slast, const rgc_mapreg_ground* ground_cur, const rgc_mapreg_ground* ground_last,
                        const rgc_mapreg_imu* imu, double poses[14], rgc_mapreg_report report[2], int* gate_failed) {
  if (!c || !poses || n_ccur < 0 || n_scur < 0 || n_clast < 0 || n_slast < 0) return RGC_ERR_INVALID;
  if (n_ccur > (1 << 27) || n_scur > (1 << 27) || n_clast > (1 << 27) || n_slast > (1 << 27)) return fail(c, RGC_ERR_INVALID, "feature cloud larger than 2^27 points");
  if ((n_ccur && !corner_cur) || (n_scur && !surf_cur) || (n_clast && !corner_last) || (n_slast && !surf_last)) return RGC_ERR_INVALID;
  if (!c->mr_map[0].ready || !c->mr_map[1].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  if (report) memset(report, 0, sizeof(rgc_mapreg_report) * 2);
  // the gate of :1069 (laserCloudCornerDSNum > 10 && laserCloudSurfDSNum > 50 && map sizes likewise)
  const bool gate = n_ccur > 10 && n_scur > 50 && c->mr_map[0].n > 10 && c->mr_map[1].n > 50;
  if (gate_failed) *gate_failed = gate ? 0 : 1;
  if (!gate) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const float* feat[4] = {corner_cur, surf_cur, corner_last, surf_last};
  const int nfeat[4] = {n_ccur, n_scur, n_clast, n_slast};
  const rgc_mapreg_ground* const ground[2] = {ground_cur, ground_last};
  int rc;
  for (int s = 0; s < 4; s++)
    if ((rc = mapreg_upload_features(c, s, feat[s], nfeat[s]))) return rc;
  const int nb = std::max(rgck::mapreg_blocks(n_ccur, n_scur), rgck::mapreg_blocks(n_clast, n_slast));
  if ((rc = ensure(c, c->mr_partials, sizeof(double) * 2 * rgck::kAccum * (size_t)(nb > 0 ? nb : 1)))) return rc;
  for (int iter = 0; iter < 2; iter++) {  // :1076
    // association at the current estimate of both poses (frozen during the solve); the factor counts (the reference's
    // corner_num / surf_num ...) ride home with the first evaluation's synchronisation
    int* dcnt = c->mr_small.as<int>() + 8;
    HIPCHK(c, hipMemsetAsync(dcnt, 0, 4 * sizeof(int), c->stream));
    rgck::MapregAssoc sets[4];
    for (int s = 0; s < 4; s++) {
      const double* q = poses + 7 * (s / 2);
      const Cloud& m = c->mr_map[s & 1];
      sets[s] = rgck::MapregAssoc{c->mr_feat[s].as<const float>(), nfeat[s], (s & 1) == 0 ? 1 : 0, rgck::Quat{q[0], q[1], q[2], q[3]}, {q[4], q[5], q[6]},
                                  m.P.as<const float4>(), m.start.as<const int>(), m.grid, c->mr_fac[s].as<double>(), dcnt + s};
    }
    rgck::mapreg_associate(c->stream, sets, 4);  // the four loops of :1092-1282 side by side
    HIPCHK(c, hipMemcpyAsync(c->h_small->mapreg.n, dcnt, sizeof(rgck::MapregCounts::n), hipMemcpyDeviceToHost, c->stream));
    // ceres::Solve restated: trust-region LM, <= 6 iterations (:1333-1341), Ceres 1.14 defaults: initial radius 1e4, damping diag(H)/radius clamped to [1e-6, 1e32], step accepted above a relative decrease of 1e-3
    double radius = 1e4, decrease_factor = 2.0;
    MapregSystem S, Sn;
    if ((rc = mapreg_eval(c, nfeat, poses, true, ground, imu, &S))) return rc;
    if (report) {
      const int* nf = c->h_small->mapreg.n;
      report[iter].n_edge_cur = nf[0]; report[iter].n_plane_cur = nf[1];
      report[iter].n_edge_last = nf[2]; report[iter].n_plane_last = nf[3];
    }
    int it = 0, n_success = 0;
    const double initial_cost = S.cost;
    for (it = 0; it < 6; it++) {
      double gmax = 0;
      for (int a = 0; a < 12; a++) gmax = std::fmax(gmax, std::fabs(S.g[a]));
      if (gmax <= 1e-10) break;
      double A[144], rhs[12], d[12], model = 0;
      memcpy(A, S.H, sizeof(A));
      for (int a = 0; a < 12; a++) {
        A[a * 13] += std::fmin(std::fmax(S.H[a * 13], 1e-6), 1e32) / radius;  // min / max_lm_diagonal
        rhs[a] = -S.g[a];
      }
      const bool ok = chol_solve(A, rhs, d, 12);
      for (int a = 0; a < 12 && ok; a++) {  // model cost change = -d^T (g + H d / 2)
        double Hd = 0;
        for (int e = 0; e < 12; e++) Hd += S.H[a * 12 + e] * d[e];
        model -= d[a] * (S.g[a] + 0.5 * Hd);
      }
      double rho = -1.0, xn[14];
      memcpy(xn, poses, sizeof(xn));
      if (ok && model > 0) {
        for (int b = 0; b < 2; b++) {
          quat_plus(poses + 7 * b, d + 6 * b, xn + 7 * b);
          for (int a = 0; a < 3; a++) xn[7 * b + 4 + a] = poses[7 * b + 4 + a] + d[6 * b + 3 + a];
        }
        // the candidate's cost AND its normal equations in one launch: nearly every step is accepted, and an accepted step
        // needs them next (a rejected one just drops them)
        if ((rc = mapreg_eval(c, nfeat, xn, true, ground, imu, &Sn))) return rc;
        rho = (S.cost - Sn.cost) / model;
      }
      if (rho > 1e-3) {
        const double old_cost = S.cost;
        memcpy(poses, xn, sizeof(xn));
        radius = std::fmin(radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3)), 1e16);
        decrease_factor = 2.0;
        n_success++;
        S = Sn;
        double step2 = 0, x2 = 0;
        for (int a = 0; a < 12; a++) step2 += d[a] * d[a];
        for (int a = 0; a < 14; a++) x2 += poses[a] * poses[a];
        if (std::fabs(old_cost - S.cost) <= 1e-6 * old_cost) { it++; break; }
        if (std::sqrt(step2) <= 1e-8 * (std::sqrt(x2) + 1e-8)) { it++; break; }
      } else {
        radius /= decrease_factor;
        decrease_factor *= 2.0;
        if (radius < 1e-32) { it++; break; }
      }
    }
    const double cost = S.cost;
    if (report) { report[iter].initial_cost = initial_cost; report[iter].final_cost = cost; report[iter].iterations = it; report[iter].successful = n_success; }
  }
  for (int b = 0; b < 2; b++) {  // q_w_last.normalize(); q_w_curr.normalize(); (:1375-1376)
    double* q = poses + 7 * b;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nn > 0) for (int a = 0; a < 4; a++) q[a] /= nn;
  }
  return RGC_OK;
}

// a read-out of what one LM iteration of rgc_mapreg_optimize sees: the association at poses_assoc (the four loops in one launch, as
// there), then the normal equations of the frozen factors at poses_eval (NULL: at poses_assoc).  No gate of :1069 -- it reports, it
// does not decide -- and any feature set may be empty.
int rgc_mapreg_linearize(rgc_ctx* c, const float* corner_cur, int n_ccur, const float* surf_cur, int n_scur, const float* corner_last,
                         int n_clast, const float* surf_last, int n_slast, const rgc_mapreg_ground* ground_cur, const rgc_mapreg_ground* ground_last,
                         const rgc_mapreg_imu* imu, const double poses_assoc[14], const double poses_eval[14], double H[144], double g[12],
                         double* cost, int n_factors[4], double* const factors8[4]) {
  if (!c || !poses_assoc || !H || !g || !cost || !n_factors || n_ccur < 0 || n_scur < 0 || n_clast < 0 || n_slast < 0) return RGC_ERR_INVALID;
  if (n_ccur > (1 << 27) || n_scur > (1 << 27) || n_clast > (1 << 27) || n_slast > (1 << 27)) return fail(c, RGC_ERR_INVALID, "feature cloud larger than 2^27 points");
  if ((n_ccur && !corner_cur) || (n_scur && !surf_cur) || (n_clast && !corner_last) || (n_slast && !surf_last)) return RGC_ERR_INVALID;
  if (!c->mr_map[0].ready || !c->mr_map[1].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  HIPCHK(c, hipSetDevice(c->device));
  const float* feat[4] = {corner_cur, surf_cur, corner_last, surf_last};
  const int nfeat[4] = {n_ccur, n_scur, n_clast, n_slast};
  const rgc_mapreg_ground* const ground[2] = {ground_cur, ground_last};
  int rc;
  for (int s = 0; s < 4; s++)
    if ((rc = mapreg_upload_features(c, s, feat[s], nfeat[s]))) return rc;
  const int nb = std::max(rgck::mapreg_blocks(n_ccur, n_scur), rgck::mapreg_blocks(n_clast, n_slast));
  if ((rc = ensure(c, c->mr_partials, sizeof(double) * 2 * rgck::kAccum * (size_t)(nb > 0 ? nb : 1)))) return rc;
  int* dcnt = c->mr_small.as<int>() + 8;
  HIPCHK(c, hipMemsetAsync(dcnt, 0, 4 * sizeof(int), c->stream));
  rgck::MapregAssoc sets[4];
  for (int s = 0; s < 4; s++) {
    const double* q = poses_assoc + 7 * (s / 2);
    const Cloud& m = c->mr_map[s & 1];
    sets[s] = rgck::MapregAssoc{c->mr_feat[s].as<const float>(), nfeat[s], (s & 1) == 0 ? 1 : 0, rgck::Quat{q[0], q[1], q[2], q[3]}, {q[4], q[5], q[6]},
                                m.P.as<const float4>(), m.start.as<const int>(), m.grid, c->mr_fac[s].as<double>(), dcnt + s};
  }
  rgck::mapreg_associate(c->stream, sets, 4);
  HIPCHK(c, hipMemcpyAsync(c->h_small->mapreg.n, dcnt, sizeof(rgck::MapregCounts::n), hipMemcpyDeviceToHost, c->stream));
  for (int s = 0; s < 4 && factors8; s++)
    if (factors8[s] && nfeat[s] > 0)
      HIPCHK(c, hipMemcpyAsync(factors8[s], c->mr_fac[s].p, sizeof(double) * 8 * (size_t)nfeat[s], hipMemcpyDeviceToHost, c->stream));
  MapregSystem S;
  if ((rc = mapreg_eval(c, nfeat, poses_eval ? poses_eval : poses_assoc, true, ground, imu, &S))) return rc;
  memcpy(H, S.H, sizeof(S.H));
  memcpy(g, S.g, sizeof(S.g));
  *cost = S.cost;
  for (int s = 0; s < 4; s++) n_factors[s] = c->h_small->mapreg.n[s];
  return RGC_OK;
}

// ---- f2: rolling local map resident on the device (replaces the keyframe deque + per-frame re-framing + re-upload of
// src/RGC_odometer.cpp:1218-1256, 985-991, 1007) ----------------------------------------------------------------------------
static int map_reserve(rgc_ctx* c, int which, size_t points, bool preserve) {
  DevBuf& b = c->map_store[which];
  const size_t bytes = points * 16;
  if (bytes <= b.cap && b.p) return RGC_OK;
  void* np = nullptr;
  const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
  HIPCHK(c, hipMalloc(&np, want));
  if (b.p) {
    if (preserve && c->map_n) HIPCHK(c, hipMemcpyAsync(np, b.p, c->map_n * 16, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(b.p));
  }
  b.p = np;
  b.cap = want;
  return RGC_OK;
}

int rgc_map_reset(rgc_ctx* c, const double origin[3]) {
  if (!c) return RGC_ERR_INVALID;
  c->map_kf.clear();
  c->map_n = 0;
  c->map_dirty = true;
  c->map_ntarget = 0;
  if (c->map_bound) { c->tgt.ready = false; c->tgt.n = 0; drop_frozen(c); c->map_bound = false; }
  for (int a = 0; a < 3; a++) c->map_origin[a] = origin ? origin[a] : 0.0;
  c->map_rev++;
  return RGC_OK;
}

int rgc_map_insert(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, const double q[4], const double t[3], int on_device, int* keyframe_id) {
  if (!c || !xyzi || !q || !t || n <= 0) return RGC_ERR_INVALID;
  if (stride_bytes < 16 || (stride_bytes & 3) || stride_bytes > 4096) return fail(c, RGC_ERR_INVALID, "a keyframe is x,y,z,intensity: stride_bytes >= 16");
  if (c->map_n + (size_t)n > ((size_t)1 << 27)) return fail(c, RGC_ERR_INVALID, "the map would exceed 2^27 points");
  HIPCHK(c, hipSetDevice(c->device));
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  if ((rc = map_reserve(c, c->map_cur, c->map_n + n, true))) return rc;
  // (the other buffer -- where the first eviction or re-basing compacts to -- grows with it: a first hipMalloc of that size is 9 ms in
  // whichever frame it falls)
  if ((rc = map_reserve(c, c->map_cur ^ 1, c->map_n + n, false))) return rc;
  // surroundingCloud.push_back(transformPointCloud(FullPointsLessFlat, q_w_curr, t_w_curr)) (:1237), relative to the origin
  const double tr[3] = {t[0] - c->map_origin[0], t[1] - c->map_origin[1], t[2] - c->map_origin[2]};
  rgck::transform_q(c->stream, d_in, stride_bytes / 4, n, rgck::Quat{q[0], q[1], q[2], q[3]}, tr, c->map_store[c->map_cur].as<float>() + 4 * c->map_n, 4);
  if (!on_device) HIPCHK(c, hipStreamSynchronize(c->stream));  // pre_in is re-used by the next staged call
  HIPCHK(c, hipGetLastError());
  rgc_ctx::MapKf kf{c->map_next_id++, c->map_n, n, {t[0], t[1], t[2]}};
  c->map_kf.push_back(kf);
  c->map_n += n;
  c->map_dirty = true;
  c->map_rev++;
  if (keyframe_id) *keyframe_id = kf.id;
  return RGC_OK;
}

int rgc_map_evict(rgc_ctx* c, int max_keyframes, const double center[3], double radius, int* n_evicted) {
  if (!c) return RGC_ERR_INVALID;
  if (n_evicted) *n_evicted = 0;
  std::vector<rgc_ctx::MapKf> keep;
  for (const auto& k : c->map_kf) {
    bool far = false;
    if (center && radius > 0 && &k != &c->map_kf.back()) {  // the newest keyframe always stays: an empty map cannot be committed
      const double dx = k.t[0] - center[0], dy = k.t[1] - center[1], dz = k.t[2] - center[2];
      far = std::sqrt(dx * dx + dy * dy + dz * dz) > radius;
    }
    if (!far) keep.push_back(k);
  }
  if (max_keyframes > 0 && (int)keep.size() > max_keyframes) keep.erase(keep.begin(), keep.end() - max_keyframes);  // pop_front, :1242-1247
  const int gone = (int)c->map_kf.size() - (int)keep.size();
  if (!gone) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  size_t total = 0;
  for (const auto& k : keep) total += k.n;
  const int other = c->map_cur ^ 1;
  int rc = map_reserve(c, other, std::max(total, (size_t)1), false);
  if (rc) return rc;
  size_t off = 0;
  for (size_t i = 0; i < keep.size();) {  // runs of surviving neighbours move with one copy
    size_t j = i, run = 0;
    const size_t base = keep[i].off;
    while (j < keep.size() && keep[j].off == base + run) { run += keep[j].n; j++; }
    HIPCHK(c, hipMemcpyAsync(c->map_store[other].as<char>() + off * 16, c->map_store[c->map_cur].as<const char>() + base * 16, run * 16,
                             hipMemcpyDeviceToDevice, c->stream));
    for (size_t k = i; k < j; k++) keep[k].off = off + (keep[k].off - base);
    off += run;
    i = j;
  }
  c->map_cur = other;
  c->map_kf.swap(keep);
  c->map_n = total;
  c->map_dirty = true;
  c->map_rev++;
  if (n_evicted) *n_evicted = gone;
  return RGC_OK;
}

int rgc_map_rebase(rgc_ctx* c, const double new_origin[3]) {
  if (!c || !new_origin) return RGC_ERR_INVALID;
  const double d[3] = {c->map_origin[0] - new_origin[0], c->map_origin[1] - new_origin[1], c->map_origin[2] - new_origin[2]};
  if (c->map_n) {
    HIPCHK(c, hipSetDevice(c->device));
    const int other = c->map_cur ^ 1;
    int rc = map_reserve(c, other, c->map_n, false);
    if (rc) return rc;
    rgck::transform_q(c->stream, c->map_store[c->map_cur].as<const float>(), 4, (int)c->map_n, rgck::Quat{0, 0, 0, 1}, d, c->map_store[other].as<float>(), 4);
    HIPCHK(c, hipGetLastError());
    c->map_cur = other;
  }
  for (int a = 0; a < 3; a++) c->map_origin[a] = new_origin[a];
  c->map_dirty = true;
  c->map_rev++;
  if (c->map_bound) {  // the committed target is in the OLD origin's coordinates: an align before the next rgc_map_commit must fail, not drift
    c->tgt.ready = false;
    drop_frozen(c);
  }
  return RGC_OK;
}

int rgc_map_commit(rgc_ctx* c, float leaf, int* n_target) {
  if (!c || !(leaf > 0.f)) return RGC_ERR_INVALID;
  if (c->map_bound && !c->map_dirty && leaf == c->map_leaf && c->tgt.ready) {  // nothing changed: the resident target stands
    if (n_target) *n_target = c->map_ntarget;
    return RGC_OK;
  }
  // (before anything is written: the filter below writes the buffer the resident target was set from -- a commit refused behind it would
  // leave a set target whose input has been overwritten, and rgc_map_download(1) returning another cloud; tests/fuzz/fuzz_api.py)
  if (solve_in_flight(c)) return fail(c, RGC_ERR_INVALID, "a solve is in flight on this context: call rgc_align_end first");
  if (!c->map_n) return fail(c, RGC_ERR_NO_INPUT, "the map holds no keyframe");
  int rc = ensure(c, c->map_target, c->map_n * 16);
  if (rc) return rc;
  int nt = 0;
  // downSizeFilter2.setInputCloud(laserCloudsubmap); filter (:985-991) -- on the resident store, nothing crosses PCIe
  if (c->map_bound) {  // from here on the buffer no longer holds the cloud the bound target was set from: whatever fails below, that target goes
    c->map_bound = false;
    c->tgt.ready = false; c->tgt.n = 0; drop_frozen(c);
  }
  if ((rc = rgc_voxelgrid(c, c->map_store[c->map_cur].as<const float>(), (int)c->map_n, 16, leaf, c->map_target.as<float>(), &nt, 1))) return rc;
  // setInputTarget (:1007): grid, exact-kNN covariances, Gaussian voxel map
  if ((rc = set_cloud(c, c->tgt, true, c->map_target.as<const float>(), nt, 16, true))) return rc;
  c->map_bound = true;
  c->map_dirty = false;
  c->map_leaf = leaf;
  c->map_ntarget = nt;
  if (n_target) *n_target = nt;
  return RGC_OK;
}

int rgc_map_get_info(rgc_ctx* c, rgc_map_info* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  out->n_keyframes = (int)c->map_kf.size();
  out->n_points = (long long)c->map_n;
  out->n_target = c->map_bound && !c->map_dirty ? c->map_ntarget : -1;
  out->revision = c->map_rev;
  out->oldest_id = c->map_kf.empty() ? -1 : c->map_kf.front().id;
  out->newest_id = c->map_kf.empty() ? -1 : c->map_kf.back().id;
  for (int a = 0; a < 3; a++) out->origin[a] = c->map_origin[a];
  return RGC_OK;
}

int rgc_map_download(rgc_ctx* c, int which, float* out_xyzi, int cap, int* n) {
  if (!c || !n || cap < 0 || (cap && !out_xyzi)) return RGC_ERR_INVALID;
  const void* src = nullptr;
  int have = 0;
  if (which == 0) { src = c->map_store[c->map_cur].p; have = (int)c->map_n; }
  else if (which == 1) {
    if (!c->map_bound || c->map_dirty) return fail(c, RGC_ERR_NO_INPUT, "rgc_map_commit first");
    src = c->map_target.p; have = c->map_ntarget;
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

// ---- f3: PointCloud2 <-> device arrays ---------------------------------------------------------------------------------
int rgc_pc2_unpack(rgc_ctx* c, const void* data, int n, const rgc_pc2_layout* L, float* xyzi_out, int* ring_out, float* time_out,
                   int out_on_device) {
  if (!c || !data || !L || !xyzi_out || n < 0) return RGC_ERR_INVALID;
  if (L->point_step <= 0) return fail(c, RGC_ERR_INVALID, "point_step must be positive");
  if (n > (1 << 24)) return fail(c, RGC_ERR_INVALID, "message has %d points, the limit is 2^24", n);
  rgck::Pc2Layout K{};
  K.point_step = L->point_step;
  K.big_endian = L->is_bigendian ? 1 : 0;
  for (int f = 0; f < 6; f++) {
    int off = L->offset[f], ty = L->datatype[f];
    if (off >= 0) {
      if (ty < 1 || ty > 8) return fail(c, RGC_ERR_INVALID, "field %d: unknown PointField datatype %d", f, ty);
      const int size = (ty == 1 || ty == 2) ? 1 : (ty == 3 || ty == 4) ? 2 : (ty == 8 ? 8 : 4);
      if (off + size > L->point_step) return fail(c, RGC_ERR_INVALID, "field %d runs past point_step", f);
      // fromROSMsg<PointXYZI> maps x, y, z, intensity only from FLOAT32 fields (a mismatching datatype leaves the default)
      if (L->strict && f < 4 && ty != 7) off = -1;
    }
    K.off[f] = off;
    K.type[f] = ty;
  }
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t bytes = (size_t)n * L->point_step;
  int rc;
  if ((rc = ensure(c, c->pre_in, bytes))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->pre_in.p, data, bytes, hipMemcpyHostToDevice, s));
  float4* d_xyzi;
  int* d_ring = nullptr;
  float* d_time = nullptr;
  if (out_on_device) {
    d_xyzi = (float4*)xyzi_out; d_ring = ring_out; d_time = time_out;
  } else {
    if ((rc = ensure(c, c->pre_out, (size_t)n * 24))) return rc;
    d_xyzi = c->pre_out.as<float4>();
    if (ring_out) d_ring = (int*)(c->pre_out.as<char>() + (size_t)n * 16);
    if (time_out) d_time = (float*)(c->pre_out.as<char>() + (size_t)n * 20);
  }
  rgck::pc2_unpack(s, c->pre_in.as<const unsigned char>(), n, K, d_xyzi, d_ring, d_time);
  if (!out_on_device) {
    HIPCHK(c, hipMemcpyAsync(xyzi_out, d_xyzi, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    if (ring_out) HIPCHK(c, hipMemcpyAsync(ring_out, d_ring, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (time_out) HIPCHK(c, hipMemcpyAsync(time_out, d_time, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

int rgc_pc2_pack(rgc_ctx* c, int kind, const float* in, int n, int in_on_device, void* data_out) {
  if (!c || !in || !data_out || n < 0 || n > (1 << 24) || (kind != 0 && kind != 1)) return RGC_ERR_INVALID;   // (a message of more than 2^24 points: rgc_pc2_unpack's limit)
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int cols = kind == 0 ? 4 : 5, step = kind == 0 ? 32 : 48;
  const float* d_in;
  int rc = stage_in(c, in, n, cols * 4, in_on_device, &d_in);
  if (rc) return rc;
  if ((rc = ensure(c, c->pre_out, (size_t)n * step))) return rc;
  rgck::pc2_pack(c->stream, d_in, cols, n, kind, c->pre_out.as<unsigned char>());
  HIPCHK(c, hipMemcpyAsync(data_out, c->pre_out.p, (size_t)n * step, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// ---- f4: loop-closure ICP (pcl::IterativeClosestPoint as configured at RGC_mapping.cpp:2050-2069) -----------------------------
// R, t minimising sum |R p + t - q|^2 from n, sum p, sum q, sum p q^T (TransformationEstimationSVD = Umeyama without scale): SVD of
// the centred correlation through the eigen decomposition of H^T H
static void rigid_from_sums(double n, const double sp[3], const double sq[3], const double spq[9], double R[9], double t[3]) {
  double cp[3], cq[3], H[9];
  for (int a = 0; a < 3; a++) { cp[a] = sp[a] / n; cq[a] = sq[a] / n; }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) H[a * 3 + b] = spq[a * 3 + b] - n * cp[a] * cq[b];
  double HtH[9] = {0};
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      for (int k = 0; k < 3; k++) HtH[a * 3 + b] += H[k * 3 + a] * H[k * 3 + b];
  const double S6[6] = {HtH[0], 0.5 * (HtH[1] + HtH[3]), 0.5 * (HtH[2] + HtH[6]), HtH[4], 0.5 * (HtH[5] + HtH[7]), HtH[8]};
  double ev[3], Va[9], V[9];
  host_eig3_sym(S6, ev, Va);  // ascending
  for (int a = 0; a < 3; a++) { V[a * 3 + 0] = Va[a * 3 + 2]; V[a * 3 + 1] = Va[a * 3 + 1]; V[a * 3 + 2] = Va[a * 3 + 0]; }  // descending
  double U[9];
  double s0 = 0.0;  // the largest singular value, |H v0|
  for (int j = 0; j < 2; j++) {
    double w[3] = {0, 0, 0};
    for (int a = 0; a < 3; a++)
      for (int k = 0; k < 3; k++) w[a] += H[a * 3 + k] * V[k * 3 + j];
    double nn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (j == 0) s0 = nn;
    // rank deficient: any unit vector orthogonal to the previous column.  The second singular value is judged RELATIVE to the first: of a
    // rank-1 correlation (a target of two points, a kept set on one line) H v1 is rounding noise of the sums, not 0, and normalising
    // that noise gave a U that was not orthogonal (det R = 0.9976 on a 2-point target).  Singular values that come from the
    // eigenvalues of H^T H are known to ~1.5e-8 of the largest, so below 1e-6 of it the direction is not information.
    if (!(nn > 1e-300) || (j == 1 && !(nn > 1e-6 * s0))) {
      if (j == 0) { w[0] = 1; w[1] = 0; w[2] = 0; }
      else {
        const double a0 = std::fabs(U[0]), a1 = std::fabs(U[3]), a2 = std::fabs(U[6]);
        double e[3] = {a0 <= a1 && a0 <= a2 ? 1.0 : 0.0, a1 < a0 && a1 <= a2 ? 1.0 : 0.0, 0.0};
        if (e[0] == 0.0 && e[1] == 0.0) e[2] = 1.0;
        w[0] = U[3] * e[2] - U[6] * e[1]; w[1] = U[6] * e[0] - U[0] * e[2]; w[2] = U[0] * e[1] - U[3] * e[0];
      }
      nn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    }
    for (int a = 0; a < 3; a++) U[a * 3 + j] = w[a] / nn;
  }
  // right-handed completions: R = [v0 v1 v0xv1] [u0 u1 u0xu1]^T is the proper rotation V diag(1, 1, det) U^T
  U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
  V[2] = V[3] * V[7] - V[6] * V[4]; V[5] = V[6] * V[1] - V[0] * V[7]; V[8] = V[0] * V[4] - V[3] * V[1];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double v = 0;
      for (int k = 0; k < 3; k++) v += V[a * 3 + k] * U[b * 3 + k];
      R[a * 3 + b] = v;
    }
  for (int a = 0; a < 3; a++) t[a] = cq[a] - (R[a * 3] * cp[0] + R[a * 3 + 1] * cp[1] + R[a * 3 + 2] * cp[2]);
}

void rgc_default_icp_params(rgc_icp_params* p) {
  if (!p) return;
  p->max_iterations = 100;                    // :2053
  p->max_correspondence_distance = 10.0;      // poseGraphSearchRadius * 2 with historyKeyframeSearchRadius = 5 (:155, :2052)
  p->transformation_epsilon = 1e-6;           // :2054
  p->euclidean_fitness_epsilon = 1e-6;        // :2055
}

// rgc_icp_align / rgc_icp_align_device: one body; on_device: source and target are read where they lie instead of being uploaded first
static int icp_align_impl(rgc_ctx* c, const float* source, int ns, const float* target, int nt, int stride_bytes, const rgc_icp_params* prm,
                          float final_T[16], rgc_icp_result* res, bool on_device) {
  if (!c || !source || !target || !prm || !final_T || !res) return RGC_ERR_INVALID;
  if (!stride_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (ns < 1 || nt < 1) return fail(c, RGC_ERR_TOO_FEW_POINTS, "ICP needs a non-empty source and target");
  if (ns > (1 << 27) || nt > (1 << 27)) return fail(c, RGC_ERR_INVALID, "cloud larger than 2^27 points");
  if (!(prm->max_correspondence_distance > 0) || prm->max_iterations < 1) return fail(c, RGC_ERR_INVALID, "bad ICP parameters");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  memset(res, 0, sizeof(*res));
  int rc;
  // target grid (icp.setInputTarget builds a kd-tree, :2066)
  Cloud& tg = c->aux;
  tg.ready = false;
  {
    const size_t bytes = (size_t)nt * stride_bytes;
    if (on_device) {
      if ((rc = check_device_range(c, target, bytes - (stride_bytes - 12), "rgc_icp_align_device: target"))) return rc;
      tg.in = target;
    } else {
      if ((rc = ensure(c, tg.in_copy, bytes))) return rc;
      HIPCHK(c, hipMemcpyAsync(tg.in_copy.p, target, bytes - (stride_bytes - 12), hipMemcpyHostToDevice, s));
      tg.in = tg.in_copy.as<const float>();
    }
    tg.stride_f = stride_bytes / 4;
    tg.n = nt;
    if ((rc = prepare_map_grid(c, tg, 1.0))) return rc;
  }
  // the source as float4, transformed in place every iteration (pcl::transformPointCloud, fp32)
  const float* d_src;
  if ((rc = stage_in(c, source, ns, stride_bytes, on_device ? 1 : 0, &d_src))) return rc;  // the raw source, kept for the fitness score
  if ((rc = ensure(c, c->pre_out, sizeof(float4) * (size_t)ns))) return rc;
  float4* cur = c->pre_out.as<float4>();
  const rgck::PoseF I{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  rgck::transform_f32(s, d_src, stride_bytes / 4, ns, I, (float*)cur, 4);  // identity guess: a plain copy to 16-byte points
  const int nb = rgck::linearize_blocks(ns);
  if ((rc = ensure(c, c->partials, sizeof(double) * (rgck::kAccum + 2) * (size_t)(nb > 0 ? nb : 1)))) return rc;
  float fin[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double rot_thr = 1.0 - prm->transformation_epsilon, trans_thr = prm->transformation_epsilon;
  double prev_mse = DBL_MAX;
  for (;;) {
    rgck::icp_accumulate(s, cur, ns, tg.sorted(), prm->max_correspondence_distance, c->partials.as<double>(), c->d_out);
    HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double) * 17, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    const double* S = c->h_out;
    const double cnt = S[0];
    res->n_correspondences = (int)cnt;
    if (cnt < 3) { res->converged = 0; res->state = RGC_ICP_NO_CORRESPONDENCES; break; }  // min_number_correspondences_
    double R[9], t[3];
    rigid_from_sums(cnt, S + 1, S + 4, S + 7, R, t);
    float T[16] = {(float)R[0], (float)R[1], (float)R[2], (float)t[0], (float)R[3], (float)R[4], (float)R[5], (float)t[1],
                   (float)R[6], (float)R[7], (float)R[8], (float)t[2], 0, 0, 0, 1};
    rgck::transform_f32(s, (const float*)cur, 4, ns, posef_from(T), (float*)cur, 4);
    float nf[16];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        float v = 0.0f;
        for (int k = 0; k < 4; k++) v += T[i * 4 + k] * fin[k * 4 + j];
        nf[i * 4 + j] = v;
      }
    memcpy(fin, nf, sizeof(fin));
    res->iterations++;
    // DefaultConvergenceCriteria::hasConverged [3P-memory]
    if (res->iterations >= prm->max_iterations) { res->converged = 1; res->state = RGC_ICP_ITERATIONS; break; }
    const double cos_angle = 0.5 * ((double)T[0] + (double)T[5] + (double)T[10] - 1.0);
    const double tr2 = (double)T[3] * T[3] + (double)T[7] * T[7] + (double)T[11] * T[11];
    if (cos_angle >= rot_thr && tr2 <= trans_thr) { res->converged = 1; res->state = RGC_ICP_TRANSFORM; break; }
    const double mse = S[16] / cnt;
    if (std::fabs(mse - prev_mse) < 1e-12) { res->converged = 1; res->state = RGC_ICP_ABS_MSE; break; }
    if (std::fabs(mse - prev_mse) / prev_mse < prm->euclidean_fitness_epsilon) { res->converged = 1; res->state = RGC_ICP_REL_MSE; break; }
    prev_mse = mse;
  }
  // getFitnessScore(): the ORIGINAL source through the final transformation (fp32), mean squared 1-NN distance
  rgck::transform_f32(s, d_src, stride_bytes / 4, ns, posef_from(fin), (float*)cur, 4);
  if ((rc = ensure(c, c->fit_partials, sizeof(double) * (size_t)rgck::fitness_blocks(ns) + 64))) return rc;
  rgck::fitness(s, cur, ns, I, tg.sorted(), c->fit_partials.as<double>(), c->d_out);
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  res->fitness = c->h_out[0] / (double)ns;
  memcpy(final_T, fin, sizeof(fin));
  return RGC_OK;
}
int rgc_icp_align(rgc_ctx* c, const float* source, int ns, const float* target, int nt, int stride_bytes, const rgc_icp_params* prm,
                  float final_T[16], rgc_icp_result* res) {
  return icp_align_impl(c, source, ns, target, nt, stride_bytes, prm, final_T, res, false);
}
int rgc_icp_align_device(rgc_ctx* c, const float* d_source, int ns, const float* d_target, int nt, int stride_bytes, const rgc_icp_params* prm,
                         float final_T[16], rgc_icp_result* res) {
  return icp_align_impl(c, d_source, ns, d_target, nt, stride_bytes, prm, final_T, res, true);
}

// ---- f5: the mapping node's keyframe store with batched sub-map assembly (src/RGC_mapping.cpp:1503-1616, 2180-2216, 2508-2537) ----------
static bool kf_pose_finite(const rgc_kf_pose& p) {
  return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::isfinite(p.roll) && std::isfinite(p.pitch) && std::isfinite(p.yaw);
}

// room for `points` 16-byte points of one kind; the content held so far moves along (like map_reserve)
static int kf_reserve(rgc_ctx* c, int kind, size_t points) {
  DevBuf& b = c->kf_store[kind];
  const size_t bytes = points * 16;
  if (bytes <= b.cap && b.p) return RGC_OK;
  void* np = nullptr;
  const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
  HIPCHK(c, hipMalloc(&np, want));
  if (b.p) {
    if (c->kf_n[kind]) HIPCHK(c, hipMemcpyAsync(np, b.p, c->kf_n[kind] * 16, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(b.p));
  }
  b.p = np;
  b.cap = want;
  return RGC_OK;
}

int rgc_kf_reset(rgc_ctx* c) {
  if (!c) return RGC_ERR_INVALID;
  if (!c->kf.empty()) c->kf_rev++;
  c->kf.clear();
  c->kf_index.clear();
  for (int k = 0; k < RGC_KF_KINDS; k++) c->kf_n[k] = 0;
  return RGC_OK;
}

int rgc_kf_push(rgc_ctx* c, int id, const rgc_kf_pose* pose, const float* corner, int n_corner, const float* surf, int n_surf, const float* scan,
                int n_scan, int stride_bytes, int on_device) {
  if (!c || !pose || n_corner < 0 || n_surf < 0 || n_scan < 0) return RGC_ERR_INVALID;
  if ((n_corner && !corner) || (n_surf && !surf) || (n_scan && !scan)) return fail(c, RGC_ERR_INVALID, "rgc_kf_push: a cloud with points and no pointer");
  if (stride_bytes < 16 || (stride_bytes & 3) || stride_bytes > 4096) return fail(c, RGC_ERR_INVALID, "a keyframe point is x,y,z,c: stride_bytes >= 16");
  if (!kf_pose_finite(*pose)) return fail(c, RGC_ERR_NONFINITE, "rgc_kf_push: the key pose is not finite");
  if (c->kf_index.count(id)) return fail(c, RGC_ERR_INVALID, "rgc_kf_push: keyframe %d is in the store already", id);
  const float* src[RGC_KF_KINDS] = {corner, surf, scan};
  const int n[RGC_KF_KINDS] = {n_corner, n_surf, n_scan};
  for (int k = 0; k < RGC_KF_KINDS; k++)
    if ((unsigned long long)c->kf_n[k] + (unsigned long long)n[k] > (1ull << 27)) return fail(c, RGC_ERR_INVALID, "the keyframe store would exceed 2^27 points of kind %d", k);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  for (int k = 0; k < RGC_KF_KINDS; k++) {
    if (!n[k]) continue;
    if (on_device && (rc = check_device_range(c, src[k], (size_t)n[k] * stride_bytes - (stride_bytes - 16), "rgc_kf_push: cloud"))) return rc;
    if ((rc = kf_reserve(c, k, c->kf_n[k] + n[k]))) return rc;
  }
  rgc_ctx::KfRec rec{};
  rec.id = id;
  rec.pose = *pose;
  rgc_host_key_pose_quat(pose->roll, pose->pitch, pose->yaw, rec.q);
  // travel_distance / travel_angle (:1887-1908), fp32, against the pose stored NOW for the previous position (cloudKeyPoses6D->back(), corrected or
  // not); never recomputed afterwards
  if (!c->kf.empty()) {
    const rgc_ctx::KfRec& last = c->kf.back();
    const float dx = pose->x - last.pose.x, dy = pose->y - last.pose.y, dz = pose->z - last.pose.z;
    rec.travel = last.travel + sqrtf((dx * dx + dy * dy) + dz * dz);
    float rad_delta = pose->yaw - last.pose.yaw;
    if (rad_delta > M_PI) rad_delta = rad_delta - M_PI * 2;    // (float op double: in double, stored as float, :1904-1905)
    if (rad_delta < -M_PI) rad_delta = rad_delta + M_PI * 2;
    rec.travel_angle = last.travel_angle + fabsf(rad_delta);
  }
  bool copied = false;
  for (int k = 0; k < RGC_KF_KINDS; k++) {
    rec.off[k] = c->kf_n[k];
    rec.n[k] = n[k];
    if (!n[k]) continue;
    char* dst = c->kf_store[k].as<char>() + c->kf_n[k] * 16;
    const hipMemcpyKind dir = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (stride_bytes == 16) HIPCHK(c, hipMemcpyAsync(dst, src[k], (size_t)n[k] * 16, dir, c->stream));
    else HIPCHK(c, hipMemcpy2DAsync(dst, 16, src[k], (size_t)stride_bytes, 16, (size_t)n[k], dir, c->stream));
    copied = true;
  }
  if (copied && !on_device) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's host buffers are the caller's again on return
  for (int k = 0; k < RGC_KF_KINDS; k++) c->kf_n[k] += n[k];
  c->kf_index[id] = (int)c->kf.size();
  c->kf.push_back(rec);
  c->kf_rev++;
  return RGC_OK;
}

int rgc_kf_set_poses(rgc_ctx* c, const int* ids, const rgc_kf_pose* poses, int n) {
  if (!c || n < 0 || (n && (!ids || !poses))) return RGC_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    if (!c->kf_index.count(ids[i])) return fail(c, RGC_ERR_INVALID, "rgc_kf_set_poses: keyframe %d is not in the store", ids[i]);
    if (!kf_pose_finite(poses[i])) return fail(c, RGC_ERR_NONFINITE, "rgc_kf_set_poses: the pose of keyframe %d is not finite", ids[i]);
  }
  for (int i = 0; i < n; i++) {
    rgc_ctx::KfRec& r = c->kf[c->kf_index[ids[i]]];
    r.pose = poses[i];
    rgc_host_key_pose_quat(poses[i].roll, poses[i].pitch, poses[i].yaw, r.q);
  }
  if (n) c->kf_rev++;
  return RGC_OK;
}

int rgc_kf_get_info(rgc_ctx* c, rgc_kf_info* out) {
  if (!c || !out) return RGC_ERR_INVALID;
  out->n_keyframes = (int)c->kf.size();
  for (int k = 0; k < RGC_KF_KINDS; k++) out->n_points[k] = (long long)c->kf_n[k];
  out->revision = c->kf_rev;
  return RGC_OK;
}

int rgc_kf_get_travel(rgc_ctx* c, const int* ids, int n, float* distance, float* angle) {
  if (!c || n < 0 || (n && !ids)) return RGC_ERR_INVALID;
  for (int i = 0; i < n; i++)
    if (!c->kf_index.count(ids[i])) return fail(c, RGC_ERR_INVALID, "rgc_kf_get_travel: keyframe %d is not in the store", ids[i]);
  for (int i = 0; i < n; i++) {
    const rgc_ctx::KfRec& r = c->kf[c->kf_index[ids[i]]];
    if (distance) distance[i] = r.travel;
    if (angle) angle[i] = r.travel_angle;
  }
  return RGC_OK;
}

}  // extern "C"

// ---- the selections: which keyframes to assemble (extractSurroundingKeyFramesAndMap :1525-1548, detectLoopClosure :2141-2225, publishGlobalMap
// :2493-2505).  One gate launch over the device mirror of the key positions, then UniformSampling's chain or a 64-bit minimum. ----
static int kf_mirror(rgc_ctx* c) {   // the mirror holds the store's current revision on return
  const size_t n = c->kf.size();
  if (c->kf_mirror_rev == c->kf_rev && c->kf_pos.p) return RGC_OK;
  int rc;
  if ((rc = ensure(c, c->kf_pos, 16 * n)) || (rc = ensure(c, c->kf_travel, 4 * n)) || (rc = ensure(c, c->kf_ids, 4 * n))) return rc;
  std::vector<float> hp(4 * n), ht(n);
  std::vector<int> hi(n);
  for (size_t p = 0; p < n; p++) {
    const rgc_ctx::KfRec& r = c->kf[p];
    const int pi = (int)p;
    hp[4 * p] = r.pose.x; hp[4 * p + 1] = r.pose.y; hp[4 * p + 2] = r.pose.z;
    memcpy(&hp[4 * p + 3], &pi, 4);   // the position's bits: the fourth float is only ever copied
    ht[p] = r.travel;
    hi[p] = r.id;
  }
  HIPCHK(c, hipMemcpyAsync(c->kf_pos.p, hp.data(), 16 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->kf_travel.p, ht.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->kf_ids.p, hi.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->kf_mirror_rev = c->kf_rev;
  return RGC_OK;
}
// the gate of every selection: r2 = (float)((double)radius * (double)radius), inside when dist2 < r2 (strict)
static float kf_gate_r2(float radius) { return (float)((double)radius * (double)radius); }
// gate launch over the mirror; small4 <- {number inside, 0, the loop search's minimum (two words)}.  flags: the in-radius flags are kept for a compaction
static int kf_run_gate(rgc_ctx* c, const float q[3], float r2, int loop, float travel_last, float thr, int min_id, bool flags, unsigned small4[4]) {
  const int n = (int)c->kf.size();
  int rc;
  if ((rc = ensure(c, c->kf_small, 16))) return rc;
  if (flags && (rc = ensure(c, c->kf_flag, 4 * (size_t)n))) return rc;
  const unsigned init[4] = {0u, 0u, ~0u, ~0u};
  HIPCHK(c, hipMemcpyAsync(c->kf_small.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  rgck::kf_gate(c->stream, c->kf_pos.as<const float4>(), c->kf_travel.as<const float>(), c->kf_ids.as<const int>(), n, q, r2, loop, travel_last, thr, min_id,
                flags ? c->kf_flag.as<int>() : nullptr, c->kf_small.as<unsigned>());
  HIPCHK(c, hipMemcpyAsync(small4, c->kf_small.p, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}
// UniformSampling of m device points {x, y, z, position} at leaf `density`; the winners' ids in ascending leaf index
static int kf_sample_ids(rgc_ctx* c, const float* d_pts, int m, float density, int* out_ids, int cap, int* n_out, const char* who) {
  int rc;
  if ((rc = ensure(c, c->kf_sel_out, 16 * (size_t)m))) return rc;
  rgc_vg_route rt{};
  rt.n = m;
  int no = 0;
  rc = voxelgrid_run(c, d_pts, m, 16, density, c->kf_sel_out.as<float>(), &no, 1, rt, rgck::kVgModePick, nullptr);
  rt.status = rc;
  rt.n_out = no;
  c->vg_route = rt;
  if (rc) return rc;
  *n_out = no;
  if (no > cap) return fail(c, RGC_ERR_INVALID, "%s: %d keyframes selected, room for %d", who, no, cap);
  std::vector<float> h(4 * (size_t)no);
  if (no) HIPCHK(c, hipMemcpyAsync(h.data(), c->kf_sel_out.p, 16 * (size_t)no, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < no; j++) {
    int p;
    memcpy(&p, &h[4 * (size_t)j + 3], 4);
    if (p < 0 || p >= (int)c->kf.size()) return fail(c, RGC_ERR_HIP, "%s: the sampling returned position %d of %d", who, p, (int)c->kf.size());
    out_ids[j] = c->kf[p].id;
  }
  return RGC_OK;
}

extern "C" {

int rgc_kf_select_surrounding(rgc_ctx* c, const float center[3], float radius, float density, int* out_ids, int cap, int* n_in_radius, int* n_out) {
  if (!c || !center || !n_in_radius || !n_out || cap < 0 || (cap && !out_ids)) return RGC_ERR_INVALID;
  *n_in_radius = *n_out = 0;
  if (!std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2]) || !std::isfinite(radius) || !std::isfinite(density) || !(radius > 0.f) ||
      !(density > 0.f))
    return fail(c, RGC_ERR_INVALID, "rgc_kf_select_surrounding: the centre, radius > 0 and density > 0 must be finite");
  const int n = (int)c->kf.size();
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = kf_mirror(c))) return rc;
  unsigned small4[4];
  if ((rc = kf_run_gate(c, center, kf_gate_r2(radius), 0, 0.f, 0.f, 0, true, small4))) return rc;
  const int m = (int)small4[0];
  *n_in_radius = m;
  if (m == 0) { rgc_vg_route rt{}; c->vg_route = rt; return RGC_OK; }
  if ((rc = ensure(c, c->kf_scan, 4 * (size_t)n)) || (rc = ensure(c, c->kf_bsum, 4 * ((size_t)n / 2048 + 2))) || (rc = ensure(c, c->kf_sel, 16 * (size_t)m))) return rc;
  rgck::exclusive_scan(c->stream, c->kf_flag.as<const int>(), c->kf_scan.as<int>(), n, c->kf_bsum.as<int>());
  rgck::kf_compact(c->stream, c->kf_pos.as<const float4>(), c->kf_flag.as<const int>(), c->kf_scan.as<const int>(), n, c->kf_sel.as<float4>());
  HIPCHK(c, hipGetLastError());
  return kf_sample_ids(c, c->kf_sel.as<const float>(), m, density, out_ids, cap, n_out, "rgc_kf_select_surrounding");
}

int rgc_kf_select_global(rgc_ctx* c, float pose_density, int* out_ids, int cap, int* n_out) {
  if (!c || !n_out || cap < 0 || (cap && !out_ids)) return RGC_ERR_INVALID;
  *n_out = 0;
  if (!std::isfinite(pose_density) || !(pose_density > 0.f)) return fail(c, RGC_ERR_INVALID, "rgc_kf_select_global: the density must be finite and > 0");
  const int n = (int)c->kf.size();
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = kf_mirror(c))) return rc;
  return kf_sample_ids(c, c->kf_pos.as<const float>(), n, pose_density, out_ids, cap, n_out, "rgc_kf_select_global");
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
  const int n = (int)c->kf.size();
  if (n == 0) return RGC_OK;
  const int L = n - 1;
  const rgc_ctx::KfRec& last = c->kf[L];
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
  const rgc_ctx::KfRec& cl = c->kf[pc];
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
      const rgc_ctx::KfRec& r = c->kf[(size_t)p];
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
    const auto it = c->kf_index.find(ids[i]);
    if (it == c->kf_index.end()) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: keyframe %d is not in the store", ids[i]);
    const rgc_ctx::KfRec& r = c->kf[it->second];
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
    if (filter) { rgc_vg_route rt{}; c->vg_route = rt; }
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
    if ((rc = ensure(c, c->kf_raw, (size_t)nr * 16))) return rc;
    d_raw = c->kf_raw.as<float4>();
  }
  // the segment table through pinned staging: [nseg segments][nseg + 1 first workgroups]
  const size_t seg_bytes = nseg * sizeof(rgck::KfSegment), tab_bytes = seg_bytes + (nseg + 1) * sizeof(int);
  if (c->kf_upload_pending) { HIPCHK(c, hipEventSynchronize(c->kf_uploaded)); c->kf_upload_pending = false; }
  if (tab_bytes > c->kf_h_cap) {
    if (c->kf_h_table) { HIPCHK(c, hipHostFree(c->kf_h_table)); c->kf_h_table = nullptr; c->kf_h_cap = 0; }
    const size_t want = tab_bytes + tab_bytes / 2 + 4096;
    HIPCHK(c, hipHostMalloc((void**)&c->kf_h_table, want, hipHostMallocDefault));
    c->kf_h_cap = want;
  }
  if ((rc = ensure(c, c->kf_table, tab_bytes))) return rc;
  rgck::KfSegment* hs = (rgck::KfSegment*)c->kf_h_table;
  int* hb = (int*)(c->kf_h_table + seg_bytes);
  size_t si = 0;
  int out0 = 0, b0 = 0;
  for (int i = 0; i < n_ids; i++) {
    const rgc_ctx::KfRec& r = c->kf[c->kf_index.find(ids[i])->second];
    for (int k = 0; k < RGC_KF_KINDS; k++) {
      if (!((kind_mask >> k) & 1u) || !r.n[k]) continue;
      rgck::KfSegment& S = hs[si];
      S.src = c->kf_store[k].as<const float4>() + r.off[k];
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
  HIPCHK(c, hipMemcpyAsync(c->kf_table.p, c->kf_h_table, tab_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->kf_uploaded, s));
  c->kf_upload_pending = true;
  if (c->main_has_target_prep && map_prep_finished(c)) c->main_has_target_prep = false;  // it has drained
  rgck::kf_assemble(s, c->kf_table.as<const rgck::KfSegment>(), (const int*)(c->kf_table.as<const char>() + seg_bytes), (int)nseg, (int)blocks, d_raw);
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
    if ((rc = ensure(c, c->kf_filt, (size_t)nr * 16))) return rc;
    d_f = c->kf_filt.as<float>();
  }
  rgc_vg_route rt{};
  rt.n = nr;
  int no = 0;
  rc = voxelgrid_run(c, (const float*)d_raw, nr, 16, leaf, d_f, &no, 1, rt);
  rt.status = rc;
  rt.n_out = no;
  c->vg_route = rt;
  if (rc) return rc;
  *n_out = no;
  if (direct) return RGC_OK;
  if (no > cap) return fail(c, RGC_ERR_INVALID, "rgc_kf_assemble: %d points after the filter, room for %d", no, cap);
  if (no > 0) HIPCHK(c, hipMemcpyAsync(out_xyzc, d_f, (size_t)no * 16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (!on_device) HIPCHK(c, hipStreamSynchronize(s));
  return RGC_OK;
}

}  // extern "C"
