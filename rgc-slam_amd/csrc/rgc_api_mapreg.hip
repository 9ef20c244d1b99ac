// rgc_api_mapreg.hip -- host side of f1, rgc_mapreg_*: the mapping node's scan-to-map FEATURE registration (RGC_mapping.cpp:1069-1358) -- the grid of a
// feature map (bbox -> counting sort; no covariances), the association, the host side of the robust LM.  The kernels are in rgc_kernels.hip.
#include "rgc_ctx.h"

using namespace rgcapi;

namespace {

// grid cell of a feature map = the largest 5th-neighbour distance that still yields a factor (1 m for edges :1098, sqrt(2) m for
// planes :1200): the 3x3x3 block of cells then proves every accepted neighbourhood, and holds as few candidates as possible
constexpr double kMapregCell[2] = {1.0, 1.4143};

int prepare_map_grid(rgc_ctx* c, Cloud& cl, double cell) {
  int rc, hsm[8];
  if ((rc = ensure(c, c->mapreg.small, 64))) return rc;
  if ((rc = build_measured_grid(c, cl, cell, c->mapreg.small.as<int>(), hsm, false, "feature map", "feature-map grid"))) return rc;
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
  for (int s = 0; s < 4; s++) { feat[s] = c->mapreg.feat[s].as<const float>(); fac[s] = c->mapreg.fac[s].as<const double>(); }
  rgck::mapreg_terms(c->stream, feat, fac, nfeat, x, 0.1, want_H ? 1 : 0, c->mapreg.partials.as<double>(), c->d_out);
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

int rgcapi::grid_strided_cloud(rgc_ctx* c, Cloud& cl, const float* p, int n, int stride_bytes, bool on_device, double cell, const char* what_device) {
  cl.ready = false;
  int rc;
  if (on_device) {
    if ((rc = check_device_range(c, p, record_bytes(n, stride_bytes, false), what_device))) return rc;
    cl.in = p;
  } else {
    if ((rc = ensure(c, cl.in_copy, (size_t)n * stride_bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(cl.in_copy.p, p, record_bytes(n, stride_bytes, false), hipMemcpyHostToDevice, c->stream));
    cl.in = cl.in_copy.as<const float>();
  }
  cl.stride_f = stride_bytes / 4;
  cl.n = n;
  return prepare_map_grid(c, cl, cell);
}

extern "C" {

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
    const int rc = grid_strided_cloud(c, c->mapreg.map[m], src[m], n[m], stride_bytes, on_device, kMapregCell[m], "rgc_mapreg_set_maps_device: feature map");
    if (rc) return rc;
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
  if ((rc = ensure(c, c->mapreg.feat[slot], sizeof(float) * 4 * (size_t)(n > 0 ? n : 1)))) return rc;
  if ((rc = ensure(c, c->mapreg.fac[slot], sizeof(double) * 8 * (size_t)(n > 0 ? n : 1)))) return rc;
  if (n > 0) HIPCHK(c, hipMemcpyAsync(c->mapreg.feat[slot].p, feat, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  return RGC_OK;
}

// What rgc_mapreg_linearize and every outer iteration of rgc_mapreg_optimize open with.  feat (null from the second iteration on: staged already): the four
// feature sets on the device and the term kernels' rows sized for them.  Then the association of all four at the two poses (the four loops of :1092-1282 side by
// side, one launch); the factor counts (the reference's corner_num / surf_num ...) ride home to h_small->mapreg.n with the next evaluation's synchronisation
static int mapreg_open(rgc_ctx* c, const float* const* feat, const int nfeat[4], const double poses[14]) {
  int rc;
  for (int s = 0; s < 4 && feat; s++)
    if ((rc = mapreg_upload_features(c, s, feat[s], nfeat[s]))) return rc;
  const int nb = std::max(rgck::mapreg_blocks(nfeat[0], nfeat[1]), rgck::mapreg_blocks(nfeat[2], nfeat[3]));
  if (feat && (rc = ensure(c, c->mapreg.partials, sizeof(double) * 2 * rgck::kAccum * (size_t)(nb > 0 ? nb : 1)))) return rc;
  int* dcnt = c->mapreg.small.as<int>() + 8;
  HIPCHK(c, hipMemsetAsync(dcnt, 0, 4 * sizeof(int), c->stream));
  rgck::MapregAssoc sets[4];
  for (int s = 0; s < 4; s++) {
    const double* q = poses + 7 * (s / 2);
    const Cloud& m = c->mapreg.map[s & 1];
    sets[s] = rgck::MapregAssoc{c->mapreg.feat[s].as<const float>(), nfeat[s], (s & 1) == 0 ? 1 : 0, rgck::Quat{q[0], q[1], q[2], q[3]}, {q[4], q[5], q[6]},
                                m.P.as<const float4>(), m.start.as<const int>(), m.grid, c->mapreg.fac[s].as<double>(), dcnt + s};
  }
  rgck::mapreg_associate(c->stream, sets, 4);
  HIPCHK(c, hipMemcpyAsync(c->h_small->mapreg.n, dcnt, sizeof(rgck::MapregCounts::n), hipMemcpyDeviceToHost, c->stream));
  return RGC_OK;
}

int rgc_mapreg_associate(rgc_ctx* c, int kind, const float* feat_xyzw, int n, const double q_xyzw[4], const double t[3], double* factors8,
                         int* n_valid) {
  if (!c || !feat_xyzw || !q_xyzw || !t || n < 0 || n > (1 << 27) || (kind != 0 && kind != 1)) return RGC_ERR_INVALID;
  if (!c->mapreg.map[kind].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = mapreg_upload_features(c, kind, feat_xyzw, n);
  if (rc) return rc;
  const Cloud& m = c->mapreg.map[kind];
  const rgck::MapregAssoc one{c->mapreg.feat[kind].as<const float>(), n, kind == 0 ? 1 : 0, rgck::Quat{q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3]},
                              {t[0], t[1], t[2]}, m.P.as<const float4>(), m.start.as<const int>(), m.grid, c->mapreg.fac[kind].as<double>(), nullptr};
  rgck::mapreg_associate(c->stream, &one, 1);
  std::vector<double> tmp;
  double* dst = factors8;
  if (!dst) { tmp.resize((size_t)8 * (n > 0 ? n : 1)); dst = tmp.data(); }
  if (n > 0) HIPCHK(c, hipMemcpyAsync(dst, c->mapreg.fac[kind].p, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
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
  if (!c->mapreg.map[0].ready || !c->mapreg.map[1].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  if (report) memset(report, 0, sizeof(rgc_mapreg_report) * 2);
  // the gate of :1069 (laserCloudCornerDSNum > 10 && laserCloudSurfDSNum > 50 && map sizes likewise)
  const bool gate = n_ccur > 10 && n_scur > 50 && c->mapreg.map[0].n > 10 && c->mapreg.map[1].n > 50;
  if (gate_failed) *gate_failed = gate ? 0 : 1;
  if (!gate) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const float* feat[4] = {corner_cur, surf_cur, corner_last, surf_last};
  const int nfeat[4] = {n_ccur, n_scur, n_clast, n_slast};
  const rgc_mapreg_ground* const ground[2] = {ground_cur, ground_last};
  int rc;
  for (int iter = 0; iter < 2; iter++) {  // :1076
    // association at the current estimate of both poses (frozen during the solve)
    if ((rc = mapreg_open(c, iter == 0 ? feat : nullptr, nfeat, poses))) return rc;
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
  if (!c->mapreg.map[0].ready || !c->mapreg.map[1].ready) return fail(c, RGC_ERR_NO_INPUT, "rgc_mapreg_set_maps first");
  HIPCHK(c, hipSetDevice(c->device));
  const float* feat[4] = {corner_cur, surf_cur, corner_last, surf_last};
  const int nfeat[4] = {n_ccur, n_scur, n_clast, n_slast};
  const rgc_mapreg_ground* const ground[2] = {ground_cur, ground_last};
  int rc;
  if ((rc = mapreg_open(c, feat, nfeat, poses_assoc))) return rc;
  for (int s = 0; s < 4 && factors8; s++)
    if (factors8[s] && nfeat[s] > 0)
      HIPCHK(c, hipMemcpyAsync(factors8[s], c->mapreg.fac[s].p, sizeof(double) * 8 * (size_t)nfeat[s], hipMemcpyDeviceToHost, c->stream));
  MapregSystem S;
  if ((rc = mapreg_eval(c, nfeat, poses_eval ? poses_eval : poses_assoc, true, ground, imu, &S))) return rc;
  memcpy(H, S.H, sizeof(S.H));
  memcpy(g, S.g, sizeof(S.g));
  *cost = S.cost;
  for (int s = 0; s < 4; s++) n_factors[s] = c->h_small->mapreg.n[s];
  return RGC_OK;
}
}  // extern "C"
