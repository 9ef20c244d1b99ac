// rgc_api_pgo.hip -- host side of the 4-DoF pose graph over the keyframe store's key poses (rgc_pgo_*): the graph is built from the store
// on the host (PoseGraphOptimize4DoF, src/RGC_mapping.cpp:2303-2466), linearised and solved on the device (rgc_pgo.hip), and the LM
// decisions of ceres::Solve as rgc_mapreg_optimize restates them are taken here, one small read-back per iteration.
#include "rgc_ctx.h"

#include <algorithm>

using namespace rgcapi;

namespace {

constexpr int kPgoMinSegment = 32;    // positions between two regular separators, at least ...
constexpr int kPgoRegularSeps = 96;   // ... and as many as keep the regular separators below this count

// the segment size of a selection of n positions (DESIGN.md "pose graph"): the dense stage takes at most rgck::kPgoMaxSep separators, of
// which the loops claim up to 2 * RGC_PGO_MAX_LOOPS + 1
int pgo_segment_size(int n) { return std::max(kPgoMinSegment, (n + kPgoRegularSeps - 1) / kPgoRegularSeps); }
static_assert(kPgoRegularSeps + 1 + 2 * RGC_PGO_MAX_LOOPS + 1 <= rgck::kPgoMaxSep, "the dense stage must hold every separator");

struct PgoHost {
  int n = 0, n_edges = 0, n_used = 0, n_ignored = 0, fixed = -1, fixed_id = -1;
  std::vector<int> ij, inc_start, inc, sep, sep_of, used;   // used: indices into the caller's loops
  std::vector<double> meas, x;
  std::vector<rgc_kf_pose> pose;
  // device views
  rgck::PgoGraph G{};
  double *x_dev[2], *terms[2], *D[2], *g[2], *out[2], *ws, *slots, *d, *part;
  int* flag;
};

// Eigen: q.inverse() * v for the stored (unit up to rounding) quaternion x, y, z, w
void pgo_inv_rotate(const double q[4], const double v[3], double o[3]) {
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const double x = -q[0] / n2, y = -q[1] / n2, z = -q[2] / n2, w = q[3] / n2;
  double ux = y * v[2] - z * v[1], uy = z * v[0] - x * v[2], uz = x * v[1] - y * v[0];
  ux += ux; uy += uy; uz += uz;
  o[0] = v[0] + w * ux + (y * uz - z * uy);
  o[1] = v[1] + w * uy + (z * ux - x * uz);
  o[2] = v[2] + w * uz + (x * uy - y * ux);
}

// the graph of a selection on the host: argument checks (nothing is touched where one fails), state, edge table, constant node, incidence, separators
int pgo_build(rgc_ctx* c, const int* ids, int n_ids, const rgc_pgo_loop* loops, int n_loops, const double* x_eval, PgoHost& P) {
  if (n_ids < 1 || !ids || n_loops < 0 || (n_loops && !loops)) return fail(c, RGC_ERR_INVALID, "rgc_pgo: at least one keyframe id, and loops where n_loops > 0");
  if (n_ids > (1 << 24)) return fail(c, RGC_ERR_INVALID, "rgc_pgo: more than 2^24 keyframes");
  const double rad2deg = 180.0 / M_PI;
  std::unordered_map<int, int> pos;
  pos.reserve((size_t)n_ids * 2);
  P.n = n_ids;
  P.pose.resize(n_ids);
  P.x.resize((size_t)4 * n_ids);
  std::vector<const KeyframeRecord::KfRec*> rec(n_ids);
  for (int i = 0; i < n_ids; i++) {
    const auto it = c->kfs.index.find(ids[i]);
    if (it == c->kfs.index.end()) return fail(c, RGC_ERR_INVALID, "rgc_pgo: keyframe %d is not in the store", ids[i]);
    if (!pos.emplace(ids[i], i).second) return fail(c, RGC_ERR_INVALID, "rgc_pgo: keyframe %d is selected twice", ids[i]);
    rec[i] = &c->kfs.recs[it->second];
    P.pose[i] = rec[i]->pose;
    P.x[4 * i] = rec[i]->pose.yaw * rad2deg;                       // euler_array[keyI][0], :2355
    P.x[4 * i + 1] = rec[i]->pose.x; P.x[4 * i + 2] = rec[i]->pose.y; P.x[4 * i + 3] = rec[i]->pose.z;
  }
  int oldest = INT_MAX;
  for (int l = 0; l < n_loops; l++) {
    const rgc_pgo_loop& L = loops[l];
    const double v[6] = {L.t_loop_curr[0], L.t_loop_curr[1], L.t_loop_curr[2], L.yaw_loop_curr_deg, L.pitch_loop_deg, L.roll_loop_deg};
    for (double a : v)
      if (!std::isfinite(a)) return fail(c, RGC_ERR_INVALID, "rgc_pgo: loop %d holds a value that is not finite", l);
    if (L.key_curr == L.key_loop) return fail(c, RGC_ERR_INVALID, "rgc_pgo: loop %d joins keyframe %d to itself", l, L.key_curr);
    const auto ic = pos.find(L.key_curr), il = pos.find(L.key_loop);
    if (ic == pos.end() || il == pos.end() || ic->second == 0) { P.n_ignored++; continue; }   // :2364 precedes :2376
    P.used.push_back(l);
    if (L.key_loop < oldest) { oldest = L.key_loop; P.fixed = il->second; }                     // oldestLoopKey, :2340-2341
  }
  P.n_used = (int)P.used.size();
  if (P.n_used > RGC_PGO_MAX_LOOPS) return fail(c, RGC_ERR_INVALID, "rgc_pgo: %d used loops, the limit is %d", P.n_used, RGC_PGO_MAX_LOOPS);
  P.fixed_id = P.n_used ? oldest : -1;
  P.n_edges = n_ids - 1 + P.n_used;
  P.ij.resize((size_t)2 * std::max(P.n_edges, 1));
  P.meas.resize((size_t)6 * std::max(P.n_edges, 1));
  for (int i = 1; i < n_ids; i++) {                                  // :2367-2373
    const int e = i - 1;
    const double dt[3] = {P.x[4 * i + 1] - P.x[4 * e + 1], P.x[4 * i + 2] - P.x[4 * e + 2], P.x[4 * i + 3] - P.x[4 * e + 3]};
    P.ij[2 * e] = e; P.ij[2 * e + 1] = i;
    pgo_inv_rotate(rec[e]->q, dt, &P.meas[6 * e]);
    P.meas[6 * e + 3] = P.x[4 * i] - P.x[4 * e];
    P.meas[6 * e + 4] = rec[e]->pose.pitch * rad2deg;
    P.meas[6 * e + 5] = rec[e]->pose.roll * rad2deg;
  }
  std::vector<int> deg(n_ids + 1, 0);
  for (int u = 0; u < P.n_used; u++) {                               // :2376-2392
    const rgc_pgo_loop& L = loops[P.used[u]];
    const int e = n_ids - 1 + u, i = pos[L.key_loop], j = pos[L.key_curr];
    P.ij[2 * e] = i; P.ij[2 * e + 1] = j;
    for (int a = 0; a < 3; a++) P.meas[6 * e + a] = L.t_loop_curr[a];
    P.meas[6 * e + 3] = L.yaw_loop_curr_deg; P.meas[6 * e + 4] = L.pitch_loop_deg; P.meas[6 * e + 5] = L.roll_loop_deg;
    deg[i]++; deg[j]++;
  }
  P.inc_start.assign(n_ids + 1, 0);
  for (int i = 0; i < n_ids; i++) P.inc_start[i + 1] = P.inc_start[i] + deg[i];
  P.inc.assign((size_t)std::max(2 * P.n_used, 1), 0);
  std::vector<int> fill(P.inc_start.begin(), P.inc_start.end() - 1);
  for (int u = 0; u < P.n_used; u++) {                               // ascending loop order inside every node's list
    const int e = n_ids - 1 + u;
    P.inc[fill[P.ij[2 * e]]++] = 2 * u;
    P.inc[fill[P.ij[2 * e + 1]]++] = 2 * u + 1;
  }
  // separators: position 0, every S-th position, the endpoints of the used loops (the constant node is one of them)
  P.sep_of.assign(n_ids, -1);
  const int S = pgo_segment_size(n_ids);
  for (int i = 0; i < n_ids; i += S) P.sep_of[i] = 0;
  for (int u = 0; u < 2 * P.n_used; u++) P.sep_of[P.ij[2 * (n_ids - 1) + u]] = 0;
  for (int i = 0; i < n_ids; i++)
    if (P.sep_of[i] == 0) { P.sep_of[i] = (int)P.sep.size(); P.sep.push_back(i); }
  if ((int)P.sep.size() > rgck::kPgoMaxSep) return fail(c, RGC_ERR_INVALID, "rgc_pgo: %d separators", (int)P.sep.size());
  if (x_eval) {
    for (size_t k = 0; k < (size_t)4 * n_ids; k++)
      if (!std::isfinite(x_eval[k])) return fail(c, RGC_ERR_INVALID, "rgc_pgo_linearize: x_eval is not finite");
    P.x.assign(x_eval, x_eval + (size_t)4 * n_ids);
  }
  return RGC_OK;
}

// the graph and the state onto the device (buffers of the pose graph's own), the views of every array of a solve
int pgo_upload(rgc_ctx* c, PgoHost& P) {
  int rc;
  const size_t n = P.n, E = std::max(P.n_edges, 1), ns = P.sep.size();
  const size_t ni = 2 * E + (n + 1) + P.inc.size() + ns + n + 4;
  const size_t nd = 6 * E + 2 * 4 * n + 2 * rgck::kPgoTerm * E + 2 * 16 * n + 2 * 4 * n + 2 * 8 + rgck::kPgoWs * n + rgck::kPgoSlot * ns + 4 * n + 4 * n;
  if ((rc = ensure(c, c->pgo.i, ni * sizeof(int)))) return rc;
  if ((rc = ensure(c, c->pgo.d, nd * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->pgo.M, 16 * ns * ns * sizeof(double)))) return rc;
  std::vector<int> hi;
  hi.reserve(ni);
  int* di = c->pgo.i.as<int>();
  auto put = [&](const std::vector<int>& v, size_t count) { const int* p = di + hi.size(); hi.insert(hi.end(), v.begin(), v.begin() + (long)count); return p; };
  P.G.n_nodes = P.n; P.G.n_edges = P.n_edges; P.G.fixed = P.fixed; P.G.n_sep = (int)ns;
  P.G.ij = put(P.ij, 2 * E);
  P.G.inc_start = put(P.inc_start, n + 1);
  P.G.inc = put(P.inc, P.inc.size());
  P.G.sep = put(P.sep, ns);
  P.G.sep_of = put(P.sep_of, n);
  P.flag = di + hi.size();
  hi.resize(hi.size() + 4, 0);
  double* dd = c->pgo.d.as<double>();
  auto take = [&](size_t count) { double* p = dd; dd += count; return p; };
  double* meas = take(6 * E);
  P.G.meas = meas;
  for (int b = 0; b < 2; b++) { P.x_dev[b] = take(4 * n); P.terms[b] = take(rgck::kPgoTerm * E); P.D[b] = take(16 * n); P.g[b] = take(4 * n); P.out[b] = take(8); }
  P.ws = take(rgck::kPgoWs * n); P.slots = take(rgck::kPgoSlot * ns); P.d = take(4 * n); P.part = take(4 * n);
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(meas, P.meas.data(), 6 * E * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P.x_dev[0], P.x.data(), 4 * n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(P.d, 0, 4 * n * sizeof(double), s));
  HIPCHK(c, hipStreamSynchronize(s));   // the staging vectors go out of scope
  return RGC_OK;
}

void pgo_fill_report(const PgoHost& P, rgc_pgo_report* r) {
  memset(r, 0, sizeof(*r));
  r->status = P.n_used ? RGC_PGO_OPTIMIZED : RGC_PGO_NO_LOOP;
  r->n_nodes = P.n; r->n_odom = P.n - 1; r->n_loops_used = P.n_used; r->n_loops_ignored = P.n_ignored; r->fixed_id = P.fixed_id;
}

int pgo_fetch(rgc_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return RGC_OK;
}

}  // namespace

extern "C" {

void rgc_default_pgo_params(rgc_pgo_params* p) {
  if (!p) return;
  p->max_iterations = 10;     // :2425
  p->initial_radius = 1e4;    // Ceres' default
}

int rgc_pgo_optimize(rgc_ctx* c, const int* ids, int n_ids, const rgc_pgo_loop* loops, int n_loops, const rgc_pgo_params* params, int apply,
                     rgc_kf_pose* out_poses, rgc_pgo_report* report) {
  if (!c) return RGC_ERR_INVALID;
  rgc_pgo_params prm;
  rgc_default_pgo_params(&prm);
  if (params) prm = *params;
  if (prm.max_iterations < 0 || prm.max_iterations > 32 || !(prm.initial_radius > 0) || !std::isfinite(prm.initial_radius))
    return fail(c, RGC_ERR_INVALID, "rgc_pgo_optimize: max_iterations in 0..32 and a positive finite initial_radius");
  PgoHost P;
  int rc;
  if ((rc = pgo_build(c, ids, n_ids, loops, n_loops, nullptr, P))) return rc;
  rgc_pgo_report rep;
  pgo_fill_report(P, &rep);
  if (!P.n_used) {            // bLoopIsClosed == false / no oldestLoopKey: nothing is optimised (:2308, 2415-2419)
    if (out_poses) memcpy(out_poses, P.pose.data(), sizeof(rgc_kf_pose) * (size_t)n_ids);
    if (report) *report = rep;
    return RGC_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = pgo_upload(c, P))) return rc;
  hipStream_t s = c->stream;
  // ceres::Solve restated as in rgc_mapreg_optimize.  cur: the accepted state with its H, g and cost; the other half receives the candidate,
  // whose normal equations are evaluated together with its cost (nearly every step is accepted, and an accepted step needs them next)
  int cur = 0, it = 0, n_success = 0, stop = RGC_PGO_STOP_CAP;
  unsigned mask = 0;
  double radius = prm.initial_radius, decrease_factor = 2.0, h[8], hn[8];
  int hflag = 0;
  rgck::pgo_evaluate(s, P.G, P.x_dev[cur], P.terms[cur], P.D[cur], P.g[cur], P.out[cur]);
  HIPCHK(c, hipGetLastError());
  if ((rc = pgo_fetch(c, h, P.out[cur], 2 * sizeof(double)))) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  double cost = h[0], gmax = h[1];
  rep.initial_cost = cost;
  for (it = 0; it < prm.max_iterations; it++) {
    if (gmax <= 1e-10) { stop = RGC_PGO_STOP_GRADIENT; break; }
    const int nxt = cur ^ 1;
    HIPCHK(c, hipMemsetAsync(P.flag, 0, sizeof(int), s));
    rgck::pgo_solve(s, P.G, P.terms[cur], P.D[cur], P.g[cur], radius, P.ws, P.slots, c->pgo.M.as<double>(), P.d, P.flag);
    rgck::pgo_step(s, P.G, P.terms[cur], P.D[cur], P.g[cur], P.x_dev[cur], P.d, P.x_dev[nxt], P.part, P.out[cur] + 2);
    rgck::pgo_evaluate(s, P.G, P.x_dev[nxt], P.terms[nxt], P.D[nxt], P.g[nxt], P.out[nxt]);
    HIPCHK(c, hipGetLastError());
    if ((rc = pgo_fetch(c, h, P.out[cur], 5 * sizeof(double)))) return rc;      // {cost, max |g|, model, |d|^2, |x+|^2}
    if ((rc = pgo_fetch(c, hn, P.out[nxt], 2 * sizeof(double)))) return rc;
    if ((rc = pgo_fetch(c, &hflag, P.flag, sizeof(int)))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    const double model = h[2];
    double rho = -1.0;
    if (!hflag && model > 0 && std::isfinite(hn[0])) rho = (cost - hn[0]) / model;
    if (rho > 1e-3) {
      const double old_cost = cost;
      cur = nxt; cost = hn[0]; gmax = hn[1];
      radius = std::fmin(radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3)), 1e16);
      decrease_factor = 2.0;
      n_success++;
      mask |= 1u << it;
      if (std::fabs(old_cost - cost) <= 1e-6 * old_cost) { it++; stop = RGC_PGO_STOP_FUNCTION; break; }
      if (std::sqrt(h[3]) <= 1e-8 * (std::sqrt(h[4]) + 1e-8)) { it++; stop = RGC_PGO_STOP_PARAMETER; break; }
    } else {
      radius /= decrease_factor;
      decrease_factor *= 2.0;
      if (radius < 1e-32) { it++; stop = RGC_PGO_STOP_RADIUS; break; }
    }
  }
  rep.final_cost = cost; rep.iterations = it; rep.successful = n_success; rep.stop = stop; rep.accepted_mask = mask;
  std::vector<double> x((size_t)4 * n_ids);
  if ((rc = pgo_fetch(c, x.data(), P.x_dev[cur], x.size() * sizeof(double)))) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  const double deg2rad = M_PI / 180.0;
  for (int i = 0; i < n_ids; i++) {                                  // :2450-2455, the constant node included; pitch and roll as stored
    rgc_kf_pose& p = P.pose[i];
    p.x = (float)x[4 * i + 1]; p.y = (float)x[4 * i + 2]; p.z = (float)x[4 * i + 3];
    p.yaw = (float)(x[4 * i] * deg2rad);
    if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z) || !std::isfinite(p.yaw))
      return fail(c, RGC_ERR_NONFINITE, "rgc_pgo_optimize: the corrected pose of keyframe %d is not finite", ids[i]);
  }
  if (out_poses) memcpy(out_poses, P.pose.data(), sizeof(rgc_kf_pose) * (size_t)n_ids);
  if (report) *report = rep;
  if (apply) return rgc_kf_set_poses(c, ids, P.pose.data(), n_ids);
  return RGC_OK;
}

int rgc_pgo_linearize(rgc_ctx* c, const int* ids, int n_ids, const rgc_pgo_loop* loops, int n_loops, const double* x_eval, double radius, int* edge_ij,
                      double* edge_meas, double* residuals, double* g, double* cost, double* H_diag, double* H_chain, double* H_loop, double* d,
                      rgc_pgo_report* report) {
  if (!c) return RGC_ERR_INVALID;
  if (!std::isfinite(radius)) return fail(c, RGC_ERR_INVALID, "rgc_pgo_linearize: the radius is not finite");
  PgoHost P;
  int rc;
  if ((rc = pgo_build(c, ids, n_ids, loops, n_loops, x_eval, P))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = pgo_upload(c, P))) return rc;
  hipStream_t s = c->stream;
  rgck::pgo_evaluate(s, P.G, P.x_dev[0], P.terms[0], P.D[0], P.g[0], P.out[0]);
  const bool solve = radius > 0 && P.n_used > 0;
  int hflag = 0;
  if (solve) {
    HIPCHK(c, hipMemsetAsync(P.flag, 0, sizeof(int), s));
    rgck::pgo_solve(s, P.G, P.terms[0], P.D[0], P.g[0], radius, P.ws, P.slots, c->pgo.M.as<double>(), P.d, P.flag);
    if ((rc = pgo_fetch(c, &hflag, P.flag, sizeof(int)))) return rc;
  }
  HIPCHK(c, hipGetLastError());
  const size_t E = (size_t)P.n_edges, n = (size_t)n_ids;
  std::vector<double> terms(rgck::kPgoTerm * std::max(E, (size_t)1));
  double h[2];
  if ((rc = pgo_fetch(c, terms.data(), P.terms[0], rgck::kPgoTerm * E * sizeof(double)))) return rc;
  if ((rc = pgo_fetch(c, h, P.out[0], sizeof(h)))) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  // a refusal leaves every output of the caller untouched: nothing is copied out before the solve's flag is known
  if (hflag) return fail(c, RGC_ERR_INVALID, "rgc_pgo_linearize: the damped system is not positive definite");
  if (g && (rc = pgo_fetch(c, g, P.g[0], 4 * n * sizeof(double)))) return rc;
  if (H_diag && (rc = pgo_fetch(c, H_diag, P.D[0], 16 * n * sizeof(double)))) return rc;
  if (d && solve && (rc = pgo_fetch(c, d, P.d, 4 * n * sizeof(double)))) return rc;
  HIPCHK(c, hipStreamSynchronize(s));
  for (size_t e = 0; e < E; e++) {
    const double* T = &terms[e * rgck::kPgoTerm];
    if (residuals) memcpy(residuals + 4 * e, T, 4 * sizeof(double));
    double* Hb = e + 1 < n ? (H_chain ? H_chain + 16 * e : nullptr) : (H_loop ? H_loop + 16 * (e - (n - 1)) : nullptr);
    if (Hb) memcpy(Hb, T + 44, 16 * sizeof(double));
  }
  if (edge_ij) memcpy(edge_ij, P.ij.data(), 2 * E * sizeof(int));
  if (edge_meas) memcpy(edge_meas, P.meas.data(), 6 * E * sizeof(double));
  if (cost) *cost = h[0];
  if (report) { pgo_fill_report(P, report); report->initial_cost = report->final_cost = h[0]; }
  return RGC_OK;
}

}  // extern "C"
