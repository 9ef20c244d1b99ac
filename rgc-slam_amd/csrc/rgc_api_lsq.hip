// rgc_api_lsq.hip -- the host LM driver every registration method shares (LsqRegistration::computeTransformation and step_lm,
// lsq_registration_impl.hpp:53-79, 125-172) and what the methods' host files share beside it: the read-out of a method's folded sums, and the
// offsets of a neighbour method.  rgc_align's host-driven route (rgc_api.hip), NDT (rgc_api_ndt.hip) and FastGICP / FastGICPSingleThread
// (rgc_api_gicp.hip) run on the driver; FastGICPMultiPoints (rgc_api_gicp.hip) has a plain Gauss-Newton loop of its own over the driver's scalar pieces.
#include "rgc_ctx.h"
#include "rgc_lm_decide.h"  // rgc_lm.h and the convergence test the device decides by (lsq_registration_impl.hpp:82-91)

using namespace rgcapi;

// LsqRegistration::computeTransformation (lsq_registration_impl.hpp:53-79) + step_lm (:125-172); SURVEY A.5.  The scalar pieces (so3_exp, the
// LDLT solve, the 4x4 product) are rgc_lm.h's, shared with the device.
int rgcapi::lm_solve(rgc_ctx* c, const LmSystem& sys, const float guess[16], LmResult* r) {
  const rgc_params& P = c->prm;
  r->open(guess);
  double* x0 = r->x0;
  double lambda = -1.0;  // :56
  for (int it = 0; it < P.max_iterations && !r->conv; it++) {  // :65
    r->iters = it + 1;
    double H[36], b[6], y0, delta[16], d[6], xi[16], yi;
    int rc;
    if (sys.may_linearize && !sys.may_linearize(x0)) { r->failed = true; break; }  // (FastGICP: a step of an empty or singular system)
    if (sys.linearize_try) {  // :128 and the first try of :135-144 in one call; :130-132 with it (lambda0 = factor * max|H_ii|)
      if ((rc = sys.linearize_try(c, x0, lambda, H, b, &y0, d, xi, &lambda, &yi))) return rc;
      double R[9];  // that try's delta = [so3_exp(d[0:3]) | d[3:6]] (:136-143)
      rgclm::so3_exp_R(d, R);
      memset(delta, 0, sizeof(delta));
      for (int a = 0; a < 3; a++) { for (int e = 0; e < 3; e++) delta[a * 4 + e] = R[a * 3 + e]; delta[a * 4 + 3] = d[3 + a]; }
      delta[15] = 1.0;
    } else {
      if ((rc = sys.linearize(c, x0, H, b, &y0))) return rc;  // :128
      if (lambda < 0.0) {  // :130-132
        double m = 0;
        for (int a = 0; a < 6; a++) m = std::fmax(m, std::fabs(H[a * 7]));
        lambda = P.lm_init_lambda_factor * m;
      }
    }
    double nu = 2.0;
    bool ok = false;
    for (int k = 0; k < P.lm_max_iterations; k++) {  // :135
      if (k > 0 || !sys.linearize_try) {  // (every try but one that linearize_try has made)
        rgclm::lm_try(H, b, lambda, x0, d, delta, xi);  // :136-143
        if ((rc = sys.error(c, xi, &yi))) return rc;    // :144
      }
      double den = 0;
      for (int i = 0; i < 6; i++) den += d[i] * (lambda * d[i] - b[i]);
      const double rho = (y0 - yi) / den;  // :145
      if (rho < 0) {  // :155-163
        if (rgck::lm_is_converged(delta, P.rotation_eps, P.translation_eps)) { ok = true; break; }
        lambda = nu * lambda;
        nu = 2 * nu;
        continue;
      }
      memcpy(x0, xi, sizeof(xi));  // :165
      lambda = lambda * std::fmax(1.0 / 3.0, 1 - std::pow(2 * rho - 1, 3));  // :166
      memcpy(r->Hfin, H, sizeof(r->Hfin));  // :167
      ok = true;
      break;
    }
    if (!ok) { r->failed = true; break; }  // :69-72 "lm not converged!!"
    r->conv = rgck::lm_is_converged(delta, P.rotation_eps, P.translation_eps);  // :74
  }
  for (int i = 0; i < 16; i++) r->fin[i] = (float)x0[i];  // :77
  return RGC_OK;
}

// the k folded sums of a method (s.out, behind the launches on the context's stream) in its pinned buffer s.h_out, the launches checked
int rgcapi::read_sums(rgc_ctx* c, const Sums& s, int k) {
  HIPCHK(c, hipMemcpyAsync(s.h_out, s.out.p, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return RGC_OK;
}

// ... of a linearisation (k >= 28): H and b out of them when both are wanted, the cost (each nullable)
int rgcapi::read_system(rgc_ctx* c, const Sums& s, int k, double* H, double* b, double* cost) {
  const int rc = read_sums(c, s, k);
  if (rc) return rc;
  if (H && b) unpack_system(s.h_out, H, b);
  if (cost) *cost = s.h_out[27];
  return RGC_OK;
}

// the offsets of a neighbour method in the reference's order (rgc_ctx.h): src/fast_gicp/cuda/ndt_cuda.cu:35-88, fast_vgicp_cuda.cu:42-95
bool rgcapi::neighbor_offsets_of(int method, double radius, std::vector<int>& o, int cap) {
  o.clear();
  if (method == RGC_NDT_DIRECT1) { o = {0, 0, 0}; return true; }
  if (method == RGC_NDT_DIRECT7) { o = {0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1}; return true; }
  if (method == RGC_NDT_DIRECT27) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) { o.push_back(i - 1); o.push_back(j - 1); o.push_back(k - 1); }
    return true;
  }
  if (radius > 16.0) return false;
  const int range = (int)std::ceil(radius);
  for (int i = -range; i <= range; i++)
    for (int j = -range; j <= range; j++)
      for (int k = -range; k <= range; k++)
        if (std::sqrt((double)(i * i + j * j + k * k)) <= radius + 1e-3) {
          if ((int)o.size() / 3 >= cap) return false;
          o.push_back(i); o.push_back(j); o.push_back(k);
        }
  return true;
}

extern "C" {

// the offset table of a neighbour method as VGICP and NDT walk it: host code, no context (rgc_hip.h)
int rgc_neighbor_offsets(int method, double radius, int* xyz, int cap, int* n) {
  if (!n || cap < 0) return RGC_ERR_INVALID;  // (xyz == NULL: the size alone)
  if (method < RGC_DIRECT27 || method > RGC_DIRECT_RADIUS) return RGC_ERR_INVALID;
  if (method == RGC_DIRECT_RADIUS && (!std::isfinite(radius) || radius < 0.0)) return RGC_ERR_INVALID;
  std::vector<int> o;
  if (!neighbor_offsets_of(method, radius, o)) return RGC_ERR_INVALID;  // more than RGC_NDT_MAX_OFFSETS
  const int total = (int)o.size() / 3;
  if (xyz) memcpy(xyz, o.data(), sizeof(int) * 3 * (size_t)std::min(cap, total));
  *n = total;
  return RGC_OK;
}

}  // extern "C"
