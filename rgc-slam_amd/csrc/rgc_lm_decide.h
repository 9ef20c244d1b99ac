// rgc_lm_decide.h -- the decision of the device LM (k_lm_step, k_lm_solve in rgc_kernels.hip): what one launch's folded sums mean, accept /
// reject / terminate, and the next LM try.  Plain scalar code on an LmState, compiled for the device by rgc_kernels.hip and for the host by
// whoever wants to check it (tests/cpp/lm_device_table.hip); the host driver (rgc_api_lsq.hip) shares the convergence test.
// rgc_kernels.hip defines LAB_TS (the developer build's phase stamps) before it includes this file; anywhere else the stamps are no-ops.
#pragma once
#include "rgc_kernels.h"
#include "rgc_lm.h"

#ifndef LAB_TS
#define LAB_TS(k)
#endif

namespace rgck {

__host__ __device__ __forceinline__ bool lm_is_converged(const double* d, double rot_eps, double trans_eps) {  // :82-91
  double m = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int e = 0; e < 3; e++) m = fmax(m, fabs(d[a * 4 + e] - (a == e ? 1.0 : 0.0)) / rot_eps);
    m = fmax(m, fabs(d[a * 4 + 3]) / trans_eps);
  }
  return m < 1;
}

// The modes of a launch of the device-chained LM (k_lm_step):
constexpr int LM_MODE_LIN = 0, LM_MODE_BA = 1, LM_MODE_B = 2;
constexpr int kStepAcc = kAccum + 2;  // 28 linearisation sums, the correspondence count, the trial cost

// The decision the sums of one launch call for, taken by lane 0 of a workgroup on its LDS copy `ls` of the state the launch ran from:
// what the folded sums mean in that launch's mode, accept / reject / terminate, and the next LM try (lsq_registration_impl.hpp:125-172).
__host__ __device__ __forceinline__ void lm_step_decide(LmState& ls, const double* folded, int mode, int cur, bool* took_xi) {
  const int first = 0;  // (the developer build's timestamps: slot of a launch that decides)
  (void)first;
  double H[36], b[6], x0[16], d[6], delta[16], xi[16];
  double lambda = ls.lambda;
  bool have_lin = false;  // H, b (registers) hold a linearisation at the pose the next try starts from
  auto adopt = [&]() {    // H, b, y0, ncorr of the linearisation just folded
    int u = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int e = a; e < 6; e++) { H[a * 6 + e] = folded[u]; H[e * 6 + a] = folded[u]; u++; }
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = folded[21 + a];
#pragma unroll
    for (int a = 0; a < 36; a++) ls.H[a] = H[a];
#pragma unroll
    for (int a = 0; a < 6; a++) ls.b[a] = b[a];
    ls.y0 = folded[27];
    ls.ncorr = (int)folded[kAccum];
    ls.n_lin++;
    have_lin = true;
  };
  if (mode == LM_MODE_LIN) {
    adopt();
    if (lambda < 0.0) {  // :130-132
      double m = 0;
#pragma unroll
      for (int a = 0; a < 6; a++) m = fmax(m, fabs(H[a * 7]));
      lambda = ls.init_factor * m;
    }
#pragma unroll
    for (int a = 0; a < 16; a++) x0[a] = ls.x0[a];
    ls.mode = LM_MODE_BA;
  } else {
    const double yi = folded[kAccum + 1];
    ls.yi = yi;
    ls.n_err++;
    double den = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) den += ls.d[a] * (lambda * ls.d[a] - ls.b[a]);
    const double rho = (ls.y0 - yi) / den;  // :145
    const bool conv_now = lm_is_converged(ls.delta, ls.rot_eps, ls.trans_eps);
    bool outer_done = false;
    if (rho < 0) {  // :155-163
      if (conv_now) {
        outer_done = true;  // step_lm returns true with x unchanged
      } else {
        lambda = ls.nu * lambda;
        ls.nu = 2 * ls.nu;
        ls.inner++;
        if (ls.inner >= ls.max_inner) { ls.failed = 1; ls.done = 1; ls.lambda = lambda; return; }  // "lm not converged!!", :69-72
#pragma unroll
        for (int a = 0; a < 36; a++) H[a] = ls.H[a];
#pragma unroll
        for (int a = 0; a < 6; a++) b[a] = ls.b[a];
#pragma unroll
        for (int a = 0; a < 16; a++) x0[a] = ls.x0[a];
        have_lin = true;  // the same linearisation, a larger lambda
        ls.mode = LM_MODE_B;
      }
    } else {  // :165-168
      *took_xi = true;
#pragma unroll
      for (int a = 0; a < 16; a++) { x0[a] = ls.xi[a]; ls.x0[a] = x0[a]; }
      const double r21 = 2 * rho - 1;
      lambda = lambda * fmax(1.0 / 3.0, 1 - r21 * r21 * r21);
#pragma unroll
      for (int a = 0; a < 36; a++) ls.Hfin[a] = ls.H[a];
      outer_done = true;
    }
    if (outer_done) {
      ls.conv = conv_now ? 1 : 0;  // :74
      ls.outer++;
      ls.nu = 2.0;
      ls.inner = 0;
      if (conv_now || ls.outer >= ls.max_outer) {  // :65
        ls.done = 1;
        ls.lambda = lambda;
        return;
      }
      // accepted and not finished (rho < 0 never gets here: it only ends an outer iteration when converged)
      if (mode == LM_MODE_BA) {
        adopt();          // the speculative linearisation was taken at xi = the new x0
        ls.cur = cur ^ 1;
      } else {
        ls.mode = LM_MODE_LIN;  // retry path: the next launch linearises at the new x0
      }
    }
  }
  ls.lambda = lambda;
  if (!have_lin) return;
  LAB_TS(5);
  rgclm::lm_try(H, b, lambda, x0, d, delta, xi);  // :136-143
  LAB_TS(6);
#pragma unroll
  for (int a = 0; a < 6; a++) ls.d[a] = d[a];
#pragma unroll
  for (int a = 0; a < 16; a++) { ls.delta[a] = delta[a]; ls.xi[a] = xi[a]; }
  LAB_TS(7);
}

}  // namespace rgck
