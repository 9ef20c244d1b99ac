// lm_device_table.hip -- the scalar code of the device LM (csrc/rgc_lm.h: so3_exp_R, solve_ldlt6, lm_try; csrc/rgc_lm_decide.h: lm_step_decide)
// evaluated on tables of designed inputs: with the HOST compile of the functions and, unless --host-only is given, with the DEVICE compile in
// one-lane, one-workgroup kernels (one launch per table).  No call to the library.  tests/lm_cases.py writes the tables and reads the results.
//
//   lm_device_table [--host-only] <tables in> <results out>
//
// Builds as plain C++ (g++ -x c++ -D__HIP_PLATFORM_AMD__ -ffp-contract=off: the host half alone, on a machine without a GPU) and with
// hipcc --offload-arch=gfx950 -ffp-contract=off (both halves).
//
// File in:  8 ints {magic, sizeof(LmState), nE, nS, nT, nD, nP, 0}, then the rows of the five tables in that order:
//   E  so3_exp_R       double w[3]
//   S  solve_ldlt6     double A[36], rhs[6]
//   T  lm_try          double H[36], b[6], lambda, x0[16]
//   D  lm_step_decide  LmState, double folded[30], int mode, int cur
//   P  scripted solves LmState, double folded[30], int start, int unused: a row with start != 0 opens a script from its state, the others go on
//                      from the state the row before left; mode and cur are the state's; a finished state (done) is passed on untouched
// File out: the same 8 ints (the last one: 1 if the device half follows), the host's five result tables, then the device's:
//   E  double R[9]     S  double ok, x[6] (x = NaN where the solve refused)     T  double d[6], delta[16], xi[16]
//   D, P  LmState after the call, int took_xi, int 0
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rgc_lm_decide.h"

using rgck::LmState;

namespace {

constexpr int kMagic = 0x4C4D5431;
struct RowE { double w[3]; };
struct RowS { double A[36], rhs[6]; };
struct RowT { double H[36], b[6], lambda, x0[16]; };
struct RowD { LmState st; double folded[30]; int mode, cur; };
struct RowP { LmState st; double folded[30]; int start, unused; };
struct OutE { double R[9]; };
struct OutS { double ok, x[6]; };
struct OutT { double d[6], delta[16], xi[16]; };
struct OutD { LmState st; int took_xi, zero; };
static_assert(rgck::kStepAcc == 30, "folded[30]");

__host__ __device__ inline void eval_E(const RowE& r, OutE& o) { rgclm::so3_exp_R(r.w, o.R); }
__host__ __device__ inline void eval_S(const RowS& r, OutS& o) {
  for (int i = 0; i < 6; i++) o.x[i] = NAN;
  o.ok = rgclm::solve_ldlt6(r.A, r.rhs, o.x) ? 1.0 : 0.0;
}
__host__ __device__ inline void eval_T(const RowT& r, OutT& o) { rgclm::lm_try(r.H, r.b, r.lambda, r.x0, o.d, o.delta, o.xi); }
__host__ __device__ inline void eval_D(const RowD& r, OutD& o) {
  o.st = r.st;
  bool took = false;
  rgck::lm_step_decide(o.st, r.folded, r.mode, r.cur, &took);
  o.took_xi = took ? 1 : 0;
  o.zero = 0;
}
// row i of the scripts, given the row before it
__host__ __device__ inline void eval_P(const RowP* rows, OutD* out, int i) {
  out[i].st = rows[i].start || i == 0 ? rows[i].st : out[i - 1].st;
  bool took = false;
  if (!out[i].st.done) rgck::lm_step_decide(out[i].st, rows[i].folded, out[i].st.mode, out[i].st.cur, &took);
  out[i].took_xi = took ? 1 : 0;
  out[i].zero = 0;
}

#ifdef __HIPCC__
// one lane walks the table
__global__ void k_table_E(const RowE* in, OutE* out, int n) { for (int i = 0; i < n; i++) eval_E(in[i], out[i]); }
__global__ void k_table_S(const RowS* in, OutS* out, int n) { for (int i = 0; i < n; i++) eval_S(in[i], out[i]); }
__global__ void k_table_T(const RowT* in, OutT* out, int n) { for (int i = 0; i < n; i++) eval_T(in[i], out[i]); }
__global__ void k_table_D(const RowD* in, OutD* out, int n) { for (int i = 0; i < n; i++) eval_D(in[i], out[i]); }
__global__ void k_table_P(const RowP* in, OutD* out, int n) { for (int i = 0; i < n; i++) eval_P(in, out, i); }

#define HIP_OK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return false; } \
  } while (0)

// a table's rows to the device, one launch of one lane, its results back (the copy back waits for the launch)
template <typename In, typename Out, typename K>
bool on_device(K kernel, const std::vector<In>& in, std::vector<Out>& out) {
  out.assign(in.size(), Out{});
  if (in.empty()) return true;
  In* d_in = nullptr;
  Out* d_out = nullptr;
  HIP_OK(hipMalloc(&d_in, in.size() * sizeof(In)));
  HIP_OK(hipMalloc(&d_out, in.size() * sizeof(Out)));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(In), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0, in.size() * sizeof(Out)));
  hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, 0, (const In*)d_in, d_out, (int)in.size());
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(out.data(), d_out, in.size() * sizeof(Out), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));
  return true;
}
#endif

template <typename T>
bool read_rows(FILE* f, std::vector<T>& v, int n) {
  v.resize((size_t)n);
  return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}
template <typename T>
bool write_rows(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char** argv) {
  bool host_only = false;
  const char* paths[2] = {nullptr, nullptr};
  int np = 0;
  for (int a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "--host-only")) host_only = true;
    else if (np < 2) paths[np++] = argv[a];
  }
  if (np != 2) { fprintf(stderr, "usage: lm_device_table [--host-only] <tables in> <results out>\n"); return 2; }
#ifndef __HIPCC__
  if (!host_only) { fprintf(stderr, "this build holds the host half only: pass --host-only\n"); return 2; }
#endif
  FILE* f = fopen(paths[0], "rb");
  int hdr[8];
  if (!f || fread(hdr, sizeof(int), 8, f) != 8 || hdr[0] != kMagic) { fprintf(stderr, "cannot read the tables of %s\n", paths[0]); return 2; }
  if (hdr[1] != (int)sizeof(LmState)) { fprintf(stderr, "sizeof(LmState) is %d, the tables were written for %d\n", (int)sizeof(LmState), hdr[1]); return 2; }
  for (int t = 2; t < 7; t++)
    if (hdr[t] < 0 || hdr[t] > 100000) { fprintf(stderr, "table %d: %d rows\n", t - 2, hdr[t]); return 2; }
  std::vector<RowE> E; std::vector<RowS> S; std::vector<RowT> T; std::vector<RowD> D; std::vector<RowP> P;
  if (!read_rows(f, E, hdr[2]) || !read_rows(f, S, hdr[3]) || !read_rows(f, T, hdr[4]) || !read_rows(f, D, hdr[5]) || !read_rows(f, P, hdr[6])) {
    fprintf(stderr, "%s is shorter than its header says\n", paths[0]);
    return 2;
  }
  fclose(f);

  std::vector<OutE> oE(E.size()); std::vector<OutS> oS(S.size()); std::vector<OutT> oT(T.size()); std::vector<OutD> oD(D.size()), oP(P.size());
  for (size_t i = 0; i < E.size(); i++) eval_E(E[i], oE[i]);
  for (size_t i = 0; i < S.size(); i++) eval_S(S[i], oS[i]);
  for (size_t i = 0; i < T.size(); i++) eval_T(T[i], oT[i]);
  for (size_t i = 0; i < D.size(); i++) eval_D(D[i], oD[i]);
  for (size_t i = 0; i < P.size(); i++) eval_P(P.data(), oP.data(), (int)i);

  std::vector<OutE> gE; std::vector<OutS> gS; std::vector<OutT> gT; std::vector<OutD> gD, gP;
#ifdef __HIPCC__
  if (!host_only) {
    if (!on_device(k_table_E, E, gE) || !on_device(k_table_S, S, gS) || !on_device(k_table_T, T, gT) || !on_device(k_table_D, D, gD) ||
        !on_device(k_table_P, P, gP))
      return 1;
  }
#endif
  FILE* g = fopen(paths[1], "wb");
  hdr[7] = host_only ? 0 : 1;
  bool ok = g && fwrite(hdr, sizeof(int), 8, g) == 8 && write_rows(g, oE) && write_rows(g, oS) && write_rows(g, oT) && write_rows(g, oD) && write_rows(g, oP);
  if (ok && !host_only) ok = write_rows(g, gE) && write_rows(g, gS) && write_rows(g, gT) && write_rows(g, gD) && write_rows(g, gP);
  if (!ok || fclose(g) != 0) { fprintf(stderr, "cannot write %s\n", paths[1]); return 2; }
  printf("lm_device_table: %d so3_exp_R, %d solve_ldlt6, %d lm_try, %d lm_step_decide, %d script rows; %s\n", hdr[2], hdr[3], hdr[4], hdr[5], hdr[6],
         host_only ? "host" : "host and device");
  return 0;
}
