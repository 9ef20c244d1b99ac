// The HOST compile of csrc/rgc_terms.h's Gauss-Newton term and R C R^T on a table of designed rows (tests/test_terms_reference.py writes the
// table, builds this as plain C++ with -ffp-contract=off, runs it once and holds the results to a longdouble reference).  No GPU, no HIP runtime.
//   terms_table <rows.bin> <results.bin>
// row in : M[6] q[3] e[3] w R[9] C[6]                      (28 doubles)
// row out: sum/H[28] sum/cost[28] set/H[28] set/cost[28] RCR[6]   (118 doubles); the accumulators start from 0
#include <cstdio>
#include <vector>

#include "rgc_terms.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[28];
  while (fread(buf, sizeof(double), 28, f) == 28) in.insert(in.end(), buf, buf + 28);
  fclose(f);
  const size_t n = in.size() / 28;
  std::vector<double> out(n * 118, 0.0);
  for (size_t i = 0; i < n; i++) {
    const double* r = &in[i * 28];
    const double M[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
    const double C[6] = {r[22], r[23], r[24], r[25], r[26], r[27]};
    const double R[9] = {r[13], r[14], r[15], r[16], r[17], r[18], r[19], r[20], r[21]};
    double a[4][28] = {}, rcr[6];
    rgck::gn_term<true>(M, r[6], r[7], r[8], r[9], r[10], r[11], r[12], 1, a[0]);
    rgck::gn_term<true>(M, r[6], r[7], r[8], r[9], r[10], r[11], r[12], 0, a[1]);
    rgck::gn_term<false>(M, r[6], r[7], r[8], r[9], r[10], r[11], r[12], 1, a[2]);
    rgck::gn_term<false>(M, r[6], r[7], r[8], r[9], r[10], r[11], r[12], 0, a[3]);
    rgck::rcrt6(R, C, rcr);
    double* o = &out[i * 118];
    for (int k = 0; k < 4; k++)
      for (int u = 0; u < 28; u++) o[k * 28 + u] = a[k][u];
    for (int u = 0; u < 6; u++) o[112 + u] = rcr[u];
  }
  f = fopen(argv[2], "wb");
  if (!f) return 4;
  const bool ok = fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return (fclose(f) == 0 && ok) ? 0 : 5;
}
