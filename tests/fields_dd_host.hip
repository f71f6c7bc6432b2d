// Test data generator (tests/test_dd_fields_host.py): csrc/fields_dd.h evaluated ON THE HOST.
// stdin: "kind deriv a freq n" then n distances, all floating-point numbers as hex floats;
// stdout: per distance one line of 12 hex floats, the high then the low parts of
// (f_w, f_l, f_f, d_w, d_l, d_f).  om / oml as gpk_api.cpp host_axis_const forms them.
#include <cstdio>
#include <vector>
#include "../gaussian-process-slover-for-high-freq-pde_amd/csrc/fields_dd.h"

using gpk::dd::D;

template <bool MATERN, bool COS>
static void eval(int deriv, double d, double a, double om, double oml, D* F) {
  if (deriv == 2) gpk::fields_dd<MATERN, COS, 2>(d, a, om, oml, F[0], F[1], F[2], F[3], F[4], F[5]);
  else gpk::fields_dd<MATERN, COS, 1>(d, a, om, oml, F[0], F[1], F[2], F[3], F[4], F[5]);
}

int main() {
  int kind, deriv, n;
  double a, freq;
  if (std::scanf("%d %d %la %la %d", &kind, &deriv, &a, &freq, &n) != 5 || n < 0) return 2;
  if (kind < 0 || kind > 3 || (deriv != 1 && deriv != 2)) return 2;
  std::vector<double> d(n);
  for (int e = 0; e < n; ++e)
    if (std::scanf("%la", &d[e]) != 1) return 2;
  const double om = gpk::TWO_PI * freq, oml = gpk::om_low(freq, om);
  for (int e = 0; e < n; ++e) {
    D F[6];
    if (kind == gpk::SE_COS) eval<false, true>(deriv, d[e], a, om, oml, F);
    else if (kind == gpk::MATERN52_COS) eval<true, true>(deriv, d[e], a, om, oml, F);
    else if (kind == gpk::SE) eval<false, false>(deriv, d[e], a, om, oml, F);
    else eval<true, false>(deriv, d[e], a, om, oml, F);
    for (int x = 0; x < 6; ++x) std::printf("%a ", F[x].h);
    for (int x = 0; x < 6; ++x) std::printf("%a ", F[x].l);
    std::printf("\n");
  }
  return 0;
}
