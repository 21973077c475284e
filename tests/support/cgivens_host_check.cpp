// CPU driver of the complex Givens / least-squares recurrence the shifted solver's GMRES kernel runs (flowcontrol_amd/csrc/fc_cgivens.hpp):
// reads cases "m g0 then the (m + 1) x m Hessenberg matrix, column by column, re im per entry" from stdin, feeds the columns to
// fc_cgivens_column one at a time as the kernel does, back-substitutes with one lane and with 64 emulated lanes, and prints per case
// "m residual" and the two solutions (re im per entry).
#include <cstdio>
#include <vector>

#include "../../flowcontrol_amd/csrc/fc_cgivens.hpp"

int main() {
  int m;
  double g0;
  while (std::scanf("%d %lf", &m, &g0) == 2) {
    const int ld = m + 1;
    std::vector<fc_cplx> R((size_t)m * ld), col((size_t)m + 2), sn((size_t)m), g((size_t)m + 1, fc_cplx{0.0, 0.0}), y((size_t)m), y64((size_t)m);
    std::vector<double> cs((size_t)m);
    g[0] = fc_cplx{g0, 0.0};
    double res = 0.0;
    for (int j = 0; j < m; ++j) {
      for (int i = 0; i <= m; ++i) {
        fc_cplx v;
        if (std::scanf("%lf %lf", &v.re, &v.im) != 2) return 2;
        if (i <= j + 1) col[(size_t)i] = v;
      }
      res = fc_cgivens_column(j, col.data(), cs.data(), sn.data(), g.data());
      if (res < 0.0) return 3;
      for (int i = 0; i <= j; ++i) R[(size_t)j * ld + i] = col[(size_t)i];
    }
    std::vector<fc_cplx> g1(g), g2(g);
    fc_cgivens_backsolve(m - 1, ld, R.data(), g1.data(), y.data(), 0, 1, [] {});
    // 64 lanes one after the other between two syncs: the order inside a phase does not matter, the lanes touch disjoint rows
    for (int i = m - 1; i >= 0; --i) {
      const fc_cplx yi = fc_cdiv(g2[(size_t)i], R[(size_t)i * ld + i]);
      y64[(size_t)i] = yi;
      for (int lane = 63; lane >= 0; --lane)
        for (int k = lane; k < i; k += 64) {
          const fc_cplx t = fc_cmul(R[(size_t)i * ld + k], yi);
          g2[(size_t)k] = fc_cplx{g2[(size_t)k].re - t.re, g2[(size_t)k].im - t.im};
        }
    }
    std::printf("%d %.17g\n", m, res);
    for (int i = 0; i < m; ++i) std::printf("%.17g %.17g\n", y[(size_t)i].re, y[(size_t)i].im);
    for (int i = 0; i < m; ++i) std::printf("%.17g %.17g\n", y64[(size_t)i].re, y64[(size_t)i].im);
  }
  return 0;
}
