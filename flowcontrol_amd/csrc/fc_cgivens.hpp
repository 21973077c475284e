// fc_cgivens.hpp — the complex Givens / least-squares recurrence of the shifted solver's GMRES (fc_cgmres_givens, fc_shifted.hip.h).
//
// One Hessenberg column at a time: the stored rotations are applied to the new column, one new rotation annihilates its subdiagonal
// entry, the rotated right-hand side g follows; |g[j + 1]| is the residual norm of the least-squares problem min |g0 e1 - H y|.  The
// back substitution y = R^-1 g runs column by column, so that several lanes can share it (every lane owns the rows lane, lane + nl,
// ...); one lane (lane = 0, nl = 1, a no-op sync) is the host's form of the same loop.
// No HIP dependency: included by the kernel and by plain C++ (tests/support/cgivens_host_check.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FC_CG_HD __host__ __device__ inline
#else
#define FC_CG_HD inline
#endif

struct fc_cplx {
  double re, im;
};
FC_CG_HD fc_cplx fc_cmul(fc_cplx a, fc_cplx b) { return fc_cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
FC_CG_HD fc_cplx fc_cmulc(fc_cplx a, fc_cplx b) { return fc_cplx{a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im}; }  // a conj(b)
FC_CG_HD fc_cplx fc_cdiv(fc_cplx a, fc_cplx b) {
  const double d = b.re * b.re + b.im * b.im;
  const fc_cplx t = fc_cmulc(a, b);
  return fc_cplx{t.re / d, t.im / d};
}

// Column j of the Hessenberg matrix (col[0 .. j + 1], overwritten by column j of R), rotations (cs real, sn complex:
// G_i = [[cs_i, sn_i], [-conj(sn_i), cs_i]]) and right-hand side g[0 .. j + 1].  Returns |g[j + 1]|, or -1 when the column is
// zero / not finite (breakdown).
FC_CG_HD double fc_cgivens_column(int j, fc_cplx* col, double* cs, fc_cplx* sn, fc_cplx* g) {
  for (int i = 0; i < j; ++i) {
    const fc_cplx x = col[i], y = col[i + 1], s = sn[i];
    const double c = cs[i];
    const fc_cplx sy = fc_cmul(s, y), sx = fc_cmulc(x, s);  // sx = conj(s) x
    col[i] = fc_cplx{c * x.re + sy.re, c * x.im + sy.im};
    col[i + 1] = fc_cplx{c * y.re - sx.re, c * y.im - sx.im};
  }
  const fc_cplx a = col[j], b = col[j + 1];
  const double na = hypot(a.re, a.im), nb = hypot(b.re, b.im), r = hypot(na, nb);
  if (!(r > 0.0) || !isfinite(r)) return -1.0;
  fc_cplx ph{1.0, 0.0};  // a / |a|
  if (na > 0.0) ph = fc_cplx{a.re / na, a.im / na};
  const double c = na / r;
  const fc_cplx s = na > 0.0 ? fc_cmulc(ph, fc_cplx{b.re / r, b.im / r}) : fc_cplx{1.0, 0.0};
  cs[j] = c;
  sn[j] = s;
  col[j] = na > 0.0 ? fc_cplx{ph.re * r, ph.im * r} : b;
  col[j + 1] = fc_cplx{0.0, 0.0};
  const fc_cplx gj = g[j], sg = fc_cmulc(gj, s);
  g[j + 1] = fc_cplx{-sg.re, -sg.im};
  g[j] = fc_cplx{c * gj.re, c * gj.im};
  return hypot(g[j + 1].re, g[j + 1].im);
}

// y[0 .. j] = R^-1 g for the upper-triangular R (column k at R + k ld); g is overwritten.  Lane `lane` of `nl` updates the rows
// lane, lane + nl, ...; sync() makes the lanes' writes to g visible to each other (nothing to do for one lane).
template <class Sync>
FC_CG_HD void fc_cgivens_backsolve(int j, int ld, const fc_cplx* R, fc_cplx* g, fc_cplx* y, int lane, int nl, Sync sync) {
  for (int i = j; i >= 0; --i) {
    sync();
    const fc_cplx yi = fc_cdiv(g[i], R[(size_t)i * ld + i]);
    if (lane == 0) y[i] = yi;
    for (int k = lane; k < i; k += nl) {
      const fc_cplx t = fc_cmul(R[(size_t)i * ld + k], yi);
      g[k] = fc_cplx{g[k].re - t.re, g[k].im - t.im};
    }
  }
}
