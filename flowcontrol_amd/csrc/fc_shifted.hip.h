// Kernels of the complex-shifted direct solver (fc_setup_shifted / fc_solve_shifted).  Included by fc_hip.hip only.
//
// The shifted operator M = sigma E - A (sigma complex, A and E real on the handle's CSR pattern) is factorised in its real-equivalent
// form: every complex unknown z_i = (re, im) becomes the dof pair (2 i, 2 i + 1) of a system of order 2 N, and every complex entry
// m = mr + i mi the real 2x2 block [[mr, -mi], [mi, mr]].  A complex vector in interleaved storage (re, im per dof) IS the real vector of
// the doubled system in its original numbering, so the factor sweeps of the real solver run on it unchanged.  The kernels here are the
// pieces that know about the complex structure:
//   fc_shifted_scatter   (A_k, E_k) read once per entry, the 2x2 block for sigma written into the doubled fronts (fc_front_scatter's role)
//   fc_shifted_spmv      y = (s E - t A) x or b - (s E - t A) x on interleaved complex vectors, two value arrays over ONE pattern
//   fc_cmultidot(+_reduce), fc_cgs_update, fc_cbasis_combine: classical Gram-Schmidt for the Arnoldi basis (complex, interleaved)
//   fc_cgmres_begin, fc_cgmres_givens, fc_cnormalize_store: the small side of the complex GMRES (fc_shifted_set_krylov): rotations,
//                        residual norm and stop flag stay in device memory (the recurrence itself: fc_cgivens.hpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_cgivens.hpp"

// fronts[dst4[4k + 2a + b]] = block entry (a, b) of m_k = sigma E_k - A_k:  (0,0) = (1,1) = mr, (0,1) = -mi, (1,0) = mi
__global__ __launch_bounds__(256) void fc_shifted_scatter(int64_t nnz, const int64_t* __restrict__ dst4, const double* __restrict__ a,
                                                          const double* __restrict__ e, double s_re, double s_im,
                                                          double* __restrict__ fronts) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const double ek = e[k];
  const double mr = s_re * ek - a[k], mi = s_im * ek;
  const longlong2 d01 = *reinterpret_cast<const longlong2*>(dst4 + 4 * k);
  const longlong2 d23 = *reinterpret_cast<const longlong2*>(dst4 + 4 * k + 2);
  fronts[d01.x] = mr;
  fronts[d01.y] = -mi;
  fronts[d23.x] = mi;
  fronts[d23.y] = mr;
}

// y_i = sum_k (s e_k - t a_k) x_j  (complex s, real t), plus pin_val x_i on row pin_row (-1: none), or b_i - that when b != nullptr.  L lanes per row (L <= 64, a power of two),
// 256 / L rows per workgroup.  partial (optional): per workgroup |y|^2 at [blockIdx.x] and |b|^2 at [gridDim.x + blockIdx.x] (the two
// segments fc_reduce_final folds in a fixed order)
template <int L>
__global__ __launch_bounds__(256) void fc_shifted_spmv(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ a, const double* __restrict__ e, double s_re, double s_im,
                                                       double t, const double2* __restrict__ x, const double2* __restrict__ b,
                                                       double2* __restrict__ y, double* __restrict__ partial, int pin_row, double pin_val) {
  const int lane = threadIdx.x % L;
  const int row = blockIdx.x * (256 / L) + threadIdx.x / L;
  double yr = 0.0, yi = 0.0;
  if (row < n) {
    const int k1 = rowptr[row + 1];
    for (int k = rowptr[row] + lane; k < k1; k += L) {
      const double ek = e[k];
      const double mr = s_re * ek - t * a[k], mi = s_im * ek;
      const double2 xv = x[col[k]];
      yr += mr * xv.x - mi * xv.y;
      yi += mr * xv.y + mi * xv.x;
    }
  }
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) {
    yr += __shfl_down(yr, off, L);
    yi += __shfl_down(yi, off, L);
  }
  double r2 = 0.0, b2 = 0.0;
  if (lane == 0 && row < n) {
    if (row == pin_row) {  // the pressure pin of an enclosed flow: pin_val = t * shift on the diagonal of this row
      const double2 xv = x[row];
      yr += pin_val * xv.x;
      yi += pin_val * xv.y;
    }
    double2 out = make_double2(yr, yi);
    if (b) {
      const double2 bv = b[row];
      out = make_double2(bv.x - yr, bv.y - yi);
      b2 = bv.x * bv.x + bv.y * bv.y;
    }
    y[row] = out;
    r2 = out.x * out.x + out.y * out.y;
  }
  if (!partial) return;
  __shared__ double red[2][256];
  red[0][threadIdx.x] = r2;
  red[1][threadIdx.x] = b2;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[gridDim.x + blockIdx.x] = red[1][0];
  }
}

// partial[(i gx + blockIdx.x)][2] = chunk of V_i^H w  (V: nv interleaved complex vectors of n entries, stride n; grid (gx, nv))
__global__ __launch_bounds__(256) void fc_cmultidot(int n, const double2* __restrict__ V, const double2* __restrict__ w,
                                                    double* __restrict__ partial) {
  const int i = blockIdx.y;
  const double2* __restrict__ v = V + (size_t)i * n;
  double sr = 0.0, si = 0.0;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
    const double2 p = v[k], q = w[k];
    sr += p.x * q.x + p.y * q.y;  // conj(p) q
    si += p.x * q.y - p.y * q.x;
  }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = sr;
  red[1][threadIdx.x] = si;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const size_t o = 2 * ((size_t)i * gridDim.x + blockIdx.x);
    partial[o] = red[0][0];
    partial[o + 1] = red[1][0];
  }
}
// h[i] = sum of the gx partials of dot i, fixed order; one wave per dot
__global__ void fc_cmultidot_reduce(int gx, const double* __restrict__ partial, double2* __restrict__ h) {
  const int i = blockIdx.x;
  double sr = 0.0, si = 0.0;
  for (int k = threadIdx.x; k < gx; k += 64) {
    sr += partial[2 * ((size_t)i * gx + k)];
    si += partial[2 * ((size_t)i * gx + k) + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sr += __shfl_down(sr, off, 64);
    si += __shfl_down(si, off, 64);
  }
  if (threadIdx.x == 0) h[i] = make_double2(sr, si);
}
// w -= sum_i h[i] V_i  (the projection of one classical Gram-Schmidt pass)
__global__ __launch_bounds__(256) void fc_cgs_update(int n, int nv, const double2* __restrict__ V, const double2* __restrict__ h,
                                                     double2* __restrict__ w) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double2 s = w[k];
  for (int i = 0; i < nv; ++i) {
    const double2 c = h[i], v = V[(size_t)i * n + k];
    s.x -= c.x * v.x - c.y * v.y;
    s.y -= c.x * v.y + c.y * v.x;
  }
  w[k] = s;
}
// out_c = sum_j V_j Q[j][c] for c < k (Q: m x k complex, row-major; out: k vectors of stride n) -- the restart of the Krylov-Schur
// iteration and the Ritz vectors
__global__ __launch_bounds__(256) void fc_cbasis_combine(int n, int m, int k, const double2* __restrict__ V, const double2* __restrict__ Q,
                                                         double2* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (row >= n || c >= k) return;
  double2 s = make_double2(0.0, 0.0);
  for (int j = 0; j < m; ++j) {
    const double2 q = Q[(size_t)j * k + c], v = V[(size_t)j * n + row];
    s.x += v.x * q.x - v.y * q.y;
    s.y += v.x * q.y + v.y * q.x;
  }
  out[(size_t)c * n + row] = s;
}
// out = alpha * in (real alpha on 2 n doubles)
__global__ void fc_scale(int n, double alpha, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = alpha * in[i];
}
// x *= alpha
__global__ void fc_scale_inplace(int n, double alpha, double* x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] *= alpha;
}
// y[r][c] = sum_k w_k X_c[idx_k] over the sparse rows of C (one thread per (row, column)): C X for the frequency response
__global__ void fc_cproject(int nrow, int nrhs, int n, const int* __restrict__ rowptr, const int* __restrict__ idx,
                            const double* __restrict__ w, const double2* __restrict__ X, double2* __restrict__ y) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nrow * nrhs) return;
  const int r = t / nrhs, c = t % nrhs;
  double2 s = make_double2(0.0, 0.0);
  for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const double2 v = X[(size_t)c * n + idx[k]];
    s.x += w[k] * v.x;
    s.y += w[k] * v.y;
  }
  y[t] = s;
}
// interleave / split complex vectors at the boundary (host arrays arrive as separate re / im parts)
__global__ void fc_cinterleave(int n, const double* __restrict__ re, const double* __restrict__ im, double2* __restrict__ z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = make_double2(re[i], im ? im[i] : 0.0);
}
__global__ void fc_csplit(int n, const double2* __restrict__ z, double* __restrict__ re, double* __restrict__ im) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const double2 v = z[i];
    re[i] = v.x;
    im[i] = v.y;
  }
}

// ── complex GMRES: the small side ──────────────────────────────────────────────────────────────────────────────────────────────
// gm (doubles), ld = m + 1: R [m][ld] complex, column-major | sn [m] complex | g [m + 1] complex | y [m] complex | rec [8] | cs [m]
// (the one real array of odd length comes last: every complex array starts on a 16-byte boundary, y is read as double2)
// rec: 0 state (0 running, 1 converged before the cycle, 3 converged, 4 cycle closed, -4 breakdown), 1 columns of the cycle,
//      2 |residual|^2 (Arnoldi estimate), 3 |b|^2, 4 norm of the vector to normalise next
constexpr int kCgmMaxRestart = 256;
enum { CG_STATE = 0, CG_USED = 1, CG_RNORM2 = 2, CG_BNORM2 = 3, CG_BETA = 4, CG_REC = 8 };
struct FcCgm {
  fc_cplx* R;
  double* cs;
  fc_cplx* sn;
  fc_cplx* g;
  fc_cplx* y;
  double* rec;
};
__host__ __device__ inline size_t fc_cgm_size(int m) { return 2 * (size_t)m * (m + 1) + m + 2 * (size_t)m + 2 * (size_t)(m + 1) + 2 * (size_t)m + CG_REC; }
__host__ __device__ inline FcCgm fc_cgm_layout(double* gm, int m) {
  FcCgm L;
  L.R = reinterpret_cast<fc_cplx*>(gm);
  L.sn = L.R + (size_t)m * (m + 1);
  L.g = L.sn + m;
  L.y = L.g + (m + 1);
  L.rec = reinterpret_cast<double*>(L.y + m);
  L.cs = L.rec + CG_REC;
  return L;
}
// start of a cycle: res2 = (|r|^2, |b|^2) of the current iterate; g = (|r|, 0, ...), state -> running or converged.  One wave.
__global__ __launch_bounds__(64) void fc_cgmres_begin(int m, double* gm, const double* __restrict__ res2, double rtol) {
  const FcCgm L = fc_cgm_layout(gm, m);
  const double r2 = res2[0], b2 = res2[1];
  for (int i = threadIdx.x; i <= m; i += 64) L.g[i] = fc_cplx{i == 0 ? sqrt(r2) : 0.0, 0.0};
  if (threadIdx.x != 0) return;
  L.rec[CG_USED] = 0.0;
  L.rec[CG_RNORM2] = r2;
  L.rec[CG_BNORM2] = b2;
  L.rec[CG_BETA] = sqrt(r2);
  L.rec[CG_STATE] = (sqrt(r2) <= rtol * sqrt(b2) || !(b2 > 0.0)) ? 1.0 : 0.0;
}
// out = w / beta (beta on the device: rec[CG_BETA]); nothing once the cycle has stopped.  double2 per lane, consecutive lanes.
__global__ __launch_bounds__(256) void fc_cnormalize_store(int n, const double2* w, const double* __restrict__ rec, double2* out) {
  if (rec[CG_STATE] != 0.0) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double inv = 1.0 / rec[CG_BETA];
  const double2 v = w[k];
  out[k] = make_double2(inv * v.x, inv * v.y);
}
// Column j of the cycle, one wave: the Hessenberg column h1 + h2 (the two Gram-Schmidt passes) with |w| below it (folded here from the
// gx partial sums of fc_cmultidot, in fc_cmultidot_reduce's order) goes through the rotations in ONE LDS array; lane 0 runs the
// recurrence (fc_cgivens_column), the wave stores the column of R and, when the estimate meets rtol or `close` is set, shares the
// back substitution y = R^-1 g.
__global__ __launch_bounds__(64) void fc_cgmres_givens(int j, int m, int close, double* gm, const double2* __restrict__ h1,
                                                       const double2* __restrict__ h2, const double* __restrict__ npart, int gx, double rtol) {
  const FcCgm L = fc_cgm_layout(gm, m);
  if (L.rec[CG_STATE] != 0.0) return;
  __shared__ fc_cplx col[kCgmMaxRestart + 2];
  __shared__ int stop;
  const int lane = threadIdx.x;
  double nsum = 0.0;
  for (int k = lane; k < gx; k += 64) nsum += npart[2 * (size_t)k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nsum += __shfl_down(nsum, off, 64);
  for (int i = lane; i <= j; i += 64) {
    const double2 a = h1[i], b = h2[i];
    col[i] = fc_cplx{a.x + b.x, a.y + b.y};
  }
  if (lane == 0) col[j + 1] = fc_cplx{sqrt(fmax(nsum, 0.0)), 0.0};
  __syncthreads();
  if (lane == 0) {
    L.rec[CG_BETA] = col[j + 1].re;
    const double res = fc_cgivens_column(j, col, L.cs, L.sn, L.g);
    if (res < 0.0) {
      L.rec[CG_STATE] = -4.0;
      stop = -1;
    } else {
      const bool conv = res <= rtol * sqrt(L.rec[CG_BNORM2]);
      L.rec[CG_USED] = (double)(j + 1);
      L.rec[CG_RNORM2] = res * res;
      stop = (conv || close) ? 1 : 0;
      if (stop) L.rec[CG_STATE] = conv ? 3.0 : 4.0;
    }
  }
  __syncthreads();
  if (stop < 0) return;
  for (int i = lane; i <= j; i += 64) L.R[(size_t)j * (m + 1) + i] = col[i];
  if (!stop) return;
  __syncthreads();
  for (int i = lane; i <= j; i += 64) col[i] = L.g[i];
  fc_cgivens_backsolve(j, m + 1, L.R, col, L.y, lane, 64, [] { __syncthreads(); });
}
