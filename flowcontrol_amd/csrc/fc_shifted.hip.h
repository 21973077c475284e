// Kernels of the complex-shifted direct solver (fc_setup_shifted / fc_solve_shifted).  Included by fc_hip.hip only.
//
// The shifted operator M = sigma E - A (sigma complex, A and E real on the handle's CSR pattern) is factorised in its real-equivalent
// form: every complex unknown z_i = (re, im) becomes the dof pair (2 i, 2 i + 1) of a system of order 2 N, and every complex entry
// m = mr + i mi the real 2x2 block [[mr, -mi], [mi, mr]].  A complex vector in interleaved storage (re, im per dof) IS the real vector of
// the doubled system in its original numbering, so the factor sweeps of the real solver run on it unchanged.  The kernels here are the
// pieces that know about the complex structure:
//   fc_shifted_scatter   (A_k, E_k) read once per entry, the 2x2 block for sigma written into the doubled fronts (fc_front_scatter's role)
//   fc_shifted_spmv      y = (s E - t A) x or b - (s E - t A) x on interleaved complex vectors, two value arrays over ONE pattern
//   fc_csr_gather_values the values of A^T, E^T on the same pattern (adjoint mode: the SpMVs then run on them with the conjugated shift)
//   fc_cmultidot(+_reduce), fc_cgs_update, fc_cbasis_combine: classical Gram-Schmidt for the Arnoldi basis (complex, interleaved)
//   fc_cgmres_begin, fc_cgmres_givens, fc_cnormalize_store: the small side of the complex GMRES (fc_shifted_set_krylov): rotations,
//                        residual norm and stop flag stay in device memory (the recurrence itself: fc_cgivens.hpp)
//   fc_snap_push, fc_snap_load, fc_snap_gram(+_reduce), fc_snap_combine: snapshot sets for balanced reduced models (fc_shifted_snap_*):
//                        scaled copies into a set, the tall-skinny product L^T W on the fp64 matrix cores, the modes
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

// a_t[k] = a[tpos[k]], e_t[k] = e[tpos[k]]: the values of A^T and E^T on the handle's own (structurally symmetric) pattern; tpos[k] is
// the position of entry (j, i) for the entry k = (i, j) (fc_shifted_set_adjoint)
__global__ __launch_bounds__(256) void fc_csr_gather_values(int64_t nnz, const int* __restrict__ tpos, const double* __restrict__ a,
                                                            const double* __restrict__ e, double* __restrict__ a_t, double* __restrict__ e_t) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int q = tpos[k];
  a_t[k] = a[q];
  e_t[k] = e[q];
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

// ── block solves (fc_shifted_set_block / fc_solve_shifted_block): KB columns side by side ──────────────────────────────────────
// A block vector is the real matrix [2 n][KB] of the batched factor apply (fc_batch.hip.h): complex entry i of column c sits at rows
// 2 i (re) and 2 i + 1 (im), the column index runs fastest.  Every column is a GMRES of its own -- own shift, basis, rotations, record
// -- and the columns advance in lock step, so that one pass over the factors, the matrix and the basis serves all of them.  A column
// whose state is not "running" is FROZEN: no kernel below writes its iterate, basis or record.  `mode` names what frozen means where
// the kernel runs: 0 inside a cycle (anything but running), 1 at a cycle's end (finished before this cycle, or broken down).
// gmb: per column an area of fc_cgm_stride_b(m) doubles (fc_cgm_layout; its own rec is unused) | rec [KB][CG_REC], read by the host
// in one copy.
__host__ __device__ inline size_t fc_cgm_stride_b(int m) { return (fc_cgm_size(m) + 1) & ~(size_t)1; }
__host__ __device__ inline size_t fc_cgm_size_b(int m, int KB) { return (size_t)KB * (fc_cgm_stride_b(m) + CG_REC); }
__host__ __device__ inline FcCgm fc_cgm_layout_b(double* gmb, int m, int c, int KB) {
  FcCgm L = fc_cgm_layout(gmb + (size_t)c * fc_cgm_stride_b(m), m);
  L.rec = gmb + (size_t)KB * fc_cgm_stride_b(m) + (size_t)c * CG_REC;
  return L;
}
__device__ inline bool fc_state_frozen(double s, int mode) { return mode == 0 ? s != 0.0 : (s == 1.0 || s < 0.0); }
__device__ inline bool fc_col_frozen(const double* __restrict__ rec, int c, int mode) {
  return fc_state_frozen(rec[(size_t)c * CG_REC + CG_STATE], mode);
}

// Y_c = (s_c E - t_c A) X_c, or B_c - that, for all KB columns: sh[c] = (s_re, s_im, t).  One wave per row: lane = (l, c) with the
// column c fastest, the L = 64 / KB lanes l of a column split the row's entries; a[k], e[k], col[k] are ONE address for the KB lanes of
// an l (read once for all columns), x a run of KB consecutive doubles.  The pin adds t_c shift x on row pin_row.  partial (optional):
// per workgroup and column |y|^2 at [2 blockIdx.x][c], |b|^2 at [2 blockIdx.x + 1][c] (fc_cnorm_reduce_b folds them in a fixed
// order).  rec (optional): frozen columns are not stored.
template <int KB, int L>
__global__ __launch_bounds__(256) void fc_shifted_spmv_b(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const double* __restrict__ a, const double* __restrict__ e,
                                                         const double* __restrict__ sh, const double* __restrict__ x,
                                                         const double* __restrict__ b, double* __restrict__ y, double* __restrict__ partial,
                                                         int pin_row, double pin_shift, const double* __restrict__ rec, int mode) {
  static_assert(KB * L == 64, "one wave per row");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane % KB, l = lane / KB;
  const int row = blockIdx.x * 4 + wave;
  const double s_re = sh[3 * c], s_im = sh[3 * c + 1], t = sh[3 * c + 2];
  double yr = 0.0, yi = 0.0;
  if (row < n) {
    const int k1 = rowptr[row + 1];
    for (int k = rowptr[row] + l; k < k1; k += L) {
      const double ek = e[k];
      const double mr = s_re * ek - t * a[k], mi = s_im * ek;
      const size_t j = (size_t)col[k];
      const double xr = x[2 * j * KB + c], xi = x[(2 * j + 1) * KB + c];
      yr += mr * xr - mi * xi;
      yi += mr * xi + mi * xr;
    }
  }
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) {
    yr += __shfl_down(yr, off * KB, 64);
    yi += __shfl_down(yi, off * KB, 64);
  }
  double r2 = 0.0, b2 = 0.0;
  if (l == 0 && row < n) {
    const size_t o = 2 * (size_t)row * KB + c;
    if (row == pin_row) {
      yr += t * pin_shift * x[o];
      yi += t * pin_shift * x[o + KB];
    }
    if (b) {
      const double br = b[o], bi = b[o + KB];
      yr = br - yr;
      yi = bi - yi;
      b2 = br * br + bi * bi;
    }
    if (!(rec && fc_col_frozen(rec, c, mode))) {
      y[o] = yr;
      y[o + KB] = yi;
    }
    r2 = yr * yr + yi * yi;
  }
  if (!partial) return;
  __shared__ double red[4][2][KB];
  if (l == 0) {
    red[wave][0][c] = r2;
    red[wave][1][c] = b2;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * KB) {
    const int w = threadIdx.x / KB, cc = threadIdx.x % KB;
    partial[((size_t)blockIdx.x * 2 + w) * KB + cc] = ((red[0][w][cc] + red[1][w][cc]) + red[2][w][cc]) + red[3][w][cc];
  }
}
// out[c] = (|y_c|^2, |b_c|^2) from the g workgroup partials of fc_shifted_spmv_b, fixed order; one workgroup per column
__global__ __launch_bounds__(256) void fc_cnorm_reduce_b(int g, int KB, const double* __restrict__ partial, double* __restrict__ out,
                                                         const double* __restrict__ rec, int mode) {
  const int c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < g; i += 256) {
    s0 += partial[((size_t)i * 2) * KB + c];
    s1 += partial[((size_t)i * 2 + 1) * KB + c];
  }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && !(rec && fc_col_frozen(rec, c, mode))) {
    out[2 * c] = red[0][0];
    out[2 * c + 1] = red[1][0];
  }
}

// partial[((i gx + blockIdx.x) KB + c)][2] = chunk of V_{i,c}^H w_c  (V: nv block vectors; grid (gx, nv)); thread = (row slice, c)
template <int KB>
__global__ __launch_bounds__(256) void fc_cmultidot_b(int n, const double* __restrict__ V, const double* __restrict__ w,
                                                      double* __restrict__ partial) {
  constexpr int R = 256 / KB;
  const int i = blockIdx.y, c = threadIdx.x % KB, r = threadIdx.x / KB;
  const double* __restrict__ v = V + (size_t)i * 2 * n * KB;
  double sr = 0.0, si = 0.0;
  for (int k = blockIdx.x * R + r; k < n; k += gridDim.x * R) {
    const size_t o = 2 * (size_t)k * KB + c;
    const double pr = v[o], pi = v[o + KB], qr = w[o], qi = w[o + KB];
    sr += pr * qr + pi * qi;  // conj(p) q
    si += pr * qi - pi * qr;
  }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = sr;
  red[1][threadIdx.x] = si;
  __syncthreads();
  for (int st = 128; st >= KB; st >>= 1) {  // (thread + st is the same column: KB divides st)
    if ((int)threadIdx.x < st) {
      red[0][threadIdx.x] += red[0][threadIdx.x + st];
      red[1][threadIdx.x] += red[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < KB) {
    const size_t o = 2 * (((size_t)i * gridDim.x + blockIdx.x) * KB + c);
    partial[o] = red[0][threadIdx.x];
    partial[o + 1] = red[1][threadIdx.x];
  }
}
// h[i][c] = sum of the gx partials of dot (i, c) in the order of the workgroups; one workgroup per i, one lane per column
__global__ __launch_bounds__(64) void fc_cmultidot_reduce_b(int gx, int KB, const double* __restrict__ partial, double2* __restrict__ h) {
  const int i = blockIdx.x, c = threadIdx.x;
  if (c >= KB) return;
  double sr = 0.0, si = 0.0;
  for (int k = 0; k < gx; ++k) {
    const size_t o = 2 * (((size_t)i * gx + k) * KB + c);
    sr += partial[o];
    si += partial[o + 1];
  }
  h[(size_t)i * KB + c] = make_double2(sr, si);
}
// w_c -= sum_i h[i][c] V_{i,c}; thread = (complex row, c)
template <int KB>
__global__ __launch_bounds__(256) void fc_cgs_update_b(int n, int nv, const double* __restrict__ V, const double2* __restrict__ h,
                                                       double* __restrict__ w, const double* __restrict__ rec) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t k = t / KB;
  if (k >= n || fc_col_frozen(rec, c, 0)) return;
  const size_t o = 2 * (size_t)k * KB + c;
  double sr = w[o], si = w[o + KB];
  for (int i = 0; i < nv; ++i) {
    const double2 hc = h[(size_t)i * KB + c];
    const double* __restrict__ v = V + (size_t)i * 2 * n * KB;
    const double vr = v[o], vi = v[o + KB];
    sr -= hc.x * vr - hc.y * vi;
    si -= hc.x * vi + hc.y * vr;
  }
  w[o] = sr;
  w[o + KB] = si;
}
// out_c = w_c / beta_c (rec[c][CG_BETA]) for the running columns
template <int KB>
__global__ __launch_bounds__(256) void fc_cnormalize_store_b(int n, const double* w, const double* __restrict__ rec, double* out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t k = t / KB;
  if (k >= n || fc_col_frozen(rec, c, 0)) return;
  const double inv = 1.0 / rec[(size_t)c * CG_REC + CG_BETA];
  const size_t o = 2 * (size_t)k * KB + c;
  out[o] = inv * w[o];
  out[o + KB] = inv * w[o + KB];
}
// out_c = V_{0 .. used_c, c} y_c, the update of a cycle in the preconditioned variable; zero for a frozen column
template <int KB>
__global__ __launch_bounds__(256) void fc_cbasis_combine_b(int n, int m, const double* __restrict__ V, double* gmb, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t k = t / KB;
  if (k >= n) return;
  const FcCgm L = fc_cgm_layout_b(gmb, m, c, KB);
  const int used = fc_state_frozen(L.rec[CG_STATE], 1) ? 0 : (int)L.rec[CG_USED];
  const size_t o = 2 * (size_t)k * KB + c;
  double sr = 0.0, si = 0.0;
  for (int j = 0; j < used; ++j) {
    const fc_cplx q = L.y[j];
    const double* __restrict__ v = V + (size_t)j * 2 * n * KB;
    const double vr = v[o], vi = v[o + KB];
    sr += vr * q.re - vi * q.im;
    si += vr * q.im + vi * q.re;
  }
  out[o] = sr;
  out[o + KB] = si;
}
// start of a cycle for column c = blockIdx.x (one wave each): fc_cgmres_begin from res2[c] = (|r|^2, |b|^2).  first: columns >= k
// (padding) start stopped; later cycles leave a finished or broken column alone.
__global__ __launch_bounds__(64) void fc_cgmres_begin_b(int m, int k, int KB, int first, double* gmb, const double* __restrict__ res2,
                                                        double rtol) {
  const int c = blockIdx.x;
  const FcCgm L = fc_cgm_layout_b(gmb, m, c, KB);
  if (first && c >= k) {
    if (threadIdx.x < CG_REC) L.rec[threadIdx.x] = threadIdx.x == CG_STATE ? 1.0 : 0.0;
    return;
  }
  if (!first && fc_state_frozen(L.rec[CG_STATE], 1)) return;
  const double r2 = res2[2 * c], b2 = res2[2 * c + 1];
  for (int i = threadIdx.x; i <= m; i += 64) L.g[i] = fc_cplx{i == 0 ? sqrt(r2) : 0.0, 0.0};
  if (threadIdx.x != 0) return;
  L.rec[CG_USED] = 0.0;
  L.rec[CG_RNORM2] = r2;
  L.rec[CG_BNORM2] = b2;
  L.rec[CG_BETA] = sqrt(r2);
  L.rec[CG_STATE] = (sqrt(r2) <= rtol * sqrt(b2) || !(b2 > 0.0)) ? 1.0 : 0.0;
}
// fc_cgmres_givens for column c = blockIdx.x: h1, h2 [i][KB], npart the gx partials of |w_c|^2 (fc_cmultidot_b with nv = 1)
__global__ __launch_bounds__(64) void fc_cgmres_givens_b(int j, int m, int KB, int close, double* gmb, const double2* __restrict__ h1,
                                                         const double2* __restrict__ h2, const double* __restrict__ npart, int gx,
                                                         double rtol) {
  const int c = blockIdx.x;
  const FcCgm L = fc_cgm_layout_b(gmb, m, c, KB);
  if (L.rec[CG_STATE] != 0.0) return;
  __shared__ fc_cplx col[kCgmMaxRestart + 2];
  __shared__ int stop;
  const int lane = threadIdx.x;
  double nsum = 0.0;
  for (int q = 0; q < gx; ++q) nsum += npart[2 * ((size_t)q * KB + c)];  // (fc_cmultidot_reduce_b's order)
  for (int i = lane; i <= j; i += 64) {
    const double2 p = h1[(size_t)i * KB + c], q = h2[(size_t)i * KB + c];
    col[i] = fc_cplx{p.x + q.x, p.y + q.y};
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
// block vector <-> the permuted work buffer of the batched apply (dev rows r of the buffer = row perm[r] of the block vector):
// dir 0 buffer <- vector, 1 vector <- buffer, 2 vector += buffer for the columns a cycle's end updates (rec, mode 1)
template <int KB>
__global__ __launch_bounds__(256) void fc_cblock_perm(int n2, const int* __restrict__ perm, const double* __restrict__ src,
                                                      double* __restrict__ dst, int dir, const double* __restrict__ rec) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t r = t / KB;
  if (r >= n2) return;
  const size_t ob = (size_t)r * KB + c, ov = (size_t)perm[r] * KB + c;
  if (dir == 0)
    dst[ob] = src[ov];
  else if (dir == 1)
    dst[ov] = src[ob];
  else if (!fc_col_frozen(rec, c, 1))
    dst[ov] += src[ob];
}
// [k][n] storage -> block vector: re / im [k][n] split (im may be null), padding columns zero
template <int KB>
__global__ __launch_bounds__(256) void fc_cblock_load(int n, int k, const double* __restrict__ re, const double* __restrict__ im,
                                                      double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t i = t / KB;
  if (i >= n) return;
  const size_t o = 2 * (size_t)i * KB + c;
  dst[o] = c < k ? re[(size_t)c * n + i] : 0.0;
  dst[o + KB] = (c < k && im) ? im[(size_t)c * n + i] : 0.0;
}
// block vector -> [k][n] interleaved complex (xz) and, optionally, split re / im [k][n]
template <int KB>
__global__ __launch_bounds__(256) void fc_cblock_store(int n, int k, const double* __restrict__ src, double2* __restrict__ xz,
                                                       double* __restrict__ re, double* __restrict__ im) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % KB);
  const int64_t i = t / KB;
  if (i >= n || c >= k) return;
  const size_t o = 2 * (size_t)i * KB + c;
  const double vr = src[o], vi = src[o + KB];
  xz[(size_t)c * n + i] = make_double2(vr, vi);
  if (re) {
    re[(size_t)c * n + i] = vr;
    im[(size_t)c * n + i] = vi;
  }
}

// ── snapshot sets (fc_shifted_snap_*): balanced reduced models from frequency snapshots ────────────────────────────────────────
// A set holds complex columns in the layout of xz, [col][n] interleaved: column a IS the pair of real columns 2 a (re), 2 a + 1 (im)
// with stride 2 in memory.
// out = scale * in over cnt doubles (a push of solutions into a set)
__global__ __launch_bounds__(256) void fc_snap_push(int64_t cnt, double scale, const double* __restrict__ in, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) out[i] = scale * in[i];
}
// z = scale * (re + i im) (im may be null): a host vector into a set
__global__ __launch_bounds__(256) void fc_snap_load(int n, double scale, const double* __restrict__ re, const double* __restrict__ im,
                                                    double2* __restrict__ z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = make_double2(scale * re[i], im ? scale * im[i] : 0.0);
}

// Tall-skinny real product: part[blockIdx.z][i][j0 + j] = sum over the slice's rows r of L[r][i] W[r][j], where real column 2 a + p of
// L (W) is part p of complex column a of Lz (Wz).  One workgroup = a 64 x 64 tile of the output (blockIdx.x: 32 complex columns of L,
// blockIdx.y: 32 of W) over the rows [blockIdx.z * slice, + slice) of N; wave w owns the 32 x 32 quarter (w & 1, w >> 1) as 2 x 2
// accumulators of v_mfma_f64_16x16x4_f64 (lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15]; D[row (l >> 4) + 4 r]
// [col l & 15] in register r), the k index running over rows of N.  Operand tiles go through LDS in chunks of 32 rows: global reads
// run along the columns (32 consecutive double2 per column), LDS holds them transposed, [real column][row] with a row stride of 36
// doubles (16 columns x 4 rows of one operand read spread over all banks twice, the minimum for 8-byte reads of a wave).  A value
// read from global memory feeds 64 products.  Columns past ncl / ncr and rows past the slice or n read as zero: no padding of the
// sets.  ld = leading dimension of the output (2 * total right columns); j0 = first real output column of this launch.
constexpr int kSnapKC = 32, kSnapLD = 36;
// hi += a with the rounding error of the sum added to lo (Knuth's two-sum, per component)
__device__ inline void fc_two_sum(fc_d4& hi, fc_d4& lo, const fc_d4 a) {
  const fc_d4 s = hi + a;
  const fc_d4 b = s - hi;
  lo += (hi - (s - b)) + (a - b);
  hi = s;
}
__global__ __launch_bounds__(256) void fc_snap_gram(int n, int slice, int ncl, int ncr, const double2* __restrict__ Lz,
                                                    const double2* __restrict__ Wz, int ld, int j0, double* __restrict__ part) {
  __shared__ double Ls[64][kSnapLD], Ws[64][kSnapLD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wi = 32 * (wave & 1), wj = 32 * (wave >> 1);
  const int a0 = 32 * blockIdx.x, b0 = 32 * blockIdx.y;
  const int r0 = blockIdx.z * slice, r1 = min(n, r0 + slice);
  const int tr = threadIdx.x & 31, tc = threadIdx.x >> 5;  // staging: row of the chunk, complex column (+ 8 per pass)
  fc_d4 acc[2][2], hi[2][2], lo[2][2];  // a chunk's products; the running sum of the chunks and its rounding errors (two-sum)
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) hi[x][y] = lo[x][y] = fc_d4{0.0, 0.0, 0.0, 0.0};
  for (int rc = r0; rc < r1; rc += kSnapKC) {
    const int row = rc + tr;
    double2 lv[4], wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = tc + 8 * u;
      lv[u] = (row < r1 && a0 + c < ncl) ? Lz[(size_t)(a0 + c) * n + row] : make_double2(0.0, 0.0);
      wv[u] = (row < r1 && b0 + c < ncr) ? Wz[(size_t)(b0 + c) * n + row] : make_double2(0.0, 0.0);
    }
    __syncthreads();  // (the previous chunk's reads are done)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = tc + 8 * u;
      Ls[2 * c][tr] = lv[u].x;
      Ls[2 * c + 1][tr] = lv[u].y;
      Ws[2 * c][tr] = wv[u].x;
      Ws[2 * c + 1][tr] = wv[u].y;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = fc_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kSnapKC / 4; ++s) {
      const double av0 = Ls[wi + lr][4 * s + lk], av1 = Ls[wi + 16 + lr][4 * s + lk];
      const double bv0 = Ws[wj + lr][4 * s + lk], bv1 = Ws[wj + 16 + lr][4 * s + lk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, bv0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, bv1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, bv0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, bv1, acc[1][1], 0, 0, 0);
    }
    // the chunk's sums join the running sum without a rounding error of their own: only the 32-term sums inside the matrix
    // instructions round, so that the Hankel matrix keeps its small singular values
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) fc_two_sum(hi[x][y], lo[x][y], acc[x][y]);
  }
  double* __restrict__ P = part + (size_t)blockIdx.z * (2 * (size_t)ncl) * ld;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 2 * a0 + wi + 16 * x + lk + 4 * r, j = 2 * b0 + wj + 16 * y + lr;
        if (i < 2 * ncl && j < 2 * ncr) P[(size_t)i * ld + j0 + j] = hi[x][y][r] + lo[x][y][r];
      }
}
// out[e] = sum of the ns slice partials of entry e, in slice order, compensated (no atomics: a repeated call returns the same bits)
__global__ __launch_bounds__(256) void fc_snap_gram_reduce(int64_t cnt, int ns, const double* __restrict__ part, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < ns; ++k) {  // (two-sum: the slices add up without a rounding error of their own)
    const double a = part[(size_t)k * cnt + e];
    const double t = s + a, b = t - s;
    c += (s - (t - b)) + (a - b);
    s = t;
  }
  out[e] = s + c;
}
// out[c][row] = sum_a Q[2 a][c] re S_a[row] + Q[2 a + 1][c] im S_a[row] (Q: 2 ncol x k real, row-major), columns in a fixed order:
// the modes Phi, Psi; grid (rows / 256, k)
__global__ __launch_bounds__(256) void fc_snap_combine(int n, int ncol, int k, const double2* __restrict__ S, const double* __restrict__ Q,
                                                       double* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (row >= n || c >= k) return;
  double s = 0.0;
  for (int a = 0; a < ncol; ++a) {
    const double2 v = S[(size_t)a * n + row];
    s += Q[(size_t)(2 * a) * k + c] * v.x;
    s += Q[(size_t)(2 * a + 1) * k + c] * v.y;
  }
  out[(size_t)c * n + row] = s;
}
