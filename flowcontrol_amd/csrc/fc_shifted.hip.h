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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// y_i = sum_k (s e_k - t a_k) x_j  (complex s, real t), or b_i - that when b != nullptr.  L lanes per row (L <= 64, a power of two),
// 256 / L rows per workgroup.  partial (optional): per workgroup |y|^2 at [blockIdx.x] and |b|^2 at [gridDim.x + blockIdx.x] (the two
// segments fc_reduce_final folds in a fixed order)
template <int L>
__global__ __launch_bounds__(256) void fc_shifted_spmv(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ a, const double* __restrict__ e, double s_re, double s_im,
                                                       double t, const double2* __restrict__ x, const double2* __restrict__ b,
                                                       double2* __restrict__ y, double* __restrict__ partial) {
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
