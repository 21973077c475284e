// fc_optpert.hip.h -- block kernels of the optimal-perturbation driver (fc_mass_solve_batch, fc_optpert_*; host side in
// fc_optpert_run.hpp).  Every block is a row-major matrix [row][KB] in the solver's permuted numbering (KB = 4, 8, 16 or
// 32, column index fastest, columns k .. KB - 1 zero) -- the layout of the batched step and of the batched adjoint march, so a block
// is a state of the one and a terminal vector of the other without a copy through the host.
//   fc_op_mass_b:      Y = M_ff X on the compacted f x f CSR (rows outside f are empty: Y = 0 there), KB lanes per row, optionally the
//                      workgroup partials of the column dots X . Y
//   fc_op_cg_init:     r = b, p = D^-1 b, x = 0 and the partials of r . D^-1 r and r . r
//   fc_op_cg_start:    (one workgroup) the partials in a fixed order -> per-column scalars; columns with b = 0 never become active
//   fc_op_cg_update:   alpha = rz / pAp from the partials (every workgroup sums them in the same fixed order), x += alpha p,
//                      r -= alpha Ap, partials of r . D^-1 r and r . r
//   fc_op_cg_dir:      beta from the partials, p = D^-1 r + beta p; workgroup 0 writes the next iteration's scalars (the other parity)
//   fc_op_gram:        workgroup partials of X^T Y over a row range, rows staged through LDS;  fc_op_gram_sum: the partials in order
//   fc_op_combine:     dst (+)= src Q (scale), columns >= k zero
//   fc_op_mask / fc_op_finite: a block onto the free rows / per-column non-finite flags
// Sums run in a fixed order (no atomics), the columns never mix: equal columns come out bit-equal, a zero column stays exactly zero and
// runs no iteration, a repeated call returns the same bits.  Vector stores only.
#pragma once

// per-column scalars of the block CG, two parities (an iteration reads parity q and writes parity 1 - q)
struct FcOpCgScalars {
  double rz[2][32];     // r . D^-1 r
  double rr[32];        // r . r of the last iteration the column ran
  double bb[32];        // b . b
  int active[2][32];    // the column still iterates
  int iters[32];        // iterations the column ran
  int any_active;       // some column still iterates (what the host reads once per chunk)
};

// the column sums of `n_part` workgroup partials part[g * KB + s], g ascending: thread (rw, s) takes g = rw, rw + RPB, ... in order, then
// the RPB lanes of a column in index order.  All 256 threads call it; the result is valid in every thread of column s.
template <int KB>
__device__ inline double fc_op_column_sum(const double* __restrict__ part, int n_part, double* red) {
  constexpr int RPB = 256 / KB;
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  double a = 0.0;
  for (int g = rw; g < n_part; g += RPB) a += part[(size_t)g * KB + s];
  red[t] = a;
  __syncthreads();
  double sum = 0.0;
  for (int g = 0; g < RPB; ++g) sum += red[g * KB + s];
  __syncthreads();
  return sum;
}

// this workgroup's share of a column dot: the RPB row lanes of column s in index order -> part[block * KB + s]
template <int KB>
__device__ inline void fc_op_block_partial(double acc, double* red, double* __restrict__ part) {
  constexpr int RPB = 256 / KB;
  const int t = threadIdx.x;
  red[t] = acc;
  __syncthreads();
  if (t < KB) {
    double sum = 0.0;
    for (int g = 0; g < RPB; ++g) sum += red[g * KB + t];
    part[(size_t)blockIdx.x * KB + t] = sum;
  }
  __syncthreads();
}

// Y = M_ff X.  thread = (row lane rw, column s); rows block * RPB + rw, + grid * RPB, ...: one nonzero is one broadcast value and index
// and one coalesced read of the KB doubles of an X row.  dot != null: part[block * KB + s] = this workgroup's share of X_s . Y_s.
// act != null: columns with act[s] == 0 are left as they are (a frozen column of the block CG).
template <int KB>
__global__ __launch_bounds__(256) void fc_op_mass_b(int N, const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                                                    const double* __restrict__ x, double* __restrict__ y, const int* __restrict__ act,
                                                    double* __restrict__ dot) {
  constexpr int RPB = 256 / KB;
  __shared__ double red[256];
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  const bool on = act ? act[s] != 0 : true;
  double acc = 0.0;
  for (int i = blockIdx.x * RPB + rw; i < N; i += gridDim.x * RPB) {
    if (!on) continue;
    double a = 0.0;
    for (int q = rp[i]; q < rp[i + 1]; ++q) a += v[q] * x[(size_t)ci[q] * KB + s];
    y[(size_t)i * KB + s] = a;
    acc += x[(size_t)i * KB + s] * a;
  }
  if (dot) fc_op_block_partial<KB>(acc, red, dot);
}

// x = 0, r = b, p = D^-1 b; part[0]: r . D^-1 r, part[1]: r . r (each [grid][KB])
template <int KB>
__global__ __launch_bounds__(256) void fc_op_cg_init(int N, const double* __restrict__ b, const double* __restrict__ dinv, double* __restrict__ x,
                                                     double* __restrict__ r, double* __restrict__ p, double* __restrict__ part) {
  constexpr int RPB = 256 / KB;
  __shared__ double red[256];
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  double rz = 0.0, rr = 0.0;
  for (int i = blockIdx.x * RPB + rw; i < N; i += gridDim.x * RPB) {
    const size_t o = (size_t)i * KB + s;
    const double bi = b[o], zi = dinv[i] * bi;
    x[o] = 0.0;
    r[o] = bi;
    p[o] = zi;
    rz += bi * zi;
    rr += bi * bi;
  }
  fc_op_block_partial<KB>(rz, red, part);
  fc_op_block_partial<KB>(rr, red, part + (size_t)gridDim.x * KB);
}

// one workgroup: the scalars of iteration 0.  A column with b . b == 0 (a zero right-hand side, a padding column) is never active.
template <int KB>
__global__ __launch_bounds__(256) void fc_op_cg_start(int n_part, const double* __restrict__ part, FcOpCgScalars* __restrict__ sc) {
  __shared__ double red[256];
  const double rz = fc_op_column_sum<KB>(part, n_part, red);
  const double bb = fc_op_column_sum<KB>(part + (size_t)n_part * KB, n_part, red);
  const int t = threadIdx.x;
  if (t < KB) {
    const int on = bb == 0.0 ? 0 : 1;  // (a NaN right-hand side stays active and ends at max_iter)
    sc->rz[0][t] = rz, sc->rz[1][t] = rz;
    sc->rr[t] = bb, sc->bb[t] = bb;
    sc->active[0][t] = on, sc->active[1][t] = on;
    sc->iters[t] = 0;
  }
  for (int s = KB + t; s < 32; s += 256) sc->active[0][s] = sc->active[1][s] = 0, sc->iters[s] = 0, sc->rr[s] = sc->bb[s] = 0.0;
  __syncthreads();
  if (t == 0) {
    int any = 0;
    for (int s = 0; s < KB; ++s) any |= sc->active[0][s];
    sc->any_active = any;
  }
}

// alpha_s = rz_s / pAp_s (pAp from the n_part partials of fc_op_mass_b), x += alpha p, r -= alpha Ap on the active columns;
// part[0]: r . D^-1 r, part[1]: r . r of the new residual.  q: the parity this iteration reads.
template <int KB>
__global__ __launch_bounds__(256) void fc_op_cg_update(int N, int q, const FcOpCgScalars* __restrict__ sc, int n_part, const double* __restrict__ dotp,
                                                       const double* __restrict__ dinv, const double* __restrict__ p, const double* __restrict__ ap,
                                                       double* __restrict__ x, double* __restrict__ r, double* __restrict__ part) {
  constexpr int RPB = 256 / KB;
  __shared__ double red[256];
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  const double pap = fc_op_column_sum<KB>(dotp, n_part, red);
  const bool on = sc->active[q][s] != 0;
  const double alpha = on ? sc->rz[q][s] / pap : 0.0;
  double rz = 0.0, rr = 0.0;
  for (int i = blockIdx.x * RPB + rw; i < N; i += gridDim.x * RPB) {
    if (!on) continue;
    const size_t o = (size_t)i * KB + s;
    const double ri = r[o] - alpha * ap[o];
    x[o] += alpha * p[o];
    r[o] = ri;
    rz += ri * (dinv[i] * ri);
    rr += ri * ri;
  }
  fc_op_block_partial<KB>(rz, red, part);
  fc_op_block_partial<KB>(rr, red, part + (size_t)gridDim.x * KB);
}

// beta_s = rz_new / rz_old, p = D^-1 r + beta p on the columns that go on; a column whose |r| <= rtol |b| stops here.  Workgroup 0
// writes parity 1 - q of the scalars (no workgroup of this launch reads it).
template <int KB>
__global__ __launch_bounds__(256) void fc_op_cg_dir(int N, int q, FcOpCgScalars* __restrict__ sc, int n_part, const double* __restrict__ part, double rtol2,
                                                    const double* __restrict__ dinv, const double* __restrict__ r, double* __restrict__ p) {
  constexpr int RPB = 256 / KB;
  __shared__ double red[256];
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  const double rz = fc_op_column_sum<KB>(part, n_part, red);
  const double rr = fc_op_column_sum<KB>(part + (size_t)n_part * KB, n_part, red);
  const bool was = sc->active[q][s] != 0;
  const bool on = was && !(rr <= rtol2 * sc->bb[s]);
  const double beta = on ? rz / sc->rz[q][s] : 0.0;
  for (int i = blockIdx.x * RPB + rw; i < N; i += gridDim.x * RPB) {
    if (!on) continue;
    const size_t o = (size_t)i * KB + s;
    p[o] = dinv[i] * r[o] + beta * p[o];
  }
  if (blockIdx.x == 0) {
    if (t < KB) {
      sc->rz[1 - q][t] = was ? rz : sc->rz[q][t];
      sc->active[1 - q][t] = on ? 1 : 0;
      if (was) sc->rr[t] = rr, sc->iters[t] += 1;
      red[t] = on ? 1.0 : 0.0;
    }
    __syncthreads();
    if (t == 0) {
      int any = 0;
      for (int c = 0; c < KB; ++c) any |= red[c] != 0.0 ? 1 : 0;
      sc->any_active = any;
    }
  }
}

// Workgroup partials of G = X^T Y: workgroup g takes rows [g * rows_per, (g + 1) * rows_per) in tiles of 16 staged through LDS; thread t
// owns the pairs (a, c) = t, t + 256, ... of the KB x KB result and adds the rows in index order.  part[g][a * KB + c].
template <int KB>
__global__ __launch_bounds__(256) void fc_op_gram(int N, int rows_per, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ part) {
  constexpr int TR = 16, NP = (KB * KB + 255) / 256;
  __shared__ double sx[TR * KB], sy[TR * KB];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * rows_per, r1 = min(N, r0 + rows_per);
  double acc[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) acc[u] = 0.0;
  for (int base = r0; base < r1; base += TR) {
    const int nr = min(TR, r1 - base);
    for (int e = t; e < nr * KB; e += 256) sx[e] = x[(size_t)base * KB + e], sy[e] = y[(size_t)base * KB + e];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int pr = t + 256 * u;
      if (pr < KB * KB) {
        const int a = pr / KB, c = pr % KB;
        double sum = acc[u];
        for (int i = 0; i < nr; ++i) sum += sx[i * KB + a] * sy[i * KB + c];
        acc[u] = sum;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int pr = t + 256 * u;
    if (pr < KB * KB) part[(size_t)blockIdx.x * KB * KB + pr] = acc[u];
  }
}

// out[a * KB + c] = the n_part partials of the pair in order
__global__ __launch_bounds__(256) void fc_op_gram_sum(int n_pairs, int n_part, const double* __restrict__ part, double* __restrict__ out) {
  const int pr = blockIdx.x * blockDim.x + threadIdx.x;
  if (pr >= n_pairs) return;
  double sum = 0.0;
  for (int g = 0; g < n_part; ++g) sum += part[(size_t)g * n_pairs + pr];
  out[pr] = sum;
}

// dst[i][c] (+)= scale[c] * sum_j src[i][j] Q[j * KB + c], j = 0 .. k - 1 in order (accumulate: onto what dst holds); columns c >= k
// are zero.  dst != src.
template <int KB>
__global__ __launch_bounds__(256) void fc_op_combine(int N, int k, const double* __restrict__ src, const double* __restrict__ Q, const double* __restrict__ scale,
                                                     int accumulate, double* __restrict__ dst) {
  __shared__ double sq[KB * KB];
  for (int e = threadIdx.x; e < KB * KB; e += 256) sq[e] = Q[e];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = t / KB;
  const int c = (int)(t % KB);
  if (i >= N) return;
  double sum = 0.0;
  if (c < k) {
    for (int j = 0; j < k; ++j) sum += src[(size_t)i * KB + j] * sq[j * KB + c];
    if (scale) sum *= scale[c];
    if (accumulate) sum = dst[(size_t)i * KB + c] + sum;
  }
  dst[(size_t)i * KB + c] = sum;
}

// dst = src on the free rows, 0 elsewhere (dst == src allowed)
template <int KB>
__global__ __launch_bounds__(256) void fc_op_mask(int N, const unsigned char* __restrict__ freep, const double* __restrict__ src, double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = t / KB;
  if (i >= N) return;
  dst[t] = freep[i] ? src[t] : 0.0;
}

// flag[s] = 1 where column s of x holds a non-finite entry (x: [N][KB]); the flags are zeroed by the caller
template <int KB>
__global__ __launch_bounds__(256) void fc_op_finite(int N, const double* __restrict__ x, int* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N * KB) return;
  if (!isfinite(x[t])) flag[t % KB] = 1;
}
