// fc_adjoint.hip.h -- the backward (adjoint) march of the linearised time stepper (fc_run_adjoint / fc_step_adjoint; host side in
// fc_adjoint_run.hpp).  A backward step is
//     r = C^T w (+ z) + M Z (cm_n mu_{m+1} + cm_nn mu_{m+2}),     mu = A^-T r,     g_k = B~_k^T mu
//   the element loop of the forward step (fc_rhs_elem*) forms the mass product on the two Dirichlet-masked vectors, then
//   fc_adj_rhs_gather: sums the element vectors on EVERY row (the transpose of Z M is M Z: the output is not masked), adds C^T w from the
//                      sensor table by row and the terminal vector, writes b and the y half of the work buffer
//   (the factor sweeps on the transposed values, the refinement steps on the transposed matrix: the forward launches)
//   fc_adj_tail:       workgroup partials of B~_k^T mu, the finiteness flag, the Dirichlet-masked copy the next mass product reads
//   fc_adj_reduce:     the partials of an actuator in a fixed order -> g_k
// and, once per setup, fc_adj_values_t (values of the transposed matrix on its own pattern) and fc_adj_control_columns (B~).
// All of it is bandwidth / latency bound work on N-long vectors; sums run in a fixed order (no atomics); vector stores only.
#pragma once

// a_t[k] = a[tpos[k]]: the values of A^T on the (structurally symmetric) pattern of A
__global__ __launch_bounds__(256) void fc_adj_values_t(int64_t nnz, const int* __restrict__ tpos, const double* __restrict__ a,
                                                       double* __restrict__ a_t) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nnz) a_t[k] = a[tpos[k]];
}

// bt[k][i] = column k of B~ at permuted row i: what fc_rhs_gather multiplies u_k with -- the profile on a Dirichlet row, -lift + F elsewhere
__global__ __launch_bounds__(256) void fc_adj_control_columns(int N, int n_act, const int* __restrict__ bcslot, const double* __restrict__ bcprof,
                                                              const double* __restrict__ lift, const double* __restrict__ fvec,
                                                              double* __restrict__ bt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int bs = bcslot[i];
  for (int k = 0; k < n_act; ++k) {
    double v;
    if (bs >= 0) {
      v = bcprof[(size_t)bs * n_act + k];
    } else {
      v = -lift[(size_t)k * N + i];
      if (fvec) v += fvec[(size_t)k * N + i];
    }
    bt[(size_t)k * N + i] = v;
  }
}

// per (permuted) row: the element contributions (list order, eight in flight as in fc_rhs_gather) on every row, Dirichlet rows
// included; + sum over the row's sensor entries of weight x w[sensor] (ct_*: the sensor table by row, w != nullptr); + term[i].
__global__ __launch_bounds__(256) void fc_adj_rhs_gather(int N, const int* __restrict__ gptr, const int* __restrict__ gidx,
                                                         const double* __restrict__ ev, const int* __restrict__ ct_ptr,
                                                         const int* __restrict__ ct_sens, const double* __restrict__ ct_w,
                                                         const double* __restrict__ w, const double* __restrict__ term,
                                                         double* __restrict__ b, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double s = 0.0;
  const int k0 = gptr[i], k1 = gptr[i + 1];
  for (int base = k0; base < k1; base += 8) {
    int id[8];
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) id[u] = base + u < k1 ? gidx[base + u] : -1;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = id[u] >= 0 ? ev[id[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (id[u] >= 0) s += v[u];
  }
  if (w)
    for (int k = ct_ptr[i]; k < ct_ptr[i + 1]; ++k) s += ct_w[k] * w[ct_sens[k]];
  if (term) s += term[i];
  b[i] = s;
  y[i] = s;  // y half of the work buffer: the first sweep starts from b
}

// mu = x (+ dx after refinement).  partial[k * gridDim.x + block] = the block's share of B~_k . mu (rows block, block + grid, ... in
// order, then a fixed tree over the 256 threads); *flag = 1 on a non-finite entry; zm[i] = mu[i] off the Dirichlet rows, 0 on them.
// Four actuators per pass over the rows (the later passes re-read mu from the caches).
__global__ __launch_bounds__(256) void fc_adj_tail(int N, const double* __restrict__ x, const double* __restrict__ dx,
                                                   const int* __restrict__ bcslot, int n_act, const double* __restrict__ bt,
                                                   double* __restrict__ zm, int* __restrict__ flag, double* __restrict__ partial) {
  __shared__ double red[4][256];
  const int t = threadIdx.x;
  const int stride = gridDim.x * 256;
  int k0 = 0;
  do {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + t; i < N; i += stride) {
      const double mu = dx ? x[i] + dx[i] : x[i];
      if (k0 == 0) {
        if (!isfinite(mu)) *flag = 1;
        zm[i] = bcslot[i] >= 0 ? 0.0 : mu;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k0 + j < n_act) acc[j] += bt[(size_t)(k0 + j) * N + i] * mu;
    }
    if (n_act > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][t] = acc[j];
      __syncthreads();
      for (int st = 128; st > 0; st >>= 1) {
        if (t < st) {
#pragma unroll
          for (int j = 0; j < 4; ++j) red[j][t] += red[j][t + st];
        }
        __syncthreads();
      }
      if (t < 4 && k0 + t < n_act) partial[(size_t)(k0 + t) * gridDim.x + blockIdx.x] = red[t][0];
      __syncthreads();
    }
    k0 += 4;
  } while (k0 < n_act);
}

// g[k] = sum of the gx partials of actuator k: one wave per actuator, lane l takes partials l, l + 64, ... in order, then a fixed
// shuffle tree (the order of fc_multidot_reduce)
__global__ __launch_bounds__(64) void fc_adj_reduce(int n_act, int gx, const double* __restrict__ partial, double* __restrict__ g) {
  const int k = blockIdx.x;
  double s = 0.0;
  for (int q = threadIdx.x; q < gx; q += 64) s += partial[(size_t)k * gx + q];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0 && k < n_act) g[k] = s;
}
