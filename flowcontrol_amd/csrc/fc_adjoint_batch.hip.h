// fc_adjoint_batch.hip.h -- the backward (adjoint) march for k lock-step runs (fc_run_adjoint_batch; host side in
// fc_adjoint_batch_run.hpp, DESIGN §5.4 "Batched march").  Every vector of fc_adjoint.hip.h becomes a row-major matrix [row][KB]
// (KB = 4, 8, 16 or 32, simulation index fastest, columns k .. KB - 1 zero), the transposed solve is the batched factor apply of
// fc_batch.hip.h (fc_nd_block_b / fc_nd_fold_b, unchanged) on a tiled copy of the slot's TRANSPOSED values.  Column s runs exactly the
// recurrence of the single march:
//     r_s = C^T w_s (+ z_s) + M Z (cm_n mu_{m+1,s} + cm_nn mu_{m+2,s}) (+ J(x_{m,s})^T Z (cc_n mu_{m+1,s} + cc_nn mu_{m+2,s})),
//     mu_s = A^-T r_s,     g_{k,s} = B~_k^T mu_s
//   linearised element loop: fc_rhs_elem_breg<KB, false> of the forward batched step on the two masked levels with cc = 0
//   fc_adj_elem_nl_b:     the nonlinear element loop, one thread per (cell, simulation): the arithmetic of fc_adj_elem_nl_reg on column s
//                         of the taped state and of the two masked levels
//   fc_adj_rhs_gather_b:  element sums on EVERY row, C^T w_s from the sensor table by row, the terminal vector; writes b and the y half
//                         of the march's work buffer
//   fc_adj_tail_b:        workgroup partials of B~_a^T mu_s per (actuator, simulation), the per-column finiteness flag, the masked copy
//   fc_adj_reduce_b:      the partials of an (actuator, simulation) in a fixed order -> g[s][a]
// Sums run in a fixed order (no atomics), the columns never mix: equal columns come out bit-equal, a zero column stays exactly zero, a
// non-finite column stays alone.  Vector stores only.
#pragma once

// The element vectors of  M Z zeta_m + J(x)^T Z zeta_c  for KB simulations, thread = (cell, simulation) -- the geometry of fc_rhs_elem_breg,
// the arithmetic and the summation order (a = 0..5 inside a point, points 0..6 into the test functions) of fc_adj_elem_nl_reg.
// x: the taped state [N][KB] (unmasked); z1, z2: the two masked levels [N][KB].  ev[(slot * nc + cell) * KB + s].
// EN (energy weights held): zeta_m also takes e_row[s] x at the node (fc_adjoint_energy.hip.h); EN = false is the loop as it always was.
template <int KB, bool EN>
__global__ __launch_bounds__(256) void fc_adj_elem_nl_b(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                        const double* __restrict__ x, const double* __restrict__ z1,
                                                        const double* __restrict__ z2, double cm_n, double cm_nn, double cc_n,
                                                        double cc_nn, const double* __restrict__ e_row, double* __restrict__ ev) {
  constexpr int CPB = 256 / KB;
  const int s = (int)threadIdx.x % KB, c = blockIdx.x * CPB + (int)threadIdx.x / KB;
  if (c >= nc) return;
  double e = 0.0;
  if constexpr (EN) e = e_row[s];
  double xx[6], xy[6], zmx[6], zmy[6], zcx[6], zcy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const size_t ix = (size_t)cnp[a * nc + c] * KB + s, iy = (size_t)cnp[(6 + a) * nc + c] * KB + s;
    const double ax = z1[ix], ay = z1[iy], bx = z2[ix], by = z2[iy];
    xx[a] = x[ix];
    xy[a] = x[iy];
    if constexpr (EN) {
      zmx[a] = cm_n * ax + cm_nn * bx + e * xx[a];
      zmy[a] = cm_n * ay + cm_nn * by + e * xy[a];
    } else {
      zmx[a] = cm_n * ax + cm_nn * bx;
      zmy[a] = cm_n * ay + cm_nn * by;
    }
    zcx[a] = cc_n * ax + cc_nn * bx;
    zcy[a] = cc_n * ay + cc_nn * by;
  }
  const double j00 = geom[c], j01 = geom[nc + c], j10 = geom[2 * nc + c], j11 = geom[3 * nc + c], hdet = 0.5 * geom[4 * nc + c];
  double accx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < FC_NQ; ++q) {
    double ux = 0, uy = 0, uxi = 0, uet = 0, vxi = 0, vet = 0;
    double mx = 0, my = 0, kx = 0, ky = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double ph = c_phi2[q * 6 + a], dx = c_dphi2[(q * 6 + a) * 2], de = c_dphi2[(q * 6 + a) * 2 + 1];
      ux += ph * xx[a];
      uy += ph * xy[a];
      uxi += dx * xx[a];
      uet += de * xx[a];
      vxi += dx * xy[a];
      vet += de * xy[a];
      mx += ph * zmx[a];
      my += ph * zmy[a];
      kx += ph * zcx[a];
      ky += ph * zcy[a];
    }
    const double ux_x = uxi * j00 + uet * j10, ux_y = uxi * j01 + uet * j11;
    const double uy_x = vxi * j00 + vet * j10, uy_y = vxi * j01 + vet * j11;
    const double wq = c_qw[q] * hdet;
    const double fx = wq * (mx + ux_x * kx + uy_x * ky), fy = wq * (my + ux_y * kx + uy_y * ky);
    const double sxi = wq * (ux * j00 + uy * j01), set = wq * (ux * j10 + uy * j11);
    const double px = sxi * kx, py = sxi * ky, ex = set * kx, ey = set * ky;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double pa = c_phi2[q * 6 + a], da = c_dphi2[(q * 6 + a) * 2], ea = c_dphi2[(q * 6 + a) * 2 + 1];
      accx[a] += pa * fx + da * px + ea * ex;
      accy[a] += pa * fy + da * py + ea * ey;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    ev[((size_t)a * nc + c) * KB + s] = accx[a];
    ev[((size_t)(6 + a) * nc + c) * KB + s] = accy[a];
  }
}

// fc_adj_rhs_gather for KB simulations, thread = (permuted row, simulation PAIR) as fc_rhs_gather_b: the element contributions in list
// order (eight in flight) on every row, Dirichlet rows included; + the row's sensor entries x w[s][sensor] (w: [k][n_sens], columns
// s >= k add nothing); + term[i][s].  Writes b and the y half of the work buffer.
template <int KB>
__global__ __launch_bounds__(256) void fc_adj_rhs_gather_b(int N, int k, const int* __restrict__ gptr, const int* __restrict__ gidx,
                                                           const double* __restrict__ ev, const int* __restrict__ ct_ptr,
                                                           const int* __restrict__ ct_sens, const double* __restrict__ ct_w, int n_sens,
                                                           const double* __restrict__ w, const double* __restrict__ term,
                                                           double* __restrict__ b, double* __restrict__ y) {
  typedef double d2 __attribute__((ext_vector_type(2), aligned(8)));
  constexpr int HP = KB / 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / HP, s = 2 * (t % HP);
  if (i >= N) return;
  double a0 = 0.0, a1 = 0.0;
  const int k0 = gptr[i], k1 = gptr[i + 1];
  for (int base = k0; base < k1; base += 8) {
    int id[8];
    d2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) id[u] = gidx[base + u < k1 ? base + u : k1 - 1];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const d2*>(ev + (size_t)id[u] * KB + s);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (base + u < k1) {
        a0 += v[u].x;
        a1 += v[u].y;
      }
  }
  if (w)
    for (int q = ct_ptr[i]; q < ct_ptr[i + 1]; ++q) {
      const double cw = ct_w[q];
      const int sn = ct_sens[q];
      if (s < k) a0 += cw * w[(size_t)s * n_sens + sn];
      if (s + 1 < k) a1 += cw * w[(size_t)(s + 1) * n_sens + sn];
    }
  if (term) {
    const d2 tv = *reinterpret_cast<const d2*>(term + (size_t)i * KB + s);
    a0 += tv.x;
    a1 += tv.y;
  }
  const d2 out = {a0, a1};
  *reinterpret_cast<d2*>(b + (size_t)i * KB + s) = out;
  *reinterpret_cast<d2*>(y + (size_t)i * KB + s) = out;
}

// mu = x [N][KB] (the solution half of the work buffer).  thread = (row lane rw < 256 / KB, simulation s): rows block * RPB + rw,
// + grid * RPB, ... in order, then the RPB row lanes of a simulation in index order through LDS:
// partial[((a * KB + s) * gridDim.x) + block] = the block's share of B~_a . mu_s.  flag[s] = 1 on a non-finite entry of column s;
// zm[i][s] = mu off the Dirichlet rows, 0 on them.  Four actuators per pass over the rows (the later passes re-read mu from the caches).
template <int KB>
__global__ __launch_bounds__(256) void fc_adj_tail_b(int N, const double* __restrict__ x, const int* __restrict__ bcslot, int n_act,
                                                     const double* __restrict__ bt, double* __restrict__ zm, int* __restrict__ flag,
                                                     double* __restrict__ partial) {
  constexpr int RPB = 256 / KB;
  __shared__ double red[4][256];
  const int t = threadIdx.x, s = t % KB, rw = t / KB;
  const int stride = gridDim.x * RPB;
  int k0 = 0;
  do {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * RPB + rw; i < N; i += stride) {
      const double mu = x[(size_t)i * KB + s];
      if (k0 == 0) {
        if (!isfinite(mu)) flag[s] = 1;
        zm[(size_t)i * KB + s] = bcslot[i] >= 0 ? 0.0 : mu;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k0 + j < n_act) acc[j] += bt[(size_t)(k0 + j) * N + i] * mu;
    }
    if (n_act > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][t] = acc[j];
      __syncthreads();
      if (t < KB) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (k0 + j >= n_act) continue;
          double sum = 0.0;
          for (int g = 0; g < RPB; ++g) sum += red[j][g * KB + t];
          partial[((size_t)(k0 + j) * KB + t) * gridDim.x + blockIdx.x] = sum;
        }
      }
      __syncthreads();
    }
    k0 += 4;
  } while (k0 < n_act);
}

// g[s * n_act + a] = sum of the gx partials of (actuator a, simulation s), block = a * k + s: one wave each, lane l takes partials
// l, l + 64, ... in order, then a fixed shuffle tree (the order of fc_adj_reduce).  Padding columns have no block: they reach no output.
__global__ __launch_bounds__(64) void fc_adj_reduce_b(int n_act, int k, int KB, int gx, const double* __restrict__ partial,
                                                      double* __restrict__ g) {
  const int a = blockIdx.x / k, s = blockIdx.x % k;
  double sum = 0.0;
  const double* __restrict__ p = partial + ((size_t)a * KB + s) * gx;
  for (int q = threadIdx.x; q < gx; q += 64) sum += p[q];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (threadIdx.x == 0 && a < n_act) g[(size_t)s * n_act + a] = sum;
}
