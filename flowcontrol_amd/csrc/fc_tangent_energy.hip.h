// fc_tangent_energy.hip.h -- the TANGENT OF THE ENERGY in the tangent marches (fc_tangent_set_energy / fc_get_tangent_energy; host side
// in fc_tangent_energy_run.hpp; DESIGN §5.6 "Energy").  Every forward step logs dE_m = 1/2 x_m^T M x_m, the integral 1/2 ∫ |u|^2 of the
// new velocity that the cell workgroups of fc_tail evaluate at the 7 Radon points.  Its directional derivative along a tangent state is
//     d(dE_m) = x_m^T M_s dx_m = ∫ u(x_m) . du(dx_m) = Σ_cells Σ_q w_q 1/2 |detJ| (u . du)(q)
// the same quadrature with the product of two fields in the place of the square (degree 4: the rule is exact).  NEITHER factor is masked:
// dE integrates the whole velocity field, and on an actuated Dirichlet row dx_m holds prof du_m, which the solve has left there (DESIGN
// §5.4 "Energy term").  x: the taped column x_m; d: the tangent level the step's tail has just written.
//   fc_tan_energy:          eight lanes per cell, 32 cells per workgroup (the geometry of fc_tail's cell workgroups); one partial per
//                           workgroup into row m of the partials [n_steps][G]
//   fc_tan_energy_b:        thread = (cell, simulation), 256 / KB cells per workgroup (the geometry of fc_tan_elem_nl_b); partials
//                           [n_steps][G][KB]
//   fc_tan_energy_fold/_b:  ONE launch behind the last step, a workgroup per step: that step's G partials in a fixed strided order
// Sums in a fixed order, no atomics, vector stores only: two marches of the same inputs give the same bits.
#pragma once

// lane a < 6 fetches node a of its cell once (both components of x and d) into LDS (row stride 9: the eight cells of a wave on different
// banks), lane q < 7 evaluates w_q (u . du) at Radon point q; the eight lanes of a cell reduce with __shfl_down (4, 2, 1), the 32 cells
// through an LDS tree.  `partial`: row m of the partials, gridDim.x entries.
__global__ __launch_bounds__(256) void fc_tan_energy(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                     const double* __restrict__ x, const double* __restrict__ d,
                                                     double* __restrict__ partial) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int cl = t >> 3, lane = t & 7;
  const bool active = cl < nc;
  const int c = active ? cl : 0;
  __shared__ double sh[4][32 * 9];
  __shared__ double red[32];
  const int cb = (threadIdx.x >> 3) * 9;
  if (lane < 6) {
    const int ix = cnp[lane * nc + c], iy = cnp[(6 + lane) * nc + c];
    sh[0][cb + lane] = x[ix];
    sh[1][cb + lane] = x[iy];
    sh[2][cb + lane] = d[ix];
    sh[3][cb + lane] = d[iy];
  }
  const int q = lane < FC_NQ ? lane : FC_NQ - 1;  // lane 7 shadows point 6 with zero weight
  const double wq = active && lane < FC_NQ ? c_qw[q] * 0.5 * geom[4 * (size_t)nc + c] : 0.0;
  double ux = 0, uy = 0, ex = 0, ey = 0;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double ph = c_phi2[q * 6 + a];
    ux += ph * sh[0][cb + a];
    uy += ph * sh[1][cb + a];
    ex += ph * sh[2][cb + a];
    ey += ph * sh[3][cb + a];
  }
  double w = wq * (ux * ex + uy * ey);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) w += __shfl_down(w, off, 8);
  if (lane == 0) red[threadIdx.x >> 3] = w;
  __syncthreads();
  for (int st = 16; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// thread = (cell, simulation s), s fastest: the cell's seven points on one thread, nodal values in registers.  Inside a point the sums
// over a = 0..5 run in the order of the eight-lane form; the seven points are then added in sequence q = 0..6, where the eight-lane form
// adds them through its shuffle tree ((0+4), (1+5), ..): the two forms agree to rounding, not bit for bit.  x: column of the batched
// tape [N][KB] -- SHARED: every simulation reads the trajectory of column ref_col; d [N][KB].  Columns s >= k (padding) read nothing and write zeros.  The 256 / KB cells of a workgroup
// reduce per column through an LDS tree; `partial`: row m of the partials, [gridDim.x][KB].
template <int KB, bool SHARED>
__global__ __launch_bounds__(256) void fc_tan_energy_b(int nc, int k, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                       const double* __restrict__ x, const double* __restrict__ d, int ref_col,
                                                       double* __restrict__ partial) {
  constexpr int CPB = 256 / KB;
  const int s = (int)threadIdx.x % KB, c = blockIdx.x * CPB + (int)threadIdx.x / KB;
  __shared__ double red[256];
  double e = 0.0;
  if (c < nc && s < k) {
    const int xs = SHARED ? ref_col : s;
    double xx[6], xy[6], dx[6], dy[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const size_t rx = (size_t)cnp[a * nc + c], ry = (size_t)cnp[(6 + a) * nc + c];
      xx[a] = x[rx * KB + xs];
      xy[a] = x[ry * KB + xs];
      dx[a] = d[rx * KB + s];
      dy[a] = d[ry * KB + s];
    }
    const double hdet = 0.5 * geom[4 * (size_t)nc + c];
#pragma unroll
    for (int q = 0; q < FC_NQ; ++q) {
      double ux = 0, uy = 0, ex = 0, ey = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double ph = c_phi2[q * 6 + a];
        ux += ph * xx[a];
        uy += ph * xy[a];
        ex += ph * dx[a];
        ey += ph * dy[a];
      }
      e += c_qw[q] * hdet * (ux * ex + uy * ey);
    }
  }
  red[threadIdx.x] = e;
  __syncthreads();
  for (int st = 128; st >= KB; st >>= 1) {  // (st is a multiple of KB: a column's cells only)
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if ((int)threadIdx.x < KB) partial[(size_t)blockIdx.x * KB + threadIdx.x] = red[threadIdx.x];
}

// Behind the last step: workgroup m folds row m of the partials [n_steps][G] -- thread t takes entries t, t + 256, .. in order, then an
// LDS tree -- into dde[m].
__global__ __launch_bounds__(256) void fc_tan_energy_fold(int G, const double* __restrict__ partial, double* __restrict__ dde) {
  const int t = threadIdx.x;
  const double* row = partial + (size_t)blockIdx.x * G;
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = t; i < G; i += 256) acc += row[i];
  red[t] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (t < st) red[t] += red[t + st];
    __syncthreads();
  }
  if (t == 0) dde[blockIdx.x] = red[0];
}

// The same per column of [n_steps][G][KB]: thread = (group r, simulation s), group r takes workgroups r, r + 256 / KB, ..; the groups
// reduce per column through the tree.  dde [n_steps][k]: padding columns reach no output.
template <int KB>
__global__ __launch_bounds__(256) void fc_tan_energy_fold_b(int G, int k, const double* __restrict__ partial, double* __restrict__ dde) {
  constexpr int GROUPS = 256 / KB;
  const int t = threadIdx.x, s = t % KB, r = t / KB;
  const double* row = partial + (size_t)blockIdx.x * G * KB;
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = r; i < G; i += GROUPS) acc += row[(size_t)i * KB + s];
  red[t] = acc;
  __syncthreads();
  for (int st = 128; st >= KB; st >>= 1) {
    if (t < st) red[t] += red[t + st];
    __syncthreads();
  }
  if (t < k) dde[(size_t)blockIdx.x * k + t] = red[t];
}
