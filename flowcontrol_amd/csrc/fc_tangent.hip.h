// fc_tangent.hip.h -- the TANGENT-LINEAR march of the nonlinear stepper (fc_run_tangent / fc_run_tangent_batch; host side in
// fc_tangent_run.hpp).  The forward step j reads the two taped states x_{j-1}, x_{j-2}; its exact tangent steps a
// perturbation along them:
//     A_s dx_j = Z [ M (cm_n dx_{j-1} + cm_nn dx_{j-2}) + cc_n J(x_{j-1}) dx_{j-1} + cc_nn J(x_{j-2}) dx_{j-2} ] + B~ du_j,   dy_j = C dx_j
// with  (J(x) d)[a,i] = ∫ φ_a ((d.∇)u + (u.∇)d)_i,  u the velocity of x -- the directional derivative of the forward loop's convective
// term, a sibling of fc_adj_elem_nl that tests against φ_a only:
//   fc_tan_elem_nl:      element vectors of the bracket, eight lanes per cell (the geometry of fc_rhs_elem / fc_adj_elem_nl)
//   fc_tan_elem_nl_reg:  the same on a thread per cell (the geometry of fc_rhs_elem_reg)
//   fc_tan_elem_nl_b:    thread = (cell, simulation), base states from the batched tape [N][KB] (the geometry of fc_adj_elem_nl_b)
//   fc_tan_tail:         dx_j = x (+ dx of a refinement sweep) into the older tangent level, the finiteness flag, dy_j = C dx_j
//   fc_tan_tail_b:       the same per column of [N][KB]
// Both tangent levels are read UNMASKED (an actuated Dirichlet row of dx_{j-1} is not zero and the loop reads it); Z sits on the output
// rows, where the unchanged gather of the forward step (fc_rhs_gather / _b) puts it.  x1, d1: the level a step's cc_n / cm_n multiply,
// x2, d2: the older one.  A level whose cc is 0 is not loaded from the tape and contributes an exact 0 (its nodal values are zeros);
// the older tangent level is not loaded either when cm_nn is 0 as well (a BDF1 step).  Per quadrature point
//     g_i = w_q ( ζm_i + Σ_l cc_l ( (d_l.∇)u_l + (u_l.∇)d_l )_i ),   ζm = cm_n d1 + cm_nn d2 combined at the node
// Element vectors to ev[slot][cell] as in the forward loop.  Sums in a fixed order, no atomics, vector stores only.
#pragma once

// one level's convective derivative at a point from the value and the reference gradients of u = (ux, uy) and d = (ex, ey)
struct FcTanPoint {
  double ux = 0, uy = 0, uxi = 0, uet = 0, vxi = 0, vet = 0;  // u: value, d/dxi, d/deta of (ux, uy)
  double ex = 0, ey = 0, exi = 0, eet = 0, fxi = 0, fet = 0;  // d: the same
  __device__ __forceinline__ void add(double ph, double dx, double de, double ax, double ay, double bx, double by) {
    ux += ph * ax;
    uy += ph * ay;
    uxi += dx * ax;
    uet += de * ax;
    vxi += dx * ay;
    vet += de * ay;
    ex += ph * bx;
    ey += ph * by;
    exi += dx * bx;
    eet += de * bx;
    fxi += dx * by;
    fet += de * by;
  }
  // ((d.∇)u + (u.∇)d)_i ; physical gradients: d/dx = d/dxi*j00 + d/deta*j10 ; d/dy = d/dxi*j01 + d/deta*j11
  __device__ __forceinline__ void conv(double j00, double j01, double j10, double j11, double& cx, double& cy) const {
    const double ux_x = uxi * j00 + uet * j10, ux_y = uxi * j01 + uet * j11;
    const double uy_x = vxi * j00 + vet * j10, uy_y = vxi * j01 + vet * j11;
    const double ex_x = exi * j00 + eet * j10, ex_y = exi * j01 + eet * j11;
    const double ey_x = fxi * j00 + fet * j10, ey_y = fxi * j01 + fet * j11;
    cx = (ex * ux_x + ey * ux_y) + (ux * ex_x + uy * ex_y);
    cy = (ex * uy_x + ey * uy_y) + (ux * ey_x + uy * ey_y);
  }
};

// EIGHT lanes per cell: lane a < 6 fetches node a of its cell once (the two taped states, the two tangent levels, ζm combined at the
// node) into LDS (row stride 9: the eight cells of a wave on different banks), lane q < 7 evaluates the weighted point value at Radon
// point q, lane a < 6 tests it with φ_a in the fixed order q = 0..6.  Every cell of the mesh (single-GPU handles only).
__global__ __launch_bounds__(256) void fc_tan_elem_nl(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                      const double* __restrict__ x1, const double* __restrict__ x2,
                                                      const double* __restrict__ d1, const double* __restrict__ d2, double cm_n, double cm_nn,
                                                      double cc_n, double cc_nn, double* __restrict__ ev) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int cl = t >> 3, lane = t & 7;
  const bool active = cl < nc;
  const int c = active ? cl : 0;
  const bool l1 = cc_n != 0.0, l2 = cc_nn != 0.0, t2 = l2 || cm_nn != 0.0;  // (uniform: which levels this step reads)
  __shared__ double sh[10][32 * 9];
  const int cb = (threadIdx.x >> 3) * 9;
  if (lane < 6) {
    const int ix = cnp[lane * nc + c], iy = cnp[(6 + lane) * nc + c];
    const double ax = d1[ix], ay = d1[iy];
    const double bx = t2 ? d2[ix] : 0.0, by = t2 ? d2[iy] : 0.0;
    sh[0][cb + lane] = l1 ? x1[ix] : 0.0;
    sh[1][cb + lane] = l1 ? x1[iy] : 0.0;
    sh[2][cb + lane] = l2 ? x2[ix] : 0.0;
    sh[3][cb + lane] = l2 ? x2[iy] : 0.0;
    sh[4][cb + lane] = ax;
    sh[5][cb + lane] = ay;
    sh[6][cb + lane] = bx;
    sh[7][cb + lane] = by;
    sh[8][cb + lane] = cm_n * ax + cm_nn * bx;
    sh[9][cb + lane] = cm_n * ay + cm_nn * by;
  }
  const int q = lane < FC_NQ ? lane : FC_NQ - 1;  // lane 7 shadows point 6 with zero weight
  const double j00 = geom[c], j01 = geom[nc + c], j10 = geom[2 * nc + c], j11 = geom[3 * nc + c];
  const double wq = lane < FC_NQ ? c_qw[q] * 0.5 * geom[4 * nc + c] : 0.0;
  FcTanPoint p1, p2;
  double mx = 0, my = 0;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double ph = c_phi2[q * 6 + a], dx = c_dphi2[(q * 6 + a) * 2], de = c_dphi2[(q * 6 + a) * 2 + 1];
    p1.add(ph, dx, de, sh[0][cb + a], sh[1][cb + a], sh[4][cb + a], sh[5][cb + a]);
    p2.add(ph, dx, de, sh[2][cb + a], sh[3][cb + a], sh[6][cb + a], sh[7][cb + a]);
    mx += ph * sh[8][cb + a];
    my += ph * sh[9][cb + a];
  }
  double c1x, c1y, c2x, c2y;
  p1.conv(j00, j01, j10, j11, c1x, c1y);
  p2.conv(j00, j01, j10, j11, c2x, c2y);
  const double gx = wq * (mx + cc_n * c1x + cc_nn * c2x), gy = wq * (my + cc_n * c1y + cc_nn * c2y);
  // lane a < 6 gathers the weighted point values and tests them with phi_a
  const int a = lane < 6 ? lane : 5;
  double accx = 0.0, accy = 0.0;
#pragma unroll
  for (int p = 0; p < FC_NQ; ++p) {
    const double pa = c_phi2[p * 6 + a];
    accx += pa * __shfl(gx, p, 8);
    accy += pa * __shfl(gy, p, 8);
  }
  if (active && lane < 6) {
    ev[(size_t)lane * nc + c] = accx;
    ev[(size_t)(6 + lane) * nc + c] = accy;
  }
}

// A cell's whole work on ONE thread, for the single march (KB = 1, column 0) and for KB simulations (thread = (cell, simulation),
// simulation fastest): nodal values in registers, basis tables through the scalar unit, no LDS, no shuffles; the sums run in the
// order of the eight-lane form.  x1, x2: [N][XS] with the simulation's base state in column xs; d1, d2, ev: [.][KB], column s.
template <int KB>
__device__ __forceinline__ void fc_tan_cell(int nc, int c, int s, int XS, int xs, const int* __restrict__ cnp, const double* __restrict__ geom,
                                            const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ d1,
                                            const double* __restrict__ d2, double cm_n, double cm_nn, double cc_n, double cc_nn,
                                            double* __restrict__ ev) {
  const bool l1 = cc_n != 0.0, l2 = cc_nn != 0.0, t2 = l2 || cm_nn != 0.0;
  double x1x[6], x1y[6], x2x[6], x2y[6], d1x[6], d1y[6], d2x[6], d2y[6], zmx[6], zmy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const size_t rx = (size_t)cnp[a * nc + c], ry = (size_t)cnp[(6 + a) * nc + c];
    const size_t ix = rx * KB + s, iy = ry * KB + s, bx = rx * XS + xs, by = ry * XS + xs;
    x1x[a] = l1 ? x1[bx] : 0.0;
    x1y[a] = l1 ? x1[by] : 0.0;
    x2x[a] = l2 ? x2[bx] : 0.0;
    x2y[a] = l2 ? x2[by] : 0.0;
    d1x[a] = d1[ix];
    d1y[a] = d1[iy];
    d2x[a] = t2 ? d2[ix] : 0.0;
    d2y[a] = t2 ? d2[iy] : 0.0;
    zmx[a] = cm_n * d1x[a] + cm_nn * d2x[a];
    zmy[a] = cm_n * d1y[a] + cm_nn * d2y[a];
  }
  const double j00 = geom[c], j01 = geom[nc + c], j10 = geom[2 * nc + c], j11 = geom[3 * nc + c], hdet = 0.5 * geom[4 * nc + c];
  double accx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < FC_NQ; ++q) {
    FcTanPoint p1, p2;
    double mx = 0, my = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double ph = c_phi2[q * 6 + a], dx = c_dphi2[(q * 6 + a) * 2], de = c_dphi2[(q * 6 + a) * 2 + 1];
      p1.add(ph, dx, de, x1x[a], x1y[a], d1x[a], d1y[a]);
      p2.add(ph, dx, de, x2x[a], x2y[a], d2x[a], d2y[a]);
      mx += ph * zmx[a];
      my += ph * zmy[a];
    }
    double c1x, c1y, c2x, c2y;
    p1.conv(j00, j01, j10, j11, c1x, c1y);
    p2.conv(j00, j01, j10, j11, c2x, c2y);
    const double wq = c_qw[q] * hdet;
    const double gx = wq * (mx + cc_n * c1x + cc_nn * c2x), gy = wq * (my + cc_n * c1y + cc_nn * c2y);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      accx[a] += c_phi2[q * 6 + a] * gx;
      accy[a] += c_phi2[q * 6 + a] * gy;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    ev[((size_t)a * nc + c) * KB + s] = accx[a];
    ev[((size_t)(6 + a) * nc + c) * KB + s] = accy[a];
  }
}

// thread per cell: for meshes whose cells alone fill the SIMDs (fc_ctx::elem_reg_min, as fc_rhs_elem_reg)
__global__ __launch_bounds__(256) void fc_tan_elem_nl_reg(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                          const double* __restrict__ x1, const double* __restrict__ x2,
                                                          const double* __restrict__ d1, const double* __restrict__ d2, double cm_n,
                                                          double cm_nn, double cc_n, double cc_nn, double* __restrict__ ev) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  fc_tan_cell<1>(nc, c, 0, 1, 0, cnp, geom, x1, x2, d1, d2, cm_n, cm_nn, cc_n, cc_nn, ev);
}

// thread = (cell, simulation s), s fastest.  x1, x2: columns of the batched tape [N][KB].  SHARED: every simulation perturbs the
// trajectory of ONE column ref_col (a broadcast load: the KB threads of a cell read the same word); else column s its own.
template <int KB, bool SHARED>
__global__ __launch_bounds__(256) void fc_tan_elem_nl_b(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                        const double* __restrict__ x1, const double* __restrict__ x2,
                                                        const double* __restrict__ d1, const double* __restrict__ d2, double cm_n,
                                                        double cm_nn, double cc_n, double cc_nn, int ref_col, double* __restrict__ ev) {
  constexpr int CPB = 256 / KB;
  const int s = (int)threadIdx.x % KB, c = blockIdx.x * CPB + (int)threadIdx.x / KB;
  if (c >= nc) return;
  fc_tan_cell<KB>(nc, c, s, KB, SHARED ? ref_col : s, cnp, geom, x1, x2, d1, d2, cm_n, cm_nn, cc_n, cc_nn, ev);
}

// Body-force actuators of the batched march: b[i][s] += Σ_k du[s][k] F_k[i] off the Dirichlet rows, F_k the load vector of profile k
// (fc_force_rows) -- what fc_rhs_gather adds for the single march; fc_rhs_gather_b has no such term, because the batched forward step
// enters its body forces in the element loop.  thread = (row, simulation); the same value into the y half of the work buffer.
template <int KB>
__global__ __launch_bounds__(256) void fc_tan_force_b(int N, const int* __restrict__ bcslot, int n_act, const double* __restrict__ fvec,
                                                      const double* __restrict__ du, double* __restrict__ b, double* __restrict__ y) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)N * KB) return;
  const int i = (int)(t / KB), s = (int)(t % KB);
  if (bcslot[i] >= 0) return;
  double acc = 0.0;
  for (int k = 0; k < n_act; ++k) acc += du[(size_t)s * n_act + k] * fvec[(size_t)k * N + i];
  const double v = b[t] + acc;
  b[t] = v;
  y[t] = v;
}

// Behind the sweeps: the new tangent level = x (+ dx, the last correction of a refined solve) into `lev` (the place of dx_{j-2}, which
// the element loop of this step has read), flag = 1 on a non-finite entry, and -- workgroup 0, a wave per sensor, lanes over the
// sensor's entries, a fixed shuffle tree -- dy[s] = C_s . dx_j read from x (+ dx) itself.
__global__ __launch_bounds__(256) void fc_tan_tail(int N, const double* __restrict__ x, const double* __restrict__ dx, double* __restrict__ lev,
                                                   int* __restrict__ flag, int n_sens, const int* __restrict__ s_rowptr,
                                                   const int* __restrict__ s_idxp, const double* __restrict__ s_w, double* __restrict__ dy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    const double v = dx ? x[i] + dx[i] : x[i];
    if (!isfinite(v)) *flag = 1;
    lev[i] = v;
  }
  if (blockIdx.x != 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int s = wave; s < n_sens; s += 4) {
    double acc = 0.0;
    for (int k = s_rowptr[s] + lane; k < s_rowptr[s + 1]; k += 64) {
      const int r = s_idxp[k];
      acc += s_w[k] * (dx ? x[r] + dx[r] : x[r]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) dy[s] = acc;
  }
}

// The same for KB simulations, x [N][KB] the solution half of the batched work buffer: thread = (row, simulation), flag[s] per
// column; workgroup 0 then forms dy[s][sensor] for the k real columns (thread = simulation, sensors and their entries in order).
// Padding columns reach no output.
template <int KB>
__global__ __launch_bounds__(256) void fc_tan_tail_b(int N, int k, const double* __restrict__ x, double* __restrict__ lev, int* __restrict__ flag,
                                                     int n_sens, const int* __restrict__ s_rowptr, const int* __restrict__ s_idxp,
                                                     const double* __restrict__ s_w, double* __restrict__ dy) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (size_t)N * KB) {
    const double v = x[t];
    if (!isfinite(v)) flag[t % KB] = 1;
    lev[t] = v;
  }
  if (blockIdx.x != 0 || (int)threadIdx.x >= k) return;
  const int s = threadIdx.x;
  for (int m = 0; m < n_sens; ++m) {
    double acc = 0.0;
    for (int q = s_rowptr[m]; q < s_rowptr[m + 1]; ++q) acc += s_w[q] * x[(size_t)s_idxp[q] * KB + s];
    dy[(size_t)s * n_sens + m] = acc;
  }
}
