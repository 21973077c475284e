// fc_adjoint_energy.hip.h -- the energy term of the cost in the backward marches (fc_set_adjoint_energy; host side in
// fc_adjoint_energy_run.hpp and the two right-hand-side functions adj_enqueue_rhs / adjb_enqueue_rhs; DESIGN §5.4 "Energy term").
// A cost term  sum_m e_m dE_m,  dE_m = 1/2 x_m^T M x_m  (velocity mass matrix, the FULL state: actuated Dirichlet values included),
// adds  e_m M x_m  to the right-hand side of backward step m, on every row, unmasked.  The mass product is linear, so the forcing is
// folded in at the nodes, in front of the quadrature:
//     M Z (cm_n mu_{m+1} + cm_nn mu_{m+2}) + e_m M x_m  =  M (cm_n z1 + cm_nn z2 + e_m x_m)
// with z1, z2 the march's Dirichlet-masked copies (the mask sits on the INPUT, as everywhere in the march) and x_m the taped state, which
// is NOT masked: dE integrates the whole velocity field.
//   fc_adj_elem_en:       element vectors of that product, eight lanes per cell (the geometry of fc_rhs_elem)
//   fc_adj_elem_en_reg:   the same on a thread per cell (the geometry of fc_rhs_elem_reg)
//   fc_adj_elem_en_b<KB>: thread = (cell, simulation), e read per column from the device row of the step (the geometry of fc_rhs_elem_breg)
// These run on LINEARISED handles, in the place of the forward loops on the two masked levels; nonlinear handles run the EN = true
// instantiations of fc_adj_elem_nl / _reg / _b, which add e x to zeta_m at the node.  e: the device row of the step (one double for a
// single march, KB for a batched one; columns >= k hold 0).  Element vectors to ev[slot][cell] as in the forward loop; fc_adj_rhs_gather /
// fc_adj_rhs_gather_b sum them on every row.  Sums in a fixed order (a = 0..5 inside a point, points 0..6 into the test functions), no
// atomics, vector stores only.
#pragma once

__global__ __launch_bounds__(256) void fc_adj_elem_en(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                      const double* __restrict__ x, const double* __restrict__ z1,
                                                      const double* __restrict__ z2, double cm_n, double cm_nn,
                                                      const double* __restrict__ e_row, double* __restrict__ ev) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int cl = t >> 3, lane = t & 7;
  const bool active = cl < nc;
  const int c = active ? cl : 0;
  __shared__ double sh[2][32 * 9];
  const int cb = (threadIdx.x >> 3) * 9;
  if (lane < 6) {
    const double e = e_row[0];
    const int ix = cnp[lane * nc + c], iy = cnp[(6 + lane) * nc + c];
    sh[0][cb + lane] = cm_n * z1[ix] + cm_nn * z2[ix] + e * x[ix];
    sh[1][cb + lane] = cm_n * z1[iy] + cm_nn * z2[iy] + e * x[iy];
  }
  const int q = lane < FC_NQ ? lane : FC_NQ - 1;  // lane 7 shadows point 6 with zero weight (its values are never read)
  const double wq = lane < FC_NQ ? c_qw[q] * 0.5 * geom[4 * nc + c] : 0.0;
  double mx = 0, my = 0;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double ph = c_phi2[q * 6 + a];
    mx += ph * sh[0][cb + a];
    my += ph * sh[1][cb + a];
  }
  const double fx = wq * mx, fy = wq * my;
  const int a = lane < 6 ? lane : 5;
  double accx = 0.0, accy = 0.0;
#pragma unroll
  for (int p = 0; p < FC_NQ; ++p) {
    const double pa = c_phi2[p * 6 + a];
    accx += pa * __shfl(fx, p, 8);
    accy += pa * __shfl(fy, p, 8);
  }
  if (active && lane < 6) {
    ev[(size_t)lane * nc + c] = accx;
    ev[(size_t)(6 + lane) * nc + c] = accy;
  }
}

__global__ __launch_bounds__(256) void fc_adj_elem_en_reg(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                          const double* __restrict__ x, const double* __restrict__ z1,
                                                          const double* __restrict__ z2, double cm_n, double cm_nn,
                                                          const double* __restrict__ e_row, double* __restrict__ ev) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const double e = e_row[0];
  double zx[6], zy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const int ix = cnp[a * nc + c], iy = cnp[(6 + a) * nc + c];
    zx[a] = cm_n * z1[ix] + cm_nn * z2[ix] + e * x[ix];
    zy[a] = cm_n * z1[iy] + cm_nn * z2[iy] + e * x[iy];
  }
  const double hdet = 0.5 * geom[4 * nc + c];
  double accx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < FC_NQ; ++q) {
    double mx = 0, my = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double ph = c_phi2[q * 6 + a];
      mx += ph * zx[a];
      my += ph * zy[a];
    }
    const double wq = c_qw[q] * hdet;
    const double fx = wq * mx, fy = wq * my;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      accx[a] += c_phi2[q * 6 + a] * fx;
      accy[a] += c_phi2[q * 6 + a] * fy;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    ev[(size_t)a * nc + c] = accx[a];
    ev[(size_t)(6 + a) * nc + c] = accy[a];
  }
}

// x: the taped state [N][KB] (unmasked); z1, z2: the two masked levels [N][KB]; e_row [KB].  ev[(slot * nc + cell) * KB + s].
template <int KB>
__global__ __launch_bounds__(256) void fc_adj_elem_en_b(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                        const double* __restrict__ x, const double* __restrict__ z1,
                                                        const double* __restrict__ z2, double cm_n, double cm_nn,
                                                        const double* __restrict__ e_row, double* __restrict__ ev) {
  constexpr int CPB = 256 / KB;
  const int s = (int)threadIdx.x % KB, c = blockIdx.x * CPB + (int)threadIdx.x / KB;
  if (c >= nc) return;
  const double e = e_row[s];
  double zx[6], zy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const size_t ix = (size_t)cnp[a * nc + c] * KB + s, iy = (size_t)cnp[(6 + a) * nc + c] * KB + s;
    zx[a] = cm_n * z1[ix] + cm_nn * z2[ix] + e * x[ix];
    zy[a] = cm_n * z1[iy] + cm_nn * z2[iy] + e * x[iy];
  }
  const double hdet = 0.5 * geom[4 * nc + c];
  double accx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, accy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < FC_NQ; ++q) {
    double mx = 0, my = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double ph = c_phi2[q * 6 + a];
      mx += ph * zx[a];
      my += ph * zy[a];
    }
    const double wq = c_qw[q] * hdet;
    const double fx = wq * mx, fy = wq * my;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      accx[a] += c_phi2[q * 6 + a] * fx;
      accy[a] += c_phi2[q * 6 + a] * fy;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    ev[((size_t)a * nc + c) * KB + s] = accx[a];
    ev[((size_t)(6 + a) * nc + c) * KB + s] = accy[a];
  }
}
