// fc_adjoint_nl.hip.h -- the adjoint of the NONLINEAR stepper (fc_run_adjoint on a handle with fc_set_time_scheme(dt, 1); host side in
// fc_adjoint_run.hpp, bookkeeping of the state tape in fc_adjoint_segments.hpp).  The forward step adds the explicit
// convective term  cc_n N(x_{j-1}) + cc_nn N(x_{j-2}),  N(x)[a,i] = ∫ φ_a ((u.∇)u)_i,  to the mass product; its exact discrete adjoint
// adds  J(x_m)^T Z (cc_n mu_{m+1} + cc_nn mu_{m+2}),  J = dN/dx, to  M Z (cm_n mu_{m+1} + cm_nn mu_{m+2}):
//   fc_adj_tape_copy:   the state a step just wrote -> its column of the tape (permuted numbering, one contiguous copy)
//   fc_adj_ctrl_rows:   the control rows a step reads <-> the control tape of the checkpointed state tape (fc_adjoint_segments.hpp)
//   fc_adj_elem_nl:     element vectors of both products, eight lanes per cell (the geometry of fc_rhs_elem)
//   fc_adj_elem_nl_reg: the same on a thread per cell (the geometry of fc_rhs_elem_reg)
// EN = true (energy weights held, fc_set_adjoint_energy): ζm also takes e x_m at the node, e = e_row[0] the weight of dE_m -- one
// multiply-add per node on a value the loop loads anyway (fc_adjoint_energy.hip.h).  EN = false is the loop as it always was.
// SRC = true (with EN; fc_set_adjoint_energy_source(1), the Gauss-Newton product of the energy cost): the energy value at the node is
// loaded from a SEPARATE column xe (a column of the tangent tape, dx_m) while J(x_m)^T still reads the taped state x: ζm takes e xe.
// SRC = false never reads xe (null) and is the code it was.
// With ζm = cm_n z1 + cm_nn z2 and ζc = cc_n z1 + cc_nn z2 (z1, z2: the march's Dirichlet-masked copies of mu_{m+1}, mu_{m+2} -- the
// mask sits on the INPUT; both forward steps that read x_m go through the same J(x_m), so the levels are combined first) and u the
// velocity of the taped state x_m (unmasked: actuated Dirichlet values included), per quadrature point
//     out[b,i] = Σ_q w_q [ φ_b ( ζm_i + Σ_j (∂_i u_j) ζc_j ) + (u.∇φ_b) ζc_i ]
// The forward loop tests against φ_b only; this one also against ∇φ_b = (∂ξ φ_b, ∂η φ_b) J^-1: six weighted point values per lane go
// round instead of two.  Element vectors to ev[slot][cell] as in the forward loop: fc_adj_rhs_gather sums them on every row.
// Sums in a fixed order, no atomics, vector stores only.
#pragma once

// dst[i] = src[i].  NT: the column is read again only by the backward march, a whole run later -- nontemporal stores keep it from
// displacing the factors in the Infinity Cache (as fc_ssnap_capture).
template <bool NT>
__global__ __launch_bounds__(256) void fc_adj_tape_copy(int n, const double* __restrict__ src, double* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = src[i];
  if (NT)
    __builtin_nontemporal_store(v, &dst[i]);
  else
    dst[i] = v;
}

// The control rows of one step between the record a plant step reads and the control tape of the checkpointed state tape (fc_ctx::Adj::
// ctape; DESIGN §5.4 "Checkpointed tape"), either way: simulation s < k, actuator a < na:  du[s][a] = u[s][a],  df[s][a] = uf[s][a]
// (uf null: the step read u for both).  Source rows src_stride doubles apart, destination rows dst_stride.  One workgroup.
__global__ __launch_bounds__(256) void fc_adj_ctrl_rows(int k, int na, const double* __restrict__ u, const double* __restrict__ uf, int src_stride,
                                                        double* __restrict__ du, double* __restrict__ df, int dst_stride) {
  for (int i = threadIdx.x; i < k * na; i += blockDim.x) {
    const int s = i / na, a = i - s * na;
    du[(size_t)s * dst_stride + a] = u[(size_t)s * src_stride + a];
    df[(size_t)s * dst_stride + a] = (uf ? uf : u)[(size_t)s * src_stride + a];
  }
}

// EIGHT lanes per cell: lane a < 6 fetches node a of its cell once (the state, the two adjoint levels, combined at the node) into LDS
// (row stride 9: the eight cells of a wave on different banks), lane q < 7 evaluates the six weighted point values at Radon point q,
// lane a < 6 tests them with φ_a, ∂ξ φ_a, ∂η φ_a in the fixed order q = 0..6.  Every cell of the mesh (single-GPU handles only).
template <bool EN, bool SRC = false>
__global__ __launch_bounds__(256) void fc_adj_elem_nl(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                      const double* __restrict__ x, const double* __restrict__ z1,
                                                      const double* __restrict__ z2, double cm_n, double cm_nn, double cc_n, double cc_nn,
                                                      const double* __restrict__ e_row, double* __restrict__ ev,
                                                      const double* __restrict__ xe = nullptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int cl = t >> 3, lane = t & 7;
  const bool active = cl < nc;
  const int c = active ? cl : 0;
  __shared__ double sh[6][32 * 9];
  const int cb = (threadIdx.x >> 3) * 9;
  if (lane < 6) {
    const int ix = cnp[lane * nc + c], iy = cnp[(6 + lane) * nc + c];
    const double ax = z1[ix], ay = z1[iy], bx = z2[ix], by = z2[iy];
    const double xv = x[ix], yv = x[iy];
    sh[0][cb + lane] = xv;
    sh[1][cb + lane] = yv;
    if constexpr (EN && SRC) {
      const double e = e_row[0];
      sh[2][cb + lane] = cm_n * ax + cm_nn * bx + e * xe[ix];
      sh[3][cb + lane] = cm_n * ay + cm_nn * by + e * xe[iy];
    } else if constexpr (EN) {
      const double e = e_row[0];
      sh[2][cb + lane] = cm_n * ax + cm_nn * bx + e * xv;
      sh[3][cb + lane] = cm_n * ay + cm_nn * by + e * yv;
    } else {
      sh[2][cb + lane] = cm_n * ax + cm_nn * bx;
      sh[3][cb + lane] = cm_n * ay + cm_nn * by;
    }
    sh[4][cb + lane] = cc_n * ax + cc_nn * bx;
    sh[5][cb + lane] = cc_n * ay + cc_nn * by;
  }
  const int q = lane < FC_NQ ? lane : FC_NQ - 1;  // lane 7 shadows point 6 with zero weight (its values are never read)
  const double j00 = geom[c], j01 = geom[nc + c], j10 = geom[2 * nc + c], j11 = geom[3 * nc + c];
  const double wq = lane < FC_NQ ? c_qw[q] * 0.5 * geom[4 * nc + c] : 0.0;
  double ux = 0, uy = 0, uxi = 0, uet = 0, vxi = 0, vet = 0;  // state: value, d/dxi, d/deta of (ux, uy)
  double mx = 0, my = 0, kx = 0, ky = 0;                      // ζm, ζc at the point
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double ax = sh[0][cb + a], ay = sh[1][cb + a];
    const double ph = c_phi2[q * 6 + a], dx = c_dphi2[(q * 6 + a) * 2], de = c_dphi2[(q * 6 + a) * 2 + 1];
    ux += ph * ax;
    uy += ph * ay;
    uxi += dx * ax;
    uet += de * ax;
    vxi += dx * ay;
    vet += de * ay;
    mx += ph * sh[2][cb + a];
    my += ph * sh[3][cb + a];
    kx += ph * sh[4][cb + a];
    ky += ph * sh[5][cb + a];
  }
  // physical gradients: d/dx = d/dxi*j00 + d/deta*j10 ; d/dy = d/dxi*j01 + d/deta*j11
  const double ux_x = uxi * j00 + uet * j10, ux_y = uxi * j01 + uet * j11;
  const double uy_x = vxi * j00 + vet * j10, uy_y = vxi * j01 + vet * j11;
  // tested with φ_b: ζm_i + Σ_j (∂_i u_j) ζc_j
  const double fx = wq * (mx + ux_x * kx + uy_x * ky), fy = wq * (my + ux_y * kx + uy_y * ky);
  // tested with ∇φ_b: u.∇φ_b = ∂ξ φ_b (ux j00 + uy j01) + ∂η φ_b (ux j10 + uy j11)
  const double sxi = wq * (ux * j00 + uy * j01), set = wq * (ux * j10 + uy * j11);
  const double px = sxi * kx, py = sxi * ky, ex = set * kx, ey = set * ky;
  const int a = lane < 6 ? lane : 5;
  double accx = 0.0, accy = 0.0;
#pragma unroll
  for (int p = 0; p < FC_NQ; ++p) {
    const double pa = c_phi2[p * 6 + a], da = c_dphi2[(p * 6 + a) * 2], ea = c_dphi2[(p * 6 + a) * 2 + 1];
    accx += pa * __shfl(fx, p, 8) + da * __shfl(px, p, 8) + ea * __shfl(ex, p, 8);
    accy += pa * __shfl(fy, p, 8) + da * __shfl(py, p, 8) + ea * __shfl(ey, p, 8);
  }
  if (active && lane < 6) {
    ev[(size_t)lane * nc + c] = accx;
    ev[(size_t)(6 + lane) * nc + c] = accy;
  }
}

// The same loop with a cell's whole work on ONE thread (nodal values in registers, basis tables through the scalar unit, no LDS, no
// shuffles; the sums run in the same order): for meshes whose cells alone fill the SIMDs (fc_ctx::elem_reg_min, as fc_rhs_elem_reg).
template <bool EN, bool SRC = false>
__global__ __launch_bounds__(256) void fc_adj_elem_nl_reg(int nc, const int* __restrict__ cnp, const double* __restrict__ geom,
                                                          const double* __restrict__ x, const double* __restrict__ z1,
                                                          const double* __restrict__ z2, double cm_n, double cm_nn, double cc_n,
                                                          double cc_nn, const double* __restrict__ e_row, double* __restrict__ ev,
                                                          const double* __restrict__ xe = nullptr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double e = 0.0;
  if constexpr (EN) e = e_row[0];
  double xx[6], xy[6], zmx[6], zmy[6], zcx[6], zcy[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const int ix = cnp[a * nc + c], iy = cnp[(6 + a) * nc + c];
    const double ax = z1[ix], ay = z1[iy], bx = z2[ix], by = z2[iy];
    xx[a] = x[ix];
    xy[a] = x[iy];
    if constexpr (EN && SRC) {
      zmx[a] = cm_n * ax + cm_nn * bx + e * xe[ix];
      zmy[a] = cm_n * ay + cm_nn * by + e * xe[iy];
    } else if constexpr (EN) {
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
    ev[(size_t)a * nc + c] = accx[a];
    ev[(size_t)(6 + a) * nc + c] = accy[a];
  }
}
