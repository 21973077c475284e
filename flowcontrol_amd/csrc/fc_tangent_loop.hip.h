// fc_tangent_loop.hip.h -- the controller inside the tangent march: the tangent of fc_ctrl_step (fc_run_tangent_closed_loop /
// fc_run_tangent_closed_loop_batch; host side in fc_tangent_loop_run.hpp; DESIGN §5.6 "Closed loop").
//
// Forward step m of a closed loop (fc_ctrl.hip.h; xi = controller state):
//     yc_m = G y_{m-1} + g0 + w_y[m]      uc_m = C xi_{m-1} + D yc_m      xi_m = Ad xi_{m-1} + Bd yc_m
//     v_m  = S uc_m + w_u[m]              u_m  = min(max(v_m, lo), hi)
// Tangent step m along (dAd, dBd, dC, dD, dG, dg0, dS, dxi_0, dy_0, dw_y, dw_u), AHEAD of the plant's tangent step m (which reads du_m
// as its control row and leaves dy_m for the controller launch of step m + 1):
//     dyc_m = G dy_{m-1} + dG y_{m-1} + dg0 + dw_y[m]
//     duc_m = C dxi_{m-1} + dC xi_{m-1} + D dyc_m + dD yc_m
//     dxi_m = Ad dxi_{m-1} + dAd xi_{m-1} + Bd dyc_m + dBd yc_m          (old dxi, old xi)
//     dv_m  = S duc_m + dS uc_m + dw_u[m]       du_m = sigma_m o dv_m     (sigma = 1 where lo < v_m < hi, else 0: the adjoint's mask)
//
// Read of the forward run: the loop tape's row of step m, [ xi_{m-1} (nx) | y_{m-1} (n_sens) | v_m (n_act) ] (fc_ctrl_step wrote it).
// yc_m and uc_m are not taped: they are formed again by the forward kernel's own loops over the same bank, bit for bit.
// The direction matrices sit in a second bank in the forward bank's TRANSPOSED per-column layout, same offsets:
//     [dAdT | dBdT | dCT | dDT | dGT | dg0 | dST]
// so every loop below is the forward kernel's with a second operand.  A null direction bank skips its terms (all parameter directions
// zero); null dw_y / dw_u skip theirs.
#pragma once
#include <hip/hip_runtime.h>

#include "fc_ctrl.hip.h"

// where tangent step m of ONE controller finds its inputs and leaves its outputs (all DEVICE memory)
struct FcCtrlTanIO {
  const double* dmat;   // the controller's block of the direction bank, or null
  const double* tape;   // tape row of step m of the loop it linearises about
  const double* w_y;    // [nyc] the signal row forward step m read, or null
  const double* u_lo;   // [n_act] limits, both or neither
  const double* u_hi;
  const double* dy;     // [n_sens] dy_{m-1}: the row the plant's tangent tail wrote, at m = 1 the dy_0 buffer
  const double* dw_y;   // [nyc] direction of the signal row, or null
  const double* dw_u;   // [n_act] or null
  double* dxi;          // [nx] dxi_{m-1} in, dxi_m out
  double* du;           // [n_act] the control row of the plant's tangent step m
};

// One workgroup of ONE wave, like fc_ctrl_step: a lane owns output rows and forms every sum in index order -- no cross-lane reduction,
// no atomics -- so two marches on the same inputs are bit-identical.  xi, dxi, y, dy, yc, dyc, uc, duc sit in LDS (5.6 KB); the new dxi
// stays in registers until every lane has finished reading the old one; the signals' directions are added last in their stage.  All
// stores are ordinary vector stores.
//
// The body of one controller's tangent step, shared by fc_ctrl_tan_step (k = 1) and fc_ctrl_tan_step_b (one wave per column of a
// batch): M = the transposed block of the bank it linearises about, io = ITS pointers.
__device__ __forceinline__ void fc_ctrl_tan_step_body(const FcCtrlBank& bk, const double* __restrict__ M, const FcCtrlTanIO& io) {
  const int lane = threadIdx.x;
  __shared__ double xs[FC_CTRL_NX_MAX];
  __shared__ double dxs[FC_CTRL_NX_MAX];
  __shared__ double ys[FC_CTRL_NSENS_MAX];
  __shared__ double dys[FC_CTRL_NSENS_MAX];
  __shared__ double ycs[FC_CTRL_NYC_MAX];
  __shared__ double dycs[FC_CTRL_NYC_MAX];
  __shared__ double ucs[FC_CTRL_NUC_MAX];
  __shared__ double ducs[FC_CTRL_NUC_MAX];
  const int nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc, ns = bk.n_sens, na = bk.n_act;
  const double* __restrict__ dM = io.dmat;
  for (int c = lane; c < nx; c += 64) {
    xs[c] = io.tape[c];
    dxs[c] = io.dxi[c];
  }
  for (int q = lane; q < ns; q += 64) {
    ys[q] = io.tape[nx + q];
    dys[q] = io.dy[q];
  }
  __syncthreads();
  // yc_m = G y_{m-1} + g0 (+ w_y): the forward kernel's sum;  dyc_m = G dy_{m-1} + dG y_{m-1} + dg0 (+ dw_y)
  if (lane < nyc) {
    const double* __restrict__ GT = M + bk.oG;
    double acc = 0.0, d1 = 0.0, d2 = 0.0;
    for (int q = 0; q < ns; ++q) acc += GT[(long long)q * nyc + lane] * ys[q];
    double t = acc + M[bk.og0 + lane];
    if (io.w_y) t += io.w_y[lane];
    ycs[lane] = t;
    for (int q = 0; q < ns; ++q) d1 += GT[(long long)q * nyc + lane] * dys[q];
    if (dM) {
      const double* __restrict__ dGT = dM + bk.oG;
      for (int q = 0; q < ns; ++q) d2 += dGT[(long long)q * nyc + lane] * ys[q];
      d2 += dM[bk.og0 + lane];
    }
    double dt = d1 + d2;
    if (io.dw_y) dt += io.dw_y[lane];
    dycs[lane] = dt;
  }
  __syncthreads();
  // uc_m = C xi_{m-1} + D yc_m: the forward kernel's sum;  duc_m = C dxi_{m-1} + D dyc_m + dC xi_{m-1} + dD yc_m
  if (lane < nuc) {
    const double* __restrict__ CT = M + bk.oC;
    const double* __restrict__ DT = M + bk.oD;
    double a1 = 0.0, a2 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0;
    for (int c = 0; c < nx; ++c) a1 += CT[(long long)c * nuc + lane] * xs[c];
    for (int j = 0; j < nyc; ++j) a2 += DT[(long long)j * nuc + lane] * ycs[j];
    ucs[lane] = a1 + a2;
    for (int c = 0; c < nx; ++c) d1 += CT[(long long)c * nuc + lane] * dxs[c];
    for (int j = 0; j < nyc; ++j) d2 += DT[(long long)j * nuc + lane] * dycs[j];
    if (dM) {
      const double* __restrict__ dCT = dM + bk.oC;
      const double* __restrict__ dDT = dM + bk.oD;
      for (int c = 0; c < nx; ++c) d3 += dCT[(long long)c * nuc + lane] * xs[c];
      for (int j = 0; j < nyc; ++j) d4 += dDT[(long long)j * nuc + lane] * ycs[j];
    }
    ducs[lane] = (d1 + d2) + (d3 + d4);
  }
  // dxi_m = Ad dxi_{m-1} + Bd dyc_m + dAd xi_{m-1} + dBd yc_m: rows lane, lane + 64, ... (<= 4 per lane), kept in registers until every
  // lane is through with dxs
  double dxn[FC_CTRL_NX_MAX / 64];
  {
    const double* __restrict__ BdT = M + bk.oBd;
#pragma unroll
    for (int i = 0; i < FC_CTRL_NX_MAX / 64; ++i) {
      const int r = lane + 64 * i;
      double d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0;
      if (r < nx) {
        for (int c = 0; c < nx; ++c) d1 += M[(long long)c * nx + r] * dxs[c];
        for (int j = 0; j < nyc; ++j) d2 += BdT[(long long)j * nx + r] * dycs[j];
        if (dM) {
          const double* __restrict__ dBdT = dM + bk.oBd;
          for (int c = 0; c < nx; ++c) d3 += dM[(long long)c * nx + r] * xs[c];
          for (int j = 0; j < nyc; ++j) d4 += dBdT[(long long)j * nx + r] * ycs[j];
        }
      }
      dxn[i] = (d1 + d2) + (d3 + d4);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FC_CTRL_NX_MAX / 64; ++i) {
    const int r = lane + 64 * i;
    if (r < nx) io.dxi[r] = dxn[i];
  }
  // du_m = sigma_m o (S duc_m + dS uc_m + dw_u): sigma from the taped unclamped v_m, the adjoint's two strict compares
  for (int a = lane; a < na; a += 64) {
    const double* __restrict__ ST = M + bk.oS;
    double d1 = 0.0, d2 = 0.0;
    for (int c = 0; c < nuc; ++c) d1 += ST[(long long)c * na + a] * ducs[c];
    if (dM) {
      const double* __restrict__ dST = dM + bk.oS;
      for (int c = 0; c < nuc; ++c) d2 += dST[(long long)c * na + a] * ucs[c];
    }
    double dv = d1 + d2;
    if (io.dw_u) dv += io.dw_u[a];
    if (io.u_lo) {
      const double v = io.tape[nx + ns + a];
      dv = (io.u_lo[a] < v && v < io.u_hi[a]) ? dv : 0.0;
    }
    io.du[a] = dv;
  }
}

__global__ __launch_bounds__(64) void fc_ctrl_tan_step(FcCtrlBank bk, FcCtrlTanIO io) {
  fc_ctrl_tan_step_body(bk, bk.mat, io);  // (k = 1: simulation 0's block)
}

// Tangent step m of all k columns: grid k, ONE wave per column.  io holds the pointers of COLUMN 0 (null where the single kernel takes
// null).  Column s reads ITS direction block, dxi, dy row and dw rows, and writes ITS du row (n_act doubles apart in the step's row of
// the padded width the batched gather reads; the columns >= k are never written and stay zero).  What it linearises about -- bank
// block, tape row, signal row, limits -- is column s's, or with REF (ref_col = c) column c's: k directions about one loop.
template <bool REF>
__global__ __launch_bounds__(64) void fc_ctrl_tan_step_b(FcCtrlBank bk, FcCtrlTanIO io, int ref_col) {
  const int s = blockIdx.x, b = REF ? ref_col : s;
  const int nx = bk.nx, nyc = bk.nyc, ns = bk.n_sens, na = bk.n_act;
  const long long TR = (long long)nx + ns + na;
  FcCtrlTanIO c = io;
  if (io.dmat) c.dmat = io.dmat + (long long)s * bk.stride;
  c.tape = io.tape + (long long)b * TR;
  if (io.w_y) c.w_y = io.w_y + (long long)b * nyc;
  if (io.u_lo) c.u_lo = io.u_lo + (long long)b * na, c.u_hi = io.u_hi + (long long)b * na;
  c.dy = io.dy + (long long)s * ns;
  if (io.dw_y) c.dw_y = io.dw_y + (long long)s * nyc;
  if (io.dw_u) c.dw_u = io.dw_u + (long long)s * na;
  c.dxi = io.dxi + (long long)s * nx;
  c.du = io.du + (long long)s * na;
  fc_ctrl_tan_step_body(bk, bk.mat + (long long)b * bk.stride, c);
}
