// fc_adjoint_loop.hip.h -- the controller inside the backward march: the adjoint of fc_ctrl_step (fc_run_adjoint_closed_loop; host side
// in fc_adjoint_loop_run.hpp, tape bookkeeping in fc_adjoint_loop_tape.hpp).
//
// Forward step m of a closed loop (fc_ctrl.hip.h, k = 1; xi = controller state):
//     yc_m = G y_{m-1} + g0 + w_y[m]      uc_m = C xi_{m-1} + D yc_m      xi_m = Ad xi_{m-1} + Bd yc_m
//     v_m  = S uc_m + w_u[m]              u_m  = min(max(v_m, lo), hi)
// Backward step m, behind the plant's backward step m (which left B~^T mu_m in the g row); lambda = adjoint of xi, eta = adjoint of yc:
//     ub_m  = B~^T mu_m + r_m             vb_m = sigma_m o ub_m     (sigma = 1 where lo < v_m < hi, else 0; all 1 without limits)
//     ucb_m = S^T vb_m                    eta_m = D^T ucb_m + Bd^T lambda_m          lambda_{m-1} = Ad^T lambda_m + C^T ucb_m
// and G^T eta_m is ADDED to the sensor weights of backward step m - 1 (at m = 1: written to the dJ/dy_0 buffer).
//
// Tape row of step m (written by fc_ctrl_step):  [ xi_{m-1} (nx) | y_{m-1} (n_sens) | v_m (n_act) ]
// Adjoint row m = 0 .. n (FcLoopRow):            [ lambda_m (nx) | eta_m (nyc) | ucb_m (nuc) | vb_m (n_act) | yc_m (nyc) | uc_m (nuc) | ub_m (n_act) ]
// (row 0 holds lambda_0 = dJ/dxi_0 only; the lambda segment of row n is zeroed by the host before the march).
//
// The forward bank stores every matrix transposed so that fc_ctrl_step's lanes read consecutive addresses.  The transposed products
// here want the other orientation: they read a second, UNTRANSPOSED (row-major) copy of the bank with the same block offsets, so a lane
// that owns output column c of M^T reads M[r][c] for r = 0, 1, ..: consecutive lanes, consecutive addresses, never a stride of nx.
#pragma once
#include <hip/hip_runtime.h>

#include "fc_ctrl.hip.h"

struct FcLoopRow {
  int eta, ucb, vb, yc, uc, ub, stride;  // offsets in doubles (lambda at 0)
};
__host__ __device__ inline FcLoopRow fc_loop_row(int nx, int nyc, int nuc, int na) {
  FcLoopRow L;
  L.eta = nx, L.ucb = L.eta + nyc, L.vb = L.ucb + nuc, L.yc = L.vb + na, L.uc = L.yc + nyc, L.ub = L.uc + nuc, L.stride = L.ub + na;
  return L;
}

// where backward step m finds its inputs and leaves its outputs (all DEVICE memory)
struct FcCtrlAdjIO {
  const double* matn;   // the untransposed copy of the bank: [Ad | Bd | C | D | G | g0 | S] row-major, offsets as FcCtrlBank's
  const double* tape;   // tape row of step m
  const double* g;      // [n_act] B~^T mu_m (fc_adj_reduce of this backward step)
  const double* r;      // [n_act] control weights r_m, or null
  const double* w_y;    // [nyc] the signal row step m read, or null
  const double* u_lo;   // [n_act] limits, both or neither
  const double* u_hi;
  double* row;          // adjoint row m (its lambda segment is read, the rest written)
  double* row_prev;     // adjoint row m - 1 (its lambda segment is written)
  double* w_prev;       // [n_sens] sensor weights of backward step m - 1: G^T eta_m is added; null at m = 1
  double* dy0;          // [n_sens] m = 1 only: G^T eta_1 is written
};

// One workgroup of ONE wave, like fc_ctrl_step.  A lane owns output entries and forms each sum in index order -- no cross-lane
// reduction, no atomics -- so two marches on the same inputs are bit-identical.  yc_m and uc_m are formed by the forward kernel's own
// loops (same bank, same order), so they are the forward values bit for bit.  All stores are ordinary vector stores.
//
// The body of one controller's backward step, shared by fc_ctrl_adj_step (k = 1) and fc_ctrl_adj_step_b (one wave per column of a
// batch, csrc/fc_adjoint_loop_batch.hip.h): M = the controller's transposed block of the bank, io = ITS pointers.  io.g may point
// into LDS (the batched kernel reduces the tail's partials itself).
__device__ __forceinline__ void fc_ctrl_adj_step_body(const FcCtrlBank& bk, const double* __restrict__ M, const FcCtrlAdjIO& io) {
  const int lane = threadIdx.x;
  __shared__ double xs[FC_CTRL_NX_MAX];
  __shared__ double ls[FC_CTRL_NX_MAX];
  __shared__ double ys[FC_CTRL_NSENS_MAX];
  __shared__ double ycs[FC_CTRL_NYC_MAX];
  __shared__ double etas[FC_CTRL_NYC_MAX];
  __shared__ double ucbs[FC_CTRL_NUC_MAX];
  __shared__ double vbs[FC_CTRL_NUC_MAX];  // (n_act <= 32 = FC_CTRL_NUC_MAX: fc_set_controllers)
  const int nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc, ns = bk.n_sens, na = bk.n_act;
  const FcLoopRow L = fc_loop_row(nx, nyc, nuc, na);
  const double* __restrict__ Mn = io.matn;  // row-major blocks (M: the transposed ones)
  for (int c = lane; c < nx; c += 64) {
    xs[c] = io.tape[c];
    ls[c] = io.row[c];
  }
  for (int q = lane; q < ns; q += 64) ys[q] = io.tape[nx + q];
  __syncthreads();
  // yc_m = G y_{m-1} + g0 (+ w_y): the forward kernel's sum
  if (lane < nyc) {
    const double* __restrict__ GT = M + bk.oG;
    double acc = 0.0;
    for (int q = 0; q < ns; ++q) acc += GT[(long long)q * nyc + lane] * ys[q];
    double t = acc + M[bk.og0 + lane];
    if (io.w_y) t += io.w_y[lane];
    ycs[lane] = t;
    io.row[L.yc + lane] = t;
  }
  __syncthreads();
  // uc_m = C xi_{m-1} + D yc_m: the forward kernel's sum
  if (lane < nuc) {
    const double* __restrict__ CT = M + bk.oC;
    const double* __restrict__ DT = M + bk.oD;
    double a1 = 0.0, a2 = 0.0;
    for (int c = 0; c < nx; ++c) a1 += CT[(long long)c * nuc + lane] * xs[c];
    for (int j = 0; j < nyc; ++j) a2 += DT[(long long)j * nuc + lane] * ycs[j];
    io.row[L.uc + lane] = a1 + a2;
  }
  // ub_m = B~^T mu_m + r_m,  vb_m = sigma_m o ub_m
  if (lane < na) {
    double ub = io.g[lane];
    if (io.r) ub += io.r[lane];
    double vb = ub;
    if (io.u_lo) {
      const double v = io.tape[nx + ns + lane];
      vb = (io.u_lo[lane] < v && v < io.u_hi[lane]) ? ub : 0.0;
    }
    vbs[lane] = vb;
    io.row[L.ub + lane] = ub;
    io.row[L.vb + lane] = vb;
  }
  __syncthreads();
  // ucb_m = S^T vb_m
  if (lane < nuc) {
    const double* __restrict__ Sn = Mn + bk.oS;  // [n_act][nuc]
    double acc = 0.0;
    for (int a = 0; a < na; ++a) acc += Sn[(long long)a * nuc + lane] * vbs[a];
    ucbs[lane] = acc;
    io.row[L.ucb + lane] = acc;
  }
  __syncthreads();
  // eta_m = D^T ucb_m + Bd^T lambda_m
  if (lane < nyc) {
    const double* __restrict__ Dn = Mn + bk.oD;    // [nuc][nyc]
    const double* __restrict__ Bdn = Mn + bk.oBd;  // [nx][nyc]
    double a1 = 0.0, a2 = 0.0;
    for (int c = 0; c < nuc; ++c) a1 += Dn[(long long)c * nyc + lane] * ucbs[c];
    for (int r = 0; r < nx; ++r) a2 += Bdn[(long long)r * nyc + lane] * ls[r];
    etas[lane] = a1 + a2;
    io.row[L.eta + lane] = a1 + a2;
  }
  // lambda_{m-1} = Ad^T lambda_m + C^T ucb_m: columns lane, lane + 64, ... (<= 4 per lane), into the row of step m - 1
  {
    const double* __restrict__ Cn = Mn + bk.oC;  // [nuc][nx]
#pragma unroll
    for (int i = 0; i < FC_CTRL_NX_MAX / 64; ++i) {
      const int c = lane + 64 * i;
      if (c < nx) {
        double a1 = 0.0, a2 = 0.0;
        for (int r = 0; r < nx; ++r) a1 += Mn[(long long)r * nx + c] * ls[r];
        for (int q = 0; q < nuc; ++q) a2 += Cn[(long long)q * nx + c] * ucbs[q];
        io.row_prev[c] = a1 + a2;
      }
    }
  }
  __syncthreads();
  // G^T eta_m into what backward step m - 1 weights its sensors with (m = 1: dJ/dy_0)
  for (int q = lane; q < ns; q += 64) {
    const double* __restrict__ Gn = Mn + bk.oG;  // [nyc][n_sens]
    double acc = 0.0;
    for (int j = 0; j < nyc; ++j) acc += Gn[(long long)j * ns + q] * etas[j];
    if (io.w_prev)
      io.w_prev[q] += acc;
    else if (io.dy0)
      io.dy0[q] = acc;
  }
}

__global__ __launch_bounds__(64) void fc_ctrl_adj_step(FcCtrlBank bk, FcCtrlAdjIO io) {
  fc_ctrl_adj_step_body(bk, bk.mat, io);  // (k = 1: simulation 0's block)
}

// The seven parameter gradients behind the whole march, laid out like the untransposed bank: [dAd | dBd | dC | dD | dG | dg0 | dS],
// each row-major.  Every entry is sum_{m=1..n} a_m[i] b_m[j] over the adjoint and tape rows,
//     dAd = lambda_m xi_{m-1}^T   dBd = lambda_m yc_m^T   dC = ucb_m xi_{m-1}^T   dD = ucb_m yc_m^T   dG = eta_m y_{m-1}^T   dg0 = eta_m
//     dS  = vb_m uc_m^T
// summed in ascending m by the one thread that owns the entry: the result does not depend on the launch geometry.  Neighbouring threads
// own neighbouring j: they read the same a_m[i] and consecutive b_m[j].
//
// Entry e of one controller's gradient block, shared by fc_ctrl_adj_grads and fc_ctrl_adj_grads_b.  tape / rows1: ITS tape row and adjoint row of step 1; st / sr: doubles between the rows of
// consecutive steps (k = 1: the row lengths; a batch: k row lengths).
__device__ __forceinline__ double fc_ctrl_adj_grad_entry(const FcCtrlBank& bk, const FcLoopRow& L, long long e, int n, const double* __restrict__ tape,
                                                         const double* __restrict__ rows1, long long st, long long sr) {
  const int nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc, ns = bk.n_sens;
  const double *pa, *pb = nullptr;  // a_m = pa[(m - 1) sr], b_m = pb[(m - 1) sb] (pb null: b = 1)
  long long sb = sr;
  if (e < bk.oBd) {
    pa = rows1 + e / nx, pb = tape + e % nx, sb = st;
  } else if (e < bk.oC) {
    const long long q = e - bk.oBd;
    pa = rows1 + q / nyc, pb = rows1 + L.yc + q % nyc;
  } else if (e < bk.oD) {
    const long long q = e - bk.oC;
    pa = rows1 + L.ucb + q / nx, pb = tape + q % nx, sb = st;
  } else if (e < bk.oG) {
    const long long q = e - bk.oD;
    pa = rows1 + L.ucb + q / nyc, pb = rows1 + L.yc + q % nyc;
  } else if (e < bk.og0) {
    const long long q = e - bk.oG;
    pa = rows1 + L.eta + q / ns, pb = tape + nx + q % ns, sb = st;
  } else if (e < bk.oS) {
    pa = rows1 + L.eta + (e - bk.og0);
  } else {
    const long long q = e - bk.oS;
    pa = rows1 + L.vb + q / nuc, pb = rows1 + L.uc + q % nuc;
  }
  double acc = 0.0;
  if (pb)
    for (int m = 0; m < n; ++m) acc += pa[(long long)m * sr] * pb[(long long)m * sb];
  else
    for (int m = 0; m < n; ++m) acc += pa[(long long)m * sr];
  return acc;
}

__global__ __launch_bounds__(256) void fc_ctrl_adj_grads(FcCtrlBank bk, int n, const double* __restrict__ tape, const double* __restrict__ rows,
                                                         double* __restrict__ out) {
  const FcLoopRow L = fc_loop_row(bk.nx, bk.nyc, bk.nuc, bk.n_act);
  const long long LR = L.stride, TR = (long long)bk.nx + bk.n_sens + bk.n_act;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < bk.stride; e += (long long)gridDim.x * blockDim.x)
    out[e] = fc_ctrl_adj_grad_entry(bk, L, e, n, tape, rows + LR, TR, LR);
}
