// fc_ctrl.hip.h — the controller of a closed loop on the device (fc_set_controllers / fc_ctrl_apply / fc_run_closed_loop*).
//
// A bank holds, for each of k simulations, a discrete-time LTI controller and the two fixed linear maps around it:
//     yc  = G y_meas + g0 + w_y    G [nyc][n_sens]       (reference loop: yc = -y_meas[0]); w_y [nyc]: reference or noise, this step's row
//     uc  = C x + D yc             C [nuc][nx], D [nuc][nyc]         -- with the state BEFORE the update (controller.py:65-72)
//     x  <- Ad x + Bd yc           Ad [nx][nx], Bd [nx][nyc]         -- the state sees the disturbed yc
//     v   = S uc + w_u             S [n_act][nuc]        ("a scalar goes to every actuator": a column of ones); w_u [n_act]: excitation
//     u   = min(max(v, u_lo), u_hi)                      plain clamp (signal.saturate), no anti-windup: x is not corrected; +-inf = no limit
// w_y, w_u (fc_set_loop_signals) and u_lo, u_hi (fc_set_control_limits) are optional: a null pointer skips its term, and with all of them
// null the launch forms exactly the sums it formed before they existed.
// Every matrix is stored TRANSPOSED ([column][row]) per simulation, so that the lanes of a wave, which own consecutive output rows,
// read consecutive addresses.  Layout of one simulation's block of FcCtrlBank::mat (offsets in doubles):
//     [AdT nx*nx | BdT nyc*nx | CT nx*nuc | DT nyc*nuc | GT n_sens*nyc | g0 nyc | ST nuc*n_act]
// Bytes read per launch and simulation: 8 (nx^2 + nx (nyc + nuc + 1) + nyc (nuc + n_sens + 1) + nuc n_act + n_sens) -- 1.8 KB for the
// 13-state cylinder controller, 512 KB at nx = 256; with signals and limits set 8 (nyc + 3 n_act) more (40 B for the cylinder's one
// controller input and two actuators); written: 8 (nx + 2 n_act) + the sequence rows, and with a closed-loop tape begun
// (fc_adjoint_loop_begin, fc_adjoint_loop_begin_batch) one tape row of 8 (nx + n_sens + n_act) bytes per simulation.
#pragma once
#include <hip/hip_runtime.h>

constexpr int FC_CTRL_NX_MAX = 256, FC_CTRL_NYC_MAX = 8, FC_CTRL_NUC_MAX = 32, FC_CTRL_NSENS_MAX = 64;

struct FcCtrlBank {
  int nx, nyc, nuc, n_sens, n_act;
  long long stride;  // doubles per simulation in mat
  long long oBd, oC, oD, oG, og0, oS;
  const double* mat;
  double* x;    // [k][nx]
  int* dead;    // [k] the simulation's velocity became non-finite in an earlier step of a batched run: u = 0, state frozen
};

// where a launch finds its inputs and leaves its outputs (all DEVICE memory; any pointer but y / u may be null)
struct FcCtrlIO {
  const double* y;        // measurements of the previous step: y[s * y_stride + q]
  long long y_stride;
  const int* flag_i;      // single run: the handle's sticky non-finite word
  const double* flag_d;   // batched run: flag_d[s * rec_stride] != 0 -- the previous step's record says "non-finite"
  const double* rec_E;    // batched run: (E, r^2, b^2) of the previous step at rec_E[s * rec_stride + 0 / 1 / 2]
  long long rec_stride;
  double* u;              // u[s * u_stride + a]: what the following step's kernels read
  double* uf;             // the body-force amplitudes (= u for the BDF slots), same stride
  long long u_stride;
  double* u_seq;          // [k][n_act] row of this step in the sequence of controls
  // harvest of the PREVIOUS step's outputs into its sequence rows (batched run: the step publishes into one record per simulation)
  double* y_seq;          // [k][n_sens]
  double* E_seq;          // [k][3]: E, r^2, b^2
  double* f_seq;          // [k]: non-finite flag
  int advance;            // 0: harvest only (behind the last step of a run)
  // this step's rows of the loop signals and the actuator limits (each may be null: that term is skipped)
  const double* w_y;      // [k][nyc]   added to yc
  const double* w_u;      // [k][n_act] added to S uc
  const double* u_lo;     // [k][n_act] u = min(max(v, u_lo), u_hi)
  const double* u_hi;
  // this step's row of the closed-loop tape (fc_adjoint_loop_reserve / fc_adjoint_loop_reserve_batch): [x before the update (nx) |
  // y read (n_sens) | v = S uc + w_u, unclamped (n_act)].  Null: nothing is stored and the launch forms exactly what it formed before
  // the tape existed.  Simulation s writes at tape + s * tape_stride (single run: 0; batched run: the row length); a dead simulation
  // writes nothing.
  double* tape;
  long long tape_stride;
};

// One workgroup of ONE wave per simulation.  A lane owns the output rows r, r + 64, ... of every product and forms each row's sum in
// COLUMN INDEX ORDER -- no cross-lane reduction -- so the result depends neither on the launch geometry nor on the call: two launches on
// the same input are bit-identical.  x, yc and uc sit in LDS (every lane reads all of them); the new state is held in registers until
// all lanes have finished reading the old one.  The signals are added LAST, behind the completed sum of their stage, and the clamp is two
// compares on the lane's own value (a NaN passes through, as through numpy's minimum / maximum).  All stores are ordinary vector stores.
__global__ __launch_bounds__(64) void fc_ctrl_step(FcCtrlBank bk, FcCtrlIO io) {
  const int s = blockIdx.x, lane = threadIdx.x;
  __shared__ double xs[FC_CTRL_NX_MAX];
  __shared__ double ys[FC_CTRL_NSENS_MAX];
  __shared__ double ycs[FC_CTRL_NYC_MAX];
  __shared__ double ucs[FC_CTRL_NUC_MAX];
  const int nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc, ns = bk.n_sens, na = bk.n_act;
  int dead = bk.dead[s];
  if (io.flag_i && io.flag_i[0] != 0) dead = 1;
  if (io.flag_d && io.flag_d[(long long)s * io.rec_stride] != 0.0) dead = 1;
  // the previous step's outputs -> its rows of the sequences
  if (io.y_seq)
    for (int q = lane; q < ns; q += 64) io.y_seq[(long long)s * ns + q] = io.y[(long long)s * io.y_stride + q];
  if (io.E_seq && lane < 3) io.E_seq[(long long)s * 3 + lane] = io.rec_E[(long long)s * io.rec_stride + lane];
  if (io.f_seq && lane == 0) io.f_seq[s] = io.flag_d ? io.flag_d[(long long)s * io.rec_stride] : 0.0;
  if (dead && io.flag_d && lane == 0) bk.dead[s] = 1;  // (every lane has read the word above and computed the same verdict)
  if (!io.advance) return;
  if (dead) {  // (uniform per workgroup)
    for (int a = lane; a < na; a += 64) {
      io.u[(long long)s * io.u_stride + a] = 0.0;
      if (io.uf) io.uf[(long long)s * io.u_stride + a] = 0.0;
      if (io.u_seq) io.u_seq[(long long)s * na + a] = 0.0;
    }
    return;
  }
  const double* __restrict__ M = bk.mat + (long long)s * bk.stride;
  double* __restrict__ x = bk.x + (long long)s * nx;
  for (int c = lane; c < nx; c += 64) xs[c] = x[c];
  for (int q = lane; q < ns; q += 64) ys[q] = io.y[(long long)s * io.y_stride + q];
  __syncthreads();
  double* __restrict__ tp = io.tape ? io.tape + (long long)s * io.tape_stride : nullptr;  // (one row per simulation and launch)
  if (tp) {
    for (int c = lane; c < nx; c += 64) tp[c] = xs[c];
    for (int q = lane; q < ns; q += 64) tp[nx + q] = ys[q];
  }
  // yc = G y + g0
  if (lane < nyc) {
    const double* __restrict__ GT = M + bk.oG;
    double acc = 0.0;
    for (int q = 0; q < ns; ++q) acc += GT[(long long)q * nyc + lane] * ys[q];
    double t = acc + M[bk.og0 + lane];
    if (io.w_y) t += io.w_y[(long long)s * nyc + lane];
    ycs[lane] = t;
  }
  __syncthreads();
  // uc = C x + D yc (old state)
  if (lane < nuc) {
    const double* __restrict__ CT = M + bk.oC;
    const double* __restrict__ DT = M + bk.oD;
    double a1 = 0.0, a2 = 0.0;
    for (int c = 0; c < nx; ++c) a1 += CT[(long long)c * nuc + lane] * xs[c];
    for (int j = 0; j < nyc; ++j) a2 += DT[(long long)j * nuc + lane] * ycs[j];
    ucs[lane] = a1 + a2;
  }
  // x <- Ad x + Bd yc: rows lane, lane + 64, ... (<= 4 per lane), kept in registers until every lane is through with xs
  double xn[FC_CTRL_NX_MAX / 64];
  {
    const double* __restrict__ BdT = M + bk.oBd;
#pragma unroll
    for (int i = 0; i < FC_CTRL_NX_MAX / 64; ++i) {
      const int r = lane + 64 * i;
      double a1 = 0.0, a2 = 0.0;
      if (r < nx) {
        for (int c = 0; c < nx; ++c) a1 += M[(long long)c * nx + r] * xs[c];
        for (int j = 0; j < nyc; ++j) a2 += BdT[(long long)j * nx + r] * ycs[j];
      }
      xn[i] = a1 + a2;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FC_CTRL_NX_MAX / 64; ++i) {
    const int r = lane + 64 * i;
    if (r < nx) x[r] = xn[i];
  }
  // u = clamp(S uc + w_u)
  for (int a = lane; a < na; a += 64) {
    const double* __restrict__ ST = M + bk.oS;
    double acc = 0.0;
    for (int c = 0; c < nuc; ++c) acc += ST[(long long)c * na + a] * ucs[c];
    if (io.w_u) acc += io.w_u[(long long)s * na + a];
    if (tp) tp[nx + ns + a] = acc;
    if (io.u_lo) {
      const double lo = io.u_lo[(long long)s * na + a], hi = io.u_hi[(long long)s * na + a];
      acc = acc < lo ? lo : acc;
      acc = acc > hi ? hi : acc;
    }
    io.u[(long long)s * io.u_stride + a] = acc;
    if (io.uf) io.uf[(long long)s * io.u_stride + a] = acc;
    if (io.u_seq) io.u_seq[(long long)s * na + a] = acc;
  }
}
