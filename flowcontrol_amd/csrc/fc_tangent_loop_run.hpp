// fc_tangent_loop_run.hpp -- host side of the tangent of a closed loop (fc_run_tangent_closed_loop, fc_run_tangent_closed_loop_batch;
// kernels in fc_tangent_loop.hip.h; DESIGN §5.6 "Closed loop").  Included at the end of fc_hip.hip, behind fc_tangent_run.hpp: the
// plant's tangent step and the staging of the state levels are that file's; the mode, the refusals around the march's own, the preamble,
// the step loop and the one synchronisation are fc_tangent_march.hpp's; its own are the direction and its bank, the controller's launch
// AHEAD of every plant step (tan_march's before_step), the loop tape's conditions, the downloads and the batched verdict.
//
// Per step m:  fc_ctrl_tan_step (reads dy_{m-1} = row m - 2 of Tan::dy, at m = 1 Tan::dy0; writes row m - 1 of Tan::du and Tan::dxi in
// place), then tan_enqueue_step / tanb_enqueue_step on that control row (its tail writes row m - 1 of Tan::dy).  Read of the forward
// run: the loop tape, the bank, the signal rows and the limits -- and, on a nonlinear scheme, the dense state tape.  A LINEARISED scheme
// is accepted: its coefficients cc_n = cc_nn = 0 switch the element kernels' reads of the taped states off, so the plant steps are
// handed null state-tape pointers and the march needs the loop tape alone.
// Written: Tan's buffers only -- never the state ring, the controller state, the loop cursor, the tapes or the step counter.
#pragma once

namespace {

// the parts of a direction that live on the device for the length of a march of n steps and kk columns; any may be null (zero)
struct TanLoopDirection {
  const double *dAd, *dBd, *dC, *dD, *dG, *dg0, *dS, *dxi0, *dy0, *dw_y, *dw_u;
  bool matrices() const { return dAd || dBd || dC || dD || dG || dg0 || dS; }
};

// the closed-loop buffers of Tan for a march of n steps and kk columns along `d`, sized next to tan_sequences, ahead of the enqueue
int tan_loop_sequences(fc_ctx* h, const TanLoopDirection& d, int n_steps, int kk) {
  fc_ctx::Tan& T = h->tan;
  const FcCtrlBank& bk = h->ctl.bank;
  const size_t n = (size_t)n_steps, k = (size_t)kk, nx = (size_t)bk.nx, ns = (size_t)bk.n_sens, nyc = (size_t)bk.nyc, na = (size_t)bk.n_act;
  if (d.matrices() && T.dbank.n < k * (size_t)bk.stride) FCCHK(T.dbank.alloc(k * (size_t)bk.stride));
  if (T.dxi.n < k * std::max<size_t>(1, nx)) FCCHK(T.dxi.alloc(k * std::max<size_t>(1, nx)));
  if (T.dy0.n < k * ns) FCCHK(T.dy0.alloc(k * ns));
  if (d.dw_y && T.dwy.n < n * k * nyc) FCCHK(T.dwy.alloc(n * k * nyc));
  if (d.dw_u && T.dwu.n < n * k * na) FCCHK(T.dwu.alloc(n * k * na));
  return FC_OK;
}

// enqueue the direction's way onto the device.  `bank` receives the packed direction bank (it must outlive the synchronisation).
// Tan::dwy / dwu keep the caller's [n][kk][.] layout.
int tan_loop_direction_in(fc_ctx* h, const TanLoopDirection& d, int n_steps, int kk, std::vector<double>& bank) {
  fc_ctx::Tan& T = h->tan;
  const FcCtrlBank& bk = h->ctl.bank;
  const size_t n = (size_t)n_steps, k = (size_t)kk, nx = (size_t)bk.nx, ns = (size_t)bk.n_sens, nyc = (size_t)bk.nyc, na = (size_t)bk.n_act;
  const auto put = [&](double* dst, const double* src, size_t count) -> int {
    if (!count) return FC_OK;
    if (src)
      HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else
      HIPCHK(hipMemsetAsync(dst, 0, count * sizeof(double), h->stream));
    return FC_OK;
  };
  if (d.matrices()) {
    ctrl_pack_bank(bk, kk, d.dAd, d.dBd, d.dC, d.dD, d.dG, d.dg0, d.dS, bank);  // (fc_set_controllers' packing: the forward bank's layout)
    FCCHK(put(T.dbank.p, bank.data(), bank.size()));
  }
  FCCHK(put(T.dxi.p, d.dxi0, k * nx));
  FCCHK(put(T.dy0.p, d.dy0, k * ns));
  if (d.dw_y) FCCHK(put(T.dwy.p, d.dw_y, n * k * nyc));
  if (d.dw_u) FCCHK(put(T.dwu.p, d.dw_u, n * k * na));
  return FC_OK;
}

// What the controller's tangent kernel reads and writes at step m of the march's lock-step loops, column 0's pointers.
// P: fc_ctx::Loop or fc_ctx::LoopB.  It reads the readings' row of step m - 1 and writes the controls' row of step m.
template <class LoopTape>
FcCtrlTanIO ctrl_tan_io(const fc_ctx* h, const LoopTape& P, const TanLoopDirection& d, int m, const TanMode& M) {
  const fc_ctx::Ctl& C = h->ctl;
  const fc_ctx::Tan& T = h->tan;
  const size_t kk = (size_t)std::max(1, M.k), na = (size_t)h->n_act, nyc = (size_t)C.bank.nyc;
  FcCtrlTanIO io = {};
  io.dmat = d.matrices() ? T.dbank.p : nullptr;
  io.tape = P.tape.p + (size_t)(m - 1) * kk * (size_t)P.row_len;
  if (C.wy.p && P.lt.row0 >= 0) io.w_y = C.wy.p + (size_t)(P.lt.row0 + m - 1) * kk * nyc;  // (the adjoint's row: ctrl_adj_io)
  if (C.ulo.p) io.u_lo = C.ulo.p, io.u_hi = C.uhi.p;
  io.dy = m > 1 ? M.dy_row(h, m - 1) : T.dy0.p;
  if (d.dw_y) io.dw_y = T.dwy.p + (size_t)(m - 1) * kk * nyc;
  if (d.dw_u) io.dw_u = T.dwu.p + (size_t)(m - 1) * kk * na;
  io.dxi = T.dxi.p;
  io.du = M.du_row(h, m);
  return io;
}

// what both closed-loop marches refuse between the front of their mode and the slots (fc_tangent_march.hpp): of the controllers, of the
// loop tape `P` and, on a nonlinear scheme, of the state tape of the mode
template <class LoopTape>
int tan_loop_refusal(fc_ctx* h, const char* who, int first_slot, int n_steps, const LoopTape& P, const TanMode& M) {
  const std::string w = std::string(who) + ": ";
  FCCHK(tan_refusal_call(h, w, first_slot, n_steps));
  FCCHK(ctrl_check(h, std::max(1, M.k), who));
  if (P.lt.capacity == 0) return fail(FC_ERR_NOT_READY, w + "no loop tape (fc_adjoint_loop_reserve / _reserve_batch, then _begin before the forward closed-loop run)");
  std::string why;
  if (!P.lt.covers(n_steps, first_slot, FC_SLOT_BDF2, &why)) return fail(FC_ERR_INVALID, w + "the loop tape does not hold this run: " + why);
  if (!P.tape.p || P.row_len != h->ctl.bank.nx + h->n_sens + h->n_act) return fail(FC_ERR_INVALID, w + "the loop tape was laid out for another bank");
  // (with the energy option also a linearised march reads the taped states: x_m of d(dE_m) -- never launched on a null column)
  if (h->nonlinear || h->tan.energy) FCCHK(tan_refusal_tape(w, first_slot, n_steps, M));
  return tan_refusal_scheme(h, w, first_slot, n_steps);
}

}  // namespace

extern "C" {

int fc_run_tangent_closed_loop(fc_handle h, int first_order_slot, int32_t n_steps, const double* dAd, const double* dBd, const double* dC, const double* dD,
                               const double* dG, const double* dg0, const double* dS, const double* dxi0, const double* dy0, const double* dw_y,
                               const double* dw_u, const double* dx0, const double* dxm1, double* dy_seq, double* du_seq, double* dxi_n, double* dxn,
                               double* dxnm1) {
  const char* who = "fc_run_tangent_closed_loop";
  TanMode M;
  FCCHK(tan_front_single(h, who, "fc_adjoint_tape_reserve, then fc_adjoint_tape_begin before the forward fc_run_closed_loop", &M));
  fc_ctx::Tan& T = h->tan;
  fc_ctx::Loop& P = h->lp;
  FCCHK(tan_loop_refusal(h, who, first_order_slot, n_steps, P, M));
  FCCHK(tan_slots_ready(h, who, M, first_order_slot, n_steps));
  FCCHK(tan_march_prepare(h, M, first_order_slot, n_steps));
  const FcCtrlBank& bk = h->ctl.bank;
  const size_t n = (size_t)n_steps, na = (size_t)h->n_act, ns = (size_t)h->n_sens, nx = (size_t)bk.nx;
  const TanLoopDirection d = {dAd, dBd, dC, dD, dG, dg0, dS, dxi0, dy0, dw_y, dw_u};
  FCCHK(tan_loop_sequences(h, d, n_steps, 1));
  std::vector<double> bank;
  int flag = 0;
  FCCHK(tan_enqueue_and_sync(h, who, n_steps, [&]() -> int {
    FCCHK(tan_loop_direction_in(h, d, n_steps, 1, bank));
    FCCHK(tan_march(h, M, first_order_slot, n_steps, dx0, dxm1, [&](int j) {
      const FcCtrlTanIO io = ctrl_tan_io(h, P, d, j, M);
      hipLaunchKernelGGL(fc_ctrl_tan_step, dim3(1), dim3(64), 0, h->stream, bk, io);
    }));
    if (dy_seq) HIPCHK(hipMemcpyAsync(dy_seq, T.dy.p, n * ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (du_seq) HIPCHK(hipMemcpyAsync(du_seq, T.du.p, n * na * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (dxi_n && nx > 0) HIPCHK(hipMemcpyAsync(dxi_n, T.dxi.p, nx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return tan_march_out(h, M, dxn, dxnm1, &flag);
  }));
  return flag ? fail(FC_ERR_DIVERGED, std::string(who) + ": non-finite tangent state after a solve") : FC_OK;
}

int fc_run_tangent_closed_loop_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, int32_t ref_col, const double* dAd, const double* dBd,
                                     const double* dC, const double* dD, const double* dG, const double* dg0, const double* dS, const double* dxi0,
                                     const double* dy0, const double* dw_y, const double* dw_u, const double* dx0, const double* dxm1, double* dy_seq,
                                     double* du_seq, double* dxi_n, double* dxn, double* dxnm1, int32_t* flags_out) {
  const char* who = "fc_run_tangent_closed_loop_batch";
  TanMode M;
  FCCHK(tan_front_batch(h, who, k, ref_col, "fc_adjoint_tape_reserve_batch, then fc_adjoint_tape_begin_batch before the forward fc_run_closed_loop_batch", &M));
  fc_ctx::Tan& T = h->tan;
  fc_ctx::LoopB& P = h->lpb;
  FCCHK(tan_loop_refusal(h, who, first_order_slot, n_steps, P, M));
  if (P.k != k) return fail(FC_ERR_INVALID, std::string(who) + ": the loop tape was laid out for another bank");
  FCCHK(tan_slots_ready(h, who, M, first_order_slot, n_steps));
  FCCHK(tan_march_prepare(h, M, first_order_slot, n_steps));
  const FcCtrlBank& bk = h->ctl.bank;
  const int N = h->N, na = h->n_act, ns = h->n_sens, nx = bk.nx, KB = M.W;
  const size_t kk = (size_t)k, n = (size_t)n_steps;
  const TanLoopDirection d = {dAd, dBd, dC, dD, dG, dg0, dS, dxi0, dy0, dw_y, dw_u};
  FCCHK(tan_loop_sequences(h, d, n_steps, k));
  std::vector<double> bank, du_host(n * KB * na), dy_host(n * kk * ns), dxi_host(kk * (size_t)std::max(1, nx));
  int flags[32] = {0};
  FCCHK(tan_enqueue_and_sync(h, who, n_steps, [&]() -> int {
    FCCHK(tan_loop_direction_in(h, d, n_steps, k, bank));
    HIPCHK(hipMemsetAsync(T.du.p, 0, n * KB * na * sizeof(double), h->stream));  // (the padding columns' rows: the gather reads all KB)
    FCCHK(tan_march(h, M, first_order_slot, n_steps, dx0, dxm1, [&](int j) {
      const FcCtrlTanIO io = ctrl_tan_io(h, P, d, j, M);
      pick_bool(ref_col >= 0, [&](auto REF) { hipLaunchKernelGGL((fc_ctrl_tan_step_b<REF>), dim3(k), dim3(64), 0, h->stream, bk, io, (int)ref_col); });
    }));
    HIPCHK(hipMemcpyAsync(dy_host.data(), T.dy.p, dy_host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(du_host.data(), T.du.p, du_host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (nx > 0) HIPCHK(hipMemcpyAsync(dxi_host.data(), T.dxi.p, kk * nx * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return tan_march_out(h, M, dxn, dxnm1, flags);
  }));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int any = 0;
  for (size_t s = 0; s < kk; ++s) {
    // a column is lost if the forward run it linearises about went non-finite, its tangent state did (the tail's flag), or its
    // controller's tangent did (fc_run_adjoint_closed_loop_batch's rule)
    const size_t base = ref_col >= 0 ? (size_t)ref_col : s;
    bool bad = flags[s] != 0 || ((P.bad >> base) & 1u) != 0;
    for (size_t m = 0; m < n && !bad; ++m) {
      for (int q = 0; q < ns && !bad; ++q) bad = !std::isfinite(dy_host[(m * kk + s) * ns + q]);
      for (int a = 0; a < na && !bad; ++a) bad = !std::isfinite(du_host[(m * KB + s) * na + a]);
    }
    for (int c = 0; c < nx && !bad; ++c) bad = !std::isfinite(dxi_host[s * nx + c]);
    if (flags_out) flags_out[s] = bad ? 1 : 0;
    any |= bad ? 1 : 0;
    for (size_t m = 0; m < n; ++m) {
      if (dy_seq)
        for (int q = 0; q < ns; ++q) dy_seq[(m * kk + s) * ns + q] = bad ? nan : dy_host[(m * kk + s) * ns + q];
      if (du_seq)
        for (int a = 0; a < na; ++a) du_seq[(m * kk + s) * na + a] = bad ? nan : du_host[(m * KB + s) * na + a];
    }
    if (dxi_n)
      for (int c = 0; c < nx; ++c) dxi_n[s * nx + c] = bad ? nan : dxi_host[s * nx + c];
    if (bad) {
      if (dxn) std::fill(dxn + s * N, dxn + (s + 1) * N, nan);
      if (dxnm1) std::fill(dxnm1 + s * N, dxnm1 + (s + 1) * N, nan);
    }
  }
  if (any)
    return fail(FC_ERR_DIVERGED, std::string(who) + ": a column's forward run or tangent state is non-finite (flags_out marks the columns; the others are valid)");
  return FC_OK;
}

}  // extern "C"
