// fc_adjoint_loop_run.hpp -- host side of the adjoint of a closed loop (fc_adjoint_loop_reserve / _begin / _info,
// fc_run_adjoint_closed_loop; kernels in fc_adjoint_loop.hip.h, tape bookkeeping in fc_adjoint_loop_tape.hpp).  Included at
// the end of fc_hip.hip, behind fc_adjoint_run.hpp.  Its own are the loop tape's layout, the controller's buffers and the unpacking of the
// adjoint rows: the march is fc_run_adjoint's on the skeleton of fc_adjoint_march.hpp, with the controller's launches in its callables.
#pragma once

static_assert(fc_rec::kMaxAct <= FC_CTRL_NUC_MAX && fc_rec::kMaxAct <= 64, "fc_ctrl_adj_step keeps one lane and one LDS word per actuator");

extern "C" {

// (re)build what a reserved loop tape keeps on the device for the PRESENT bank: the tape rows and the untransposed copy of the bank.
// Called by fc_adjoint_loop_reserve and, with a reserve, by fc_set_controllers.  The tape is not begun afterwards.
static int loop_tape_layout(fc_ctx* h) {
  fc_ctx::Loop& P = h->lp;
  const fc_ctx::Ctl& C = h->ctl;
  P.lt.end("fc_set_controllers");
  if (P.lt.capacity == 0 || C.k == 0) return FC_OK;
  P.lt.ended_by = "fc_set_controllers (the tape was laid out again for the new bank)";  // (whatever had ended it before)
  const FcCtrlBank& b = C.bank;
  P.row_len = b.nx + b.n_sens + b.n_act;
  DevBuf<double> tape, matn;
  int code = tape.alloc((size_t)P.lt.capacity * (size_t)P.row_len);
  if (code == FC_OK) code = matn.alloc((size_t)b.stride);
  if (code != FC_OK) {
    (void)hipGetLastError();
    return code;
  }
  // the bank as fc_ctrl_step holds it (simulation 0), every block transposed back
  std::vector<double> t((size_t)b.stride), m((size_t)b.stride);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(t.data(), C.mat.p, t.size() * sizeof(double), hipMemcpyDeviceToHost));
  auto put = [&](long long off, int rows, int cols) {  // t holds [cols][rows] at off -> m [rows][cols]
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) m[(size_t)off + (size_t)r * cols + c] = t[(size_t)off + (size_t)c * rows + r];
  };
  put(0, b.nx, b.nx), put(b.oBd, b.nx, b.nyc), put(b.oC, b.nuc, b.nx), put(b.oD, b.nuc, b.nyc), put(b.oG, b.nyc, b.n_sens);
  put(b.og0, 1, b.nyc), put(b.oS, b.n_act, b.nuc);
  HIPCHK(hipMemcpy(matn.p, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice));
  P.tape = std::move(tape);
  P.matn = std::move(matn);
  return FC_OK;
}

static void loop_tape_release(fc_ctx* h) {
  fc_ctx::Loop& P = h->lp;
  P.tape.release(), P.matn.release(), P.rows.release(), P.rseq.release(), P.out.release(), P.dy0.release();
  P.row_len = 0;
}

int fc_adjoint_loop_reserve(fc_handle h, int32_t capacity) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: null handle");
  if (capacity < 0 || capacity > (1 << 24)) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: capacity must be in [0, 2^24]");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: a step is in flight");
  if (capacity > 0) {
    if (h->partitioned || exchanges(h))
      return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: partitioned (multi-GPU) handles keep no loop tape: their closed loops are stepped one by one");
    if (h->bat.k > 0) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: the handle has a batch set (fc_set_batch): batched closed loops are not taped");
    if (h->ctl.k == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_reserve: no controller bank (fc_set_controllers): a tape row is laid out for the bank");
    if (h->ctl.k != 1) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve: the bank holds k = " + std::to_string(h->ctl.k) + " controllers: only a single closed loop (k = 1) is taped");
  }
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  fc_ctx::Loop& P = h->lp;
  P.lt.reserve(capacity);
  if (capacity == 0) {
    loop_tape_release(h);
    return FC_OK;
  }
  const int code = loop_tape_layout(h);
  if (code != FC_OK) {  // (nothing of the old tape is kept: a failed reserve leaves the handle without one)
    P.lt.reserve(0);
    loop_tape_release(h);
  }
  P.lt.ended_by.clear();  // (a new tape: nothing has ended it)
  return code;
}

int fc_adjoint_loop_begin(fc_handle h) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_loop_begin: null handle");
  fc_ctx::Loop& P = h->lp;
  if (P.lt.capacity == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_begin: no loop tape (fc_adjoint_loop_reserve)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_loop_begin: collect the step in flight first (fc_step_end)");
  if (h->bat.k > 0) return fail(FC_ERR_INVALID, "fc_adjoint_loop_begin: the handle has a batch set (fc_set_batch): batched closed loops are not taped");
  if (h->ctl.k != 1 || !P.tape.p) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_begin: no single controller on the device (fc_set_controllers)");
  P.lt.begin(h->step_count);
  return FC_OK;
}

int fc_adjoint_loop_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_adjoint_loop_info: null argument");
  const fc_ctx::Loop& P = h->lp;
  info[0] = P.lt.capacity, info[1] = P.lt.count(), info[2] = P.lt.overflowed() ? 1 : 0;
  info[3] = 8 * (int64_t)(P.tape.n + P.matn.n + P.rows.n + P.rseq.n + P.out.n + P.dy0.n);
  info[4] = P.lt.begun ? 1 : 0, info[5] = P.lt.lost, info[6] = P.lt.bad ? 1 : 0, info[7] = P.row_len;
  return FC_OK;
}

int fc_run_adjoint_closed_loop(fc_handle h, int first_order_slot, int32_t n_steps, const double* w_seq, const double* r_seq,
                               const double* z_terminal, double* gAd, double* gBd, double* gC, double* gD, double* gG, double* gg0, double* gS,
                               double* dxc0, double* dy0, double* dwy, double* dwu, double* ubar_seq, double* dx0, double* dxm1) {
  const char* who = "fc_run_adjoint_closed_loop";
  if (!h) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop: null handle");
  if (n_steps <= 0) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop: n_steps must be positive");
  if (first_order_slot != FC_SLOT_BDF1 && first_order_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, "order_slot must be BDF1/BDF2");
  fc_ctx::Loop& P = h->lp;
  fc_ctx::Ctl& C = h->ctl;
  if (C.k > 1) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop: the bank holds k = " + std::to_string(C.k) + " controllers: the adjoint of a closed loop is built for k = 1");
  if (P.lt.capacity == 0) return fail(FC_ERR_NOT_READY, "fc_run_adjoint_closed_loop: no loop tape (fc_adjoint_loop_reserve, then fc_adjoint_loop_begin before the forward fc_run_closed_loop)");
  FCCHK(ctrl_check(h, 1, who));
  {
    std::string why;
    if (!P.lt.covers(n_steps, first_order_slot, FC_SLOT_BDF2, &why))
      return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop: the loop tape does not hold this run: " + why);
  }
  const bool nl = h->nonlinear;
  const char* remedy = "fc_adjoint_tape_reserve, then fc_adjoint_tape_begin before the forward fc_run_closed_loop";
  const bool taped = nl || h->adjen.n > 0;  // (energy weights: a linearised handle marches over its taped run too)
  fc_ctx::StateTape& T = h->adj.st;
  FCCHK(adj_tape_refusal(h, who, T, n_steps, first_order_slot, "state tape", remedy));
  FCCHK(adjen_march_check(h, who, nl, n_steps, 0, T, first_order_slot));
  FCCHK(adj_step_ready(h, first_order_slot, who, nl));
  if (n_steps > 1 && first_order_slot != FC_SLOT_BDF2) FCCHK(adj_step_ready(h, FC_SLOT_BDF2, who, nl));
  FCCHK(adj_march_prepare(h, first_order_slot, n_steps, 0));
  fc_ctx::Adj& A = h->adj;
  const FcCtrlBank& bk = C.bank;
  const int na = h->n_act, ns = h->n_sens, nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc;
  const FcLoopRow L = fc_loop_row(nx, nyc, nuc, na);
  const size_t n = (size_t)n_steps, LR = (size_t)L.stride;
  if (P.rows.n < (n + 1) * LR) FCCHK(P.rows.alloc((n + 1) * LR));
  if (r_seq && P.rseq.n < n * na) FCCHK(P.rseq.alloc(n * na));
  if (P.out.n < (size_t)bk.stride) FCCHK(P.out.alloc((size_t)bk.stride));
  if (P.dy0.n < (size_t)ns) FCCHK(P.dy0.alloc((size_t)ns));
  int flag = 0, rflags[2] = {0, 0};
  std::vector<double> rows((n + 1) * LR), out((size_t)bk.stride);
  // (the replays of a checkpointed tape read the control tape: no controller runs, the loop tape and the adjoint rows stay where they are)
  bool replays = false;
  FCCHK(stape_march_begin(T, taped, n_steps, adj_tape_layout(h), &replays));
  AdjReplayHost forward_state(h, replays);
  const AdjReplay replay = adj_replay_single(h, n_steps, rflags);
  const int code = adj_enqueue_and_sync(h, who, &A.run_ms, [&]() -> int {  // (run_ms, fc_adjoint_info: with or without the controller)
    // the sensor weights live on the device: backward step m adds G^T eta_m to the row of step m - 1
    if (w_seq)
      HIPCHK(hipMemcpyAsync(A.wseq.p, w_seq, n * ns * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else
      HIPCHK(hipMemsetAsync(A.wseq.p, 0, n * ns * sizeof(double), h->stream));
    if (r_seq) HIPCHK(hipMemcpyAsync(P.rseq.p, r_seq, n * na * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (nx > 0) HIPCHK(hipMemsetAsync(P.rows.p + n * LR, 0, (size_t)nx * sizeof(double), h->stream));  // lambda_n = 0
    FCCHK(adj_reset(h, z_terminal));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    FCCHK(adj_march(
        h, first_order_slot, n_steps, taped ? T.tape.p : nullptr, T.col, dx0, dxm1,
        [&](int m, int slot, const StepCoeffs& c, const double* xm, const double* er) -> int {
          double* g_row = A.gseq.p + (size_t)(m - 1) * na;
          FCCHK(adj_enqueue_step(h, slot, c, xm, A.wseq.p + (size_t)(m - 1) * ns, g_row, er, adjen_source_column(h, m)));
          FcCtrlAdjIO io = ctrl_adj_io(h, P, A.wseq.p, r_seq != nullptr, m, 1, LR);
          io.g = g_row;
          hipLaunchKernelGGL(fc_ctrl_adj_step, dim3(1), dim3(64), 0, h->stream, bk, io);
          return FC_OK;
        },
        [&](const StepCoeffs& c, const double* xm, int which, double* dst) { return adj_enqueue_mass_product(h, c, xm, which, dst); },
        [&]() -> int {
          hipLaunchKernelGGL(fc_ctrl_adj_grads, dim3((unsigned)std::min<long long>(2048, (bk.stride + 255) / 256)), dim3(256), 0, h->stream, bk, (int)n_steps,
                             (const double*)P.tape.p, (const double*)P.rows.p, P.out.p);
          HIPCHK(hipGetLastError());
          return FC_OK;
        },
        taped ? &replay : nullptr));
    HIPCHK(hipMemcpyAsync(rows.data(), P.rows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out.data(), P.out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (dy0) HIPCHK(hipMemcpyAsync(dy0, P.dy0.p, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&flag, A.flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return FC_OK;
  });
  FCCHK(taped ? stape_verdict(T, who, n_steps, 1, code, rflags) : code);
  if (flag) return fail(FC_ERR_DIVERGED, "fc_run_adjoint_closed_loop: non-finite adjoint state after a solve");
  const auto give = [&](double* dst, long long off, size_t count) {
    if (dst && count) std::copy(out.begin() + (std::ptrdiff_t)off, out.begin() + (std::ptrdiff_t)(off + (long long)count), dst);
  };
  give(gAd, 0, (size_t)nx * nx), give(gBd, bk.oBd, (size_t)nx * nyc), give(gC, bk.oC, (size_t)nuc * nx), give(gD, bk.oD, (size_t)nuc * nyc);
  give(gG, bk.oG, (size_t)nyc * ns), give(gg0, bk.og0, (size_t)nyc), give(gS, bk.oS, (size_t)na * nuc);
  if (dxc0) std::copy(rows.begin(), rows.begin() + nx, dxc0);
  for (size_t m = 1; m <= n; ++m) {
    const double* row = rows.data() + m * LR;
    if (dwy) std::copy(row + L.eta, row + L.eta + nyc, dwy + (m - 1) * nyc);
    if (dwu) std::copy(row + L.vb, row + L.vb + na, dwu + (m - 1) * na);
    if (ubar_seq) std::copy(row + L.ub, row + L.ub + na, ubar_seq + (m - 1) * na);
  }
  return FC_OK;
}

}  // extern "C"
