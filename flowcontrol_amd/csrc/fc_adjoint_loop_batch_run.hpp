// fc_adjoint_loop_batch_run.hpp -- host side of the adjoint of k lock-step closed loops (fc_adjoint_loop_reserve_batch / _begin_batch /
// _info_batch, fc_run_adjoint_closed_loop_batch; kernels in fc_adjoint_loop_batch.hip.h, tape bookkeeping in fc_adjoint_loop_tape.hpp;
// DESIGN §5.4 "Batched closed loops").  Included at the end of fc_hip.hip, behind fc_adjoint_batch_run.hpp and fc_adjoint_loop_run.hpp:
// its own are the batched loop tape's layout and the per-column unpacking (a bad column is NaN-filled); the march is
// fc_run_adjoint_batch's on the skeleton of fc_adjoint_march.hpp, with the controllers' launches in its callables.  The state is
// fc_ctx::LoopB, beside fc_ctx::Loop: the single run's entry points keep every refusal they have.
#pragma once

extern "C" {

// (re)build what a reserved batched loop tape keeps on the device for the PRESENT bank (k = the batch's): the tape rows and the
// untransposed copy of all k blocks.  Called by fc_adjoint_loop_reserve_batch and, with a reserve, by fc_set_controllers.  The tape is
// not begun afterwards.
static int loopb_layout(fc_ctx* h) {
  fc_ctx::LoopB& P = h->lpb;
  const fc_ctx::Ctl& C = h->ctl;
  P.lt.end("fc_set_controllers");
  if (P.lt.capacity == 0 || C.k == 0) return FC_OK;
  P.lt.ended_by = "fc_set_controllers (the tape was laid out again for the new bank)";
  const FcCtrlBank& b = C.bank;
  const size_t k = (size_t)C.k, st = (size_t)b.stride;
  const int row_len = b.nx + b.n_sens + b.n_act;
  DevBuf<double> tape, matn;
  int code = tape.alloc((size_t)P.lt.capacity * k * (size_t)row_len);
  if (code == FC_OK) code = matn.alloc(k * st);
  if (code != FC_OK) {
    (void)hipGetLastError();
    return code;
  }
  // the bank as fc_ctrl_step holds it, every block of every simulation transposed back
  std::vector<double> t(k * st), m(k * st);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(t.data(), C.mat.p, t.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t s = 0; s < k; ++s) {
    auto put = [&](long long off, int rows, int cols) {  // t holds [cols][rows] at off -> m [rows][cols]
      const size_t o = s * st + (size_t)off;
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m[o + (size_t)r * cols + c] = t[o + (size_t)c * rows + r];
    };
    put(0, b.nx, b.nx), put(b.oBd, b.nx, b.nyc), put(b.oC, b.nuc, b.nx), put(b.oD, b.nuc, b.nyc), put(b.oG, b.nyc, b.n_sens);
    put(b.og0, 1, b.nyc), put(b.oS, b.n_act, b.nuc);
  }
  HIPCHK(hipMemcpy(matn.p, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice));
  P.tape = std::move(tape);
  P.matn = std::move(matn);
  P.k = C.k, P.row_len = row_len;
  P.bad = 0;
  return FC_OK;
}

int fc_adjoint_loop_reserve_batch(fc_handle h, int32_t capacity) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve_batch: null handle");
  if (capacity < 0 || capacity > (1 << 24)) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve_batch: capacity must be in [0, 2^24]");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve_batch: a step is in flight");
  if (capacity > 0) {
    if (h->partitioned || exchanges(h))
      return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve_batch: partitioned (multi-GPU) handles keep no loop tape: their closed loops are stepped one by one");
    if (h->bat.k == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_reserve_batch: fc_set_batch not called (the single loop's tape: fc_adjoint_loop_reserve)");
    if (h->ctl.k == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_reserve_batch: no controller bank (fc_set_controllers): a tape row is laid out for the bank");
    if (h->ctl.k != h->bat.k)
      return fail(FC_ERR_INVALID, "fc_adjoint_loop_reserve_batch: the bank holds k = " + std::to_string(h->ctl.k) + " controllers, the batch " + std::to_string(h->bat.k) +
                                      " simulations: one controller per simulation is taped");
  }
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  loopb_release(h);
  if (capacity == 0) return FC_OK;
  h->lpb.lt.reserve(capacity);
  const int code = loopb_layout(h);
  if (code != FC_OK) loopb_release(h);  // (a failed reserve leaves the handle without one)
  h->lpb.lt.ended_by.clear();           // (a new tape: nothing has ended it)
  return code;
}

int fc_adjoint_loop_begin_batch(fc_handle h) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_loop_begin_batch: null handle");
  fc_ctx::LoopB& P = h->lpb;
  if (P.lt.capacity == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_begin_batch: no loop tape (fc_adjoint_loop_reserve_batch)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_loop_begin_batch: collect the step in flight first (fc_step_batch_end)");
  if (h->bat.k == 0 || h->ctl.k != h->bat.k || P.k != h->bat.k || !P.tape.p)
    return fail(FC_ERR_NOT_READY, "fc_adjoint_loop_begin_batch: the tape was laid out for another bank or batch (fc_adjoint_loop_reserve_batch after fc_set_controllers)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(P.tape.zero(h->stream));  // a column whose run ends early is read as zeros, never as stale memory
  P.lt.begin(h->bat.step_count);
  P.bad = 0;
  return FC_OK;
}

int fc_adjoint_loop_info_batch(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_adjoint_loop_info_batch: null argument");
  const fc_ctx::LoopB& P = h->lpb;
  info[0] = P.lt.capacity, info[1] = P.lt.count(), info[2] = P.lt.overflowed() ? 1 : 0;
  info[3] = 8 * (int64_t)(P.tape.n + P.matn.n + P.rows.n + P.rseq.n + P.out.n + P.dy0.n);
  info[4] = P.lt.begun ? 1 : 0, info[5] = P.lt.lost, info[6] = (int64_t)P.bad, info[7] = P.row_len;
  return FC_OK;
}

int fc_run_adjoint_closed_loop_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, const double* w_seq, const double* r_seq,
                                     const double* z_terminal, double* gAd, double* gBd, double* gC, double* gD, double* gG, double* gg0, double* gS,
                                     double* dxc0, double* dy0, double* dwy, double* dwu, double* ubar_seq, double* dx0, double* dxm1, int32_t* flags_out) {
  const char* who = "fc_run_adjoint_closed_loop_batch";
  if (!h) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: null handle");
  if (n_steps <= 0) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: n_steps must be positive");
  if (first_order_slot != FC_SLOT_BDF1 && first_order_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, "order_slot must be BDF1/BDF2");
  fc_ctx::LoopB& P = h->lpb;
  fc_ctx::Ctl& C = h->ctl;
  fc_ctx::AdjB& A = h->adjb;
  fc_ctx::Batch& B = h->bat;
  if (B.k > 0 && C.k > 0 && C.k != B.k)
    return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: the bank holds k = " + std::to_string(C.k) + " controllers, the batch " + std::to_string(B.k) +
                                    " simulations (ctl.k != bat.k)");
  if (P.lt.capacity == 0)
    return fail(FC_ERR_NOT_READY, "fc_run_adjoint_closed_loop_batch: no loop tape (fc_adjoint_loop_reserve_batch, then fc_adjoint_loop_begin_batch before the forward "
                                  "fc_run_closed_loop_batch)");
  FCCHK(ctrl_check(h, k, who));
  {
    std::string why;
    if (!P.lt.covers(n_steps, first_order_slot, FC_SLOT_BDF2, &why))
      return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: the loop tape does not hold this run: " + why);
  }
  if (P.k != k || !P.tape.p) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: the loop tape was laid out for another bank");
  const bool nl = h->nonlinear;
  const char* remedy = "fc_adjoint_tape_reserve_batch, then fc_adjoint_tape_begin_batch before the forward fc_run_closed_loop_batch";
  const bool taped = nl || h->adjen.n > 0;  // (energy weights: a linearised handle marches over its taped run too)
  fc_ctx::StateTape& T = A.st;
  FCCHK(adj_tape_refusal(h, who, T, n_steps, first_order_slot, "batched state tape", remedy));
  FCCHK(adjb_step_ready(h, first_order_slot, k, who));
  FCCHK(adjen_march_check(h, who, nl, n_steps, k, T, first_order_slot, B.KB));
  if (n_steps > 1 && first_order_slot != FC_SLOT_BDF2) FCCHK(adjb_step_ready(h, FC_SLOT_BDF2, k, who));
  if (nl && T.KB != B.KB) return fail(FC_ERR_INVALID, "fc_run_adjoint_closed_loop_batch: the batched state tape was laid out for another batch width");
  FCCHK(adj_march_prepare(h, first_order_slot, n_steps, k));
  const FcCtrlBank& bk = C.bank;
  const int N = h->N, KB = B.KB, na = h->n_act, ns = h->n_sens, nx = bk.nx, nyc = bk.nyc, nuc = bk.nuc;
  const FcLoopRow L = fc_loop_row(nx, nyc, nuc, na);
  const size_t n = (size_t)n_steps, kk = (size_t)k, LR = (size_t)L.stride, st = (size_t)bk.stride;
  if (P.rows.n < (n + 1) * kk * LR) FCCHK(P.rows.alloc((n + 1) * kk * LR));
  if (r_seq && P.rseq.n < n * kk * na) FCCHK(P.rseq.alloc(n * kk * na));
  if (P.out.n < kk * st) FCCHK(P.out.alloc(kk * st));
  if (P.dy0.n < kk * ns) FCCHK(P.dy0.alloc(kk * ns));
  // The g reduction stays fc_adj_reduce_b's launch: summed inside the controller launch (FC_ADJ_LOOP_FUSE=1, same bits) the k serial
  // controller waves take n_act sums each into their dependent chain, and the step measured 2.4 us (k = 8) to 2.9 us (k = 32) SLOWER on
  // O1 than with the n_act k parallel waves of the launch it saves.  The switch is kept as a measurement aid.
  const bool fuse = [] {
    const char* e = std::getenv("FC_ADJ_LOOP_FUSE");
    return e && e[0] == '1';
  }();
  const int gx = adjb_tail_grid(N, KB);
  int flags[32] = {0}, rflags[64] = {0};
  std::vector<double> rows((n + 1) * kk * LR), out(kk * st), dy0h(kk * ns);
  // (the replays of a checkpointed tape read the control tape: no controller runs, the loop tape and the adjoint rows stay where they are)
  bool replays = false;
  FCCHK(stape_march_begin(T, taped, n_steps, adjb_tape_layout(h), &replays));
  AdjbReplayHost forward_state(h, replays);
  const AdjReplay replay = adjb_replay(h, n_steps, rflags);
  const int code = adj_enqueue_and_sync(h, who, &A.run_ms, [&]() -> int {  // (run_ms, fc_adjoint_batch_info: with or without the controllers)
    // the sensor weights live on the device: backward step m adds G_s^T eta_{m,s} to column s of the row of step m - 1
    if (w_seq)
      HIPCHK(hipMemcpyAsync(A.wseq.p, w_seq, n * kk * ns * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else
      HIPCHK(hipMemsetAsync(A.wseq.p, 0, n * kk * ns * sizeof(double), h->stream));
    if (r_seq) HIPCHK(hipMemcpyAsync(P.rseq.p, r_seq, n * kk * na * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(P.rows.p + n * kk * LR, 0, kk * LR * sizeof(double), h->stream));  // lambda_n = 0 in every column
    FCCHK(adjb_reset(h, z_terminal));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    FCCHK(adj_march(
        h, first_order_slot, n_steps, taped ? T.tape.p : nullptr, T.col, dx0, dxm1,
        [&](int m, int slot, const StepCoeffs& c, const double* xm, const double* er) -> int {
          double* g_row = A.gseq.p + (size_t)(m - 1) * kk * na;
          FCCHK(adjb_enqueue_step(h, slot, c, xm, A.wseq.p + (size_t)(m - 1) * kk * ns, (m == n_steps && z_terminal) ? A.term.p : nullptr, g_row, !fuse, er));
          hipLaunchKernelGGL(fc_ctrl_adj_step_b, dim3(k), dim3(64), 0, h->stream, bk, ctrl_adj_io(h, P, A.wseq.p, r_seq != nullptr, m, kk, LR), g_row,
                             fuse ? (const double*)A.part.p : (const double*)nullptr, gx, KB);
          return FC_OK;
        },
        [&](const StepCoeffs& c, const double* xm, int which, double* dst) { return adjb_state_gradient(h, c, xm, which, dst); },
        [&]() -> int {
          hipLaunchKernelGGL(fc_ctrl_adj_grads_b, dim3((unsigned)std::min<long long>(2048, ((long long)kk * bk.stride + 255) / 256)), dim3(256), 0, h->stream, bk,
                             (int)k, (int)n_steps, (const double*)P.tape.p, (const double*)P.rows.p, P.out.p);
          HIPCHK(hipGetLastError());
          return FC_OK;
        },
        taped ? &replay : nullptr));
    HIPCHK(hipMemcpyAsync(rows.data(), P.rows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(out.data(), P.out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(dy0h.data(), P.dy0.p, dy0h.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(flags, A.flag.p, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return FC_OK;
  });
  FCCHK(taped ? stape_verdict(T, who, n_steps, k, code, rflags) : code);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int any = 0;
  for (size_t s = 0; s < kk; ++s) {
    // a column is lost if its forward run went non-finite, its adjoint state did (the tail's flag), or its controller's adjoint did
    bool bad = flags[s] != 0 || ((P.bad >> s) & 1u) != 0;
    for (size_t e = 0; e < st && !bad; ++e) bad = !std::isfinite(out[s * st + e]);
    for (size_t m = 0; m <= n && !bad; ++m)
      for (size_t e = 0; e < (m == 0 ? (size_t)nx : LR) && !bad; ++e) bad = !std::isfinite(rows[(m * kk + s) * LR + e]);
    for (int q = 0; q < ns && !bad; ++q) bad = !std::isfinite(dy0h[s * ns + q]);
    if (flags_out) flags_out[s] = bad ? 1 : 0;
    any |= bad ? 1 : 0;
    const double* o = out.data() + s * st;
    const auto give = [&](double* dst, long long off, size_t count) {  // dst: [k][count]
      if (!dst || !count) return;
      if (bad)
        std::fill(dst + s * count, dst + (s + 1) * count, nan);
      else
        std::copy(o + off, o + off + (long long)count, dst + s * count);
    };
    give(gAd, 0, (size_t)nx * nx), give(gBd, bk.oBd, (size_t)nx * nyc), give(gC, bk.oC, (size_t)nuc * nx), give(gD, bk.oD, (size_t)nuc * nyc);
    give(gG, bk.oG, (size_t)nyc * ns), give(gg0, bk.og0, (size_t)nyc), give(gS, bk.oS, (size_t)na * nuc);
    const auto rowcopy = [&](double* dst, const double* src, size_t count) {
      if (bad)
        std::fill(dst, dst + count, nan);
      else
        std::copy(src, src + count, dst);
    };
    if (dxc0) rowcopy(dxc0 + s * nx, rows.data() + s * LR, (size_t)nx);
    if (dy0) rowcopy(dy0 + s * ns, dy0h.data() + s * ns, (size_t)ns);
    for (size_t m = 1; m <= n; ++m) {
      const double* row = rows.data() + (m * kk + s) * LR;
      if (dwy) rowcopy(dwy + ((m - 1) * kk + s) * nyc, row + L.eta, (size_t)nyc);
      if (dwu) rowcopy(dwu + ((m - 1) * kk + s) * na, row + L.vb, (size_t)na);
      if (ubar_seq) rowcopy(ubar_seq + ((m - 1) * kk + s) * na, row + L.ub, (size_t)na);
    }
    if (bad) {
      if (dx0) std::fill(dx0 + s * N, dx0 + (s + 1) * N, nan);
      if (dxm1) std::fill(dxm1 + s * N, dxm1 + (s + 1) * N, nan);
    }
  }
  if (any)
    return fail(FC_ERR_DIVERGED, "fc_run_adjoint_closed_loop_batch: a column's forward run or adjoint state is non-finite (flags_out marks the columns; the others are valid)");
  return FC_OK;
}

}  // extern "C"
