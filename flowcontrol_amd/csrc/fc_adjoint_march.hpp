// fc_adjoint_march.hpp -- what the four backward marches share (fc_run_adjoint, _batch, _closed_loop, _closed_loop_batch; DESIGN §5.4
// "One skeleton"): the device part of the preamble, the tape refusal, the step loop over fc_adjoint_schedule.hpp -- segment by segment
// over a checkpointed tape (fc_adjoint_segments.hpp) --, the controller's FcCtrlAdjIO, and the one exit of every call that copies
// into the caller's arrays.  Included at the end of fc_hip.hip, behind
// fc_adjoint_energy_run.hpp and in front of the run files, which define what is only declared here.
#pragma once

namespace {

int adj_march_setup(fc_ctx* h, int slot);  // fc_adjoint_run.hpp
int adjb_repack(fc_ctx* h, int slot);      // fc_adjoint_batch_run.hpp
int adjb_buffers(fc_ctx* h);

// The exit of a call that copies out of or into the caller's arrays or its own frame: `enqueue` holds everything from the first such
// asynchronous copy to the record of ev1, and the stream is synchronised whatever it returned -- no copy lands after the call.  Its
// error comes first, the synchronisation's second; then the device time from ev0 to ev1 goes to `run_ms` (null: no events recorded).
template <class Enqueue>
int adj_enqueue_and_sync(fc_ctx* h, const char* who, double* run_ms, Enqueue&& enqueue) {
  const int code = enqueue();
  const hipError_t sync = hipStreamSynchronize(h->stream);  // the one synchronisation of the call
  if (code != FC_OK) return code;
  if (sync != hipSuccess) return fail(FC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(sync));
  if (!run_ms) return FC_OK;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *run_ms = (double)ms;
  return FC_OK;
}

// A nonlinear handle marches over its taped forward run: FC_OK if `tp` holds exactly this run (or the handle is linearised).  The
// march words `tape_name` ("state tape" / "batched state tape") and `remedy` (the calls that would have taped the run).
template <class Tape>
int adj_tape_refusal(const fc_ctx* h, const char* who, const Tape& tp, int n_steps, int first_slot, const char* tape_name, const char* remedy) {
  std::string why;
  if (!h->nonlinear || tp.covers(n_steps, first_slot, FC_SLOT_BDF2, &why)) return FC_OK;
  return fail(FC_ERR_INVALID, std::string(who) + ": the time scheme is nonlinear and the " + tape_name + " does not hold this run: " + why + " (" + remedy + ")");
}

// The device part of a march's preamble: tables and buffers of n_steps steps from `first_slot`, k columns wide (0: the single march,
// whose sensor table and control columns serve any width), and room for the sensor weights and control gradients on the device.
int adj_march_prepare(fc_ctx* h, int first_slot, int n_steps, int k) {
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(adj_march_setup(h, first_slot));
  if (n_steps > 1) FCCHK(adj_march_setup(h, FC_SLOT_BDF2));
  if (k > 0) {
    FCCHK(adjb_repack(h, first_slot));
    if (n_steps > 1) FCCHK(adjb_repack(h, FC_SLOT_BDF2));
    FCCHK(adjb_buffers(h));
  }
  const size_t rows = (size_t)n_steps * (size_t)std::max(1, k), na = (size_t)std::max(1, h->n_act), ns = (size_t)std::max(1, h->n_sens);
  DevBuf<double>& wseq = k > 0 ? h->adjb.wseq : h->adj.wseq;
  DevBuf<double>& gseq = k > 0 ? h->adjb.gseq : h->adj.gseq;
  if (wseq.n < rows * ns) FCCHK(wseq.alloc(rows * ns));
  if (gseq.n < rows * na) FCCHK(gseq.alloc(rows * na));
  if (k > 0 && h->adjb.stage.n < 2 * (size_t)k * h->N) FCCHK(h->adjb.stage.alloc(2 * (size_t)k * h->N));
  return FC_OK;
}

// What a march over a checkpointed tape needs beside the tape's bookkeeping: three plain functions of the handle (the single marches'
// in fc_adjoint_run.hpp, the batched ones' in fc_adjoint_batch_run.hpp) and where the replays' flags go.
struct AdjReplay {
  const FcAdjointSegments* sg = nullptr;
  int n_steps = 0;
  int* flags = nullptr;                                   // host words the non-finite flags land in behind the call's synchronisation
  int (*begin)(fc_ctx*) = nullptr;                        // save what the replays overwrite: the state ring, the forward non-finite flag
  int (*segment)(fc_ctx*, int j, int n_steps) = nullptr;  // checkpoint j -> ring and buffer columns 0, 1; segment j's forward steps onto the buffer
  int (*end)(fc_ctx*, int* flags) = nullptr;              // put the ring and the flag back, the replays' flag towards the host
};

// The host side of the forward stepper's state while replays are enqueued: the ring cursor, the right-hand side in use, the route
// records, what the residual monitor and the Krylov drivers last reported -- all as on entry when this goes out of scope.
// on = false: nothing is restored.
struct AdjReplayHost {
  fc_ctx* h;
  bool on;
  int cur, last_krylov_iters;
  int64_t last_solve_xchg;
  bool last_checked;
  double* b;
  fc_ctx::StepRoute pend, route;
  AdjReplayHost(fc_ctx* h_, bool on_)
      : h(h_), on(on_), cur(h_->cur), last_krylov_iters(h_->last_krylov_iters), last_solve_xchg(h_->last_solve_xchg), last_checked(h_->last_checked),
        b(h_->b.p), pend(h_->pend), route(h_->route) {}
  ~AdjReplayHost() {
    if (!on) return;
    h->cur = cur;
    ring_point(h);
    h->last_krylov_iters = last_krylov_iters, h->last_solve_xchg = last_solve_xchg, h->last_checked = last_checked;
    h->b.p = b;
    h->pend = pend, h->route = route;
    h->pre_slot = -1;  // (the replays' element loops wrote the element vectors a speculated loop had left)
  }
  AdjReplayHost(const AdjReplayHost&) = delete;
  AdjReplayHost& operator=(const AdjReplayHost&) = delete;
};
// ... and while the forward steps of ONE segment are enqueued: no residual monitor, no timing marks
struct AdjReplayQuiet {
  fc_ctx* h;
  int check_residual;
  bool timing, phase_timing;
  explicit AdjReplayQuiet(fc_ctx* h_) : h(h_), check_residual(h_->check_residual), timing(h_->timing), phase_timing(h_->phase_timing) {
    h->check_residual = 0;
    h->timing = h->phase_timing = false;
  }
  ~AdjReplayQuiet() { h->check_residual = check_residual, h->timing = timing, h->phase_timing = phase_timing; }
  AdjReplayQuiet(const AdjReplayQuiet&) = delete;
  AdjReplayQuiet& operator=(const AdjReplayQuiet&) = delete;
};

// The step loop of a march of n_steps steps from `first_slot` and the state-gradient products behind it.  `tape`: column 0 of the state
// tape the march reads, its columns `stride` doubles apart (null: it reads no forward trajectory).  step(m, slot, c, xm, er) enqueues
// backward step m, after_steps() (optional) what stands behind the last one, product(c, xm, which, dst) the product and its copy into
// the caller's dx0 (which = 0) or dxm1 (1), where that is not null.
// A march over a CHECKPOINTED tape (`rp` not null; DESIGN §5.4 "Checkpointed tape"): `tape` is then the segment buffer, and the loop
// runs segment by segment from the last to the first.  In front of every segment the buffer does not hold, rp->segment(j) enqueues --
// on the same stream, no host synchronisation -- the restore of checkpoint j and the forward steps of the segment; rp->begin() stands in
// front of the first such replay, rp->end() behind the products (both only when something is replayed).  The schedule's columns are
// global: the segments map them into the buffer.  Coefficients, energy rows and everything the callbacks index by m stay global.
template <class Step, class Product, class After = std::nullptr_t>
int adj_march(fc_ctx* h, int first_slot, int n_steps, const double* tape, size_t stride, double* dx0, double* dxm1, Step&& step, Product&& product,
              After&& after_steps = nullptr, const AdjReplay* rp = nullptr) {
  const FcAdjointSchedule S{n_steps, first_slot, FC_SLOT_BDF2, coeffs_for(h, first_slot), coeffs_for(h, FC_SLOT_BDF2)};
  const FcAdjointSegments* sg = rp ? rp->sg : nullptr;
  int seg = 0;  // the segment the buffer holds while the loop reads it
  const auto column = [&](int col) { return tape ? tape + stride * (size_t)(sg ? sg->local_column(col, seg) : col) : (const double*)nullptr; };
  adjen_begin(h);
  bool replaying = false;
  const auto body = [&]() -> int {
    for (seg = sg ? sg->n_segments(n_steps) - 1 : 0; seg >= 0; --seg) {
      if (sg && sg->replay(seg, n_steps)) {
        if (!replaying) FCCHK(rp->begin(h));
        replaying = true;
        FCCHK(rp->segment(h, seg, n_steps));
      }
      for (int m = sg ? sg->seg_last(seg, n_steps) : n_steps; m >= (sg ? sg->seg_first(seg) : 1); --m) {
        const FcAdjointSchedule::Item s = S.step(m);
        FCCHK(step(m, s.slot, s.c, column(s.column), adjen_row(h, s.energy_row)));
      }
    }
    seg = 0;
    if constexpr (!std::is_same_v<std::decay_t<After>, std::nullptr_t>) FCCHK(after_steps());
    if (dx0) FCCHK(product(S.dx0().c, column(S.dx0().column), 0, dx0));
    if (dxm1) FCCHK(product(S.dxm1().c, column(S.dxm1().column), 1, dxm1));
    return FC_OK;
  };
  const int code = body();
  const int put_back = replaying ? rp->end(h, rp->flags) : FC_OK;  // (whatever the loop returned: the forward state goes back where it was)
  return code != FC_OK ? code : put_back;
}

// What the controller's adjoint kernel reads and writes at backward step m of kk lock-step loops (1: the single loop), column 0's
// pointers.  P: fc_ctx::Loop or fc_ctx::LoopB, `wseq` the march's sensor weights, LR the doubles of one adjoint row.  io.g stays null.
template <class LoopTape>
FcCtrlAdjIO ctrl_adj_io(const fc_ctx* h, const LoopTape& P, double* wseq, bool have_r, int m, size_t kk, size_t LR) {
  const fc_ctx::Ctl& C = h->ctl;
  const size_t na = kk * (size_t)h->n_act, ns = kk * (size_t)h->n_sens;
  FcCtrlAdjIO io = {};
  io.matn = P.matn.p;
  io.tape = P.tape.p + (size_t)(m - 1) * kk * (size_t)P.row_len;
  io.r = have_r ? P.rseq.p + (size_t)(m - 1) * na : nullptr;
  if (C.wy.p && P.lt.row0 >= 0) io.w_y = C.wy.p + (size_t)(P.lt.row0 + m - 1) * kk * (size_t)C.bank.nyc;
  if (C.ulo.p) io.u_lo = C.ulo.p, io.u_hi = C.uhi.p;
  io.row = P.rows.p + (size_t)m * kk * LR;
  io.row_prev = P.rows.p + (size_t)(m - 1) * kk * LR;
  io.w_prev = m > 1 ? wseq + (size_t)(m - 2) * ns : nullptr;
  io.dy0 = m > 1 ? nullptr : P.dy0.p;
  return io;
}

}  // namespace
