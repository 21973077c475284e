// fc_adjoint_march.hpp -- what the four backward marches share (fc_run_adjoint, _batch, _closed_loop, _closed_loop_batch; DESIGN §5.4
// "One skeleton"): the device part of the preamble, the tape refusal, the step loop over fc_adjoint_schedule.hpp -- segment by segment
// over the state tape (fc_adjoint_segments.hpp) --, the controller's FcCtrlAdjIO, and the one exit of every call that copies
// into the caller's arrays; and what the eight state-tape entry points share (fc_ctx::StateTape: reserve, begin, info, the verdict
// behind a march; copy, append and release stand in fc_hip.hip, in front of the forward step).  Included at the end of fc_hip.hip, behind
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

// A nonlinear handle marches over its taped forward run: FC_OK if `T` holds exactly this run (or the handle is linearised).  The
// march words `tape_name` ("state tape" / "batched state tape") and `remedy` (the calls that would have taped the run).
int adj_tape_refusal(const fc_ctx* h, const char* who, const fc_ctx::StateTape& T, int n_steps, int first_slot, const char* tape_name, const char* remedy) {
  std::string why;
  if (!h->nonlinear || T.sg.covers(n_steps, first_slot, FC_SLOT_BDF2, &why)) return FC_OK;
  return fail(FC_ERR_INVALID, std::string(who) + ": the time scheme is nonlinear and the " + tape_name + " does not hold this run: " + why + " (" + remedy + ")");
}

// ── the state tape's entry points (fc_adjoint_tape_reserve / _sparse / _batch / _sparse_batch, _begin, _info): one body each ─────────
// What a reserve call names: the layout of its mode (fc_ctx::StateTape) and the sizes of what a replaying march borrows.
struct StapeLayout {
  size_t col;
  int rows, KB, nflag;
  size_t n_ring, n_scratch;
};
// what every reserve call refuses, in its own name; `some`: the call asks for a tape (it frees one otherwise)
int stape_reserve_refusal(const fc_ctx* h, const std::string& who, int capacity, int every, bool some) {
  if (!h) return fail(FC_ERR_INVALID, who + ": null handle");
  if (every < 0 || every > (1 << 24)) return fail(FC_ERR_INVALID, who + ": every must be in [0, 2^24] (0 frees the reserve)");
  if (capacity < 0 || capacity > (1 << 24)) return fail(FC_ERR_INVALID, who + ": capacity must be in [0, 2^24]");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, who + ": a step is in flight");
  if (some && (h->partitioned || exchanges(h)))
    return fail(FC_ERR_INVALID, who + ": partitioned (multi-GPU) handles keep no state tape: a rank holds its own rows only");
  return FC_OK;
}
// A tape of `capacity` steps in segments of `every` (dense: every == capacity, `tape` alone) laid out as L; capacity or every 0 frees
// the reserve -- a sparse call frees a checkpointed one only: a dense tape is not its to free.  One policy: free memory is checked
// before anything is released (what T holds counts as free: it goes for the new tape), then everything is allocated into temporaries
// and moved in only when all of it succeeded; a failed allocation leaves no tape.
int stape_reserve(fc_ctx* h, fc_ctx::StateTape& T, const std::string& who, int capacity, int every, bool sparse, const StapeLayout& L) {
  if (capacity > 0 && every > 0 && !h->have_perm) return fail(FC_ERR_NOT_READY, who + ": no permutation (fc_setup_solver): the tape is kept in the solver's numbering");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (capacity == 0 || every == 0) {
    if (!sparse || T.sparse) stape_release(T);
    return FC_OK;
  }
  FcAdjointSegments plan;
  plan.reserve(capacity, every);
  const size_t n_buf = L.col * (size_t)plan.buffer_columns(), n_ck = sparse ? 2 * L.col * (size_t)plan.checkpoints() : 0,
               n_ct = sparse ? std::max<size_t>(1, 2 * (size_t)h->n_act * (size_t)L.rows * (size_t)capacity) : 0, n_ring = sparse ? L.n_ring : 0,
               n_scratch = sparse ? L.n_scratch : 0, need = n_buf + n_ck + n_ct + n_ring + n_scratch;
  size_t fr = 0, tot = 0;
  HIPCHK(hipMemGetInfo(&fr, &tot));
  const size_t held = 8 * (T.tape.n + T.ckpt.n + T.ctape.n + T.ring_save.n + T.scratch.n);
  if (need > (fr + held) / 8)
    return fail(FC_ERR_INVALID, who + ": a tape of " + std::to_string(capacity) + " steps" + (sparse ? " in segments of " + std::to_string(every) : std::string()) + " needs " +
                                    std::to_string(8 * need) + " bytes (" + std::to_string(8 * L.col) + " per column, " +
                                    std::to_string(sparse ? plan.columns() : plan.buffer_columns()) + " columns), the device has " + std::to_string(fr + held) + " free");
  stape_release(T);
  DevBuf<double> buf, ck, ct, rs, sc;
  DevBuf<int> rf;
  int code = buf.alloc(n_buf);
  if (code == FC_OK) code = ck.alloc(n_ck);
  if (code == FC_OK) code = ct.alloc(n_ct);
  if (code == FC_OK) code = rs.alloc(n_ring);
  if (code == FC_OK) code = sc.alloc(n_scratch);
  if (code == FC_OK) code = rf.alloc(sparse ? (size_t)L.nflag : 0);
  if (code != FC_OK) {
    (void)hipGetLastError();
    return code;
  }
  T.tape = std::move(buf), T.ckpt = std::move(ck), T.ctape = std::move(ct);
  T.ring_save = std::move(rs), T.scratch = std::move(sc), T.rflag = std::move(rf);
  T.sg = plan;
  T.sparse = sparse;
  T.col = L.col, T.rows = L.rows, T.KB = L.KB, T.nflag = L.nflag;
  T.ctape_na = sparse ? h->n_act : 0;
  const char* e = std::getenv("FC_ADJ_TAPE_NT");
  T.tape_nt = !(e && e[0] == '0');
  return FC_OK;
}
// The present two time levels into buffer columns 0 and 1 (checkpointed: and into checkpoint 0); `laid_out_by` names the reserve call
// whose control tape must still fit the actuators.
int stape_begin(fc_ctx* h, fc_ctx::StateTape& T, const char* who, const char* laid_out_by, const double* x_prev, const double* x_now) {
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  if (T.sparse && T.ctape_na != h->n_act) return fail(FC_ERR_NOT_READY, std::string(who) + ": the actuators changed since " + laid_out_by + " laid the control tape out");
  FCCHK(stape_copy(h, T, T.col, x_prev, T.tape.p));
  FCCHK(stape_copy(h, T, T.col, x_now, T.tape.p + T.col));
  if (T.sparse) FCCHK(stape_copy(h, T, 2 * T.col, T.tape.p, T.ckpt.p));
  T.sg.begin();
  return FC_OK;
}
// info[0 .. 5] of both info calls: capacity, steps held, overflowed, bytes (buffer, pairs and control tape), begun, steps lost
void stape_info(const fc_ctx::StateTape& T, int64_t* info) {
  info[0] = T.sg.capacity, info[1] = T.sg.count(), info[2] = T.sg.overflowed() ? 1 : 0, info[3] = T.tape_bytes();
  info[4] = T.sg.begun ? 1 : 0, info[5] = T.sg.lost;
}
// In a march's preamble, `taped`: it reads T (which then covers its n_steps steps).  *replays: it recomputes segments -- never on a
// dense tape, which is one segment.  What the replays borrow exists since the reserve; a ring or a sensor set that grew since then
// gets its room here (in front of ev0: nothing is allocated between the two events).
int stape_march_begin(fc_ctx::StateTape& T, bool taped, int n_steps, const StapeLayout& L, bool* replays) {
  *replays = taped && T.sg.replayed_steps(n_steps) > 0;
  if (taped) T.replayed = 0;
  if (!*replays) return FC_OK;
  if (T.ring_save.n < L.n_ring) FCCHK(T.ring_save.alloc(L.n_ring));
  if (T.scratch.n < L.n_scratch) FCCHK(T.scratch.alloc(L.n_scratch));
  if (T.rflag.n < (size_t)T.nflag) FCCHK(T.rflag.alloc((size_t)T.nflag));
  return FC_OK;
}
// Behind the synchronisation of a march over T (`code`: what it returned): the bookkeeping moves on, and a replay that went
// non-finite where the taped run did not -- in one of the first `ncol` columns; `flags` as StateTape::rflag -- did not reproduce the run.
int stape_verdict(fc_ctx::StateTape& T, const char* who, int n_steps, int ncol, int code, const int* flags) {
  if (code != FC_OK) {  // (a march that stopped between two segments left the buffer half written)
    if (T.sg.replayed_steps(n_steps) > 0) T.sg.invalidate();
    return code;
  }
  T.sg.marched();
  const int half = T.nflag / 2;
  for (int s = 0; s < ncol && s < half; ++s)
    if (flags[half + s] && !flags[s])
      return fail(FC_ERR_HIP, std::string(who) + ": a replayed forward step went non-finite" + (half > 1 ? " in column " + std::to_string(s) : std::string()) +
                                  " where the taped run did not: the replay did not reproduce the run");
  return FC_OK;
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
// A march over the state tape (`rp` not null; DESIGN §5.4 "Checkpointed tape"): `tape` is the segment buffer, and the loop runs
// segment by segment from the last to the first -- a dense tape is one segment, which the buffer holds: nothing is replayed.
// In front of every segment the buffer does not hold, rp->segment(j) enqueues --
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
