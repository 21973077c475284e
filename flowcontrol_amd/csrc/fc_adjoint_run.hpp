// fc_adjoint_run.hpp -- host side of the adjoint time stepping (fc_set_adjoint_factors, fc_solve_transposed, fc_run_adjoint,
// fc_step_adjoint; kernels in fc_adjoint.hip.h).  Included at the end of fc_hip.hip, behind fc_adjoint_march.hpp (what the
// four marches share: preamble, step loop, exit); here: the single march's tables, buffers, backward step and mass product.
//
// The transposed system of a slot is solved by the launches of the direct one: the sweeps read whatever array OrderSys::f_val names and
// the SpMVs whatever OrderSys::Ap_val names, so an adjoint solve is two pointer swaps (AdjUse) around apply_factors / solve_permuted,
// undone before the call returns.  The backward march keeps its own work buffer, right-hand side, element vectors and masked copies:
// the state ring, the speculated element vectors, the step counter and the snapshot bank never see it.
//
// On a nonlinear handle fc_run_adjoint marches over the state tape (fc_adjoint_tape_reserve / _begin below; kernels in
// fc_adjoint_nl.hip.h, bookkeeping in fc_adjoint_segments.hpp): the element loop of a backward step then also applies the transposed
// Jacobian of the convective term at the taped state x_m.  The tape is filled by the forward steps (stape_append in fc_hip.hip).
#pragma once

namespace {

// While it lives the slot's sweeps and SpMVs run on the transposed values; with `march` the solve also works in the march's own
// buffers, without the forward path's residual monitor, finiteness test and timing marks.  Everything is back on destruction.
struct AdjUse {
  fc_ctx* h;
  OrderSys& S;
  fc_ctx::Adj::Slot& T;
  bool march;
  fc_ctx::BufView buf0, b0;
  int check0;
  bool sweep_check0, timing0, phase0;
  AdjUse(fc_ctx* h_, int slot, bool march_) : h(h_), S(h_->sys[slot]), T(h_->adj.s[slot]), march(march_) {
    std::swap(S.f_val.p, T.f_t.p);
    std::swap(S.Ap_val.p, T.ap_t.p);
    buf0 = h->buf, b0 = h->b;
    check0 = h->check_residual;
    sweep_check0 = h->sweep_check, timing0 = h->timing, phase0 = h->phase_timing;
    if (march) {
      h->buf.p = h->adj.work.p, h->buf.n = h->adj.work.n;
      h->b.p = h->adj.b.p, h->b.n = h->adj.b.n;
      h->check_residual = 0;
      h->sweep_check = h->timing = h->phase_timing = false;
    }
  }
  ~AdjUse() {
    std::swap(S.f_val.p, T.f_t.p);
    std::swap(S.Ap_val.p, T.ap_t.p);
    h->buf = buf0, h->b = b0;
    h->check_residual = check0;
    h->sweep_check = sweep_check0, h->timing = timing0, h->phase_timing = phase0;
  }
  AdjUse(const AdjUse&) = delete;
  AdjUse& operator=(const AdjUse&) = delete;
};

// why a slot cannot have (or use) transposed factors; FC_OK if it can
int adj_refusal(fc_ctx* h, int slot, const char* who) {
  const OrderSys& S = h->sys[slot];
  const std::string w = std::string(who) + ": ";
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, w + "partitioned handles are not supported (the transposed export needs every front on one device)");
  if (S.factor_free) return fail(FC_ERR_INVALID, w + "the slot has no factors (fc_setup_krylov)");
  if (!S.structured || !h->have_plan || !S.ready) return fail(FC_ERR_NOT_READY, w + "the slot is not factorised (fc_setup_solver / fc_refactor)");
  if (S.bits != 64) return fail(FC_ERR_INVALID, w + "compressed factors (fc_set_factor_precision " + std::to_string(S.bits) + "): the transposed export is fp64");
  if (S.truncated) return fail(FC_ERR_INVALID, w + "truncated factors are a preconditioner, not a solve");
  if (S.inexact) return fail(FC_ERR_INVALID, w + "the slot's factors are inexact (they precondition GMRES): no direct transposed solve");
  if (h->method != FC_METHOD_REFINE) return fail(FC_ERR_INVALID, w + "a Krylov method is selected (fc_set_solver_options): the adjoint runs on the direct factor apply");
  if (h->root_x0 >= 0) return fail(FC_ERR_INVALID, w + "the handle stores a block of the root's rows only (fc_set_root_rows)");
  return FC_OK;
}

// the slot's transposed arrays are there, current and switched on
int adj_usable(fc_ctx* h, int slot, const char* who) {
  FCCHK(adj_refusal(h, slot, who));
  const fc_ctx::Adj::Slot& T = h->adj.s[slot];
  const std::string w = std::string(who) + ": ";
  if (!T.avail) return fail(FC_ERR_NOT_READY, w + "no transposed factors for this slot (fc_set_adjoint_factors)");
  if (T.stale) return fail(FC_ERR_NOT_READY, w + "the transposed factors are stale (the slot's operator, Dirichlet rows or permutation changed: fc_set_adjoint_factors again)");
  if (!T.use) return fail(FC_ERR_NOT_READY, w + "the transposed factors are switched off (fc_set_adjoint_factors(on = 1))");
  if (T.f_t.n != h->sys[slot].f_val.n || (int64_t)T.ap_t.n != h->sys[slot].Ap_nnz) return fail(FC_ERR_NOT_READY, w + "the transposed factors belong to another structure");
  return FC_OK;
}

int64_t adj_slot_bytes(const fc_ctx::Adj::Slot& T) { return 8 * (int64_t)(T.f_t.n + T.ap_t.n + T.bt.n) + 4 * (int64_t)T.tpos.n; }
int64_t adj_shared_bytes(const fc_ctx::Adj& A) {
  return (int64_t)sizeof(FcExpTItem) * (int64_t)A.texp.n + 4 * (int64_t)(A.ct_ptr.n + A.ct_sens.n + A.flag.n + A.st.rflag.n) +
         8 * (int64_t)(A.ct_w.n + A.work.n + A.b.n + A.zm.n + A.ev.n + A.term.n + A.part.n + A.wseq.n + A.gseq.n) + A.st.tape_bytes() +
         8 * (int64_t)(A.st.ring_save.n + A.st.scratch.n);  // (the state tape and what its replays borrow)
}
void adj_release_shared(fc_ctx::Adj& A) {
  A.texp.release(), A.ct_ptr.release(), A.ct_sens.release(), A.ct_w.release();
  A.work.release(), A.b.release(), A.zm.release(), A.ev.release(), A.term.release(), A.part.release(), A.wseq.release(), A.gseq.release();
  A.flag.release();
  A.texp_n = 0;
  A.texp_ok = A.ct_ok = A.march_ok = A.term_pending = false;
}

// workgroups of fc_adj_tail (and partials per actuator)
inline int adj_tail_grid(int N) { return std::min(2048, nblocks(N, 256)); }

// buffers of the march (once per N / n_act), the sensor table by row and the slot's control columns (once per set of tables;
// slot = -1: none)
int adj_march_setup(fc_ctx* h, int slot) {
  fc_ctx::Adj& A = h->adj;
  const int N = h->N, na = std::max(1, h->n_act), ns = std::max(1, h->n_sens);
  if (!A.march_ok) {
    FCCHK(A.work.alloc(2 * (size_t)N));
    FCCHK(A.b.alloc((size_t)N));
    FCCHK(A.zm.alloc(2 * (size_t)N));
    FCCHK(A.ev.alloc((size_t)12 * h->nc));
    FCCHK(A.term.alloc((size_t)N));
    FCCHK(A.part.alloc((size_t)na * adj_tail_grid(N)));
    FCCHK(A.flag.alloc(1));
    FCCHK(A.wseq.alloc((size_t)ns));
    FCCHK(A.gseq.alloc((size_t)na));
    FCCHK(A.work.zero(h->stream));
    FCCHK(A.zm.zero(h->stream));
    FCCHK(A.ev.zero(h->stream));
    FCCHK(A.flag.zero(h->stream));
    A.zm_cur = 0;
    A.term_pending = false;
    A.march_ok = true;
    h->adj_route = fc_ctx::AdjRoute{};  // (the buffers the last step's record points into are gone)
  }
  if (!A.ct_ok) {
    std::vector<int> ip((size_t)N), cnt((size_t)N + 1, 0);
    for (int i = 0; i < N; ++i) ip[(size_t)h->h_perm[i]] = i;
    const int nz = h->n_sens ? h->h_s_rowptr[(size_t)h->n_sens] : 0;
    for (int k = 0; k < nz; ++k) ++cnt[(size_t)ip[(size_t)h->h_s_idx[(size_t)k]] + 1];
    for (int i = 0; i < N; ++i) cnt[(size_t)i + 1] += cnt[(size_t)i];
    std::vector<int> fill(cnt.begin(), cnt.end() - 1), sens((size_t)std::max(1, nz), 0);
    std::vector<double> wt((size_t)std::max(1, nz), 0.0);
    for (int s = 0; s < h->n_sens; ++s)  // sensors ascending, a sensor's entries in the caller's order: the order of a row's sum
      for (int k = h->h_s_rowptr[(size_t)s]; k < h->h_s_rowptr[(size_t)s + 1]; ++k) {
        const int q = fill[(size_t)ip[(size_t)h->h_s_idx[(size_t)k]]]++;
        sens[(size_t)q] = s;
        wt[(size_t)q] = h->h_s_w[(size_t)k];
      }
    FCCHK(A.ct_ptr.upload(cnt, h->stream));
    FCCHK(A.ct_sens.upload(sens, h->stream));
    FCCHK(A.ct_w.upload(wt, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (the host vectors go out of scope)
    A.ct_ok = true;
  }
  if (slot < 0) return FC_OK;
  fc_ctx::Adj::Slot& T = A.s[slot];
  if (!T.bt_ok) {
    const OrderSys& S = h->sys[slot];
    if (!S.have_lift) return fail(FC_ERR_NOT_READY, "adjoint: fc_apply_bc not called for this order");
    if (h->have_force && !h->fvec_ok) return fail(FC_ERR_NOT_READY, "adjoint: force vectors not built");
    if (T.bt.n != (size_t)na * N) FCCHK(T.bt.alloc((size_t)na * N));
    FCCHK(T.bt.zero(h->stream));
    if (h->n_act > 0)
      hipLaunchKernelGGL(fc_adj_control_columns, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->n_act, h->bcslot_p.p, h->bcprof.p, S.lift_p.p,
                         h->have_force ? h->fvec.p : (const double*)nullptr, T.bt.p);
    HIPCHK(hipGetLastError());
    T.bt_ok = true;
  }
  return FC_OK;
}

// what every adjoint step needs of the handle and the slot.  `taped`: the caller reads the forward trajectory from the state tape
// (fc_run_adjoint), so a nonlinear time scheme is not refused here -- its tape is checked by the caller.
int adj_step_ready(fc_ctx* h, int slot, const char* who, bool taped = false) {
  FCCHK(check_step_ready(h, slot));
  if (h->nonlinear && !taped)
    return fail(FC_ERR_INVALID, std::string(who) + ": the time scheme is nonlinear (fc_set_time_scheme(dt, 0)): the adjoint of the nonlinear stepper needs the forward "
                                                   "trajectory, which only fc_run_adjoint reads (fc_adjoint_tape_reserve / fc_adjoint_tape_begin)");
  if (h->sys[slot].have_c) return fail(FC_ERR_INVALID, std::string(who) + ": the slot has an explicit right-hand-side operator (Crank-Nicolson)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": collect the step in flight first (fc_step_end)");
  return adj_usable(h, slot, who);
}

// M Z (cm_n zm_cur + cm_nn zm_prev) (+ C^T w) (+ term) into the march's right-hand side and the y half of its work buffer.  On a
// nonlinear handle `xm` is the taped state the two forward steps read (permuted numbering) and the element loop adds
// J(xm)^T Z (cc_n zm_cur + cc_nn zm_prev): fc_adj_elem_nl in the place of the forward loop, chosen by the same rule (launch_elem_on).
// `er`: the device energy weight of this backward step (adjen_row) -- e xm joins the two masked levels at the nodes of the element
// loop -- or null: no energy term (no rows held, fc_step_adjoint, the dx0 / dxm1 products, since dE_0 is not in the sum).
// `xe` (with `er`): the column e multiplies when it is not xm -- dx_m of the tangent tape (adjen_source_column); J(xm)^T still reads xm.
int adj_enqueue_rhs(fc_ctx* h, const StepCoeffs& c, const double* xm, const double* d_w, const double* d_term, const double* er = nullptr,
                    const double* xe = nullptr) {
  fc_ctx::Adj& A = h->adj;
  const int N = h->N;
  const double* z1 = A.zm.p + (size_t)A.zm_cur * N;
  const double* z2 = A.zm.p + (size_t)(1 - A.zm_cur) * N;
  fc_ctx::AdjRoute& R = h->adj_pend;
  R = fc_ctx::AdjRoute{};
  if (er && !xm) return fail(FC_ERR_INVALID, "adjoint: the energy term needs a taped state");
  if (!er) xe = nullptr;
  const bool reg = h->elem_reg_min > 0 && h->nc >= h->elem_reg_min;  // (launch_elem_on's rule)
  if (!h->nonlinear && !er) {
    R.elem = launch_elem_on(h, h->stream, StepCoeffs{c.cm_n, c.cm_nn, 0.0, 0.0}, z1, z2, A.ev.p, nullptr, h->nc);  // 1 fc_rhs_elem, 2 fc_rhs_elem_reg
    R.g_elem = R.elem == 2 ? nblocks(h->nc, 256) : nblocks((int64_t)h->nc * 8, 256);
  } else if (!h->nonlinear) {
    R.elem = xe ? (reg ? FC_ADJ_ELEM_EN_REG_SRC : FC_ADJ_ELEM_EN_SRC) : (reg ? FC_ADJ_ELEM_EN_REG : FC_ADJ_ELEM_EN);
    R.g_elem = reg ? nblocks(h->nc, 256) : nblocks((int64_t)h->nc * 8, 256);
    const double* xs = xe ? xe : xm;  // (the kernels take the energy column as a pointer: they are handed the tangent tape's)
    if (reg)
      hipLaunchKernelGGL(fc_adj_elem_en_reg, dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xs, z1, z2, c.cm_n, c.cm_nn, er, A.ev.p);
    else
      hipLaunchKernelGGL(fc_adj_elem_en, dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xs, z1, z2, c.cm_n, c.cm_nn, er, A.ev.p);
    ++h->adjen.steps;
  } else {
    if (!xm) return fail(FC_ERR_INVALID, "adjoint: the nonlinear element loop needs a taped state");
    R.elem = er ? (reg ? FC_ADJ_ELEM_NL_REG_EN : FC_ADJ_ELEM_NL_EN) : (reg ? FC_ADJ_ELEM_NL_REG : FC_ADJ_ELEM_NL);
    R.g_elem = reg ? nblocks(h->nc, 256) : nblocks((int64_t)h->nc * 8, 256);
    if (xe) {
      R.elem = reg ? FC_ADJ_ELEM_NL_REG_EN_SRC : FC_ADJ_ELEM_NL_EN_SRC;
      if (reg)
        hipLaunchKernelGGL((fc_adj_elem_nl_reg<true, true>), dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xm, z1, z2, c.cm_n, c.cm_nn,
                           c.cc_n, c.cc_nn, er, A.ev.p, xe);
      else
        hipLaunchKernelGGL((fc_adj_elem_nl<true, true>), dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xm, z1, z2, c.cm_n, c.cm_nn, c.cc_n,
                           c.cc_nn, er, A.ev.p, xe);
    } else {
      pick_bool(er != nullptr, [&](auto EN) {
        if (reg)
          hipLaunchKernelGGL(fc_adj_elem_nl_reg<EN>, dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xm, z1, z2, c.cm_n, c.cm_nn, c.cc_n,
                             c.cc_nn, er, A.ev.p, (const double*)nullptr);
        else
          hipLaunchKernelGGL(fc_adj_elem_nl<EN>, dim3(R.g_elem), dim3(256), 0, h->stream, h->nc, h->cnp.p, h->geom.p, xm, z1, z2, c.cm_n, c.cm_nn, c.cc_n,
                             c.cc_nn, er, A.ev.p, (const double*)nullptr);
      });
    }
    if (er) ++h->adjen.steps;
  }
  hipLaunchKernelGGL(fc_adj_rhs_gather, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->gptr_p.p, h->gidx_p.p, A.ev.p, A.ct_ptr.p, A.ct_sens.p,
                     A.ct_w.p, h->n_sens > 0 ? d_w : (const double*)nullptr, d_term, A.b.p, A.work.p);
  R.g_gather = nblocks(N, 256);
  R.have_w = (h->n_sens > 0 && d_w) ? 1 : 0;
  R.have_term = d_term ? 1 : 0;
  h->adj_route.b_live = false;  // (the last step's right-hand side is gone; adj_enqueue_step commits this one)
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// one backward step on `slot`: right-hand side, transposed solve, tail (g -> d_g, flag, masked copy); the masked copies move on
int adj_enqueue_step(fc_ctx* h, int slot, const StepCoeffs& c, const double* xm, const double* d_w, double* d_g, const double* er = nullptr,
                     const double* xe = nullptr) {
  fc_ctx::Adj& A = h->adj;
  const int N = h->N;
  FCCHK(adj_enqueue_rhs(h, c, xm, d_w, A.term_pending ? A.term.p : nullptr, er, xe));
  A.term_pending = false;
  const double *x = nullptr, *dx = nullptr;
  {
    AdjUse use(h, slot, true);
    int nrp = 0;
    FCCHK(solve_permuted(h, h->sys[slot], &x, &dx, &nrp));
  }
  const int g = adj_tail_grid(N);
  double* znew = A.zm.p + (size_t)(1 - A.zm_cur) * N;  // (mu_{m+2}'s copy was read by the element loop above: its place is free)
  hipLaunchKernelGGL(fc_adj_tail, dim3(g), dim3(256), 0, h->stream, N, x, dx, h->bcslot_p.p, h->n_act, A.s[slot].bt.p, znew, A.flag.p, A.part.p);
  if (h->n_act > 0) hipLaunchKernelGGL(fc_adj_reduce, dim3(h->n_act), dim3(64), 0, h->stream, h->n_act, g, A.part.p, d_g);
  HIPCHK(hipGetLastError());
  A.zm_cur = 1 - A.zm_cur;
  fc_ctx::AdjRoute& R = h->adj_pend;
  R.g_tail = g, R.passes = std::max(1, (h->n_act + 3) / 4);
  R.reduced = h->n_act > 0 ? 1 : 0, R.gx = h->n_act > 0 ? g : 0;
  R.slot = slot, R.x = x, R.dx = dx, R.b_live = true, R.have = true;
  h->adj_route = R;
  return FC_OK;
}

// mu_{m+1} = mu_{m+2} = 0; z (W layout, host) waits for the next step
int adj_reset(fc_ctx* h, const double* z_terminal) {
  fc_ctx::Adj& A = h->adj;
  const int N = h->N;
  FCCHK(A.zm.zero(h->stream));
  FCCHK(A.flag.zero(h->stream));
  A.zm_cur = 0;
  A.term_pending = z_terminal != nullptr;
  if (z_terminal) {
    HIPCHK(hipMemcpyAsync(h->tmpN.p, z_terminal, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(fc_gather_perm, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->perm.p, h->tmpN.p, A.term.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's vector was staged through pageable memory)
  }
  return FC_OK;
}

// M Z (cm_n mu_last + cm_nn mu_before) (nonlinear: + J(xm)^T Z (cc_n mu_last + cc_nn mu_before), xm a taped state) in the W layout into
// the caller's `dst`, staged through tmpN (which = 0: dx0) or tmpN2 (1: dxm1); the copy is enqueued, the caller synchronises
int adj_enqueue_mass_product(fc_ctx* h, const StepCoeffs& c, const double* xm, int which, double* dst) {
  double* stage = which == 0 ? h->tmpN.p : h->tmpN2.p;
  FCCHK(adj_enqueue_rhs(h, c, xm, nullptr, nullptr));
  hipLaunchKernelGGL(fc_scatter_perm, dim3(nblocks(h->N, 256)), dim3(256), 0, h->stream, h->N, h->perm.p, (const double*)h->adj.b.p,
                     (const double*)nullptr, stage);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst, stage, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}

// ── replays of the single marches over a checkpointed state tape (DESIGN §5.4 "Checkpointed tape") ──────────────────────────────────────────
// the single run's layout: columns of N doubles, one control row per step, 2 flag words; a replay borrows the ring and sinks (y | E | r^2, b^2)
StapeLayout adj_tape_layout(const fc_ctx* h) { return StapeLayout{(size_t)h->N, 1, 0, 2, h->ring.n, (size_t)std::max(1, h->n_sens) + 4}; }
// What the two single marches hand adj_march.  A replayed step is the taped step's launches again -- enqueue_step_launches on the
// step's order slot, reading the control row the step read from the control tape -- and the ring's advance; nothing of enqueue_step's
// counting (step counter, snapshot bank, tapes).  It publishes into a sink, forms no residual and no energy.
// `flags`: [0] the forward non-finite flag as the march found it, [1] as the replays left it (valid behind the call's synchronisation).
int adj_replay_begin(fc_ctx* h) {
  fc_ctx::StateTape& A = h->adj.st;
  const size_t ring = h->ring.n;
  HIPCHK(hipMemcpyAsync(A.ring_save.p, h->ring.p, ring * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(A.rflag.p, h->flag.p, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  h->b.p = h->bstore.p;
  return FC_OK;
}
int adj_replay_segment(fc_ctx* h, int j, int n_steps) {
  fc_ctx::StateTape& A = h->adj.st;
  const FcAdjointSegments& sg = A.sg;
  const size_t N = (size_t)h->N, na = (size_t)h->n_act, ns = (size_t)std::max(1, h->n_sens);
  const double* pair = A.ckpt.p + 2 * N * (size_t)j;
  FCCHK(stape_copy(h, A, N, pair, st_nn(h)));
  FCCHK(stape_copy(h, A, N, pair + N, st_n(h)));
  FCCHK(stape_copy(h, A, 2 * N, pair, A.tape.p));
  AdjReplayQuiet quiet(h);  // (no residual monitor, no timing marks -- the backward steps in between keep theirs)
  for (int m = sg.seg_first(j); m <= sg.seg_last(j, n_steps); ++m) {
    const double* row = na > 0 ? A.ctape.p + (size_t)(m - 1) * 2 * na : nullptr;
    h->pre_slot = -1;  // (no element loop ran ahead of a replayed step)
    FCCHK(enqueue_step_launches(h, sg.slots[(size_t)m - 1], row, A.scratch.p, A.scratch.p + ns, A.scratch.p + ns + 1, nullptr, 0, row ? row + na : nullptr, nullptr, 0.0));
    ring_advance(h);
    FCCHK(stape_copy(h, A, N, st_n(h), A.tape.p + N * (size_t)sg.local_column(m + 1, j)));
    ++A.replayed;
  }
  return FC_OK;
}
int adj_replay_end(fc_ctx* h, int* flags) {
  fc_ctx::StateTape& A = h->adj.st;
  HIPCHK(hipMemcpyAsync(A.rflag.p + 1, h->flag.p, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->flag.p, A.rflag.p, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->ring.p, A.ring_save.p, h->ring.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(flags, A.rflag.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}
AdjReplay adj_replay_single(fc_ctx* h, int n_steps, int* flags) { return AdjReplay{&h->adj.st.sg, n_steps, flags, adj_replay_begin, adj_replay_segment, adj_replay_end}; }

}  // namespace

extern "C" {

// behind the elimination of fc_refactor(slot), while the fronts hold it: the transposed factor values and matrix values of the slot
static int adjoint_after_refactor(fc_ctx* h, int slot) {
  fc_ctx::Adj& A = h->adj;
  fc_ctx::Adj::Slot& T = A.s[slot];
  if (!T.avail) return FC_OK;
  h->adjb.tile_ok[slot] = false;  // (f_t is rewritten or marked stale below: the batched march's tiled copy of it is out of date)
  OrderSys& S = h->sys[slot];
  if (h->partitioned || h->root_x0 >= 0 || S.bits != 64 || T.f_t.n != S.f_val.n || (int64_t)T.ap_t.n != S.Ap_nnz || (int64_t)T.tpos.n != S.Ap_nnz) {
    T.stale = true;  // another layout: fc_set_adjoint_factors decides (and says why not)
    return FC_OK;
  }
  if (!A.texp_ok) {
    std::vector<FcExpTItem> items;
    try {
      items = export_t_items(h);
    } catch (const std::exception& e) {
      return fail(FC_ERR_INVALID, std::string("fc_set_adjoint_factors: ") + e.what());
    }
    A.texp_n = (int64_t)items.size();
    if (items.empty()) items.push_back(FcExpTItem{0, 0, 0, 0});
    FCCHK(A.texp.upload(items, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    A.texp_ok = true;
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  // (values outside the fronts' blocks -- the padding behind the last one -- as in the direct array)
  HIPCHK(hipMemcpyAsync(T.f_t.p, S.f_val.p, S.f_val.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (A.texp_n > 0)
    hipLaunchKernelGGL(fc_fe_export_t, dim3((unsigned)A.texp_n), dim3(256), 0, h->stream, h->pfront.p, A.texp.p, h->fronts.p, T.f_t.p);
  hipLaunchKernelGGL(fc_adj_values_t, dim3(nblocks(S.Ap_nnz, 256)), dim3(256), 0, h->stream, (int64_t)S.Ap_nnz, T.tpos.p, S.Ap_val.p, T.ap_t.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  T.export_ms = (double)ms;
  ++T.n_export;
  T.stale = false;
  return FC_OK;
}

int fc_set_adjoint_factors(fc_handle h, int slot, int32_t on) {
  if (!h || slot < 0 || slot > 1 || on < -1 || on > 1)
    return fail(FC_ERR_INVALID, "fc_set_adjoint_factors: slot must be 0 / 1 and on 1 (build), 0 (keep, do not use) or -1 (free)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  fc_ctx::Adj& A = h->adj;
  fc_ctx::Adj::Slot& T = A.s[slot];
  if (on == -1) {
    HIPCHK(hipStreamSynchronize(h->stream));
    adj_drop(h, slot);
    if (!A.s[0].avail && !A.s[1].avail) adj_release_shared(A);
    return FC_OK;
  }
  if (on == 0) {
    if (!T.avail) return fail(FC_ERR_NOT_READY, "fc_set_adjoint_factors: no transposed factors for this slot to switch off");
    T.use = false;
    return FC_OK;
  }
  FCCHK(adj_refusal(h, slot, "fc_set_adjoint_factors"));
  OrderSys& S = h->sys[slot];
  if (S.have_c) return fail(FC_ERR_INVALID, "fc_set_adjoint_factors: the slot has an explicit right-hand-side operator (Crank-Nicolson)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_set_adjoint_factors: collect the step in flight first (fc_step_end)");
  if (T.avail && !T.stale && T.f_t.n == S.f_val.n && (int64_t)T.ap_t.n == S.Ap_nnz) {
    T.use = true;
    return FC_OK;
  }
  // the transpose-position map of the slot's permuted pattern
  {
    std::vector<int> rp((size_t)h->N + 1), col((size_t)S.Ap_nnz), tpos;
    HIPCHK(hipMemcpy(rp.data(), S.Ap_rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(col.data(), S.Ap_col.p, col.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (rp[0] != 0 || rp[(size_t)h->N] != (int)S.Ap_nnz) return fail(FC_ERR_INVALID, "fc_set_adjoint_factors: bad row pointers of the permuted matrix");
    FCCHK(transpose_map(rp, col, tpos, "fc_set_adjoint_factors"));
    FCCHK(T.tpos.upload(tpos, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  FCCHK(T.f_t.alloc(S.f_val.n));
  FCCHK(T.ap_t.alloc((size_t)S.Ap_nnz));
  T.avail = true;
  T.stale = true;  // until the export below
  T.use = true;
  T.bt_ok = false;
  // The fronts buffer is shared by both slots and by every fc_refactor: the export needs THIS slot's elimination in it, so the
  // elimination runs again (deterministic: the direct values, the permuted matrix and the batch's tiled copy come out bit for bit
  // as they were) and fc_refactor's hook (adjoint_after_refactor) exports behind it.  What the caller can ask of the last
  // factorisation (its time, its flops) is kept.
  const double ms0 = h->refactor_ms[slot], fl0 = h->refactor_flops, fl1 = h->refactor_flops_full;
  const int code = fc_refactor(h, slot, nullptr);
  h->refactor_ms[slot] = ms0, h->refactor_flops = fl0, h->refactor_flops_full = fl1;
  if (code != FC_OK || T.stale) {
    adj_drop(h, slot);
    if (!A.s[0].avail && !A.s[1].avail) adj_release_shared(A);
    return code != FC_OK ? code : fail(FC_ERR_INVALID, "fc_set_adjoint_factors: the slot's layout does not take a transposed export");
  }
  return FC_OK;
}

int fc_adjoint_info(fc_handle h, int slot, int64_t* info, double* dinfo) {
  if (!h || slot < 0 || slot > 1) return fail(FC_ERR_INVALID, "fc_adjoint_info: bad argument");
  const fc_ctx::Adj::Slot& T = h->adj.s[slot];
  if (info) {
    info[0] = T.avail ? 1 : 0;
    info[1] = T.stale ? 1 : 0;
    info[2] = (T.avail && T.use) ? 1 : 0;
    info[3] = adj_slot_bytes(T);
    info[4] = adj_shared_bytes(h->adj);
    info[5] = T.n_export;
    info[6] = info[7] = 0;
  }
  if (dinfo) {
    dinfo[0] = T.export_ms;
    dinfo[1] = h->adj.run_ms;
  }
  return FC_OK;
}

// ── state tape of single steps (fc_ctx::StateTape; the shared bodies in fc_adjoint_march.hpp) ──────────────────────────────────────
static int adj_tape_reserve(fc_handle h, const char* who, int32_t capacity, int32_t every, bool sparse) {
  const bool some = capacity > 0 && every > 0;
  FCCHK(stape_reserve_refusal(h, who, capacity, sparse ? every : 0, some));
  if (some && h->bat.k > 0) return fail(FC_ERR_INVALID, std::string(who) + ": the handle has a batch set (fc_set_batch): batched steps are not taped");
  return stape_reserve(h, h->adj.st, who, capacity, every, sparse, adj_tape_layout(h));
}
int fc_adjoint_tape_reserve(fc_handle h, int32_t capacity) { return adj_tape_reserve(h, "fc_adjoint_tape_reserve", capacity, capacity, false); }
int fc_adjoint_tape_reserve_sparse(fc_handle h, int32_t capacity, int32_t every) { return adj_tape_reserve(h, "fc_adjoint_tape_reserve_sparse", capacity, every, true); }

int fc_adjoint_tape_begin(fc_handle h) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_tape_begin: null handle");
  fc_ctx::StateTape& T = h->adj.st;
  if (T.sg.capacity == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_tape_begin: no state tape (fc_adjoint_tape_reserve)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_tape_begin: collect the step in flight first (fc_step_end)");
  if (!h->have_perm || !h->state_live || T.col != (size_t)h->N)
    return fail(FC_ERR_NOT_READY, "fc_adjoint_tape_begin: the handle holds no state on the device yet (fc_setup_solver, fc_set_state)");
  return stape_begin(h, T, "fc_adjoint_tape_begin", "fc_adjoint_tape_reserve_sparse", st_nn(h), st_n(h));
}

int fc_adjoint_tape_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_adjoint_tape_info: null argument");
  const fc_ctx::StateTape& T = h->adj.st;
  stape_info(T, info);
  info[6] = T.every_reported(), info[7] = T.replayed;  // (a dense tape reports no `every`, and its marches replay nothing)
  return FC_OK;
}

// columns [col0, col0 + ncol) of the checkpointed tape's segment buffer as they sit on the device (permuted numbering; test aid).
// `segment` receives the segment the buffer holds: column i + 1 is x_{segment * every + i}.
int fc_debug_get_adjoint_segment(fc_handle h, int32_t col0, int32_t ncol, double* out, int32_t* segment) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_segment: null argument");
  const fc_ctx::StateTape& A = h->adj.st;
  if (!A.sparse || !A.sg.begun) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_segment: no begun checkpointed state tape (fc_adjoint_tape_reserve_sparse / fc_adjoint_tape_begin)");
  if (col0 < 0 || ncol <= 0 || col0 + ncol > A.sg.buffer_columns())
    return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_segment: columns beyond the " + std::to_string(A.sg.buffer_columns()) + " the segment buffer has");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipMemcpyAsync(out, A.tape.p + (size_t)h->N * col0, (size_t)h->N * ncol * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (segment) *segment = A.sg.resident;
  return FC_OK;
}

// the handle's step counters (single steps; batched steps) -- test aid: a march that replays forward steps must leave them alone
int fc_debug_get_step_count(fc_handle h, int64_t* single, int64_t* batched) {
  if (!h) return fail(FC_ERR_INVALID, "fc_debug_get_step_count: null handle");
  if (single) *single = (int64_t)h->step_count;
  if (batched) *batched = (int64_t)h->bat.step_count;
  return FC_OK;
}

// columns [col0, col0 + ncol) of the tape as they sit on the device (permuted numbering; test aid)
int fc_debug_get_adjoint_tape(fc_handle h, int32_t col0, int32_t ncol, double* out) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_tape: null argument");
  const fc_ctx::StateTape& A = h->adj.st;
  if (A.sparse || !A.sg.begun) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_tape: no begun state tape (fc_adjoint_tape_reserve / fc_adjoint_tape_begin)");
  if (col0 < 0 || ncol <= 0 || col0 + ncol > A.sg.count() + 2) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_tape: columns beyond the " + std::to_string(A.sg.count() + 2) + " the tape holds");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipMemcpyAsync(out, A.tape.p + (size_t)h->N * col0, (size_t)h->N * ncol * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return FC_OK;
}

int fc_debug_get_adjoint_factors(fc_handle h, int slot, int64_t n, double* out) {
  if (!h || slot < 0 || slot > 1 || !out) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_factors: bad argument");
  const fc_ctx::Adj::Slot& T = h->adj.s[slot];
  if (!T.avail || T.stale) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_factors: no current transposed factors (fc_set_adjoint_factors)");
  if (n != h->sys[slot].f_nnz || (size_t)n > T.f_t.n) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_factors: size differs from the slot's factors");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(out, T.f_t.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return FC_OK;
}

int fc_solve_transposed(fc_handle h, int slot, const double* b, double* x, double* info_out) {
  if (!h || slot < 0 || slot > 1 || !b || !x) return fail(FC_ERR_INVALID, "fc_solve_transposed: bad argument");
  FCCHK(adj_usable(h, slot, "fc_solve_transposed"));
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_solve_transposed: collect the step in flight first (fc_step_end)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  AdjUse use(h, slot, false);  // (solve_once synchronises before it returns: nothing is in flight when the arrays go back)
  return solve_once(h, slot, b, x, info_out);
}

int fc_adjoint_reset(fc_handle h, const double* z_terminal) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_reset: null handle");
  if (!h->adj.s[0].avail && !h->adj.s[1].avail) return fail(FC_ERR_NOT_READY, "fc_adjoint_reset: no transposed factors (fc_set_adjoint_factors)");
  if (!h->have_perm) return fail(FC_ERR_NOT_READY, "fc_adjoint_reset: no permutation");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(adj_march_setup(h, -1));
  return adj_reset(h, z_terminal);
}

int fc_step_adjoint(fc_handle h, int slot, double cm_n, double cm_nn_next, const double* w, double* g_out) {
  if (!h || slot < 0 || slot > 1) return fail(FC_ERR_INVALID, "fc_step_adjoint: bad argument");
  if (h->n_act > 0 && !g_out) return fail(FC_ERR_INVALID, "fc_step_adjoint: g_out is null");
  if (h->adjen.source == 1)
    return fail(FC_ERR_INVALID, "fc_step_adjoint: the energy source is the tangent tape (fc_set_adjoint_energy_source): a single backward step reads no tape "
                                "(fc_run_adjoint, or set the source back to 0)");
  if (h->adjen.n > 0)
    return fail(FC_ERR_INVALID, "fc_step_adjoint: energy weights are held (fc_set_adjoint_energy): the energy term reads the forward trajectory, and a single "
                                "backward step carries no state (fc_run_adjoint, or clear the weights)");
  FCCHK(adj_step_ready(h, slot, "fc_step_adjoint"));
  FCCHK(adj_march_prepare(h, slot, 1, 0));
  fc_ctx::Adj& A = h->adj;
  int flag = 0;
  const double* d_w = (w && h->n_sens > 0) ? A.wseq.p : nullptr;
  FCCHK(adj_enqueue_and_sync(h, "fc_step_adjoint", nullptr, [&]() -> int {
    if (d_w) HIPCHK(hipMemcpyAsync(A.wseq.p, w, (size_t)h->n_sens * sizeof(double), hipMemcpyHostToDevice, h->stream));
    FCCHK(adj_enqueue_step(h, slot, StepCoeffs{cm_n, cm_nn_next, 0.0, 0.0}, nullptr, d_w, A.gseq.p));
    if (h->n_act > 0) HIPCHK(hipMemcpyAsync(g_out, A.gseq.p, (size_t)h->n_act * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&flag, A.flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return FC_OK;
  }));
  if (flag) return fail(FC_ERR_DIVERGED, "fc_step_adjoint: non-finite adjoint state after the solve");
  return FC_OK;
}

int fc_adjoint_mass_product(fc_handle h, double cm_n, double cm_nn, double* out) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_adjoint_mass_product: null argument");
  if (!h->adj.march_ok || !h->adj.ct_ok) return fail(FC_ERR_NOT_READY, "fc_adjoint_mass_product: no adjoint march yet (fc_adjoint_reset / fc_step_adjoint)");
  if (h->nonlinear)
    return fail(FC_ERR_INVALID, "fc_adjoint_mass_product: the time scheme is nonlinear: the state gradients need the taped trajectory, which only fc_run_adjoint reads");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  return adj_enqueue_and_sync(h, "fc_adjoint_mass_product", nullptr, [&] { return adj_enqueue_mass_product(h, StepCoeffs{cm_n, cm_nn, 0.0, 0.0}, nullptr, 0, out); });
}

int fc_run_adjoint(fc_handle h, int first_order_slot, int32_t n_steps, const double* w_seq, const double* z_terminal, double* g_seq,
                   double* dx0, double* dxm1) {
  if (!h) return fail(FC_ERR_INVALID, "fc_run_adjoint: null handle");
  if (n_steps <= 0) return fail(FC_ERR_INVALID, "fc_run_adjoint: n_steps must be positive");
  if (h->n_act > 0 && !g_seq) return fail(FC_ERR_INVALID, "fc_run_adjoint: g_seq is null");
  if (first_order_slot != FC_SLOT_BDF1 && first_order_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, "order_slot must be BDF1/BDF2");
  const char* who = "fc_run_adjoint";
  const bool nl = h->nonlinear;
  const char* remedy = "fc_adjoint_tape_reserve, then fc_adjoint_tape_begin before the forward fc_run";
  const bool taped = nl || h->adjen.n > 0;  // (energy weights: a linearised handle marches over its taped run too)
  fc_ctx::Adj& A = h->adj;
  fc_ctx::StateTape& T = A.st;
  FCCHK(adj_tape_refusal(h, who, T, n_steps, first_order_slot, "state tape", remedy));
  FCCHK(adjen_march_check(h, who, nl, n_steps, 0, T, first_order_slot));
  FCCHK(adj_step_ready(h, first_order_slot, who, nl));
  if (n_steps > 1 && first_order_slot != FC_SLOT_BDF2) FCCHK(adj_step_ready(h, FC_SLOT_BDF2, who, nl));
  FCCHK(adj_march_prepare(h, first_order_slot, n_steps, 0));
  bool replays = false;  // (a taped march walks the tape's segments and recomputes all but the buffer's)
  FCCHK(stape_march_begin(T, taped, n_steps, adj_tape_layout(h), &replays));
  const bool have_w = w_seq && h->n_sens > 0;
  int flag = 0, rflags[2] = {0, 0};
  AdjReplayHost forward_state(h, replays);
  const AdjReplay replay = adj_replay_single(h, n_steps, rflags);
  const int code = adj_enqueue_and_sync(h, who, &A.run_ms, [&]() -> int {
    if (have_w) HIPCHK(hipMemcpyAsync(A.wseq.p, w_seq, (size_t)n_steps * h->n_sens * sizeof(double), hipMemcpyHostToDevice, h->stream));
    FCCHK(adj_reset(h, z_terminal));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    FCCHK(adj_march(
        h, first_order_slot, n_steps, taped ? T.tape.p : nullptr, T.col, dx0, dxm1,
        [&](int m, int slot, const StepCoeffs& c, const double* xm, const double* er) {
          return adj_enqueue_step(h, slot, c, xm, have_w ? A.wseq.p + (size_t)(m - 1) * h->n_sens : nullptr, A.gseq.p + (size_t)(m - 1) * h->n_act, er,
                                  adjen_source_column(h, m));
        },
        [&](const StepCoeffs& c, const double* xm, int which, double* dst) { return adj_enqueue_mass_product(h, c, xm, which, dst); }, nullptr,
        taped ? &replay : nullptr));
    if (h->n_act > 0) HIPCHK(hipMemcpyAsync(g_seq, A.gseq.p, (size_t)n_steps * h->n_act * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&flag, A.flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return FC_OK;
  });
  FCCHK(taped ? stape_verdict(T, who, n_steps, 1, code, rflags) : code);
  if (flag) return fail(FC_ERR_DIVERGED, "fc_run_adjoint: non-finite adjoint state after a solve");
  return FC_OK;
}

}  // extern "C"
