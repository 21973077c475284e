// fc_adjoint_batch_run.hpp -- host side of the batched adjoint march (fc_set_adjoint_batch, fc_solve_transposed_batch,
// fc_run_adjoint_batch, fc_adjoint_tape_*_batch, fc_adjoint_batch_info; kernels in fc_adjoint_batch.hip.h).  Included at
// the end of fc_hip.hip, behind fc_adjoint_run.hpp; preamble, step loop and exit of the march are fc_adjoint_march.hpp's.
//
// The transposed solve of k columns is batch_apply on a tiled copy of the slot's transposed factor values (Adj::Slot::f_t through
// fc_b_repack, into an array of its own): that array and the march's work buffer are handed to batch_apply as arguments, so
// Batch::ftile and Batch::buf are not read.  The batch's state ring, Batch::ftile, graphs and step counter never see the march; the
// apply's own scratch (the partial slots and arrival counters of split tiles, Batch::part / Batch::ticket) is shared with the forward
// steps, which is safe because every march is enqueued behind a quiesce on the one main stream and synchronises before it returns.
// The tables that do not depend on the width -- the sensor table by row and the slot's control columns B~ -- are the single march's
// (adj_march_setup).
#pragma once

namespace {

inline int adjb_tail_grid(int N, int KB) { return std::min(1024, nblocks(N, 256 / KB)); }

// why the handle cannot run a batched adjoint call on `slot`; FC_OK if it can
int adjb_usable(fc_ctx* h, int slot, int32_t k, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (h->bat.k == 0) return fail(FC_ERR_NOT_READY, w + "fc_set_batch not called");
  if (k != h->bat.k) return fail(FC_ERR_INVALID, w + "k differs from fc_set_batch");
  if (h->method != FC_METHOD_REFINE || h->max_iter != 0)
    return fail(FC_ERR_INVALID, w + "the batched march applies the factors directly (FC_METHOD_REFINE, no refinement sweeps: fc_set_solver_options refine = 0)");
  FCCHK(adj_usable(h, slot, who));  // (partitioned, factor-free, compressed, truncated, inexact: FC_ERR_INVALID with the reason)
  if (!h->bat.tables || h->bat.tasks.n == 0) return fail(FC_ERR_NOT_READY, w + "the batch has no apply tables (fc_set_batch after fc_setup_solver)");
  if (!h->adjb.on[slot]) return fail(FC_ERR_NOT_READY, w + "no batched adjoint setup for this slot (fc_set_adjoint_batch)");
  return FC_OK;
}

// the tiled copy of the slot's transposed values is current (one fc_b_repack launch if it is not)
int adjb_repack(fc_ctx* h, int slot) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  if (A.tile_ok[slot] && A.ttile[slot].n == (size_t)B.tiled_values) return FC_OK;
  if (A.ttile[slot].n != (size_t)B.tiled_values) FCCHK(A.ttile[slot].alloc((size_t)B.tiled_values));
  hipLaunchKernelGGL(fc_b_repack, dim3((unsigned)B.tasks.n), dim3(256), 0, h->stream, B.tasks.p, (const double*)h->adj.s[slot].f_t.p, A.ttile[slot].p);
  HIPCHK(hipGetLastError());
  A.tile_ok[slot] = true;
  ++A.n_repack[slot];
  return FC_OK;
}

// the march's [row][KB] buffers (once per width / structure)
int adjb_buffers(fc_ctx* h) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const size_t N = (size_t)h->N, KB = (size_t)B.KB;
  const size_t wd = batch_slot_doubles(B, N, B.KB);
  const int na = std::max(1, h->n_act);
  const size_t part_n = (size_t)na * KB * adjb_tail_grid(h->N, B.KB);  // (the tail's partials: per actuator, simulation and workgroup)
  if (A.march_ok && A.KB == B.KB && A.work_doubles == wd && A.ev.n == (size_t)12 * h->nc * KB && A.part.n == part_n) return FC_OK;
  FCCHK(A.work.alloc(wd));
  FCCHK(A.b.alloc(N * KB));
  FCCHK(A.zm.alloc(2 * N * KB));
  FCCHK(A.ev.alloc((size_t)12 * h->nc * KB));
  FCCHK(A.term.alloc(N * KB));
  FCCHK(A.part.alloc(part_n));
  FCCHK(A.flag.alloc(32));
  for (DevBuf<double>* d : {&A.work, &A.b, &A.zm, &A.ev, &A.term, &A.part}) FCCHK(d->zero(h->stream));
  FCCHK(A.flag.zero(h->stream));
  A.KB = B.KB;
  A.work_doubles = wd;
  A.zm_cur = 0;
  A.march_ok = true;
  h->adj_route = fc_ctx::AdjRoute{};  // (the buffers the last step's record points into are gone)
  return FC_OK;
}

int64_t adjb_march_bytes(const fc_ctx::AdjB& A) {
  return 8 * (int64_t)(A.work.n + A.b.n + A.zm.n + A.ev.n + A.term.n + A.part.n + A.wseq.n + A.gseq.n + A.stage.n) + 4 * (int64_t)A.flag.n +
         8 * (int64_t)(A.st.ring_save.n + A.st.scratch.n) + 4 * (int64_t)A.st.rflag.n;  // (what the replays of a checkpointed tape borrow, as adj_shared_bytes)
}

// host [k][N] (W layout) -> device [N][KB] (permuted numbering, columns >= k zero), staged through `stage` (k N doubles at `off`)
int adjb_upload(fc_ctx* h, const double* host, size_t off, double* dev) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const size_t n = (size_t)B.k * h->N;
  HIPCHK(hipMemcpyAsync(A.stage.p + off, host, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  pick_width(B.KB, [&](auto K) {
    hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)h->N * B.KB, 256)), dim3(256), 0, h->stream, h->N, B.k, (const double*)(A.stage.p + off), dev, 1,
                       (const int*)h->perm.p);
  });
  HIPCHK(hipGetLastError());
  return FC_OK;
}
// device [N][KB] -> host [k][N] (W layout); the copy is enqueued, the caller synchronises
int adjb_download(fc_ctx* h, const double* dev, size_t off, double* host) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const size_t n = (size_t)B.k * h->N;
  pick_width(B.KB, [&](auto K) {
    hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)h->N * B.KB, 256)), dim3(256), 0, h->stream, h->N, B.k, dev, A.stage.p + off, 0, (const int*)h->perm.p);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host, A.stage.p + off, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}

// M Z (cm_n zm_cur + cm_nn zm_prev) (+ J(xm)^T Z (cc_n zm_cur + cc_nn zm_prev)) (+ C^T w) (+ term) of every column into the march's
// right-hand side and the y half of its work buffer.  xm: the taped state [N][KB] (nonlinear handles), d_w: [k][n_sens] or null.
// `er`: the device energy weights [KB] of this backward step (adjen_row), or null: no energy term (no rows held, the dx0 / dxm1
// products, since dE_0 is not in the sum).
int adjb_enqueue_rhs(fc_ctx* h, const StepCoeffs& c, const double* xm, const double* d_w, const double* d_term, const double* er = nullptr) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const int N = h->N, KB = B.KB, nc = h->nc;
  const size_t lvl = (size_t)N * KB;
  const double* z1 = A.zm.p + (size_t)A.zm_cur * lvl;
  const double* z2 = A.zm.p + (size_t)(1 - A.zm_cur) * lvl;
  const int g_elem = nblocks(nc, 256 / KB);
  fc_ctx::AdjRoute& R = h->adj_pend;
  R = fc_ctx::AdjRoute{};
  if (er && !xm) return fail(FC_ERR_INVALID, "batched adjoint: the energy term needs a taped state");
  R.elem = h->nonlinear ? (er ? FC_ADJ_ELEM_NL_B_EN : FC_ADJ_ELEM_NL_B) : (er ? FC_ADJ_ELEM_EN_B : FC_ADJ_ELEM_BREG);
  R.g_elem = g_elem, R.g_gather = nblocks((int64_t)N * (KB / 2), 256);
  R.have_w = (h->n_sens > 0 && d_w) ? 1 : 0, R.have_term = d_term ? 1 : 0;
  R.KB = KB, R.k = B.k;
  h->adj_route.b_live = false;  // (the last step's right-hand side is gone; adjb_enqueue_step commits this one)
  if (!h->nonlinear && er) {
    pick_width(KB, [&](auto K) {
      hipLaunchKernelGGL((fc_adj_elem_en_b<K>), dim3(g_elem), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, xm, z1, z2, c.cm_n,
                         c.cm_nn, er, A.ev.p);
    });
    ++h->adjen.steps;
  } else if (!h->nonlinear) {
    // the forward batched loop on the two masked levels, no convection, no body force
    pick_width(KB, [&](auto K) {
      hipLaunchKernelGGL((fc_rhs_elem_breg<K, false>), dim3(g_elem), dim3(256), 0, h->stream, nc, h->nn, (const int*)h->cn.p, (const int*)h->cnp.p,
                         (const double*)h->geom.p, z1, z2, (const double*)nullptr, 0, (const double*)nullptr, 0, c.cm_n, c.cm_nn, 0.0, 0.0, A.ev.p);
    });
  } else {
    if (!xm) return fail(FC_ERR_INVALID, "batched adjoint: the nonlinear element loop needs a taped state");
    pick_width(KB, [&](auto K) {
      pick_bool(er != nullptr, [&](auto EN) {
        hipLaunchKernelGGL((fc_adj_elem_nl_b<K, EN>), dim3(g_elem), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, xm, z1, z2,
                           c.cm_n, c.cm_nn, c.cc_n, c.cc_nn, er, A.ev.p);
      });
    });
    if (er) ++h->adjen.steps;
  }
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL((fc_adj_rhs_gather_b<K>), dim3(nblocks((int64_t)N * (K / 2), 256)), dim3(256), 0, h->stream, N, B.k, (const int*)h->gptr_p.p,
                       (const int*)h->gidx_p.p, (const double*)A.ev.p, (const int*)h->adj.ct_ptr.p, (const int*)h->adj.ct_sens.p, (const double*)h->adj.ct_w.p,
                       h->n_sens, h->n_sens > 0 ? d_w : (const double*)nullptr, d_term, A.b.p, A.work.p);
  });
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// one backward step of all columns on `slot`: right-hand side, transposed block solve, tail (g -> d_g [k][n_act], flags, masked copy).
// reduce = false leaves the tail's partials (AdjB::part, adjb_tail_grid workgroups) to the caller: the closed-loop march sums them in
// its controller launch.
int adjb_enqueue_step(fc_ctx* h, int slot, const StepCoeffs& c, const double* xm, const double* d_w, const double* d_term, double* d_g, bool reduce = true,
                      const double* er = nullptr) {
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const int N = h->N, KB = B.KB;
  const size_t lvl = (size_t)N * KB;
  FCCHK(adjb_enqueue_rhs(h, c, xm, d_w, d_term, er));
  FCCHK(batch_apply(h, slot, false, A.ttile[slot].p, A.work.p));
  const int g = adjb_tail_grid(N, KB);
  double* znew = A.zm.p + (size_t)(1 - A.zm_cur) * lvl;  // (mu_{m+2}'s copy was read by the element loop above: its place is free)
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL((fc_adj_tail_b<K>), dim3(g), dim3(256), 0, h->stream, N, (const double*)(A.work.p + lvl), (const int*)h->bcslot_p.p, h->n_act,
                       (const double*)h->adj.s[slot].bt.p, znew, A.flag.p, A.part.p);
  });
  if (h->n_act > 0 && reduce) hipLaunchKernelGGL(fc_adj_reduce_b, dim3(h->n_act * B.k), dim3(64), 0, h->stream, h->n_act, B.k, KB, g, (const double*)A.part.p, d_g);
  HIPCHK(hipGetLastError());
  A.zm_cur = 1 - A.zm_cur;
  fc_ctx::AdjRoute& R = h->adj_pend;
  R.g_tail = g, R.passes = std::max(1, (h->n_act + 3) / 4);
  R.reduced = (h->n_act > 0 && reduce) ? 1 : 0, R.gx = R.reduced ? g : 0;
  R.slot = slot, R.x = A.work.p + lvl, R.dx = nullptr, R.b_live = true, R.have = true;
  h->adj_route = R;
  return FC_OK;
}

// what a batched backward step needs of the handle and the slot
int adjb_step_ready(fc_ctx* h, int slot, int32_t k, const char* who) {
  FCCHK(check_step_ready(h, slot));
  if (h->sys[slot].have_c) return fail(FC_ERR_INVALID, std::string(who) + ": the slot has an explicit right-hand-side operator (Crank-Nicolson)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": collect the step in flight first (fc_step_end / fc_step_batch_end)");
  return adjb_usable(h, slot, k, who);
}

// mu_{n+1} = mu_{n+2} = 0 in every column; the terminal vectors ([k][N], host) wait in AdjB::term for the first backward step
int adjb_reset(fc_ctx* h, const double* z_terminal) {
  fc_ctx::AdjB& A = h->adjb;
  FCCHK(A.zm.zero(h->stream));
  FCCHK(A.flag.zero(h->stream));
  A.zm_cur = 0;
  if (z_terminal) FCCHK(adjb_upload(h, z_terminal, 0, A.term.p));
  return FC_OK;
}

// a batched march's state gradient `which` (0: dx0, 1: dxm1; adj_march) of every column, [N][KB] -> [k][N] in the W layout, into the
// caller's `dst`; the copy is enqueued, the caller synchronises
int adjb_state_gradient(fc_ctx* h, const StepCoeffs& c, const double* xm, int which, double* dst) {
  FCCHK(adjb_enqueue_rhs(h, c, xm, nullptr, nullptr));
  return adjb_download(h, h->adjb.b.p, which == 0 ? 0 : (size_t)h->bat.k * h->N, dst);
}

// ── replays of the batched marches over a checkpointed state tape (DESIGN §5.4 "Checkpointed tape") ────────────────────────────────────────
// The host side of the batched stepper while replays are enqueued (AdjReplayHost): ring cursor, right-hand side in use, record page,
// monitor flag, route records and the debug capture as on entry when this goes out of scope; what a step had gathered ahead is gone.
struct AdjbReplayHost {
  fc_ctx* h;
  bool on;
  int cur;
  double *b, *rec_dev;
  bool pend_checked, cap_on;
  fc_ctx::Batch::Route route, rpend;
  AdjbReplayHost(fc_ctx* h_, bool on_)
      : h(h_), on(on_), cur(h_->bat.cur), b(h_->bat.b.p), rec_dev(h_->bat.rec_dev), pend_checked(h_->bat.pend_checked), cap_on(h_->bat.cap_on),
        route(h_->bat.route), rpend(h_->bat.rpend) {}
  ~AdjbReplayHost() {
    if (!on) return;
    fc_ctx::Batch& B = h->bat;
    B.cur = cur;
    bat_point(h);
    B.b.p = b, B.rec_dev = rec_dev, B.pend_checked = pend_checked, B.cap_on = cap_on;
    B.route = route, B.rpend = rpend;
    B.pre_slot = -1, B.pre_gather = false;  // (the replays' element loops and gathers wrote the buffers a step had filled ahead)
  }
  AdjbReplayHost(const AdjbReplayHost&) = delete;
  AdjbReplayHost& operator=(const AdjbReplayHost&) = delete;
};

// the batched tape's layout: columns of N KB doubles, KB control rows per step, 64 flag words; a replay borrows the batch's ring and a record page
StapeLayout adjb_tape_layout(const fc_ctx* h) {
  return StapeLayout{(size_t)h->N * (size_t)h->bat.KB, h->bat.KB, h->bat.KB, 64, h->bat.ring.n, (size_t)fc_rec::kPinDoubles};
}
// What the two batched marches hand adj_march on a checkpointed tape (adj_replay_single).  A replayed step is batch_launches on the
// step's order slot in its plain form -- element loop, full gather, factor apply, tail on one stream, no residual monitor, no energy,
// nothing run ahead for a next step -- reading the taped control rows from a record page of the march's own, where it also publishes.
// `flags`: [0, 32) the forward non-finite flags as the march found them, [32, 64) as the replays left them.
int adjb_replay_begin(fc_ctx* h) {
  fc_ctx::StateTape& A = h->adjb.st;
  fc_ctx::Batch& B = h->bat;
  FCCHK(A.scratch.zero(h->stream));
  FCCHK(A.rflag.zero(h->stream));
  const size_t nf = std::min<size_t>(32, B.flag.n);
  HIPCHK(hipMemcpyAsync(A.ring_save.p, B.ring.p, B.ring.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(A.rflag.p, B.flag.p, nf * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemsetAsync(B.flag.p, 0, nf * sizeof(int), h->stream));
  return FC_OK;
}
int adjb_replay_segment(fc_ctx* h, int j, int n_steps) {
  fc_ctx::StateTape& A = h->adjb.st;
  fc_ctx::Batch& B = h->bat;
  const FcAdjointSegments& sg = A.sg;
  const int KB = B.KB, na = h->n_act;
  const size_t col = (size_t)h->N * (size_t)KB;
  const double* pair = A.ckpt.p + 2 * col * (size_t)j;
  FCCHK(stape_copy(h, A, col, pair, bat_nn(h)));
  FCCHK(stape_copy(h, A, col, pair + col, bat_n(h)));
  FCCHK(stape_copy(h, A, 2 * col, pair, A.tape.p));
  B.rec_dev = A.scratch.p;
  B.pend_checked = false;
  B.cap_on = false;
  for (int m = sg.seg_first(j); m <= sg.seg_last(j, n_steps); ++m) {
    if (na > 0) {
      const double* row = A.ctape.p + (size_t)(m - 1) * (size_t)KB * 2 * (size_t)na;
      hipLaunchKernelGGL(fc_adj_ctrl_rows, dim3(1), dim3(256), 0, h->stream, KB, na, row, row + na, 2 * na, A.scratch.p + fc_rec::kCtrl, A.scratch.p + fc_rec::kForce,
                         (int)fc_rec::kRecStride);
    }
    B.b.p = B.bstore.p;
    B.pre_slot = -1, B.pre_gather = false;
    B.rpend = fc_ctx::Batch::Route{};
    FCCHK(batch_launches(h, sg.slots[(size_t)m - 1], 0, 2, -1, false, false));
    B.cur = (B.cur + 1) % 4;
    bat_point(h);
    FCCHK(stape_copy(h, A, col, bat_n(h), A.tape.p + col * (size_t)sg.local_column(m + 1, j)));
    ++A.replayed;
  }
  return FC_OK;
}
int adjb_replay_end(fc_ctx* h, int* flags) {
  fc_ctx::StateTape& A = h->adjb.st;
  fc_ctx::Batch& B = h->bat;
  const size_t nf = std::min<size_t>(32, B.flag.n);
  HIPCHK(hipMemcpyAsync(A.rflag.p + 32, B.flag.p, nf * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(B.flag.p, A.rflag.p, nf * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(B.ring.p, A.ring_save.p, B.ring.n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(flags, A.rflag.p, 64 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}
AdjReplay adjb_replay(fc_ctx* h, int n_steps, int* flags) { return AdjReplay{&h->adjb.st.sg, n_steps, flags, adjb_replay_begin, adjb_replay_segment, adjb_replay_end}; }

}  // namespace

extern "C" {

int fc_set_adjoint_batch(fc_handle h, int slot, int32_t on) {
  if (!h || slot < 0 || slot > 1 || (on != 1 && on != -1)) return fail(FC_ERR_INVALID, "fc_set_adjoint_batch: slot must be 0 / 1 and on 1 (build) or -1 (free)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_set_adjoint_batch: collect the step in flight first (fc_step_end / fc_step_batch_end)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  fc_ctx::AdjB& A = h->adjb;
  if (on == -1) {
    HIPCHK(hipStreamSynchronize(h->stream));
    A.ttile[slot].release();
    A.on[slot] = A.tile_ok[slot] = false;
    A.n_repack[slot] = 0;
    if (!A.on[0] && !A.on[1]) {
      A.work.release(), A.b.release(), A.zm.release(), A.ev.release(), A.term.release(), A.part.release(), A.wseq.release(), A.gseq.release();
      A.stage.release(), A.flag.release();
      A.march_ok = false;
      A.KB = 0, A.work_doubles = 0;
    }
    return FC_OK;
  }
  if (h->bat.k == 0) return fail(FC_ERR_NOT_READY, "fc_set_adjoint_batch: fc_set_batch not called");
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, "fc_set_adjoint_batch: partitioned handles are not supported");
  if (h->method != FC_METHOD_REFINE || h->max_iter != 0)
    return fail(FC_ERR_INVALID, "fc_set_adjoint_batch: the batched march applies the factors directly (FC_METHOD_REFINE, no refinement sweeps: fc_set_solver_options refine = 0)");
  FCCHK(adj_usable(h, slot, "fc_set_adjoint_batch"));
  if (!h->bat.tables || h->bat.tasks.n == 0) return fail(FC_ERR_NOT_READY, "fc_set_adjoint_batch: the batch has no apply tables (fc_set_batch after fc_setup_solver)");
  A.on[slot] = true;
  int code = adjb_repack(h, slot);
  if (code == FC_OK) code = adjb_buffers(h);
  if (code == FC_OK && hipStreamSynchronize(h->stream) != hipSuccess) code = fail(FC_ERR_HIP, "fc_set_adjoint_batch: the repack failed");
  if (code != FC_OK) {
    A.ttile[slot].release();
    A.on[slot] = A.tile_ok[slot] = false;
  }
  return code;
}

int fc_adjoint_batch_info(fc_handle h, int slot, int64_t* info, double* dinfo) {
  if (!h || slot < 0 || slot > 1) return fail(FC_ERR_INVALID, "fc_adjoint_batch_info: bad argument");
  const fc_ctx::AdjB& A = h->adjb;
  if (info) {
    info[0] = A.on[slot] ? 1 : 0;
    info[1] = (A.on[slot] && !A.tile_ok[slot]) ? 1 : 0;
    info[2] = 8 * (int64_t)A.ttile[slot].n;
    info[3] = adjb_march_bytes(A);
    info[4] = A.st.tape_bytes();  // (a checkpointed tape: buffer, pairs and control tape, as _info_batch [3])
    info[5] = A.n_repack[slot];
    info[6] = A.KB;
    info[7] = A.st.replayed;  // forward steps the last march over a checkpointed batched tape recomputed
  }
  if (dinfo) dinfo[0] = A.run_ms, dinfo[1] = 0.0;
  return FC_OK;
}

// parity hook: A_slot^T X = B for k right-hand sides through the batched factor apply on the tiled transposed values (B, X: [k][N], W numbering)
int fc_solve_transposed_batch(fc_handle h, int slot, int32_t k, const double* b, double* x) {
  if (!h || slot < 0 || slot > 1 || !b || !x) return fail(FC_ERR_INVALID, "fc_solve_transposed_batch: bad argument");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_solve_transposed_batch: collect the step in flight first");
  FCCHK(adjb_usable(h, slot, k, "fc_solve_transposed_batch"));
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(adjb_repack(h, slot));
  FCCHK(adjb_buffers(h));
  fc_ctx::AdjB& A = h->adjb;
  const size_t n = (size_t)k * h->N;
  if (A.stage.n < 2 * n) FCCHK(A.stage.alloc(2 * n));
  return adj_enqueue_and_sync(h, "fc_solve_transposed_batch", nullptr, [&]() -> int {
    FCCHK(adjb_upload(h, b, 0, A.work.p));
    FCCHK(batch_apply(h, slot, false, A.ttile[slot].p, A.work.p));
    return adjb_download(h, A.work.p + (size_t)h->N * h->bat.KB, 0, x);
  });
}

// ── state tape of batched steps (fc_ctx::StateTape; the shared bodies in fc_adjoint_march.hpp) ─────────────────────────────────────
static int adjb_tape_reserve(fc_handle h, const char* who, const char* single, int32_t capacity, int32_t every, bool sparse) {
  const bool some = capacity > 0 && every > 0;
  FCCHK(stape_reserve_refusal(h, who, capacity, sparse ? every : 0, some));
  if (some && h->bat.k == 0) return fail(FC_ERR_NOT_READY, std::string(who) + ": fc_set_batch not called (the single run's tape: " + single + ")");
  return stape_reserve(h, h->adjb.st, who, capacity, every, sparse, adjb_tape_layout(h));
}
int fc_adjoint_tape_reserve_batch(fc_handle h, int32_t capacity) {
  return adjb_tape_reserve(h, "fc_adjoint_tape_reserve_batch", "fc_adjoint_tape_reserve", capacity, capacity, false);
}
int fc_adjoint_tape_reserve_sparse_batch(fc_handle h, int32_t capacity, int32_t every) {
  return adjb_tape_reserve(h, "fc_adjoint_tape_reserve_sparse_batch", "fc_adjoint_tape_reserve_sparse", capacity, every, true);
}

int fc_adjoint_tape_begin_batch(fc_handle h) {
  if (!h) return fail(FC_ERR_INVALID, "fc_adjoint_tape_begin_batch: null handle");
  fc_ctx::StateTape& T = h->adjb.st;
  if (T.sg.capacity == 0) return fail(FC_ERR_NOT_READY, "fc_adjoint_tape_begin_batch: no batched state tape (fc_adjoint_tape_reserve_batch)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_adjoint_tape_begin_batch: collect the step in flight first (fc_step_batch_end)");
  if (h->bat.k == 0 || !h->have_perm || T.KB != h->bat.KB || T.col != (size_t)h->N * (size_t)h->bat.KB)
    return fail(FC_ERR_NOT_READY, "fc_adjoint_tape_begin_batch: the tape was laid out for another batch (fc_adjoint_tape_reserve_batch after fc_set_batch)");
  return stape_begin(h, T, "fc_adjoint_tape_begin_batch", "fc_adjoint_tape_reserve_sparse_batch", bat_nn(h), bat_n(h));
}

int fc_adjoint_tape_info_batch(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_adjoint_tape_info_batch: null argument");
  const fc_ctx::StateTape& T = h->adjb.st;
  stape_info(T, info);
  info[6] = T.KB, info[7] = T.every_reported();  // (one free slot: the replayed steps of the last march are fc_adjoint_batch_info's info[7])
  return FC_OK;
}

// columns [col0, col0 + ncol) of the checkpointed batched tape's segment buffer, out [ncol][k][N] in the W layout; *segment = the
// segment the buffer holds (test aid, as fc_debug_get_adjoint_segment)
int fc_debug_get_adjoint_segment_batch(fc_handle h, int32_t col0, int32_t ncol, int32_t k, double* out, int32_t* segment) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_segment_batch: null argument");
  FCCHK(batch_check(h, k, "fc_debug_get_adjoint_segment_batch"));
  fc_ctx::StateTape& A = h->adjb.st;
  if (!A.sparse || !A.sg.begun) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_segment_batch: no begun checkpointed batched state tape");
  if (col0 < 0 || ncol <= 0 || col0 + ncol > A.sg.buffer_columns())
    return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_segment_batch: columns beyond the " + std::to_string(A.sg.buffer_columns()) + " the segment buffer has");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  const size_t col = (size_t)h->N * (size_t)h->bat.KB;
  for (int c = 0; c < ncol; ++c) FCCHK(batch_copy(h, h->N, out + (size_t)c * k * h->N, A.tape.p + col * (size_t)(col0 + c), false, h->perm.p));
  if (segment) *segment = A.sg.resident;
  return FC_OK;
}

// columns [col0, col0 + ncol) of the batched tape, out [ncol][k][N] in the W layout (test aid)
int fc_debug_get_adjoint_tape_batch(fc_handle h, int32_t col0, int32_t ncol, int32_t k, double* out) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_tape_batch: null argument");
  FCCHK(batch_check(h, k, "fc_debug_get_adjoint_tape_batch"));
  fc_ctx::StateTape& A = h->adjb.st;
  if (A.sparse || !A.sg.begun) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_tape_batch: no begun batched state tape");
  if (col0 < 0 || ncol <= 0 || col0 + ncol > A.sg.count() + 2)
    return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_tape_batch: columns beyond the " + std::to_string(A.sg.count() + 2) + " the tape holds");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  const size_t col = (size_t)h->N * (size_t)h->bat.KB;
  for (int c = 0; c < ncol; ++c) FCCHK(batch_copy(h, h->N, out + (size_t)c * k * h->N, A.tape.p + col * (size_t)(col0 + c), false, h->perm.p));
  return FC_OK;
}

int fc_run_adjoint_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, const double* w_seq, const double* z_terminal, double* g_seq,
                         double* dx0, double* dxm1, int32_t* flags_out) {
  if (!h) return fail(FC_ERR_INVALID, "fc_run_adjoint_batch: null handle");
  if (n_steps <= 0) return fail(FC_ERR_INVALID, "fc_run_adjoint_batch: n_steps must be positive");
  if (h->n_act > 0 && !g_seq) return fail(FC_ERR_INVALID, "fc_run_adjoint_batch: g_seq is null");
  if (first_order_slot != FC_SLOT_BDF1 && first_order_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, "order_slot must be BDF1/BDF2");
  const char* who = "fc_run_adjoint_batch";
  fc_ctx::AdjB& A = h->adjb;
  const bool nl = h->nonlinear;
  const char* remedy = "fc_adjoint_tape_reserve_batch, then fc_adjoint_tape_begin_batch before the forward fc_step_batch calls";
  const bool taped = nl || h->adjen.n > 0;  // (energy weights: a linearised handle marches over its taped run too)
  fc_ctx::StateTape& T = A.st;
  FCCHK(adj_tape_refusal(h, who, T, n_steps, first_order_slot, "batched state tape", remedy));
  FCCHK(adjb_step_ready(h, first_order_slot, k, who));
  FCCHK(adjen_march_check(h, who, nl, n_steps, k, T, first_order_slot, h->bat.KB));
  if (n_steps > 1 && first_order_slot != FC_SLOT_BDF2) FCCHK(adjb_step_ready(h, FC_SLOT_BDF2, k, who));
  if (nl && T.KB != h->bat.KB) return fail(FC_ERR_INVALID, "fc_run_adjoint_batch: the batched state tape was laid out for another batch width");
  FCCHK(adj_march_prepare(h, first_order_slot, n_steps, k));
  const size_t kk = (size_t)k;
  const bool have_w = w_seq && h->n_sens > 0;
  int flags[32] = {0}, rflags[64] = {0};
  bool replays = false;  // (a taped march walks the tape's segments and recomputes all but the buffer's)
  FCCHK(stape_march_begin(T, taped, n_steps, adjb_tape_layout(h), &replays));
  AdjbReplayHost forward_state(h, replays);
  const AdjReplay replay = adjb_replay(h, n_steps, rflags);
  const int code = adj_enqueue_and_sync(h, who, &A.run_ms, [&]() -> int {
    if (have_w) HIPCHK(hipMemcpyAsync(A.wseq.p, w_seq, (size_t)n_steps * kk * h->n_sens * sizeof(double), hipMemcpyHostToDevice, h->stream));
    FCCHK(adjb_reset(h, z_terminal));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    FCCHK(adj_march(
        h, first_order_slot, n_steps, taped ? T.tape.p : nullptr, T.col, dx0, dxm1,
        [&](int m, int slot, const StepCoeffs& c, const double* xm, const double* er) {
          return adjb_enqueue_step(h, slot, c, xm, have_w ? A.wseq.p + (size_t)(m - 1) * kk * h->n_sens : nullptr, (m == n_steps && z_terminal) ? A.term.p : nullptr,
                                   A.gseq.p + (size_t)(m - 1) * kk * h->n_act, true, er);
        },
        [&](const StepCoeffs& c, const double* xm, int which, double* dst) { return adjb_state_gradient(h, c, xm, which, dst); }, nullptr,
        taped ? &replay : nullptr));
    if (h->n_act > 0) HIPCHK(hipMemcpyAsync(g_seq, A.gseq.p, (size_t)n_steps * kk * h->n_act * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(flags, A.flag.p, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return FC_OK;
  });
  FCCHK(taped ? stape_verdict(T, who, n_steps, k, code, rflags) : code);
  int any = 0;
  for (int s = 0; s < k; ++s) {
    if (flags_out) flags_out[s] = flags[s] ? 1 : 0;
    any |= flags[s];
  }
  if (any) return fail(FC_ERR_DIVERGED, "fc_run_adjoint_batch: non-finite adjoint state in a column (flags_out marks the columns; the others are valid)");
  return FC_OK;
}

// what the last backward step launched, single or batched (fc_ctx::AdjRoute, filled at the launch sites); no launch, no synchronisation
int fc_get_adjoint_route(fc_handle h, int32_t n, int32_t* out) {
  if (!h || !out || n < 0) return fail(FC_ERR_INVALID, "fc_get_adjoint_route: bad argument");
  const fc_ctx::AdjRoute& r = h->adj_route;
  if (!r.have) return fail(FC_ERR_NOT_READY, "fc_get_adjoint_route: no backward step yet (fc_step_adjoint / fc_run_adjoint / fc_run_adjoint_batch)");
  if (n < FC_ADJ_ROUTE_COLS) return fail(FC_ERR_INVALID, "fc_get_adjoint_route: buffer shorter than FC_ADJ_ROUTE_COLS entries");
  const int32_t row[FC_ADJ_ROUTE_COLS] = {r.elem,   r.g_elem, r.g_gather, r.have_w, r.have_term, r.KB, r.k, r.g_tail,
                                          r.passes, r.reduced, r.gx,      r.KB > 0 ? h->adjb.st.tape_last : h->adj.st.tape_last};
  std::copy(row, row + FC_ADJ_ROUTE_COLS, out);
  return FC_OK;
}

// the buffers of the last backward step as the march holds them (permuted numbering; test aid).  Any output may be null.
int fc_debug_get_adjoint_stage(fc_handle h, int32_t kb, int32_t gx, double* b, double* x, double* dx, int32_t* has_dx, double* zm_new, double* zm_prev,
                               double* partial, double* bt, double* lift, double* fvec, int32_t* has_fvec) {
  if (!h) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_stage: null handle");
  const fc_ctx::AdjRoute& r = h->adj_route;
  const bool batched = r.KB > 0;
  if (!r.have || r.slot < 0 || !(batched ? h->adjb.march_ok && h->adjb.KB == r.KB : h->adj.march_ok) || !h->adj.s[r.slot].bt_ok)
    return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_stage: no backward step yet, or its buffers were released or laid out again since");
  if (b && !r.b_live) return fail(FC_ERR_NOT_READY, "fc_debug_get_adjoint_stage: a mass product has overwritten the last backward step's right-hand side");
  if (kb != r.KB || gx != r.g_tail) return fail(FC_ERR_INVALID, "fc_debug_get_adjoint_stage: kb / gx differ from the last backward step's (fc_get_adjoint_route)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  const size_t lvl = (size_t)h->N * (size_t)std::max(1, r.KB), na = (size_t)h->n_act;
  const double* d_b = batched ? h->adjb.b.p : h->adj.b.p;
  const double* d_zm = batched ? h->adjb.zm.p : h->adj.zm.p;
  const int cur = batched ? h->adjb.zm_cur : h->adj.zm_cur;  // (the step has moved on: the newer copy is the one its tail wrote)
  const double* d_part = batched ? h->adjb.part.p : h->adj.part.p;
  const auto get = [&](double* dst, const double* src, size_t n) -> int {
    if (dst && src && n > 0) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return FC_OK;
  };
  int code = get(b, d_b, lvl);
  if (code == FC_OK) code = get(x, r.x, lvl);
  if (code == FC_OK && r.dx) code = get(dx, r.dx, lvl);
  if (has_dx) *has_dx = r.dx ? 1 : 0;
  if (code == FC_OK) code = get(zm_new, d_zm + (size_t)cur * lvl, lvl);
  if (code == FC_OK) code = get(zm_prev, d_zm + (size_t)(1 - cur) * lvl, lvl);
  if (code == FC_OK) code = get(partial, d_part, na * (size_t)std::max(1, r.KB) * (size_t)r.g_tail);
  if (code == FC_OK) code = get(bt, h->adj.s[r.slot].bt.p, na * (size_t)h->N);
  // what fc_adj_control_columns read off the Dirichlet rows: the slot's lifting and the load vectors (permuted numbering)
  const bool force = h->have_force && h->fvec_ok && h->fvec.n >= na * (size_t)h->N;
  if (code == FC_OK && h->sys[r.slot].lift_p.n >= na * (size_t)h->N) code = get(lift, h->sys[r.slot].lift_p.p, na * (size_t)h->N);
  if (code == FC_OK && force) code = get(fvec, h->fvec.p, na * (size_t)h->N);
  if (has_fvec) *has_fvec = force ? 1 : 0;
  const hipError_t e = hipStreamSynchronize(h->stream);  // (also on a failure: no copy into the caller's arrays is in flight afterwards)
  if (code == FC_OK && e != hipSuccess) return fail(FC_ERR_HIP, std::string("fc_debug_get_adjoint_stage: ") + hipGetErrorString(e));
  return code;
}

}  // extern "C"
