// fc_tangent_run.hpp -- host side of the tangent-linear march (fc_tangent_reserve, fc_run_tangent, fc_run_tangent_batch,
// fc_tangent_info; kernels in fc_tangent.hip.h).  Included at the end of fc_hip.hip, behind fc_tangent_march.hpp: the
// mode, the shared refusals, the preamble, the step loop and the exit of a march are that file's; this one's are the reserve, the
// plant's step (single and batched) with its route record, the staging of the levels, the open-loop marches' own refusal, uploads,
// downloads and verdicts, and the two readers of the last step.
//
// A tangent step is a forward step on other vectors: the element loop of fc_tangent.hip.h in the place of fc_rhs_elem, the forward
// step's own gather with the control columns (fc_rhs_gather / fc_rhs_gather_b: B~ du on the Dirichlet rows, - lift du + F du on the
// others), the sweeps on the slot's DIRECT factors (solve_permuted with the handle's refinement sweeps / batch_apply on Batch::ftile),
// and a tail that moves the solution into the older tangent level and forms dy = C dx and the finiteness flag.  The march keeps its own
// tangent levels, work buffer, right-hand side, element vectors and du / dy sequences (fc_ctx::Tan): the state ring, the speculated
// element vectors, the step counter, the snapshot bank, the loop cursor, the tapes, the batch's ring and its record pages never see it.
// What it does share with every other call behind a quiesce is the handle's scratch: the single march stages dx0 / dxm1 and dx_n /
// dx_{n-1} through tmpN / tmpN2, a refined solve accumulates in xsol, and the batched apply uses Batch::part / Batch::ticket -- none of
// them carries anything from one call to the next.  The trajectory is read from the dense state tape the adjoint marches read.
#pragma once

namespace {

// While it lives the single solve works in the march's buffers, without the forward path's residual monitor, finiteness test of the
// sweeps and timing marks (what AdjUse does for a backward step, on the direct values).
struct TanUse {
  fc_ctx* h;
  fc_ctx::BufView buf0, b0;
  int check0;
  bool sweep_check0, timing0, phase0;
  explicit TanUse(fc_ctx* h_) : h(h_), buf0(h_->buf), b0(h_->b), check0(h_->check_residual), sweep_check0(h_->sweep_check), timing0(h_->timing), phase0(h_->phase_timing) {
    h->buf.p = h->tan.work.p, h->buf.n = h->tan.work.n;
    h->b.p = h->tan.b.p, h->b.n = h->tan.b.n;
    h->check_residual = 0;
    h->sweep_check = h->timing = h->phase_timing = false;
  }
  ~TanUse() {
    h->buf = buf0, h->b = b0;
    h->check_residual = check0;
    h->sweep_check = sweep_check0, h->timing = timing0, h->phase_timing = phase0;
  }
  TanUse(const TanUse&) = delete;
  TanUse& operator=(const TanUse&) = delete;
};

int64_t tan_bytes(const fc_ctx::Tan& T) {
  return 8 * (int64_t)(T.lev.n + T.work.n + T.b.n + T.ev.n + T.du.n + T.dy.n + T.stage.n + T.dbank.n + T.dxi.n + T.dy0.n + T.dwy.n + T.dwu.n + T.epart.n + T.dde.n) + 4 * (int64_t)T.flag.n;
}

// what both open-loop marches refuse between the front of their mode and the slots (fc_tangent_march.hpp)
int tan_refusal(fc_ctx* h, const char* who, int first_slot, int n_steps, const TanMode& M) {
  const std::string w = std::string(who) + ": ";
  FCCHK(tan_refusal_call(h, w, first_slot, n_steps));
  if (!h->nonlinear)
    return fail(FC_ERR_INVALID, w + "the time scheme is linearised (fc_set_time_scheme(dt, 0)): its forward run is its own tangent (fc_run / fc_step_batch on the perturbation)");
  FCCHK(tan_refusal_tape(w, first_slot, n_steps, M));
  return tan_refusal_scheme(h, w, first_slot, n_steps);
}

// the part of the route record both steps fill alike: which taped levels the coefficients read, the slot, the rows of the step
void tan_route_step(fc_ctx::Tan& T, const StepCoeffs& c, int slot, const double* d_du, const double* d_dy) {
  fc_ctx::Tan::Route& r = T.rt;
  r.l1 = c.cc_n != 0.0, r.l2 = c.cc_nn != 0.0, r.t2 = c.cc_nn != 0.0 || c.cm_nn != 0.0, r.slot = slot;
  r.du_off = (size_t)(d_du - T.du.p), r.dy_off = (size_t)(d_dy - T.dy.p);
  r.have = true;
}

// one tangent step of the single march on `slot`: x1 / x2 the taped states x_{j-1} / x_{j-2}, d_du the control row, d_dy the sensor row
int tan_enqueue_step(fc_ctx* h, int slot, const double* x1, const double* x2, const double* d_du, double* d_dy) {
  fc_ctx::Tan& T = h->tan;
  OrderSys& S = h->sys[slot];
  const int N = h->N, nc = h->nc;
  const StepCoeffs c = coeffs_for(h, slot);
  const double* d1 = T.lev.p + (size_t)T.cur * N;
  double* d2 = T.lev.p + (size_t)(1 - T.cur) * N;
  const bool reg = h->elem_reg_min > 0 && nc >= h->elem_reg_min;  // (launch_elem_on's rule)
  if (reg)
    hipLaunchKernelGGL(fc_tan_elem_nl_reg, dim3(nblocks(nc, 256)), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, x1, x2, d1,
                       (const double*)d2, c.cm_n, c.cm_nn, c.cc_n, c.cc_nn, T.ev.p);
  else
    hipLaunchKernelGGL(fc_tan_elem_nl, dim3(nblocks((int64_t)nc * 8, 256)), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, x1, x2, d1,
                       (const double*)d2, c.cm_n, c.cm_nn, c.cc_n, c.cc_nn, T.ev.p);
  T.route = reg ? 2 : 1;
  hipLaunchKernelGGL(fc_rhs_gather, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->gptr_p.p, h->gidx_p.p, T.ev.p, h->bcslot_p.p, h->bcprof.p, S.lift_p.p,
                     h->n_act, d_du, T.b.p, T.work.p, (const unsigned char*)nullptr, 1, (const int*)nullptr, (const int*)nullptr, (const double*)nullptr,
                     (const double*)nullptr, (const unsigned char*)nullptr, h->have_force ? h->fvec.p : nullptr, d_du);
  const double *x = nullptr, *dx = nullptr;
  {
    TanUse use(h);
    int nrp = 0;
    FCCHK(solve_permuted(h, S, &x, &dx, &nrp));
  }
  hipLaunchKernelGGL(fc_tan_tail, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, x, dx, d2, T.flag.p, h->n_sens, h->s_rowptr.p, h->s_idxp.p, h->s_w.p, d_dy);
  HIPCHK(hipGetLastError());
  T.cur = 1 - T.cur;
  // (fc_get_tangent_route: the conditions above, as they were taken)
  fc_ctx::Tan::Route& r = T.rt;
  r.elem = reg ? 2 : 1, r.g_elem = reg ? nblocks(nc, 256) : nblocks((int64_t)nc * 8, 256), r.g_gather = nblocks(N, 256);
  r.KB = 0, r.k = 0, r.ref_col = -1, r.force_b = 0, r.fvec = h->have_force ? 1 : 0, r.refined = dx ? 1 : 0, r.g_tail = nblocks(N, 256);
  r.x = x, r.dx = dx;
  tan_route_step(T, c, slot, d_du, d_dy);
  return FC_OK;
}

// one tangent step of all columns: x1 / x2 columns of the batched tape [N][KB]
int tanb_enqueue_step(fc_ctx* h, int slot, const double* x1, const double* x2, int ref_col, const double* d_du, double* d_dy) {
  fc_ctx::Tan& T = h->tan;
  fc_ctx::Batch& B = h->bat;
  OrderSys& S = h->sys[slot];
  const int N = h->N, nc = h->nc, KB = B.KB, na = h->n_act;
  const size_t lvl = (size_t)N * KB;
  const StepCoeffs c = coeffs_for(h, slot);
  const double* d1 = T.lev.p + (size_t)T.cur * lvl;
  double* d2 = T.lev.p + (size_t)(1 - T.cur) * lvl;
  pick_width(KB, [&](auto K) {
    pick_bool(ref_col >= 0, [&](auto SHARED) {
      hipLaunchKernelGGL((fc_tan_elem_nl_b<K, SHARED>), dim3(nblocks(nc, 256 / K)), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, x1, x2,
                         d1, (const double*)d2, c.cm_n, c.cm_nn, c.cc_n, c.cc_nn, ref_col, T.ev.p);
    });
    hipLaunchKernelGGL((fc_rhs_gather_b<K>), dim3(nblocks((int64_t)N * (K / 2), 256)), dim3(256), 0, h->stream, N, h->gptr_p.p, h->gidx_p.p, T.ev.p, h->bcslot_p.p,
                       h->bcprof.p, S.lift_p.p, na, d_du, std::max(1, na), T.b.p, T.work.p, (const int*)nullptr, (const int*)nullptr, (const double*)nullptr,
                       (const double*)nullptr, 1);
    // (the batched forward step enters its body forces in the element loop; here they come as the load vectors the single gather adds)
    if (h->have_force && na > 0)
      hipLaunchKernelGGL((fc_tan_force_b<K>), dim3(nblocks((int64_t)N * K, 256)), dim3(256), 0, h->stream, N, h->bcslot_p.p, na, (const double*)h->fvec.p, d_du, T.b.p,
                         T.work.p);
  });
  T.route = ref_col >= 0 ? 4 : 3;
  FCCHK(batch_apply(h, slot, false, B.ftile[slot].p, T.work.p));
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL((fc_tan_tail_b<K>), dim3(nblocks((int64_t)N * K, 256)), dim3(256), 0, h->stream, N, B.k, (const double*)(T.work.p + lvl), d2, T.flag.p, h->n_sens,
                       h->s_rowptr.p, h->s_idxp.p, h->s_w.p, d_dy);
  });
  HIPCHK(hipGetLastError());
  T.cur = 1 - T.cur;
  fc_ctx::Tan::Route& r = T.rt;
  r.elem = ref_col >= 0 ? 4 : 3, r.g_elem = nblocks(nc, 256 / KB), r.g_gather = nblocks((int64_t)N * (KB / 2), 256);
  r.KB = KB, r.k = B.k, r.ref_col = ref_col, r.force_b = h->have_force && na > 0 ? 1 : 0, r.fvec = 0, r.refined = 0, r.g_tail = nblocks((int64_t)N * KB, 256);
  r.x = T.work.p + lvl, r.dx = nullptr;
  tan_route_step(T, c, slot, d_du, d_dy);
  return FC_OK;
}

// Where level l = 0 / 1 is staged on its way from or to the caller: the handle's scratch vectors (single), Tan::stage (a batch: [k][N]).
double* tan_stage(fc_ctx* h, const TanMode& M, int l) {
  return M.k > 0 ? h->tan.stage.p + (size_t)l * M.k * h->N : l == 0 ? h->tmpN.p : h->tmpN2.p;
}
// The two tangent levels from the caller's dx0 / dxm1 (W layout, a batch [k][N]; null: zero) into the solver's numbering (a batch
// [N][KB]): level 0 = dx_0, level 1 = dx_{-1} ...
int tan_levels_in(fc_ctx* h, const TanMode& M, const double* dx0, const double* dxm1) {
  fc_ctx::Tan& T = h->tan;
  const int N = h->N, k = M.k;
  T.cur = 0;
  const double* init[2] = {dx0, dxm1};
  for (int l = 0; l < 2; ++l) {
    double *lev = T.lev.p + (size_t)l * M.lvl, *stage = tan_stage(h, M, l);
    if (!init[l]) {
      HIPCHK(hipMemsetAsync(lev, 0, M.lvl * sizeof(double), h->stream));
      continue;
    }
    HIPCHK(hipMemcpyAsync(stage, init[l], (size_t)std::max(1, k) * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (k == 0)
      hipLaunchKernelGGL(fc_gather_perm, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->perm.p, (const double*)stage, lev);
    else
      pick_width(M.W, [&](auto K) {
        hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)N * M.W, 256)), dim3(256), 0, h->stream, N, k, (const double*)stage, lev, 1, (const int*)h->perm.p);
      });
  }
  return FC_OK;
}
// ... and dx_n / dx_{n-1} back to the caller behind the last step (either may be null)
int tan_levels_out(fc_ctx* h, const TanMode& M, double* dxn, double* dxnm1) {
  fc_ctx::Tan& T = h->tan;
  const int N = h->N, k = M.k;
  double* out[2] = {dxn, dxnm1};
  for (int l = 0; l < 2; ++l) {
    if (!out[l]) continue;
    const double* lev = T.lev.p + (size_t)(l == 0 ? T.cur : 1 - T.cur) * M.lvl;
    double* stage = tan_stage(h, M, l);
    if (k == 0)
      hipLaunchKernelGGL(fc_scatter_perm, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, h->perm.p, lev, (const double*)nullptr, stage);
    else
      pick_width(M.W, [&](auto K) {
        hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)N * M.W, 256)), dim3(256), 0, h->stream, N, k, lev, stage, 0, (const int*)h->perm.p);
      });
    HIPCHK(hipMemcpyAsync(out[l], stage, (size_t)std::max(1, k) * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipGetLastError());
  return FC_OK;
}

}  // namespace

extern "C" {

int fc_tangent_reserve(fc_handle h, int32_t on) {
  const char* who = "fc_tangent_reserve";
  if (!h || on < 0 || on > 1) return fail(FC_ERR_INVALID, std::string(who) + ": on must be 1 (reserve) or 0 (free)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": a step is in flight");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  fc_ctx::Tan& T = h->tan;
  tan_release(h, false);  // (the tangent tape is its own reserve: fc_tangent_tape_reserve)
  if (!on) return FC_OK;
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, std::string(who) + ": " + kTanPartitioned);
  if (!h->have_perm) return fail(FC_ERR_NOT_READY, std::string(who) + ": no permutation (fc_setup_solver): the march works in the solver's numbering");
  const size_t N = (size_t)h->N;
  const int KB = h->bat.k > 0 ? h->bat.KB : 0;
  const size_t w = (size_t)std::max(1, KB);
  int code = T.lev.alloc(2 * N * w);
  if (code == FC_OK) code = T.work.alloc(KB > 0 ? batch_slot_doubles(h->bat, N, KB) : 2 * N);
  if (code == FC_OK) code = T.b.alloc(N * w);
  if (code == FC_OK) code = T.ev.alloc((size_t)12 * h->nc * w);
  if (code == FC_OK) code = T.flag.alloc(32);
  if (code == FC_OK && KB > 0) code = T.stage.alloc(2 * (size_t)h->bat.k * N);
  if (code == FC_OK)
    for (DevBuf<double>* d : {&T.lev, &T.work, &T.b, &T.ev})  // (the work buffer's zero row and scratch rows; padding columns stay zero)
      if (code == FC_OK) code = d->zero(h->stream);
  if (code == FC_OK) code = T.flag.zero(h->stream);
  if (code != FC_OK) {
    tan_release(h, false);
    (void)hipGetLastError();
    return code;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  T.reserved = true;
  T.KB = KB;
  return FC_OK;
}

int fc_tangent_info(fc_handle h, int64_t* info, double* dinfo) {
  if (!h) return fail(FC_ERR_INVALID, "fc_tangent_info: null handle");
  const fc_ctx::Tan& T = h->tan;
  if (info) {
    info[0] = T.reserved ? 1 : 0, info[1] = T.KB, info[2] = tan_bytes(T), info[3] = T.steps, info[4] = T.route, info[5] = T.marches;
    info[6] = info[7] = 0;
  }
  if (dinfo) dinfo[0] = T.run_ms, dinfo[1] = 0.0;
  return FC_OK;
}

int fc_run_tangent(fc_handle h, int first_order_slot, int32_t n_steps, const double* du_seq, const double* dx0, const double* dxm1, double* dy_seq,
                   double* dxn, double* dxnm1) {
  const char* who = "fc_run_tangent";
  TanMode M;
  FCCHK(tan_front_single(h, who, "fc_adjoint_tape_reserve, then fc_adjoint_tape_begin before the forward fc_run", &M));
  FCCHK(tan_refusal(h, who, first_order_slot, n_steps, M));
  FCCHK(tan_slots_ready(h, who, M, first_order_slot, n_steps));
  FCCHK(tan_march_prepare(h, M, first_order_slot, n_steps));
  fc_ctx::Tan& T = h->tan;
  const size_t n = (size_t)n_steps, na = (size_t)h->n_act, ns = (size_t)h->n_sens;
  int flag = 0;
  FCCHK(tan_enqueue_and_sync(h, who, n_steps, [&]() -> int {
    if (du_seq && na > 0)
      HIPCHK(hipMemcpyAsync(T.du.p, du_seq, n * na * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else
      HIPCHK(hipMemsetAsync(T.du.p, 0, n * std::max<size_t>(1, na) * sizeof(double), h->stream));
    FCCHK(tan_march(h, M, first_order_slot, n_steps, dx0, dxm1));
    if (dy_seq && ns > 0) HIPCHK(hipMemcpyAsync(dy_seq, T.dy.p, n * ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return tan_march_out(h, M, dxn, dxnm1, &flag);
  }));
  return flag ? fail(FC_ERR_DIVERGED, std::string(who) + ": non-finite tangent state after a solve") : FC_OK;
}

int fc_run_tangent_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, int32_t ref_col, const double* du_seq, const double* dx0,
                         const double* dxm1, double* dy_seq, double* dxn, double* dxnm1, int32_t* flags_out) {
  const char* who = "fc_run_tangent_batch";
  TanMode M;
  FCCHK(tan_front_batch(h, who, k, ref_col, "fc_adjoint_tape_reserve_batch, then fc_adjoint_tape_begin_batch before the forward fc_step_batch calls", &M));
  FCCHK(tan_refusal(h, who, first_order_slot, n_steps, M));
  FCCHK(tan_slots_ready(h, who, M, first_order_slot, n_steps));
  FCCHK(tan_march_prepare(h, M, first_order_slot, n_steps));
  fc_ctx::Tan& T = h->tan;
  const size_t n = (size_t)n_steps, kk = (size_t)k, KB = (size_t)M.W, na = (size_t)h->n_act, ns = (size_t)h->n_sens, nas = std::max<size_t>(1, na);
  // du [n][k][n_act] -> [n][KB][n_act], the padding columns' rows zero (the gather reads every column's row)
  std::vector<double> du_host(n * KB * nas, 0.0);
  if (du_seq && na > 0)
    for (size_t j = 0; j < n; ++j) std::copy(du_seq + j * kk * na, du_seq + (j + 1) * kk * na, du_host.begin() + j * KB * nas);
  int flags[32] = {0};
  FCCHK(tan_enqueue_and_sync(h, who, n_steps, [&]() -> int {
    HIPCHK(hipMemcpyAsync(T.du.p, du_host.data(), du_host.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    FCCHK(tan_march(h, M, first_order_slot, n_steps, dx0, dxm1));
    if (dy_seq && ns > 0) HIPCHK(hipMemcpyAsync(dy_seq, T.dy.p, n * kk * ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return tan_march_out(h, M, dxn, dxnm1, flags);
  }));
  int any = 0;
  for (int s = 0; s < k; ++s) {
    if (flags_out) flags_out[s] = flags[s] ? 1 : 0;
    any |= flags[s];
  }
  if (any) return fail(FC_ERR_DIVERGED, std::string(who) + ": non-finite tangent state in a column (flags_out marks the columns; the others are valid)");
  return FC_OK;
}

// what the last tangent step launched, single or batched (fc_ctx::Tan::Route, filled at the launch sites); no launch, no synchronisation
int fc_get_tangent_route(fc_handle h, int32_t n, int32_t* out) {
  if (!h || !out || n < 0) return fail(FC_ERR_INVALID, "fc_get_tangent_route: bad argument");
  const fc_ctx::Tan::Route& r = h->tan.rt;
  if (!r.have) return fail(FC_ERR_NOT_READY, "fc_get_tangent_route: no tangent step yet (fc_run_tangent / fc_run_tangent_batch), or fc_tangent_reserve has laid the buffers out again");
  if (n < FC_TAN_ROUTE_COLS) return fail(FC_ERR_INVALID, "fc_get_tangent_route: buffer shorter than FC_TAN_ROUTE_COLS entries");
  const int32_t row[FC_TAN_ROUTE_COLS] = {r.elem, r.g_elem, r.g_gather, r.KB, r.k, r.ref_col, r.force_b, r.fvec, r.refined, r.g_tail, r.l1, r.l2, r.t2, r.slot};
  std::copy(row, row + FC_TAN_ROUTE_COLS, out);
  return FC_OK;
}

// the buffers of the last tangent step as the march holds them (permuted numbering; test aid).  Any output may be null.
int fc_debug_get_tangent_stage(fc_handle h, int32_t kb, double* ev, double* b, double* x, double* dx, int32_t* has_dx, double* lev_new, double* lev_other,
                               double* du, double* dy, int32_t* flags, double* lift, double* fvec, int32_t* has_fvec) {
  if (!h) return fail(FC_ERR_INVALID, "fc_debug_get_tangent_stage: null handle");
  const fc_ctx::Tan& T = h->tan;
  const fc_ctx::Tan::Route& r = T.rt;
  if (!r.have || !T.reserved || r.slot < 0)
    return fail(FC_ERR_NOT_READY, "fc_debug_get_tangent_stage: no tangent step yet, or its buffers were released or laid out again since");
  if (kb != r.KB) return fail(FC_ERR_INVALID, "fc_debug_get_tangent_stage: kb differs from the last tangent step's (fc_get_tangent_route)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  const size_t W = (size_t)std::max(1, r.KB), lvl = (size_t)h->N * W, na = (size_t)h->n_act, ns = (size_t)h->n_sens;
  const auto get = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst && src && bytes > 0) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    return FC_OK;
  };
  const size_t D = sizeof(double);
  int code = get(ev, T.ev.p, (size_t)12 * h->nc * W * D);
  if (code == FC_OK) code = get(b, T.b.p, lvl * D);
  if (code == FC_OK) code = get(x, r.x, lvl * D);
  if (code == FC_OK && r.dx) code = get(dx, r.dx, lvl * D);
  if (has_dx) *has_dx = r.dx ? 1 : 0;
  // (the march has moved on: the newer level is the one the step's tail wrote)
  if (code == FC_OK) code = get(lev_new, T.lev.p + (size_t)T.cur * lvl, lvl * D);
  if (code == FC_OK) code = get(lev_other, T.lev.p + (size_t)(1 - T.cur) * lvl, lvl * D);
  if (code == FC_OK) code = get(du, T.du.p + r.du_off, W * na * D);
  if (code == FC_OK) code = get(dy, T.dy.p + r.dy_off, (size_t)std::max(1, r.k) * ns * D);
  if (code == FC_OK) code = get(flags, T.flag.p, 32 * sizeof(int));
  const bool force = h->have_force && h->fvec_ok && h->fvec.n >= na * (size_t)h->N;
  if (code == FC_OK && h->sys[r.slot].lift_p.n >= na * (size_t)h->N) code = get(lift, h->sys[r.slot].lift_p.p, na * (size_t)h->N * D);
  if (code == FC_OK && force) code = get(fvec, h->fvec.p, na * (size_t)h->N * D);
  if (has_fvec) *has_fvec = force ? 1 : 0;
  const hipError_t e = hipStreamSynchronize(h->stream);  // (also on a failure: no copy into the caller's arrays is in flight afterwards)
  if (code == FC_OK && e != hipSuccess) return fail(FC_ERR_HIP, std::string("fc_debug_get_tangent_stage: ") + hipGetErrorString(e));
  return code;
}

}  // extern "C"
