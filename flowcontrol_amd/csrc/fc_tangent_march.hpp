// fc_tangent_march.hpp -- what the four tangent marches share (fc_run_tangent, _batch, fc_run_tangent_closed_loop, _batch; DESIGN §5.6
// "One skeleton"): the mode of a march with its rows of Tan::du / Tan::dy, the refusals in front of and behind the march's own, the
// device part of the preamble, the one body from the flag memset to the record of ev1, the levels and flags behind it, the one exit.
// Included at the end of fc_hip.hip, behind fc_tangent_energy_run.hpp and in front of fc_tangent_run.hpp, which defines what is only
// declared here.
#pragma once

namespace {

int tan_enqueue_step(fc_ctx* h, int slot, const double* x1, const double* x2, const double* d_du, double* d_dy);  // fc_tangent_run.hpp
int tanb_enqueue_step(fc_ctx* h, int slot, const double* x1, const double* x2, int ref_col, const double* d_du, double* d_dy);
// The mode of a march, filled by tan_front_single / tan_front_batch once the handle is known to be in it.
struct TanMode {
  int k, W, ref_col;             // columns (0: the single march), padded width (KB or 1), the shared column of the trajectory or -1
  size_t lvl;                    // doubles of one level and of one column of the state tape
  const fc_ctx::StateTape* st;   // the state tape of the mode ...
  const char* remedy;            // ... and the calls that would have taped the run
  // rows of step j: the controls of every PADDED column (the batched gather reads all W), the readings of the k columns; an empty
  // actuator or sensor set keeps one double per row, as tan_sequences sizes them (no kernel reads or writes such a row)
  double* du_row(const fc_ctx* h, int j) const { return h->tan.du.p + (size_t)(j - 1) * W * std::max(1, h->n_act); }
  double* dy_row(const fc_ctx* h, int j) const { return h->tan.dy.p + (size_t)(j - 1) * std::max(1, k) * std::max(1, h->n_sens); }
};
int tan_levels_in(fc_ctx* h, const TanMode& M, const double* dx0, const double* dxm1);
int tan_levels_out(fc_ctx* h, const TanMode& M, double* dxn, double* dxnm1);

// The refusals: the front of the mode, the march's own (tan_refusal / tan_loop_refusal, of the three parts below), the slots.
// (a partitioned handle before anything else: it can hold no reserve to ask for)
int tan_front(fc_ctx* h, const char* who) {
  if (!h) return fail(FC_ERR_INVALID, std::string(who) + ": null handle");
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, std::string(who) + ": " + kTanPartitioned);
  if (!h->tan.reserved) return fail(FC_ERR_NOT_READY, std::string(who) + ": no tangent buffers (fc_tangent_reserve)");
  return FC_OK;
}
int tan_front_single(fc_ctx* h, const char* who, const char* remedy, TanMode* M) {
  FCCHK(tan_front(h, who));
  if (h->bat.k > 0 || h->tan.KB != 0)
    return fail(FC_ERR_INVALID, std::string(who) + ": the handle has a batch set (fc_set_batch) or the buffers were reserved for one: " + who + "_batch");
  *M = TanMode{0, 1, -1, (size_t)h->N, &h->adj.st, remedy};
  return FC_OK;
}
int tan_front_batch(fc_ctx* h, const char* who, int k, int ref_col, const char* remedy, TanMode* M) {
  FCCHK(tan_front(h, who));
  const fc_ctx::Batch& B = h->bat;
  FCCHK(batch_check(h, k, who));
  if (h->tan.KB != B.KB || h->tan.work.n != batch_slot_doubles(B, (size_t)h->N, B.KB))
    return fail(FC_ERR_NOT_READY, std::string(who) + ": the tangent buffers were reserved for another mode or batch width (fc_tangent_reserve again)");
  if (ref_col < -1 || ref_col >= k) return fail(FC_ERR_INVALID, std::string(who) + ": ref_col must be in [-1, k)");
  *M = TanMode{k, B.KB, ref_col, (size_t)h->N * B.KB, &h->adjb.st, remedy};
  return FC_OK;
}

// The three parts of a march's own refusals: the call itself ...
int tan_refusal_call(fc_ctx* h, const std::string& w, int first_slot, int n_steps) {
  if (n_steps <= 0) return fail(FC_ERR_INVALID, w + "n_steps must be positive");
  if (first_slot != FC_SLOT_BDF1 && first_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, w + "order_slot must be BDF1/BDF2");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, w + "collect the step in flight first (fc_step_end / fc_step_batch_end)");
  return FC_OK;
}
// ... the state tape of the mode, which a march of a nonlinear scheme or with the energy option reads ...
int tan_refusal_tape(const std::string& w, int first_slot, int n_steps, const TanMode& M) {
  if (M.st->sparse)
    return fail(FC_ERR_INVALID, w + "the state tape is checkpointed (fc_adjoint_tape_reserve_sparse): a tangent march over a checkpointed tape is not built -- reserve the dense tape");
  std::string why;
  if (!M.st->sg.covers(n_steps, first_slot, FC_SLOT_BDF2, &why)) return fail(FC_ERR_INVALID, w + "the state tape does not hold this run: " + why + " (" + M.remedy + ")");
  return FC_OK;
}
// ... and the time scheme of the slots the march steps on
int tan_refusal_scheme(fc_ctx* h, const std::string& w, int first_slot, int n_steps) {
  for (int slot : {first_slot, n_steps > 1 ? (int)FC_SLOT_BDF2 : first_slot})
    if (h->sys[slot].have_c) return fail(FC_ERR_INVALID, w + "the slot has an explicit right-hand-side operator (Crank-Nicolson)");
  return FC_OK;
}

// what fc_run refuses on a slot of the run (enqueue_step_launches, check_step_ready), with the march's own condition that the sweeps
// apply the direct factors
int tan_slot_ready(fc_ctx* h, const char* who, int slot) {
  const std::string w = std::string(who) + ": ";
  const OrderSys& S = h->sys[slot];
  if (!S.ready) return fail(FC_ERR_NOT_READY, w + "fc_solver_setup not called for this order");
  if (S.factor_free) return fail(FC_ERR_INVALID, w + "this slot has no factors (fc_setup_krylov): the tangent march applies the direct factors");
  if (S.truncated) return fail(FC_ERR_INVALID, w + "truncated factors are a preconditioner, not a solve");
  if (S.inexact) return fail(FC_ERR_INVALID, w + "the slot's factors are inexact (they precondition GMRES): the tangent march applies the direct factors");
  if (h->method != FC_METHOD_REFINE) return fail(FC_ERR_INVALID, w + "a Krylov method is selected (fc_set_solver_options): the tangent march runs on the direct factor apply");
  // last, behind every refusal above: it may assemble the load vectors of new body-force profiles (build_force_vectors launches, as in
  // fc_run) -- an accepted march is the only call that gets that far
  return check_step_ready(h, slot);
}
// the tail of the refusals, slot by slot: the first step's and, on a longer march from BDF1, BDF2's
int tan_slots_ready(fc_ctx* h, const char* who, const TanMode& M, int first_slot, int n_steps) {
  const int last = n_steps > 1 ? (int)FC_SLOT_BDF2 : first_slot;
  if (M.k == 0) {
    FCCHK(tan_slot_ready(h, who, first_slot));
    return last != first_slot ? tan_slot_ready(h, who, last) : FC_OK;
  }
  if ((h->nonlinear || h->tan.energy) && M.st->KB != M.W) return fail(FC_ERR_INVALID, std::string(who) + ": the batched state tape was laid out for another batch width");
  FCCHK(batch_ready(h, first_slot, M.k, who));
  if (last != first_slot) FCCHK(batch_ready(h, last, M.k, who));
  for (int slot : {first_slot, last})
    if (!h->bat.ftile_ok[slot]) return fail(FC_ERR_NOT_READY, std::string(who) + ": the slot's factors have no tiled copy (fc_set_batch after fc_setup_solver)");
  return FC_OK;
}

// the sequences of a march of n steps, `cols` columns wide (du rows of every padded column: the batched gather reads all KB of them)
int tan_sequences(fc_ctx* h, int n_steps, int cols) {
  fc_ctx::Tan& T = h->tan;
  const size_t nu = (size_t)n_steps * cols * std::max(1, h->n_act), ny = (size_t)n_steps * cols * std::max(1, h->n_sens);
  if (T.du.n < nu) FCCHK(T.du.alloc(nu));
  if (T.dy.n < ny) FCCHK(T.dy.alloc(ny));
  return tan_energy_sequences(h, n_steps);  // (with fc_tangent_set_energy: the partials and the rows; without: the record starts over)
}
// the device part of the preamble (the tangent tape keeps single marches only; the closed loops add tan_loop_sequences behind it)
int tan_march_prepare(fc_ctx* h, const TanMode& M, int first_slot, int n_steps) {
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(tan_sequences(h, n_steps, M.W));
  if (M.k == 0) tan_tape_begin(h, first_slot, n_steps);
  return FC_OK;
}

// From the flag memset to the record of ev1: the levels in, the steps j = 1 .. n on `first_slot`, then BDF2, the energy's fold.  Step j
// reads columns j (x_{j-1}) and j - 1 (x_{j-2}) of the state tape on a nonlinear scheme -- a linearised scheme's coefficients switch
// the element kernels' reads off, and the step is handed null -- and the energy column j + 1 (x_j) with the option on.
// before_step(j) (optional): the closed loops launch the controller there, which writes M.du_row(h, j).  A march over a checkpointed
// tape puts its segment loop around this step loop.
template <class Before = std::nullptr_t>
int tan_march(fc_ctx* h, const TanMode& M, int first_slot, int n_steps, const double* dx0, const double* dxm1, Before&& before_step = nullptr) {
  fc_ctx::Tan& T = h->tan;
  const double* tape = M.st->tape.p;
  const auto column = [&](bool read, int c) { return read && tape ? tape + M.lvl * (size_t)c : (const double*)nullptr; };
  HIPCHK(hipMemsetAsync(T.flag.p, 0, 32 * sizeof(int), h->stream));
  FCCHK(tan_levels_in(h, M, dx0, dxm1));
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int j = 1; j <= n_steps; ++j) {
    const int slot = j == 1 ? first_slot : (int)FC_SLOT_BDF2;
    const double *x1 = column(h->nonlinear, j), *x2 = column(h->nonlinear, j - 1), *du = M.du_row(h, j);
    if constexpr (!std::is_same_v<std::decay_t<Before>, std::nullptr_t>) before_step(j);
    FCCHK(M.k > 0 ? tanb_enqueue_step(h, slot, x1, x2, M.ref_col, du, M.dy_row(h, j)) : tan_enqueue_step(h, slot, x1, x2, du, M.dy_row(h, j)));
    FCCHK(tan_energy_step(h, j, column(T.energy, j + 1), M.ref_col));  // (a null column is refused there, never launched on)
    if (M.k == 0) FCCHK(tan_tape_step(h, j));
  }
  FCCHK(tan_energy_fold(h));
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  return FC_OK;
}
// ... and behind the caller's downloads: dx_n / dx_{n-1} (either may be null) and the flags, one word of a single march, 32 of a batch
int tan_march_out(fc_ctx* h, const TanMode& M, double* dxn, double* dxnm1, int* flags) {
  FCCHK(tan_levels_out(h, M, dxn, dxnm1));
  HIPCHK(hipMemcpyAsync(flags, h->tan.flag.p, (M.k > 0 ? 32 : 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}

// The exit of the four marches (§5.4's rule): `enqueue` holds the entry point's uploads, tan_march, its downloads and tan_march_out;
// the stream is synchronised whatever it returned, then the device time goes to Tan::run_ms.
template <class Enqueue>
int tan_enqueue_and_sync(fc_ctx* h, const char* who, int n_steps, Enqueue&& enqueue) {
  fc_ctx::Tan& T = h->tan;
  const int code = enqueue();
  const hipError_t sync = hipStreamSynchronize(h->stream);  // the one synchronisation of the call
  if (code != FC_OK || sync != hipSuccess) T.en.have = false, T.tt.count = 0;  // (no energy rows, no tangent tape of a march that did not complete)
  if (code != FC_OK) return code;
  if (sync != hipSuccess) return fail(FC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(sync));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  T.run_ms = (double)ms;
  T.steps = n_steps;
  ++T.marches;
  return FC_OK;
}

}  // namespace
