// fc_adjoint_energy_run.hpp -- host side of the energy term of the marches' cost (fc_set_adjoint_energy, fc_adjoint_energy_info; kernels
// in fc_adjoint_energy.hip.h and the EN instantiations of fc_adjoint_nl.hip.h / fc_adjoint_batch.hip.h; DESIGN §5.4 "Energy term").
// Included at the end of fc_hip.hip, in front of fc_adjoint_march.hpp: the four marches call adjen_march_check before they enqueue; their
// step loop (adj_march) calls adjen_begin and hands the schedule's adjen_row through adj_enqueue_step / adjb_enqueue_step to
// adj_enqueue_rhs / adjb_enqueue_rhs.  Every other caller of those two (fc_step_adjoint, the dx0 / dxm1 mass products) passes no row.
#pragma once

namespace {

// The rows held fit a march of n_steps steps and k columns (0: a single march) over the forward run the state tape `T` holds; FC_OK
// without rows.  `nl`: the handle is nonlinear -- the march has then made the two tape checks itself, with its own message, and they are
// not repeated.  `kb`: the padded width of the batch (single: 0).
int adjen_march_check(fc_ctx* h, const char* who, bool nl, int n_steps, int k, const fc_ctx::StateTape& T, int first_slot, int kb = 0) {
  const fc_ctx::AdjEn& E = h->adjen;
  if (E.n == 0) return FC_OK;
  const std::string w = std::string(who) + ": energy weights are held (fc_set_adjoint_energy): ";
  if ((E.k == 0) != (k == 0))
    return fail(FC_ERR_INVALID, w + (E.k == 0 ? "they are rows of a single march (k = 0), this march is batched" : "they are rows of a batched march (k = " + std::to_string(E.k) + "), this march is single"));
  if (E.k != k) return fail(FC_ERR_INVALID, w + "they have k = " + std::to_string(E.k) + " columns, the march has k = " + std::to_string(k));
  if (E.n != n_steps) return fail(FC_ERR_INVALID, w + "they have n_steps = " + std::to_string(E.n) + " rows, the march has n_steps = " + std::to_string(n_steps));
  if (k > 0 && E.KB != kb) return fail(FC_ERR_INVALID, w + "they were padded for another batch width (fc_set_adjoint_energy after fc_set_batch)");
  if (E.source == 1) {  // the forcing column of backward step m is dx_m of the tangent tape (fc_set_adjoint_energy_source)
    const std::string ws = w + "the energy source is the tangent tape (fc_set_adjoint_energy_source): ";
    const fc_ctx::Tan::Tape& tt = h->tan.tt;
    if (k > 0) return fail(FC_ERR_INVALID, ws + "it holds a single march: a batched product is not built");
    if (T.sparse) return fail(FC_ERR_INVALID, ws + "the state tape is checkpointed (fc_adjoint_tape_reserve_sparse): a march that reads both is not built -- reserve the dense tape");
    if (tt.capacity == 0) return fail(FC_ERR_INVALID, ws + "no tangent tape is reserved (fc_tangent_tape_reserve, then the tangent march)");
    if (tt.count != n_steps)
      return fail(FC_ERR_INVALID, ws + "it holds a march of " + std::to_string(tt.count) + " steps, this march has n_steps = " + std::to_string(n_steps));
    if (tt.first_slot != first_slot)
      return fail(FC_ERR_INVALID, ws + "its march started on order slot " + std::to_string(tt.first_slot) + ", this march on " + std::to_string(first_slot));
  }
  if (nl) return FC_OK;
  std::string why;
  if (!T.sg.covers(n_steps, first_slot, FC_SLOT_BDF2, &why))
    return fail(FC_ERR_INVALID, w + "the energy term reads the forward trajectory and the " + (k > 0 ? "batched " : "") + "state tape does not hold this run: " + why +
                                    (k > 0 ? " (fc_adjoint_tape_reserve_batch, then fc_adjoint_tape_begin_batch before the forward steps)"
                                           : " (fc_adjoint_tape_reserve, then fc_adjoint_tape_begin before the forward run)"));
  if (k > 0 && T.KB != kb) return fail(FC_ERR_INVALID, w + "the batched state tape was laid out for another batch width");
  return FC_OK;
}

// A march with rows held counts its energy steps from zero (fc_adjoint_energy_info [3]); without rows the last count stays.
void adjen_begin(fc_ctx* h) {
  if (h->adjen.n > 0) h->adjen.steps = 0;
}

// The device row `row` of the weights (backward step m reads row m - 1: [1] single, [KB] batched); null without rows.
const double* adjen_row(const fc_ctx* h, int row) {
  const fc_ctx::AdjEn& E = h->adjen;
  return E.n > 0 ? E.rows.p + (size_t)row * (size_t)std::max(1, E.KB) : nullptr;
}

// The column the weight of backward step m multiplies when it is not the taped state: dx_m of the tangent tape with source 1 (the
// marches have checked that the tape holds this march: adjen_march_check); null with source 0 or without rows.
const double* adjen_source_column(const fc_ctx* h, int m) {
  const fc_ctx::AdjEn& E = h->adjen;
  return E.n > 0 && E.source == 1 ? h->tan.tt.cols.p + (size_t)(m - 1) * (size_t)h->N : nullptr;
}

}  // namespace

extern "C" {

int fc_set_adjoint_energy(fc_handle h, int32_t n_steps, int32_t k, const double* e_seq) {
  if (!h) return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: null handle");
  if (n_steps < 0 || n_steps > (1 << 24) || k < 0) return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: n_steps must be in [0, 2^24] and k >= 0");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: collect the step in flight first (fc_step_end)");
  fc_ctx::AdjEn& E = h->adjen;
  HIPCHK(hipSetDevice(h->device));
  if (n_steps == 0 || !e_seq) {
    if (E.n > 0) {
      FCCHK(quiesce(h));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    E.rows.release();
    E.n = E.k = E.KB = 0;
    E.source = 0;  // (the source is a property of the rows held: it goes with them)
    return FC_OK;
  }
  if (h->partitioned || exchanges(h))
    return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: partitioned handles are not supported (the adjoint marches run on single-GPU handles)");
  int KB = 0;
  if (k > 0) {
    if (h->bat.k == 0) return fail(FC_ERR_NOT_READY, "fc_set_adjoint_energy: k > 0 and fc_set_batch not called");
    if (k != h->bat.k) return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: k differs from fc_set_batch");
    KB = h->bat.KB;
  }
  const size_t W = (size_t)std::max(1, KB), kk = (size_t)std::max(1, (int)k);
  std::vector<double> rows((size_t)n_steps * W, 0.0);
  for (size_t m = 0; m < (size_t)n_steps; ++m)
    for (size_t s = 0; s < kk; ++s) {
      const double v = e_seq[m * kk + s];
      if (!std::isfinite(v)) return fail(FC_ERR_INVALID, "fc_set_adjoint_energy: non-finite weight in row " + std::to_string(m));
      rows[m * W + s] = v;
    }
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));  // (a march that read the present rows has finished; the host vector goes out of scope below)
  const int code = E.rows.upload(rows, h->stream);
  const hipError_t sync = hipStreamSynchronize(h->stream);
  if (code != FC_OK || sync != hipSuccess) {
    E.rows.release();
    E.n = E.k = E.KB = 0;
    return code != FC_OK ? code : fail(FC_ERR_HIP, std::string("fc_set_adjoint_energy: ") + hipGetErrorString(sync));
  }
  E.n = n_steps, E.k = k, E.KB = KB;
  return FC_OK;
}

int fc_set_adjoint_energy_source(fc_handle h, int32_t source) {
  const char* who = "fc_set_adjoint_energy_source";
  if (!h || source < 0 || source > 1) return fail(FC_ERR_INVALID, std::string(who) + ": source must be 0 (the state tape) or 1 (the tangent tape)");
  if (source == 1 && (h->partitioned || exchanges(h)))
    return fail(FC_ERR_INVALID, std::string(who) + ": partitioned handles are not supported (the adjoint marches run on single-GPU handles)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": collect the step in flight first (fc_step_end)");
  h->adjen.source = source;
  return FC_OK;
}

int fc_adjoint_energy_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_adjoint_energy_info: null argument");
  const fc_ctx::AdjEn& E = h->adjen;
  info[0] = E.n, info[1] = E.k, info[2] = 8 * (int64_t)E.rows.n, info[3] = E.steps, info[4] = E.KB;
  info[5] = E.source, info[6] = info[7] = 0;
  return FC_OK;
}

}  // extern "C"
