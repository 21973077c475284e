// fc_tangent_energy_run.hpp -- host side of the tangent of the energy (fc_tangent_set_energy, fc_get_tangent_energy,
// fc_tangent_energy_info; kernels in fc_tangent_energy.hip.h; DESIGN §5.6 "Energy").  Included at the end of fc_hip.hip, in front of
// fc_tangent_march.hpp: the skeleton of the four tangent marches (fc_run_tangent, _batch, fc_run_tangent_closed_loop, _batch) sizes the
// rows in tan_sequences, enqueues tan_energy_step behind every step's tail and tan_energy_fold behind the last step.  With the option off
// (fc_ctx::Tan::energy == false, the state of every handle that never calls fc_tangent_set_energy) each of the three returns before it
// touches the device: nothing is allocated and every march enqueues what it enqueued before the option existed.
#pragma once

namespace {

// what every tangent entry point that needs the whole trajectory answers a partitioned handle (this file is the first of the four)
const char* const kTanPartitioned = "partitioned handles are not supported (a rank holds its own rows of the trajectory only)";

// workgroups of a step's energy launch for the width the tangent buffers were laid out for
int tan_energy_grid(const fc_ctx* h) {
  const int KB = h->tan.KB;
  return KB > 0 ? nblocks(h->nc, 256 / KB) : nblocks((int64_t)h->nc * 8, 256);
}

// the record of the last march starts over with every march; with the option on the partials and the rows of a march of n steps are
// sized here (tan_sequences calls it ahead of the enqueue)
int tan_energy_sequences(fc_ctx* h, int n_steps) {
  fc_ctx::Tan& T = h->tan;
  T.en = fc_ctx::Tan::En();
  if (!T.energy) return FC_OK;
  const int G = tan_energy_grid(h), k = T.KB > 0 ? h->bat.k : 0;
  const size_t np = (size_t)n_steps * G * std::max(1, T.KB), nd = (size_t)n_steps * std::max(1, k);
  if (T.epart.n < np) FCCHK(T.epart.alloc(np));
  if (T.dde.n < nd) FCCHK(T.dde.alloc(nd));
  T.dde_host.assign(nd, 0.0);
  T.en.n = n_steps, T.en.k = k, T.en.KB = T.KB, T.en.G = G;
  return FC_OK;
}

// behind the tail of step j: x the taped column x_j (batched: [N][KB]), the new tangent level the one the tail has just written
// (Tan::cur has moved on to it)
int tan_energy_step(fc_ctx* h, int j, const double* x, int ref_col) {
  fc_ctx::Tan& T = h->tan;
  if (!T.energy) return FC_OK;
  if (!x) return fail(FC_ERR_INVALID, "tangent energy: no taped state for the step (a march with the option reads the dense state tape)");
  const int N = h->N, nc = h->nc, KB = T.KB, G = T.en.G;
  const size_t lvl = (size_t)N * std::max(1, KB);
  const double* d = T.lev.p + (size_t)T.cur * lvl;
  double* part = T.epart.p + (size_t)(j - 1) * G * std::max(1, KB);
  if (KB == 0) {
    hipLaunchKernelGGL(fc_tan_energy, dim3(G), dim3(256), 0, h->stream, nc, (const int*)h->cnp.p, (const double*)h->geom.p, x, d, part);
    T.en.code = 1;
  } else {
    pick_width(KB, [&](auto K) {
      pick_bool(ref_col >= 0, [&](auto SHARED) {
        hipLaunchKernelGGL((fc_tan_energy_b<K, SHARED>), dim3(G), dim3(256), 0, h->stream, nc, T.en.k, (const int*)h->cnp.p, (const double*)h->geom.p, x, d, ref_col,
                           part);
      });
    });
    T.en.code = ref_col >= 0 ? 3 : 2;
  }
  HIPCHK(hipGetLastError());
  ++T.en.launches;
  return FC_OK;
}

// behind the last step: one fold launch for all rows, and their way to the host (read behind the march's one synchronisation)
int tan_energy_fold(fc_ctx* h) {
  fc_ctx::Tan& T = h->tan;
  if (!T.energy) return FC_OK;
  const int n = T.en.n, G = T.en.G, KB = T.KB;
  if (KB == 0)
    hipLaunchKernelGGL(fc_tan_energy_fold, dim3(n), dim3(256), 0, h->stream, G, (const double*)T.epart.p, T.dde.p);
  else
    pick_width(KB, [&](auto K) { hipLaunchKernelGGL((fc_tan_energy_fold_b<K>), dim3(n), dim3(256), 0, h->stream, G, T.en.k, (const double*)T.epart.p, T.dde.p); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(T.dde_host.data(), T.dde.p, T.dde_host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  T.en.have = true;
  return FC_OK;
}

// The tape records the step count and the first slot of the march it holds, nothing else: adjen_march_check can tell a tape of another
// length or order, NOT a tape left from an earlier run of the same n and first slot -- the caller marches the tangent over the state
// tape's run before it marches back with source 1 (the drivers of flowcontrol_amd/tangent.py do; the tape is freed on their way out).
// The tangent tape (fc_tangent_tape_reserve): a single march of n <= capacity steps keeps every new level, column m - 1 = dx_m in the
// solver's numbering; a longer march keeps none.  begin: ahead of the enqueue (the record of an earlier march ends here); step: behind
// the tail of step j, 8 N bytes; tan_enqueue_and_sync drops the record again if the march fails.
void tan_tape_begin(fc_ctx* h, int first_slot, int n_steps) {
  fc_ctx::Tan::Tape& tt = h->tan.tt;
  tt.count = 0, tt.first_slot = -1;
  if (tt.capacity > 0 && n_steps <= tt.capacity) tt.count = n_steps, tt.first_slot = first_slot;
}
int tan_tape_step(fc_ctx* h, int j) {
  fc_ctx::Tan& T = h->tan;
  if (T.tt.count == 0) return FC_OK;
  const int N = h->N;
  hipLaunchKernelGGL(fc_adj_tape_copy<true>, dim3(nblocks(N, 256)), dim3(256), 0, h->stream, N, (const double*)(T.lev.p + (size_t)T.cur * N),
                     T.tt.cols.p + (size_t)(j - 1) * N);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

}  // namespace

extern "C" {

int fc_tangent_set_energy(fc_handle h, int32_t on) {
  const char* who = "fc_tangent_set_energy";
  if (!h || on < 0 || on > 1) return fail(FC_ERR_INVALID, std::string(who) + ": on must be 1 or 0");
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, std::string(who) + ": " + kTanPartitioned);
  fc_ctx::Tan& T = h->tan;
  if (!T.reserved) return fail(FC_ERR_NOT_READY, std::string(who) + ": no tangent buffers (fc_tangent_reserve): the option belongs to a reserve and goes with it");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": a step is in flight");
  if (!on && T.energy) {
    HIPCHK(hipSetDevice(h->device));
    FCCHK(quiesce(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    T.epart.release(), T.dde.release();
    T.dde_host.clear();
    T.en = fc_ctx::Tan::En();
  }
  T.energy = on == 1;
  return FC_OK;
}

int fc_get_tangent_energy(fc_handle h, int32_t n_steps, int32_t k, double* dde) {
  const char* who = "fc_get_tangent_energy";
  if (!h || !dde) return fail(FC_ERR_INVALID, std::string(who) + ": null argument");
  const fc_ctx::Tan& T = h->tan;
  if (!T.en.have)
    return fail(FC_ERR_NOT_READY, std::string(who) + ": the last tangent march ran without the energy option (fc_tangent_set_energy), or there was none since the reserve");
  if (n_steps != T.en.n || k != T.en.k)
    return fail(FC_ERR_INVALID, std::string(who) + ": the last march had n_steps = " + std::to_string(T.en.n) + ", k = " + std::to_string(T.en.k) + " (0: a single march)");
  std::copy(T.dde_host.begin(), T.dde_host.end(), dde);
  return FC_OK;
}

int fc_tangent_energy_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_tangent_energy_info: null argument");
  const fc_ctx::Tan& T = h->tan;
  info[0] = T.energy ? 1 : 0, info[1] = T.en.have ? 1 : 0, info[2] = T.en.code, info[3] = T.en.G, info[4] = T.en.n, info[5] = T.en.k;
  info[6] = T.en.launches, info[7] = 8 * (int64_t)(T.epart.n + T.dde.n);
  return FC_OK;
}

int fc_tangent_tape_reserve(fc_handle h, int32_t n_steps) {
  const char* who = "fc_tangent_tape_reserve";
  if (!h || n_steps < 0 || n_steps > (1 << 24)) return fail(FC_ERR_INVALID, std::string(who) + ": n_steps must be in [0, 2^24] (0 frees)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, std::string(who) + ": a step is in flight");
  // (every refusal of a reserve comes first: a refused call leaves the tape and the source as they are)
  if (n_steps > 0) {
    if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, std::string(who) + ": " + kTanPartitioned);
    if (h->bat.k > 0) return fail(FC_ERR_INVALID, std::string(who) + ": the handle has a batch set (fc_set_batch): the tangent tape keeps single marches only");
    if (!h->have_perm) return fail(FC_ERR_NOT_READY, std::string(who) + ": no permutation (fc_setup_solver): the tape is kept in the solver's numbering");
  }
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int source = h->adjen.source;
  tan_tape_release(h);
  if (n_steps == 0) return FC_OK;  // (freed: the source has gone back to 0 with it)
  fc_ctx::Tan::Tape& tt = h->tan.tt;
  const int code = tt.cols.alloc((size_t)n_steps * (size_t)h->N);
  if (code != FC_OK) {
    tan_tape_release(h);
    (void)hipGetLastError();
    return code;
  }
  tt.capacity = n_steps;
  h->adjen.source = source;  // (a new tape in the place of the old one: the source stands; the tape holds no march yet)
  return FC_OK;
}

int fc_tangent_tape_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_tangent_tape_info: null argument");
  const fc_ctx::Tan::Tape& tt = h->tan.tt;
  info[0] = tt.capacity, info[1] = tt.count, info[2] = tt.first_slot, info[3] = 8 * (int64_t)tt.cols.n;
  info[4] = info[5] = info[6] = info[7] = 0;
  return FC_OK;
}

// columns first_col .. first_col + ncol - 1 of the tangent tape as they lie on the device (solver's numbering; test aid)
int fc_debug_get_tangent_tape(fc_handle h, int32_t first_col, int32_t ncol, double* out) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_debug_get_tangent_tape: null argument");
  const fc_ctx::Tan::Tape& tt = h->tan.tt;
  if (first_col < 0 || ncol < 0 || first_col + ncol > tt.count)
    return fail(FC_ERR_INVALID, "fc_debug_get_tangent_tape: columns outside the march the tape holds (" + std::to_string(tt.count) + " steps)");
  if (ncol == 0) return FC_OK;
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  HIPCHK(hipMemcpyAsync(out, tt.cols.p + (size_t)first_col * h->N, (size_t)ncol * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return FC_OK;
}

}  // extern "C"
