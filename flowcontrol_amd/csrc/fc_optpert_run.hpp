// fc_optpert_run.hpp -- host side of the optimal-perturbation driver (fc_mass_solve_batch, fc_optpert_reserve / _load / _get / _apply /
// _mass_solve / _gram / _combine / _info; kernels in fc_optpert.hip.h).  Included at the end of fc_hip.hip, behind the
// adjoint run files: the backward part of an apply is adj_march of fc_adjoint_march.hpp with the step of fc_adjoint_batch_run.hpp, its
// terminal vectors and its dx0 product staying on the device; the forward part is batch_enqueue of the batched step on a record page
// in device memory that holds zero controls, as fc_run_closed_loop_batch keeps its records.
//
// M_ff is held as a compacted CSR by permuted row (rows outside f empty, columns = permuted rows), built on the host from the mass
// slot's values when the tables are first needed and again whenever those values or the permutation have changed since.
#pragma once

namespace {

constexpr int kOptpertCgChunk = 8;     // block-CG iterations enqueued between two reads of the scalars ("some column still iterates")
constexpr int kOptpertMaxGrid = 256;   // workgroups of the row-lane kernels (their partials are summed by every workgroup)
constexpr int kOptpertGramGrid = 128;  // row ranges of a block Gram

inline int optp_grid(int N, int KB) { return std::min(kOptpertMaxGrid, nblocks(N, 256 / KB)); }
inline double* optp_cg(fc_ctx* h, int which) { return h->opt.cg.p + (size_t)which * (size_t)h->N * (size_t)h->opt.KB; }  // 0 r, 1 p, 2 Ap, 3 b, 4 x

// what every entry point here needs: a batch, the mass slot, no step in flight
int optp_usable(fc_ctx* h, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (!h) return fail(FC_ERR_INVALID, w + "null handle");
  if (h->partitioned || exchanges(h)) return fail(FC_ERR_INVALID, w + "partitioned handles are not supported");
  if (h->bat.k == 0) return fail(FC_ERR_NOT_READY, w + "fc_set_batch not called");
  if (!h->slot_ok[FC_SLOT_MASS]) return fail(FC_ERR_NOT_READY, w + "FC_SLOT_MASS not assembled");
  if (!h->have_perm) return fail(FC_ERR_NOT_READY, w + "no permutation (fc_setup_solver)");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, w + "collect the step in flight first (fc_step_end / fc_step_batch_end)");
  return FC_OK;
}

bool optp_stale(const fc_ctx* h) {
  const fc_ctx::OptP& O = h->opt;
  return !O.tables || O.mass_gen != h->mass_gen || O.perm_gen != h->perm_gen || O.KB != h->bat.KB;
}

// the compacted M_ff, its Jacobi diagonal, the free-row mask and the CG's buffers for the present batch width, mass values and permutation
int optp_tables(fc_ctx* h) {
  fc_ctx::OptP& O = h->opt;
  if (!optp_stale(h)) return FC_OK;
  const int N = h->N, KB = h->bat.KB, nv2 = 2 * h->nn;
  std::vector<double> val((size_t)h->nnz);
  HIPCHK(hipMemcpyAsync(val.data(), h->vals[FC_SLOT_MASS].p, val.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<unsigned char> free_w((size_t)N, 0), free_p((size_t)N, 0);
  for (int w = 0; w < nv2; ++w) free_w[(size_t)w] = 1;
  for (int q = 0; q < h->n_bc; ++q) free_w[(size_t)h->h_bc_dofs[(size_t)q]] = 0;
  std::vector<int> ip((size_t)N), rp((size_t)N + 1, 0), ci;
  std::vector<double> v, dinv((size_t)N, 0.0);
  for (int i = 0; i < N; ++i) ip[(size_t)h->h_perm[(size_t)i]] = i;
  int n_free = 0;
  for (int i = 0; i < N; ++i) {
    const int w = h->h_perm[(size_t)i];
    if (free_w[(size_t)w]) {
      free_p[(size_t)i] = 1;
      ++n_free;
      for (int q = h->h_rowptr[(size_t)w]; q < h->h_rowptr[(size_t)w + 1]; ++q) {
        const int c = h->h_col[(size_t)q];
        if (!free_w[(size_t)c]) continue;
        ci.push_back(ip[(size_t)c]);
        v.push_back(val[(size_t)q]);
        if (c == w) dinv[(size_t)i] = val[(size_t)q];
      }
      if (!(dinv[(size_t)i] > 0.0)) return fail(FC_ERR_INVALID, "fc_optpert: FC_SLOT_MASS has a non-positive diagonal entry on a free velocity row (not a mass matrix)");
      dinv[(size_t)i] = 1.0 / dinv[(size_t)i];
    }
    rp[(size_t)i + 1] = (int)ci.size();
  }
  O.nnz_ff = (int64_t)ci.size(), O.n_free = n_free;
  if (ci.empty()) ci.push_back(0), v.push_back(0.0);
  FCCHK(O.rp.upload(rp, h->stream));
  FCCHK(O.ci.upload(ci, h->stream));
  FCCHK(O.v.upload(v, h->stream));
  FCCHK(O.dinv.upload(dinv, h->stream));
  FCCHK(O.freep.upload(free_p.data(), free_p.size(), h->stream));
  const size_t blk = (size_t)N * KB;
  if (O.cg.n != 5 * blk) FCCHK(O.cg.alloc(5 * blk));
  if (O.part.n != (size_t)3 * kOptpertMaxGrid * KB) FCCHK(O.part.alloc((size_t)3 * kOptpertMaxGrid * KB));
  if (O.gpart.n != (size_t)kOptpertGramGrid * KB * KB) FCCHK(O.gpart.alloc((size_t)kOptpertGramGrid * KB * KB));
  if (O.gout.n != (size_t)KB * KB + 32) FCCHK(O.gout.alloc((size_t)KB * KB + 32));
  if (O.Q.n != (size_t)KB * KB) FCCHK(O.Q.alloc((size_t)KB * KB));
  if (O.scale.n != 32) FCCHK(O.scale.alloc(32));
  if (O.stage.n != (size_t)h->bat.k * N) FCCHK(O.stage.alloc((size_t)h->bat.k * N));
  if (O.sc.n != 1) FCCHK(O.sc.alloc(1));
  if (O.flag.n != 32) FCCHK(O.flag.alloc(32));
  FCCHK(O.cg.zero(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (the host vectors above go out of scope)
  O.KB = KB, O.mass_gen = h->mass_gen, O.perm_gen = h->perm_gen;
  O.tables = true;
  return FC_OK;
}

int optp_block(fc_ctx* h, int32_t b, const char* who, double** out) {
  fc_ctx::OptP& O = h->opt;
  if (!O.reserved || O.blocks_KB != h->bat.KB || O.blocks_perm_gen != h->perm_gen)
    return fail(FC_ERR_NOT_READY, std::string(who) + ": no resident blocks for the present batch and permutation (fc_optpert_reserve)");
  if (b < 0 || b >= fc_ctx::OptP::kBlocks) return fail(FC_ERR_INVALID, std::string(who) + ": no such block (FC_OPTPERT_U .. FC_OPTPERT_RESPONSE)");
  *out = O.blk[b].p;
  return FC_OK;
}

// y = M_ff x; dot: the workgroup partials of the column dots x . y go to O.part (null: none)
int optp_mass(fc_ctx* h, const double* x, double* y, const int* act, bool dot) {
  fc_ctx::OptP& O = h->opt;
  pick_width(O.KB, [&](auto K) {
    hipLaunchKernelGGL((fc_op_mass_b<K>), dim3(optp_grid(h->N, K)), dim3(256), 0, h->stream, h->N, (const int*)O.rp.p, (const int*)O.ci.p, (const double*)O.v.p, x, y, act,
                       dot ? O.part.p : (double*)nullptr);
  });
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// The block CG on M_ff: x = M_ff^-1 b for a block b that is zero outside f.  Iterations go out in chunks of kOptpertCgChunk; behind each
// chunk the host reads the scalars (one copy of sizeof(FcOpCgScalars) bytes, one synchronisation): ceil(iterations / chunk)
// synchronisations per solve and no other.  A block of zero columns costs one chunk of launches that write nothing.
// info [k][2]: iterations and |r| / |b| per column.  FC_ERR_NOT_CONVERGED when max_iter ran out.
int optp_cg_solve(fc_ctx* h, const double* b, double* x, double rtol, int max_iter, double* info, const char* who) {
  fc_ctx::OptP& O = h->opt;
  const int N = h->N, KB = O.KB, G = optp_grid(N, KB);
  double *r = optp_cg(h, 0), *p = optp_cg(h, 1), *ap = optp_cg(h, 2);
  FcOpCgScalars* sc = O.sc.p;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL((fc_op_cg_init<K>), dim3(G), dim3(256), 0, h->stream, N, b, (const double*)O.dinv.p, x, r, p, O.part.p + (size_t)kOptpertMaxGrid * K);
    hipLaunchKernelGGL((fc_op_cg_start<K>), dim3(1), dim3(256), 0, h->stream, G, (const double*)(O.part.p + (size_t)kOptpertMaxGrid * K), sc);
  });
  HIPCHK(hipGetLastError());
  int it = 0;
  FcOpCgScalars hs;
  hs.any_active = 1;
  while (hs.any_active && it < max_iter) {
    const int n = std::min(kOptpertCgChunk, max_iter - it);
    for (int j = 0; j < n; ++j, ++it) {
      const int q = it & 1;
      FCCHK(optp_mass(h, p, ap, sc->active[q], true));
      pick_width(KB, [&](auto K) {
        double* part = O.part.p + (size_t)kOptpertMaxGrid * K;  // [0]: p . Ap; [1], [2]: r . z and r . r
        hipLaunchKernelGGL((fc_op_cg_update<K>), dim3(G), dim3(256), 0, h->stream, N, q, (const FcOpCgScalars*)sc, G, (const double*)O.part.p, (const double*)O.dinv.p,
                           (const double*)p, (const double*)ap, x, r, part);
        hipLaunchKernelGGL((fc_op_cg_dir<K>), dim3(G), dim3(256), 0, h->stream, N, q, sc, G, (const double*)part, rtol * rtol, (const double*)O.dinv.p, (const double*)r, p);
      });
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(&hs, sc, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // the one synchronisation of the chunk
  }
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  O.solve_ms = (double)ms;
  O.cg_iters = 0;
  for (int s = 0; s < h->bat.k; ++s) {
    O.cg_iters = std::max<int64_t>(O.cg_iters, hs.iters[s]);
    if (info) info[2 * s] = (double)hs.iters[s], info[2 * s + 1] = hs.bb[s] > 0.0 ? std::sqrt(hs.rr[s] / hs.bb[s]) : (hs.bb[s] == 0.0 ? 0.0 : std::numeric_limits<double>::quiet_NaN());
  }
  if (hs.any_active) return fail(FC_ERR_NOT_CONVERGED, std::string(who) + ": the block CG on the mass matrix did not reach rtol in max_iter iterations (info holds iterations and residual per column)");
  return FC_OK;
}

// out (device, KB x KB) = X^T Y
int optp_gram(fc_ctx* h, const double* x, const double* y, double* out) {
  fc_ctx::OptP& O = h->opt;
  const int N = h->N, KB = O.KB;
  const int rows_per = std::max(16, (N + kOptpertGramGrid - 1) / kOptpertGramGrid), G = nblocks(N, rows_per);
  pick_width(KB, [&](auto K) { hipLaunchKernelGGL((fc_op_gram<K>), dim3(G), dim3(256), 0, h->stream, N, rows_per, x, y, O.gpart.p); });
  hipLaunchKernelGGL(fc_op_gram_sum, dim3(nblocks(KB * KB, 256)), dim3(256), 0, h->stream, KB * KB, G, (const double*)O.gpart.p, out);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// host [k][N] (W layout) <-> device block, through O.stage; an upload is masked to f
int optp_upload(fc_ctx* h, const double* host, double* dev) {
  fc_ctx::OptP& O = h->opt;
  HIPCHK(hipMemcpyAsync(O.stage.p, host, (size_t)h->bat.k * h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  pick_width(O.KB, [&](auto K) {
    hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)h->N * K, 256)), dim3(256), 0, h->stream, h->N, h->bat.k, (const double*)O.stage.p, dev, 1, (const int*)h->perm.p);
    hipLaunchKernelGGL((fc_op_mask<K>), dim3(nblocks((int64_t)h->N * K, 256)), dim3(256), 0, h->stream, h->N, (const unsigned char*)O.freep.p, (const double*)dev, dev);
  });
  HIPCHK(hipGetLastError());
  return FC_OK;
}
int optp_download(fc_ctx* h, const double* dev, double* host) {
  fc_ctx::OptP& O = h->opt;
  pick_width(O.KB, [&](auto K) {
    hipLaunchKernelGGL((fc_b_interleave<K>), dim3(nblocks((int64_t)h->N * K, 256)), dim3(256), 0, h->stream, h->N, h->bat.k, dev, O.stage.p, 0, (const int*)h->perm.p);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host, O.stage.p, (size_t)h->bat.k * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return FC_OK;
}

// k x k host matrix <- the KB x KB device matrix at `dev`
void optp_unpad(const std::vector<double>& pad, int KB, int k, double* out) {
  for (int a = 0; a < k; ++a)
    for (int c = 0; c < k; ++c) out[(size_t)a * k + c] = pad[(size_t)a * KB + c];
}

}  // namespace

extern "C" {

int fc_mass_solve_batch(fc_handle h, int32_t k, const double* b, double* x, double rtol, int32_t max_iter, double* info) {
  const char* who = "fc_mass_solve_batch";
  FCCHK(optp_usable(h, who));
  if (!b || !x) return fail(FC_ERR_INVALID, "fc_mass_solve_batch: null argument");
  if (k != h->bat.k) return fail(FC_ERR_INVALID, "fc_mass_solve_batch: k differs from fc_set_batch");
  if (!(rtol > 0.0) || max_iter < 1) return fail(FC_ERR_INVALID, "fc_mass_solve_batch: rtol must be positive and max_iter >= 1");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  double *db = optp_cg(h, 3), *dx = optp_cg(h, 4);
  FCCHK(optp_upload(h, b, db));
  const int code = optp_cg_solve(h, db, dx, rtol, max_iter, info, who);
  if (code != FC_OK && code != FC_ERR_NOT_CONVERGED) return code;
  int copy = optp_download(h, dx, x);
  const hipError_t sync = hipStreamSynchronize(h->stream);
  if (copy == FC_OK && sync != hipSuccess) copy = fail(FC_ERR_HIP, std::string("fc_mass_solve_batch: ") + hipGetErrorString(sync));
  return copy != FC_OK ? copy : code;
}

int fc_optpert_reserve(fc_handle h, int32_t on) {
  const char* who = "fc_optpert_reserve";
  if (!h) return fail(FC_ERR_INVALID, "fc_optpert_reserve: null handle");
  if (h->step_pending || h->bat.pending) return fail(FC_ERR_INVALID, "fc_optpert_reserve: collect the step in flight first (fc_step_end / fc_step_batch_end)");
  HIPCHK(hipSetDevice(h->device));
  fc_ctx::OptP& O = h->opt;
  if (!on) {
    FCCHK(quiesce(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    O.release();
    return FC_OK;
  }
  FCCHK(optp_usable(h, who));
  if (h->nonlinear) return fail(FC_ERR_INVALID, "fc_optpert_reserve: the time scheme is nonlinear: optimal perturbations are those of the linearised stepper (fc_set_time_scheme)");
  // what a run will use: the batched march on both slots (a run of one step needs its first slot only; the reserve cannot know n)
  for (int slot = 0; slot < 2; ++slot) {
    if (!h->adjb.on[slot]) continue;
    FCCHK(adjb_usable(h, slot, h->bat.k, who));
  }
  if (!h->adjb.on[0] && !h->adjb.on[1]) return fail(FC_ERR_NOT_READY, "fc_optpert_reserve: no batched adjoint setup (fc_set_adjoint_batch on the slots a run will use)");
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  const size_t blk = (size_t)h->N * O.KB;
  int code = FC_OK;
  for (DevBuf<double>& b : O.blk) {
    if (code == FC_OK && b.n != blk) code = b.alloc(blk);
    if (code == FC_OK) code = b.zero(h->stream);
  }
  if (code == FC_OK && O.rec.n != (size_t)fc_rec::kPinDoubles) code = O.rec.alloc((size_t)fc_rec::kPinDoubles);
  if (code == FC_OK && hipStreamSynchronize(h->stream) != hipSuccess) code = fail(FC_ERR_HIP, "fc_optpert_reserve: clearing the blocks failed");
  if (code != FC_OK) {
    O.release();
    (void)hipGetLastError();
    return code;
  }
  O.reserved = true;
  O.blocks_KB = O.KB, O.blocks_perm_gen = h->perm_gen;  // (set here only: a later rebuild of the tables does not make old blocks valid)
  return FC_OK;
}

int fc_optpert_load(fc_handle h, int32_t block, int32_t k, const double* X) {
  const char* who = "fc_optpert_load";
  FCCHK(optp_usable(h, who));
  if (!X) return fail(FC_ERR_INVALID, "fc_optpert_load: null argument");
  if (k != h->bat.k) return fail(FC_ERR_INVALID, "fc_optpert_load: k differs from fc_set_batch");
  double* d = nullptr;
  FCCHK(optp_block(h, block, who, &d));
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  return adj_enqueue_and_sync(h, who, nullptr, [&]() -> int { return optp_upload(h, X, d); });
}

int fc_optpert_get(fc_handle h, int32_t block, int32_t k, double* out) {
  const char* who = "fc_optpert_get";
  FCCHK(optp_usable(h, who));
  if (!out) return fail(FC_ERR_INVALID, "fc_optpert_get: null argument");
  if (k != h->bat.k) return fail(FC_ERR_INVALID, "fc_optpert_get: k differs from fc_set_batch");
  double* d = nullptr;
  FCCHK(optp_block(h, block, who, &d));
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  return adj_enqueue_and_sync(h, who, nullptr, [&]() -> int { return optp_download(h, d, out); });
}

int fc_optpert_mass_solve(fc_handle h, int32_t dst_block, int32_t src_block, double rtol, int32_t max_iter, double* info) {
  const char* who = "fc_optpert_mass_solve";
  FCCHK(optp_usable(h, who));
  if (!(rtol > 0.0) || max_iter < 1) return fail(FC_ERR_INVALID, "fc_optpert_mass_solve: rtol must be positive and max_iter >= 1");
  double *dst = nullptr, *src = nullptr;
  FCCHK(optp_block(h, dst_block, who, &dst));
  FCCHK(optp_block(h, src_block, who, &src));
  if (dst == src) return fail(FC_ERR_INVALID, "fc_optpert_mass_solve: dst and src must be different blocks");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  return optp_cg_solve(h, src, dst, rtol, max_iter, info, who);
}

int fc_optpert_gram(fc_handle h, int32_t a_block, int32_t b_block, int32_t weighted, double* out) {
  const char* who = "fc_optpert_gram";
  FCCHK(optp_usable(h, who));
  if (!out) return fail(FC_ERR_INVALID, "fc_optpert_gram: null argument");
  double *a = nullptr, *b = nullptr;
  FCCHK(optp_block(h, a_block, who, &a));
  FCCHK(optp_block(h, b_block, who, &b));
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  fc_ctx::OptP& O = h->opt;
  const int KB = O.KB, k = h->bat.k;
  std::vector<double> pad((size_t)KB * KB);
  FCCHK(adj_enqueue_and_sync(h, who, nullptr, [&]() -> int {
    const double* y = b;
    if (weighted) {
      FCCHK(optp_mass(h, b, optp_cg(h, 2), nullptr, false));  // (M_ff Y into the CG's Ap block: no solve is in flight)
      y = optp_cg(h, 2);
    }
    FCCHK(optp_gram(h, a, y, O.gout.p));
    HIPCHK(hipMemcpyAsync(pad.data(), O.gout.p, pad.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return FC_OK;
  }));
  optp_unpad(pad, KB, k, out);
  return FC_OK;
}

int fc_optpert_combine(fc_handle h, int32_t dst_block, int32_t src_block, const double* Q, const double* scale, int32_t accumulate) {
  const char* who = "fc_optpert_combine";
  FCCHK(optp_usable(h, who));
  if (!Q) return fail(FC_ERR_INVALID, "fc_optpert_combine: null argument");
  double *dst = nullptr, *src = nullptr;
  FCCHK(optp_block(h, dst_block, who, &dst));
  FCCHK(optp_block(h, src_block, who, &src));
  if (dst == src) return fail(FC_ERR_INVALID, "fc_optpert_combine: dst and src must be different blocks");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  FCCHK(optp_tables(h));
  fc_ctx::OptP& O = h->opt;
  const int KB = O.KB, k = h->bat.k;
  std::vector<double> pad((size_t)KB * KB, 0.0), sc(32, 0.0);
  for (int a = 0; a < k; ++a)
    for (int c = 0; c < k; ++c) pad[(size_t)a * KB + c] = Q[(size_t)a * k + c];
  if (scale) std::copy(scale, scale + k, sc.begin());
  return adj_enqueue_and_sync(h, who, nullptr, [&]() -> int {
    HIPCHK(hipMemcpyAsync(O.Q.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (scale) HIPCHK(hipMemcpyAsync(O.scale.p, sc.data(), 32 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    pick_width(KB, [&](auto K) {
      hipLaunchKernelGGL((fc_op_combine<K>), dim3(nblocks((int64_t)h->N * K, 256)), dim3(256), 0, h->stream, h->N, k, (const double*)src, (const double*)O.Q.p,
                         scale ? (const double*)O.scale.p : (const double*)nullptr, accumulate ? 1 : 0, dst);
    });
    HIPCHK(hipGetLastError());
    return FC_OK;
  });
}

int fc_optpert_apply(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, double* H_out, double* E_out, int32_t* flags_out) {
  const char* who = "fc_optpert_apply";
  FCCHK(optp_usable(h, who));
  if (first_order_slot != FC_SLOT_BDF1 && first_order_slot != FC_SLOT_BDF2) return fail(FC_ERR_INVALID, "fc_optpert_apply: first_order_slot must be BDF1/BDF2");
  if (n_steps < 1) return fail(FC_ERR_INVALID, "fc_optpert_apply: n_steps must be at least 1");
  if (k != h->bat.k) return fail(FC_ERR_INVALID, "fc_optpert_apply: k differs from fc_set_batch");
  if (h->adjen.n > 0) return fail(FC_ERR_INVALID, "fc_optpert_apply: energy weights are held (fc_set_adjoint_energy): the backward march would add them to K U");
  if (h->nonlinear) return fail(FC_ERR_INVALID, "fc_optpert_apply: the time scheme is nonlinear");
  double *U = nullptr, *Gb = nullptr, *Y = nullptr;
  FCCHK(optp_block(h, FC_OPTPERT_U, who, &U));
  FCCHK(optp_block(h, FC_OPTPERT_G, who, &Gb));
  FCCHK(optp_block(h, FC_OPTPERT_RESPONSE, who, &Y));
  FCCHK(batch_ready(h, first_order_slot, k, who));
  FCCHK(adjb_step_ready(h, first_order_slot, k, who));
  if (n_steps > 1) {
    FCCHK(batch_ready(h, FC_SLOT_BDF2, k, who));
    FCCHK(adjb_step_ready(h, FC_SLOT_BDF2, k, who));
  }
  FCCHK(adj_march_prepare(h, first_order_slot, n_steps, k));
  FCCHK(optp_tables(h));
  fc_ctx::OptP& O = h->opt;
  fc_ctx::Batch& B = h->bat;
  fc_ctx::AdjB& A = h->adjb;
  const int N = h->N, KB = B.KB;
  const size_t lvl = (size_t)N * KB;
  // the state is set from here: what fc_set_state_batch ends, ends
  B.pre_slot = -1;
  h->pre_slot = -1;
  adj_tape_end(h);
  std::vector<double> Hp((size_t)KB * KB), Ep(32);
  int fwd[32] = {0}, bwd[32] = {0}, mine[32] = {0};
  struct RecGuard {  // the batched launches go back to the host-mapped page whatever happens below
    fc_ctx::Batch& B;
    ~RecGuard() { B.rec_dev = nullptr; }
  } guard{B};
  O.fwd_steps = O.bwd_steps = 0;
  FCCHK(adj_enqueue_and_sync(h, who, &O.apply_ms, [&]() -> int {
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // forward: x_0 = U, x_{-1} = 0, zero controls in a record page of its own, n_steps batched steps back to back
    FCCHK(O.rec.zero(h->stream));
    FCCHK(B.flag.zero(h->stream));
    FCCHK(O.flag.zero(h->stream));
    HIPCHK(hipMemcpyAsync(bat_n(h), U, lvl * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetAsync(bat_nn(h), 0, lvl * sizeof(double), h->stream));
    B.rec_dev = O.rec.p;
    for (int s = 0; s < n_steps; ++s) {
      B.pend_checked = false;  // (no residual monitor, no energy: nothing of a step is read back)
      ++B.step_count;
      FCCHK(batch_enqueue(h, s == 0 ? first_order_slot : FC_SLOT_BDF2, 0, false));
      ++O.fwd_steps;
    }
    B.rec_dev = nullptr;
    // response block, terminal weight z = M_ff x_n (x_n is zero outside f), energies from the same pass
    HIPCHK(hipMemcpyAsync(Y, bat_n(h), lvl * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    pick_width(KB, [&](auto K) {
      hipLaunchKernelGGL((fc_op_finite<K>), dim3(nblocks((int64_t)lvl, 256)), dim3(256), 0, h->stream, N, (const double*)Y, O.flag.p);
    });
    FCCHK(adjb_reset(h, nullptr));
    FCCHK(optp_mass(h, Y, A.term.p, nullptr, true));
    hipLaunchKernelGGL(fc_op_gram_sum, dim3(1), dim3(256), 0, h->stream, KB, optp_grid(N, KB), (const double*)O.part.p, O.gout.p + (size_t)KB * KB);
    // backward: the batched march's schedule with the terminal and the dx0 product on the device
    FCCHK(adj_march(
        h, first_order_slot, n_steps, nullptr, lvl, Gb, nullptr,
        [&](int m, int slot, const StepCoeffs& c, const double* xm, const double* er) {
          ++O.bwd_steps;
          return adjb_enqueue_step(h, slot, c, xm, nullptr, m == n_steps ? A.term.p : nullptr, A.gseq.p + (size_t)(m - 1) * (size_t)k * h->n_act, true, er);
        },
        [&](const StepCoeffs& c, const double* xm, int, double* dst) -> int {
          FCCHK(adjb_enqueue_rhs(h, c, xm, nullptr, nullptr));
          pick_width(KB, [&](auto K) {
            hipLaunchKernelGGL((fc_op_mask<K>), dim3(nblocks((int64_t)lvl, 256)), dim3(256), 0, h->stream, N, (const unsigned char*)O.freep.p, (const double*)A.b.p, dst);
          });
          HIPCHK(hipGetLastError());
          return FC_OK;
        }));
    FCCHK(optp_gram(h, U, Gb, O.gout.p));
    HIPCHK(hipMemcpyAsync(Hp.data(), O.gout.p, Hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(Ep.data(), O.gout.p + (size_t)KB * KB, 32 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(fwd, B.flag.p, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(bwd, A.flag.p, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(mine, O.flag.p, 32 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return FC_OK;
  }));
  ++O.applies;
  if (H_out) optp_unpad(Hp, KB, k, H_out);
  int any = 0;
  for (int s = 0; s < k; ++s) {
    const int f = (fwd[s] || bwd[s] || mine[s]) ? 1 : 0;
    if (E_out) E_out[s] = 0.5 * Ep[(size_t)s];
    if (flags_out) flags_out[s] = f;
    any |= f;
  }
  if (any) return fail(FC_ERR_DIVERGED, "fc_optpert_apply: non-finite state in a column (flags_out marks the columns; the others are valid)");
  return FC_OK;
}

// a resident block as it lies on the device, out [N][kb] in the permuted numbering, padding columns included (test aid)
int fc_debug_get_optpert_block(fc_handle h, int32_t block, int32_t kb, double* out) {
  const char* who = "fc_debug_get_optpert_block";
  FCCHK(optp_usable(h, who));
  if (!out) return fail(FC_ERR_INVALID, "fc_debug_get_optpert_block: null argument");
  double* d = nullptr;
  FCCHK(optp_block(h, block, who, &d));
  if (kb != h->opt.blocks_KB) return fail(FC_ERR_INVALID, "fc_debug_get_optpert_block: kb differs from the padded width (fc_optpert_info)");
  HIPCHK(hipSetDevice(h->device));
  FCCHK(quiesce(h));
  return adj_enqueue_and_sync(h, who, nullptr, [&]() -> int {
    HIPCHK(hipMemcpyAsync(out, d, (size_t)h->N * (size_t)kb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return FC_OK;
  });
}

int fc_optpert_info(fc_handle h, int64_t* info, double* dinfo) {
  if (!h) return fail(FC_ERR_INVALID, "fc_optpert_info: null handle");
  const fc_ctx::OptP& O = h->opt;
  if (info) {
    info[0] = O.reserved ? 1 : 0;
    info[1] = (O.tables && optp_stale(h)) ? 1 : 0;
    info[2] = O.bytes();
    info[3] = O.KB;
    info[4] = O.applies;
    info[5] = O.cg_iters;
    info[6] = O.fwd_steps;
    info[7] = O.bwd_steps;
  }
  if (dinfo) dinfo[0] = O.apply_ms, dinfo[1] = O.solve_ms;
  return FC_OK;
}

}  // extern "C"
