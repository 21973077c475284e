// Complex-shifted direct solver (fc_setup_shifted ... fc_release_shifted): host side.  Included at the end of fc_hip.hip,
// whose handle internals (fc_ctx, OrderSys, DevBuf, the sweep / elimination launchers) it uses.
//
// M = sigma E - A in its real-equivalent form: dof i -> the pair (2 i, 2 i + 1), entry m -> [[mr, -mi], [mi, mr]].  The doubled system
// gets a solver context of its own (`in`: stream, tree permutation, sweep tables, factorisation plan, fronts, factor values, work
// buffer) built by the same symbolic phase and eliminated by the same front kernels as the real operators; only the scatter of the
// matrix into the fronts (fc_shifted_scatter) and the residual (fc_shifted_spmv) know that the entries are complex.  Nothing of the
// handle's own solver state (sys[0/1], perm, sym_*, perm_gen, slots) is read or written.
//
// Enclosed flows (fc_shifted_set_pin): M' = M + s e_k e_k^T, the shift added to the two diagonal front slots of dof k after the scatter
// and to row k of every residual.  Krylov (fc_shifted_set_krylov): right-preconditioned complex GMRES(m) on the device, mat-vec at the
// operator's CURRENT shift, preconditioner = the held factors of the FACTORED shift -- the rescue of a solve whose refinement steps
// stall, and the solve on lagged factors after fc_shifted_set_shift.
//
// Block solves (fc_shifted_set_block / fc_solve_shifted_block): `in` is an fc_ctx, so the batched factor apply of fc_set_batch
// (build_batch_tables, batch_repack, batch_apply) runs on it: k <= 32 complex columns are k columns of that apply, and the factors are
// read once per GMRES iteration for all of them.  Every column is the GMRES of shifted_gmres at a shift of its own, in lock step.
//
// Adjoint (fc_shifted_set_adjoint): a SECOND factor-value array in the identical layout holds the per-front transposition of the values
// (fc_fe_export_t, one more export pass over the fronts, which stay intact after the elimination).  In the real-equivalent form the
// transpose of the doubled matrix is the doubled form of M^H, so every apply path above solves with M^H = conj(sigma) E^T - A^T once
// in->sys[0].f_val names that array: a pointer swap (shifted_use).  The mat-vecs then run on (a_t, e_t), the values of A^T and E^T on
// the handle's own pattern (fc_csr_gather_values), with the conjugated shift.
//
// Snapshot sets (fc_shifted_snap_*): up to three sets of complex columns in the layout of xz.  A push is a scaled copy of the last
// solutions; a Gram L^T Op R runs the operator on <= 32 right-hand columns at a time (fc_shifted_spmv on the held direct values, no pin)
// and multiplies with fc_snap_gram, slices of N on different workgroups, their partials added in slice order (no atomics).  Nothing
// of it is allocated or launched unless a set is reserved.
#pragma once

struct ShiftedSolver {
  fc_ctx* in = nullptr;   // the doubled system's solver context
  int n = 0;              // complex order (= N of the handle)
  int64_t nnz = 0;        // entries of the handle's pattern
  double s_re = 0.0, s_im = 0.0;  // the operator's shift (residuals, mat-vecs)
  double f_re = 0.0, f_im = 0.0;  // the shift the held factors belong to (differs after fc_shifted_set_shift)
  int refine = 2;
  // pressure pin (fc_shifted_set_pin): dof (W numbering, -1 none), shift, the two diagonal front slots
  int pin_dof = -1;
  double pin_shift = 0.0;
  DevBuf<int64_t> pin_slot;
  DevBuf<double> pin_val;
  int pin_slot_dof = -1;       // the dof whose two diagonal front slots shifted_build looked up
  int64_t pin_slot_h[2] = {-1, -1};
  // Krylov (fc_shifted_set_krylov): max_iter = 0 is off
  int k_max_iter = 0, k_restart = 0;
  double k_rtol = 0.0;
  DevBuf<double> KV, kt, kz, gm, kh;  // basis [(restart + 1)][n] complex, combination, preconditioned vector, rotations / record, projections
  std::vector<int> last_iters;
  int64_t n_refactor = 0, n_apply = 0, n_matvec = 0, n_gmres = 0, n_rescue = 0;  // n_gmres: solves that ran GMRES; n_rescue: of them, rescues
  bool pin_dirty = false;  // the pin's value changed since it was uploaded
  bool factored = false;
  DevBuf<double> a, e;        // held values of A and E (handle's CSR pattern)
  DevBuf<int64_t> dst4;       // [nnz][4]: front slots of the 2x2 block of every entry
  DevBuf<double> bz, xz;      // right-hand sides / solutions of the last fc_solve_shifted: [nrhs][n] interleaved complex
  DevBuf<double> rz, wz, st;  // residual, operator work vector, staging of split host vectors ([2][n])
  DevBuf<double> part, scal;  // reductions
  DevBuf<double> V, T, Q, hd; // Arnoldi basis [(m + 1)][n] complex, combination target [m][n], small complex matrix, projections
  int m = 0;                  // basis vectors beyond the first
  int nrhs_last = 0;
  std::vector<double> last_res;
  double refactor_ms = 0.0, refactor_flops = 0.0;
  int64_t factor_values = 0;
  // block solves (fc_shifted_set_block): width, the doubled system's tree and factor layout (what the batched apply's tables are built
  // from), block vectors [2 n][KB] -- right-hand sides, iterates, residuals, combination, preconditioned vector, basis [(restart + 1)]
  int blk_k = 0, blk_KB = 0;
  int64_t blk_launched = 0, blk_cycles = 0;  // last block solve: lock-step iterations launched, cycles that ran any
  fcsym::Tree sym_tree;
  fcsym::Factors sym_fac;
  DevBuf<double> BB, BX, BR, BT, BZ, BKV, Bgm, Bh, Bsh, Bres2, Bpart, Bst;
  // adjoint (fc_shifted_set_adjoint): f_other is the factor-value array in->sys[0].f_val does NOT name at the moment (the adjoint one
  // while adj_cur is false, the direct one while it is true); adj_on is the mode the API set, adj_cur what the sweeps read right now
  // (they differ only inside the resolvent operator); a_t, e_t, tpos: the transposed matrix values and the map that gathers them
  bool adj_avail = false, adj_on = false, adj_cur = false;
  DevBuf<double> f_other, a_t, e_t;
  DevBuf<int> tpos;
  DevBuf<FcExpTItem> texp;  // work list of fc_fe_export_t
  int64_t texp_n = 0, n_texport = 0, n_switch = 0;
  double texp_ms = 0.0, texp_bytes = 0.0;
  int arn_kind = 0;          // Arnoldi operator: 0 shift-invert, 1 resolvent (fc_shifted_arnoldi_set_op)
  // snapshot sets (fc_shifted_snap_*): 0 direct solutions, 1 adjoint solutions, 2 loaded vectors; [col][n] interleaved complex like xz.
  // snap_w: Op * (a chunk of <= 32 right-hand columns), snap_part: the slice partials of a Gram, snap_out: their sum; they live only while a
  // set does
  DevBuf<double> snap[3], snap_w, snap_part, snap_out;
  int snap_cnt[3] = {0, 0, 0}, snap_cap[3] = {0, 0, 0};
  int64_t n_gram = 0;
  double gram_ms = 0.0, gram_bytes = 0.0, gram_flops = 0.0;  // the last fc_shifted_snap_gram (HIP events; algorithmic bytes and flops)
  bool arn_started = false;  // a mode switch drops a started Arnoldi
  ~ShiftedSolver() {
    if (!in) return;
    (void)hipStreamSynchronize(in->stream);
    if (in->ev0) (void)hipEventDestroy(in->ev0);
    if (in->ev1) (void)hipEventDestroy(in->ev1);
    hipStream_t s = in->stream;
    delete in;
    if (s) (void)hipStreamDestroy(s);
  }
};

static void shifted_free(fc_ctx* h) {
  delete h->shf;
  h->shf = nullptr;
}

namespace {

// the handle's CSR pattern doubled: row 2 i + a holds, for every entry k = (i, j), the columns 2 j, 2 j + 1; code[q] = 4 k + 2 a + b names
// the entry and the block position behind doubled CSR index q
void doubled_pattern(const std::vector<int>& rp, const std::vector<int>& col, std::vector<int>& rp2, std::vector<int>& col2,
                     std::vector<int64_t>& code) {
  const int N = (int)rp.size() - 1;
  const int64_t nnz = rp[(size_t)N];
  rp2.assign(2 * (size_t)N + 1, 0);
  col2.resize(4 * (size_t)nnz);
  code.resize(4 * (size_t)nnz);
  for (int i = 0; i < N; ++i) {
    const int len = rp[i + 1] - rp[i];
    for (int a = 0; a < 2; ++a) {
      const int64_t r0 = 4 * (int64_t)rp[i] + 2 * (int64_t)a * len;
      rp2[2 * (size_t)i + a] = (int)r0;
      for (int q = 0; q < len; ++q) {
        const int64_t k = rp[i] + q;
        for (int b = 0; b < 2; ++b) {
          col2[(size_t)(r0 + 2 * q + b)] = 2 * col[(size_t)k] + b;
          code[(size_t)(r0 + 2 * q + b)] = 4 * k + 2 * a + b;
        }
      }
    }
  }
  rp2[2 * (size_t)N] = (int)(4 * nnz);
}

// every cell's 15 dofs -> 30 (the pair of each), same centroids
std::vector<int> doubled_cell_dofs(const std::vector<int>& cd) {
  std::vector<int> cd2(2 * cd.size());
  for (size_t q = 0; q < cd.size(); ++q) cd2[2 * q] = 2 * cd[q], cd2[2 * q + 1] = 2 * cd[q] + 1;
  return cd2;
}

struct ShiftedSym {
  fcsym::Tree t;
  fcsym::Factors fac;
  fcsym::Plan pl;
};

// the symbolic phase of the doubled system through the real solver's code: tree (30 dofs per cell, the default shape of the mesh, no
// skipped dofs: general matrices), factor layout, elimination plan
ShiftedSym shifted_symbolic(const std::vector<int>& cd, const std::vector<double>& cent, int nc, const std::vector<int>& rp2,
                            const std::vector<int>& col2, int depth, int merge) {
  ShiftedSym y;
  const int N2 = (int)rp2.size() - 1;
  const std::vector<int> bits = depth == 0 ? fcsym::default_bits(nc, merge, 0) : fcsym::uniform_bits(depth, merge, 0);
  y.t = fcsym::build_tree(doubled_cell_dofs(cd), 30, cent, nc, N2, bits, nullptr, 0);
  y.fac = fcsym::layout_factors(y.t, fcsym::Keep{});
  y.pl = fcsym::factor_plan(y.t, y.fac, rp2, col2, nullptr, fcsym::Keep{});
  return y;
}

// device bytes of the adjoint side: the second factor-value array, the transposed matrix values and their map, the export's work list
int64_t shifted_adjoint_bytes(const ShiftedSolver& Z) {
  return 8 * (int64_t)(Z.f_other.n + Z.a_t.n + Z.e_t.n) + 4 * (int64_t)Z.tpos.n + (int64_t)sizeof(FcExpTItem) * (int64_t)Z.texp.n;
}

// device bytes of the snapshot sets and their workspaces
int64_t shifted_snap_bytes(const ShiftedSolver& Z) {
  return 8 * (int64_t)(Z.snap[0].n + Z.snap[1].n + Z.snap[2].n + Z.snap_w.n + Z.snap_part.n + Z.snap_out.n);
}

int64_t shifted_bytes(const ShiftedSolver& Z) {
  const fc_ctx* in = Z.in;
  int64_t b = 8 * (int64_t)(Z.a.n + Z.e.n + Z.dst4.n + Z.bz.n + Z.xz.n + Z.rz.n + Z.wz.n + Z.st.n + Z.part.n + Z.scal.n + Z.V.n + Z.T.n +
                            Z.Q.n + Z.hd.n + Z.pin_slot.n + Z.pin_val.n + Z.KV.n + Z.kt.n + Z.kz.n + Z.gm.n + Z.kh.n);
  b += 8 * (int64_t)(Z.BB.n + Z.BX.n + Z.BR.n + Z.BT.n + Z.BZ.n + Z.BKV.n + Z.Bgm.n + Z.Bh.n + Z.Bsh.n + Z.Bres2.n + Z.Bpart.n + Z.Bst.n);
  b += shifted_adjoint_bytes(Z);
  b += shifted_snap_bytes(Z);
  if (!in) return b;
  const OrderSys& S = in->sys[0];
  const fc_ctx::Batch& T = in->bat;  // the batched apply of a block: tiled factor copy, work buffer, tables
  b += 8 * (int64_t)(T.ftile[0].n + T.ring.n + T.part.n) + (int64_t)sizeof(FcBTask) * (int64_t)T.tasks.n +
       4 * (int64_t)(T.ticket.n + T.olist.n + T.fptr.n + T.fsrc.n);
  b += 8 * (int64_t)(in->fronts.n + in->pscratch.n + S.f_val.n + in->ring.n + in->pa_src.n + in->pa_dst.n + S.seg_ptr.n);
  b += (int64_t)sizeof(FcSeg) * (int64_t)S.seg.n + (int64_t)sizeof(FcBlk) * (int64_t)S.blk.n +
       4 * (int64_t)(S.f_idx.n + S.wg_order.n + in->perm.n + in->iperm.n + in->pext_p.n);
  b += (int64_t)sizeof(FcFront) * (int64_t)in->pfront.n + (int64_t)sizeof(FcExt) * (int64_t)(in->pext.n + in->pext2.n) +
       (int64_t)sizeof(FcExpItem) * (int64_t)in->pexp.n;
  return b;
}

int shifted_build(fc_ctx* h, ShiftedSolver& Z) {
  const int N = h->N, N2 = 2 * N;
  std::vector<int> rp2, col2;
  std::vector<int64_t> code;
  doubled_pattern(h->h_rowptr, h->h_col, rp2, col2, code);
  ShiftedSym y = shifted_symbolic(h->h_cell_dofs, h->h_cent, h->nc, rp2, col2, 0, 2);
  const fcsym::Plan& pl = y.pl;
  const fcsym::Factors& fac = y.fac;
  // (entry, block position) -> front slot; every one of the 4 nnz has exactly one
  std::vector<int64_t> dst4(4 * (size_t)h->nnz, -1);
  for (size_t q = 0; q < pl.a_src.size(); ++q) dst4[(size_t)code[(size_t)pl.a_src[q]]] = pl.a_dst[q];
  for (int64_t v : dst4)
    if (v < 0 || v >= pl.front_size) return fail(FC_ERR_INVALID, "fc_setup_shifted: an entry of the doubled matrix has no front slot");
  fcsym::Partition part = fcsym::partition(y.t, fac, 0, 1);
  fcsym::Blocks B = fcsym::down_blocks(y.t, fac, 0, 1, 32, block_target(N2), 512);
  retile_flat(B);
  // the doubled system's own context: no mesh, no state, no sensors -- a stream, a permutation, one solver slot and its plan
  fc_ctx* in = new fc_ctx();
  Z.in = in;
  in->device = h->device;
  in->n_cu = h->n_cu;
  in->up_form = 1;  // row-form up-sweeps (the column form's tables come from the handle's symbolic state, which `in` does not keep)
  HIPCHK(hipStreamCreateWithFlags(&in->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&in->ev0));
  HIPCHK(hipEventCreate(&in->ev1));
  in->N = N2;
  in->nnz = 4 * h->nnz;
  in->h_perm = y.t.perm;
  FCCHK(in->perm.upload(y.t.perm, in->stream));
  FCCHK(in->iperm.upload(y.t.iperm, in->stream));
  in->have_perm = true;
  FCCHK(in->ring.alloc(2 * (size_t)N2));
  FCCHK(in->ring.zero(in->stream));
  in->buf.p = in->ring.p;
  in->buf.n = in->ring.n;
  FCCHK(in->flag.alloc(1));
  FCCHK(in->flag.zero(in->stream));
  // the sweeps never read the permuted system matrix (residuals run through fc_shifted_spmv): a one-entry stand-in
  std::vector<int> ap_rp((size_t)N2 + 1, 1);
  ap_rp[0] = 0;
  const int ap_col = 0;
  const int64_t ap_src = 0, zero64 = 0;
  const int zero32 = 0;
  FCCHK(fc_solver_setup(in, 0, ap_rp.data(), &ap_col, nullptr, (int)part.stage_kind.size(), part.stage_begin.data(), part.stage_row0.data(),
                        part.stage_nrows.data(), part.stage_kind.data(), part.seg_ptr.data(), (int64_t)part.seg_val.size(),
                        part.seg_val.empty() ? &zero64 : part.seg_val.data(), part.seg_col.empty() ? &zero32 : part.seg_col.data(),
                        part.seg_len.empty() ? &zero32 : part.seg_len.data(), (int64_t)fac.idx.size(), fac.idx.empty() ? &zero32 : fac.idx.data(),
                        std::max<int64_t>(1, fac.n_val), nullptr, -1, 0, 0, -1));
  FCCHK(fc_solver_set_blocks(in, 0, (int)B.begin.size(), B.begin.data(), B.count.data(), B.lpr.data(), (int64_t)B.val.size(),
                             B.val.empty() ? &zero64 : B.val.data(), B.row0.empty() ? &zero32 : B.row0.data(),
                             B.nrows.empty() ? &zero32 : B.nrows.data(), B.i0.empty() ? &zero32 : B.i0.data(), B.ni.empty() ? &zero32 : B.ni.data(),
                             B.idx.empty() ? &zero32 : B.idx.data(), B.nb.empty() ? &zero32 : B.nb.data(), (int64_t)fac.idx.size(),
                             std::max<int64_t>(1, fac.n_val)));
  FCCHK(fc_factor_plan(in, (int)(pl.nodes.size() / 7), pl.nodes.data(), (int)pl.level_ptr.size() - 1, pl.level_ptr.data(), pl.front_size,
                       (int64_t)pl.a_src.size(), pl.a_src.empty() ? &zero64 : pl.a_src.data(), pl.a_dst.empty() ? &zero64 : pl.a_dst.data(),
                       pl.a_ptr.data(), pl.ext_off.data(), (int64_t)pl.ext_p.size(), pl.ext_p.data(), 1, &ap_src, pl.max_slots));
  FCCHK(fc_set_root_rows(in, -1, 0));
  // the scatter reads (entry, position) -> slot directly: the plan's own scatter lists are not kept on the device
  in->pa_src.release();
  in->pa_dst.release();
  FCCHK(Z.dst4.upload(dst4, in->stream));
  Z.factor_values = fac.n_val;
  // the diagonal front slots (2k, 2k), (2k + 1, 2k + 1) of the pinned dof k, looked up once (as apply_pressure_pin does for the real solver)
  Z.pin_slot_dof = -1;
  if (Z.pin_dof >= 0) {
    for (int a = 0; a < 2; ++a) {
      const int ip = y.t.iperm[2 * (size_t)Z.pin_dof + a];
      int64_t slot = -1;
      for (size_t g = 0; g < pl.node_i0.size() && slot < 0; ++g) {
        const int64_t i0 = pl.node_i0[g], nf = pl.nodes[g * 7 + 2], ni = pl.nodes[g * 7 + 3];
        if (ip >= i0 && ip < i0 + ni) slot = pl.nodes[g * 7 + 1] + (ip - i0) * (nf + 1);
      }
      if (slot < 0 || slot >= pl.front_size) return fail(FC_ERR_INVALID, "fc_setup_shifted: the pinned dof has no diagonal front slot");
      Z.pin_slot_h[a] = slot;
    }
    Z.pin_slot_dof = Z.pin_dof;
  }
  const size_t n2 = 2 * (size_t)N;
  FCCHK(Z.rz.alloc(n2));
  FCCHK(Z.wz.alloc(n2));
  FCCHK(Z.st.alloc(n2));
  FCCHK(Z.part.alloc(2 * (size_t)nblocks(N, 8) + 4096));
  FCCHK(Z.scal.alloc(8));
  HIPCHK(hipStreamSynchronize(in->stream));
  Z.sym_tree = std::move(y.t);
  Z.sym_fac = std::move(y.fac);
  return FC_OK;
}

// (the transpose-position map of a pattern and the work list of fc_fe_export_t: transpose_map, export_t_items in fc_hip.hip -- the
// adjoint time stepping builds its transposed factors with the same two)
int shifted_transpose_map(const std::vector<int>& rp, const std::vector<int>& col, std::vector<int>& tpos) {
  return transpose_map(rp, col, tpos, "fc_shifted_set_adjoint");
}

void shifted_use(ShiftedSolver& Z, bool adjoint);  // (below)

// everything fc_shifted_set_adjoint holds; the direct array goes back under in->sys[0].f_val first
void shifted_release_adjoint(ShiftedSolver& Z) {
  if (Z.in && Z.f_other.p) shifted_use(Z, false);
  Z.f_other.release(), Z.a_t.release(), Z.e_t.release(), Z.tpos.release(), Z.texp.release();
  Z.texp_n = 0;
  Z.adj_avail = Z.adj_on = Z.adj_cur = false;
  if (Z.arn_kind == 1) Z.arn_kind = 0, Z.arn_started = false;
}

// which factor-value array the sweeps read: a pointer swap; the block's tiled copy goes stale (repacked by the next block solve)
void shifted_use(ShiftedSolver& Z, bool adjoint) {
  if (adjoint == Z.adj_cur) return;
  std::swap(Z.in->sys[0].f_val.p, Z.f_other.p);
  Z.adj_cur = adjoint;
  Z.in->bat.ftile_ok[0] = false;
}

// the imaginary part of the shift the mat-vecs of a solve run at: M^H = conj(sigma) E^T - A^T while the adjoint array is in use
inline double shifted_sim(const ShiftedSolver& Z) { return Z.adj_cur ? -Z.s_im : Z.s_im; }

// the adjoint factor values from the fronts the last elimination left (one launch; timed on its own)
int shifted_export_adjoint(ShiftedSolver& Z) {
  fc_ctx* in = Z.in;
  double* dst = Z.adj_cur ? in->sys[0].f_val.p : Z.f_other.p;
  HIPCHK(hipEventRecord(in->ev0, in->stream));
  if (Z.texp_n > 0)
    hipLaunchKernelGGL(fc_fe_export_t, dim3((unsigned)Z.texp_n), dim3(256), 0, in->stream, in->pfront.p, Z.texp.p, in->fronts.p, dst);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(in->ev1, in->stream));
  HIPCHK(hipEventSynchronize(in->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, in->ev0, in->ev1));
  Z.texp_ms = (double)ms;
  Z.texp_bytes = 16.0 * (double)Z.factor_values;  // every value read once from the fronts and written once
  ++Z.n_texport;
  return FC_OK;
}

// a_t, e_t from the held values
int shifted_gather_transposed(ShiftedSolver& Z) {
  hipLaunchKernelGGL(fc_csr_gather_values, dim3(nblocks(Z.nnz, 256)), dim3(256), 0, Z.in->stream, Z.nnz, Z.tpos.p, Z.a.p, Z.e.p, Z.a_t.p, Z.e_t.p);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

int shifted_refactor(ShiftedSolver& Z) {
  fc_ctx* in = Z.in;
  OrderSys& S = in->sys[0];
  shifted_use(Z, false);  // the elimination exports the direct values into the array f_val names
  HIPCHK(hipEventRecord(in->ev0, in->stream));
  HIPCHK(hipMemsetAsync(in->fronts.p, 0, in->fronts.n * sizeof(double), in->stream));
  hipLaunchKernelGGL(fc_shifted_scatter, dim3(nblocks(Z.nnz, 256)), dim3(256), 0, in->stream, Z.nnz, Z.dst4.p, Z.a.p, Z.e.p, Z.s_re, Z.s_im,
                     in->fronts.p);
  if (Z.pin_dof >= 0)
    hipLaunchKernelGGL(fc_front_shift, dim3(1), dim3(64), 0, in->stream, 2, Z.pin_slot.p, Z.pin_val.p, in->fronts.p, (int64_t)0, (int64_t)0);
  HIPCHK(hipGetLastError());
  in->refactor_flops = in->refactor_flops_full = 0.0;
  FCCHK(eliminate_fronts(in, S, false));
  HIPCHK(hipEventRecord(in->ev1, in->stream));
  HIPCHK(hipEventSynchronize(in->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, in->ev0, in->ev1));
  Z.refactor_ms = (double)ms;
  Z.refactor_flops = in->refactor_flops;
  S.ready = true;
  Z.factored = true;
  Z.f_re = Z.s_re;
  Z.f_im = Z.s_im;
  ++Z.n_refactor;
  if (Z.adj_avail) {
    FCCHK(shifted_export_adjoint(Z));
    shifted_use(Z, Z.adj_on);
  }
  if (in->bat.tables) {  // a block is set: its apply streams a tiled copy of these values
    in->bat.ftile_ok[0] = false;
    FCCHK(batch_repack(in, 0));
  }
  return FC_OK;
}

// the pin's slots (from shifted_build) and shift onto the device
int shifted_upload_pin(ShiftedSolver& Z) {
  if (Z.pin_dof < 0) return FC_OK;
  if (Z.pin_dof != Z.pin_slot_dof) return fail(FC_ERR_INVALID, "fc_setup_shifted: the pin was registered after the solver's structure was built");
  const double val[2] = {Z.pin_shift, Z.pin_shift};
  FCCHK(Z.pin_slot.upload(Z.pin_slot_h, 2, Z.in->stream));
  FCCHK(Z.pin_val.upload(val, 2, Z.in->stream));
  HIPCHK(hipStreamSynchronize(Z.in->stream));  // (the host array goes out of scope)
  return FC_OK;
}

// y = (s E - t A') x, or b - (s E - t A') x; |y|^2 (and |b|^2) into out[0] (out[1]) when out != nullptr.  Interleaved complex vectors.
// A' = A - shift e_k e_k^T with a pin registered (s E - A' = M'), A otherwise.  While the adjoint array is in use: E^T and A'^T, s as
// given (the solves pass the conjugated shift, shifted_sim).
int shifted_spmv(fc_ctx* h, ShiftedSolver& Z, double s_re, double s_im, double t, const double* x, const double* b, double* y, double* out) {
  const int n = Z.n;
  const double mean = (double)Z.nnz / std::max(1, n);
  const int L = mean <= 24 ? 8 : (mean <= 64 ? 16 : 32);
  const int grid = nblocks(n, 256 / L);
  if ((size_t)(2 * grid) > Z.part.n) return fail(FC_ERR_INVALID, "shifted_spmv: reduction buffer too small");
  double* part = out ? Z.part.p : nullptr;
  hipStream_t st = Z.in->stream;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  const double2* b2 = reinterpret_cast<const double2*>(b);
  double2* y2 = reinterpret_cast<double2*>(y);
  const int pr = (Z.pin_dof >= 0 && t != 0.0) ? Z.pin_dof : -1;
  const double pv = t * Z.pin_shift;
  const double* av = Z.adj_cur ? Z.a_t.p : Z.a.p;  // (the adjoint array in use: A^T, E^T)
  const double* ev = Z.adj_cur ? Z.e_t.p : Z.e.p;
  ++Z.n_matvec;
  auto launch = [&](auto LANES) {
    hipLaunchKernelGGL(fc_shifted_spmv<LANES>, dim3(grid), dim3(256), 0, st, n, h->rowptr.p, h->col.p, av, ev, s_re, s_im, t, x2, b2, y2, part, pr, pv);
  };
  if (!pick(fc_dispatch::ShiftedSpmvLanes{}, L, launch)) launch(int_c<32>{});
  if (out) hipLaunchKernelGGL(fc_reduce_final, dim3(b ? 2 : 1), dim3(256), 0, st, grid, Z.part.p, 1.0, out);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

constexpr double kShiftedTol = 1e-8;  // relative residual a shifted solve must reach after its refinement steps

// out = (held factors)^-1 src (device, interleaved; out may be src)
int shifted_apply(ShiftedSolver& Z, const double* src, double* out) {
  fc_ctx* in = Z.in;
  const int n2 = 2 * Z.n, g = nblocks(n2, 256);
  hipStream_t st = in->stream;
  hipLaunchKernelGGL(fc_gather_perm, dim3(g), dim3(256), 0, st, n2, in->perm.p, src, in->buf.p);
  FCCHK(apply_factors(in, in->sys[0]));
  hipLaunchKernelGGL(fc_scatter_perm, dim3(g), dim3(256), 0, st, n2, in->perm.p, in->buf.p + n2, (const double*)nullptr, out);
  ++Z.n_apply;
  return FC_OK;
}

// x = M^-1 b (device, interleaved) with Z.refine refinement steps against M; |b - M x|^2, |b|^2 of the final x into res2[0..1]
int shifted_solve_dev(fc_ctx* h, ShiftedSolver& Z, const double* b, double* x, double* res2) {
  const int n2 = 2 * Z.n, g = nblocks(n2, 256);
  hipStream_t st = Z.in->stream;
  FCCHK(shifted_apply(Z, b, x));
  for (int it = 0; it < Z.refine; ++it) {
    FCCHK(shifted_spmv(h, Z, Z.s_re, shifted_sim(Z), 1.0, x, b, Z.rz.p, nullptr));
    FCCHK(shifted_apply(Z, Z.rz.p, Z.rz.p));
    hipLaunchKernelGGL(fc_axpy, dim3(g), dim3(256), 0, st, n2, 1.0, Z.rz.p, x);
  }
  FCCHK(shifted_spmv(h, Z, Z.s_re, shifted_sim(Z), 1.0, x, b, Z.rz.p, res2));
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// the handle's shifted solver, created empty (no structure yet) by the first call that configures it
ShiftedSolver& shifted_get(fc_ctx* h) {
  if (!h->shf) {
    h->shf = new ShiftedSolver();
    h->shf->n = h->N;
    h->shf->nnz = h->nnz;
  }
  return *h->shf;
}

int shifted_ready(fc_ctx* h, const char* who) {
  if (!h) return fail(FC_ERR_INVALID, std::string(who) + ": null handle");
  if (!h->shf || !h->shf->factored) return fail(FC_ERR_NOT_READY, std::string(who) + ": call fc_setup_shifted first");
  return FC_OK;
}

int shifted_solve_col(fc_ctx* h, ShiftedSolver& Z, const double* b, double* x, int* iters);  // (below, with the GMRES it may call)

// w = s (held operator)^-1 (E or E^T) v (device, interleaved; w may be v): the matrices and factors of the array in use; relative
// residual of the inner solve into *rel
int shifted_op_half(fc_ctx* h, ShiftedSolver& Z, double s, const double* v, double* w, double* rel) {
  FCCHK(shifted_spmv(h, Z, s, 0.0, 0.0, v, nullptr, Z.wz.p, nullptr));
  int iters = 0;
  FCCHK(shifted_solve_col(h, Z, Z.wz.p, w, &iters));
  double r2[2];
  HIPCHK(hipMemcpyAsync(r2, Z.scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, Z.in->stream));
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  *rel = std::sqrt(r2[0] / (r2[1] > 0.0 ? r2[1] : 1.0));
  if (!(*rel <= (iters > 0 ? std::max(kShiftedTol, Z.k_rtol) : kShiftedTol)))
    return fail(FC_ERR_NOT_CONVERGED, "shifted solve inside the Arnoldi step: relative residual " + sci(*rel) + " after " +
                                          std::to_string(Z.refine) + " refinement steps");
  return FC_OK;
}

// w = Op v (device, interleaved); the larger relative residual of the inner solves into *rel.
//   kind 0: Op = (A - sigma E)^-1 E = -M^-1 E; in the adjoint mode -(M^H)^-1 E^T, the shift-invert of (A^T, E^T) at conj(sigma)
//   kind 1: Op_R = M^-H E^T M^-1 E (the resolvent: its eigenvalues are the squared gains for symmetric positive semidefinite E),
//           the direct half on the direct array, the adjoint half on the adjoint one, whatever the mode is; the mode's array is
//           back in place on return
int shifted_op(fc_ctx* h, ShiftedSolver& Z, const double* v, double* w, double* rel) {
  if (Z.arn_kind == 0) return shifted_op_half(h, Z, -1.0, v, w, rel);
  double r1 = 0.0, r2 = 0.0;
  shifted_use(Z, false);
  int code = shifted_op_half(h, Z, 1.0, v, w, &r1);
  if (code == FC_OK) {
    shifted_use(Z, true);
    code = shifted_op_half(h, Z, 1.0, w, w, &r2);  // (v is only read by the mat-vec, before w is written)
  }
  shifted_use(Z, Z.adj_on);
  *rel = std::max(r1, r2);
  return code;
}

// out[0 .. nv) = V[0 .. nv)^H w (complex), fixed reduction order; reduce = false leaves the gx partial sums per dot in Z.part
int shifted_multidot_to(ShiftedSolver& Z, int nv, const double* Vp, const double* w, double* out, bool reduce, int* gx_out) {
  const int n = Z.n;
  const int gx = std::min(64, nblocks(n, 256));
  if ((size_t)(2 * gx * nv) > Z.part.n) return fail(FC_ERR_INVALID, "shifted_multidot: reduction buffer too small");
  hipStream_t st = Z.in->stream;
  hipLaunchKernelGGL(fc_cmultidot, dim3(gx, nv), dim3(256), 0, st, n, reinterpret_cast<const double2*>(Vp), reinterpret_cast<const double2*>(w),
                     Z.part.p);
  if (reduce) hipLaunchKernelGGL(fc_cmultidot_reduce, dim3(nv), dim3(64), 0, st, gx, Z.part.p, reinterpret_cast<double2*>(out));
  if (gx_out) *gx_out = gx;
  HIPCHK(hipGetLastError());
  return FC_OK;
}

constexpr int kShiftedKrylovCheck = 4;  // GMRES iterations between two reads of the device's record

// Right-preconditioned GMRES(restart) for M x = b at the operator's current shift, preconditioner = the held factors; x holds the
// start iterate (x0 = false: zero).  Everything but one 8-double record per kShiftedKrylovCheck iterations and two per cycle stays on
// the device.  |b - M x|^2, |b|^2 of the final x into res2[0..1]; FC_ERR_NOT_CONVERGED if k_rtol is missed within k_max_iter.
int shifted_gmres(fc_ctx* h, ShiftedSolver& Z, const double* b, double* x, bool x0, double* res2, int* iters) {
  const int n = Z.n, m = Z.k_restart, g = nblocks(n, 256);
  const size_t n2 = 2 * (size_t)n;
  hipStream_t st = Z.in->stream;
  if (Z.KV.n != n2 * (m + 1)) FCCHK(Z.KV.alloc(n2 * (m + 1)));
  if (Z.kt.n != n2) FCCHK(Z.kt.alloc(n2));
  if (Z.kz.n != n2) FCCHK(Z.kz.alloc(n2));
  if (Z.gm.n != fc_cgm_size(m)) FCCHK(Z.gm.alloc(fc_cgm_size(m)));
  if (Z.kh.n != 4 * (size_t)m) FCCHK(Z.kh.alloc(4 * (size_t)m));
  if (Z.part.n < 2 * 64 * (size_t)(m + 1)) FCCHK(Z.part.alloc(2 * 64 * (size_t)(m + 1)));
  const FcCgm L = fc_cgm_layout(Z.gm.p, m);
  double* h1 = Z.kh.p;
  double* h2 = Z.kh.p + 2 * (size_t)m;
  double rec[CG_REC];
  auto read_rec = [&]() -> int {
    HIPCHK(hipMemcpyAsync(rec, L.rec, sizeof rec, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FC_OK;
  };
  *iters = 0;
  if (!x0) HIPCHK(hipMemsetAsync(x, 0, n2 * sizeof(double), st));
  FCCHK(shifted_spmv(h, Z, Z.s_re, shifted_sim(Z), 1.0, x, b, Z.rz.p, res2));
  for (;;) {
    hipLaunchKernelGGL(fc_cgmres_begin, dim3(1), dim3(64), 0, st, m, Z.gm.p, res2, Z.k_rtol);
    hipLaunchKernelGGL(fc_cnormalize_store, dim3(g), dim3(256), 0, st, n, reinterpret_cast<const double2*>(Z.rz.p), L.rec,
                       reinterpret_cast<double2*>(Z.KV.p));
    FCCHK(read_rec());
    if (rec[CG_STATE] == 1.0) return FC_OK;  // the iterate meets rtol (or b = 0)
    const int jend = std::min(m, Z.k_max_iter - *iters);
    if (jend <= 0) {
      return fail(FC_ERR_NOT_CONVERGED, "shifted GMRES: relative residual " + sci(std::sqrt(rec[CG_RNORM2] / rec[CG_BNORM2])) + " after " +
                                            std::to_string(*iters) + " iterations (rtol " + sci(Z.k_rtol) + ", factors of sigma = " +
                                            sci(Z.f_re) + " + " + sci(Z.f_im) + "i)");
    }
    for (int j = 0; j < jend; ++j) {
      double* vj = Z.KV.p + n2 * j;
      double* w = Z.KV.p + n2 * (j + 1);
      FCCHK(shifted_apply(Z, vj, Z.kz.p));
      FCCHK(shifted_spmv(h, Z, Z.s_re, shifted_sim(Z), 1.0, Z.kz.p, nullptr, w, nullptr));
      // classical Gram-Schmidt, twice; the column h1 + h2 and the fold of |w|^2 ride in the rotation kernel
      int gx = 0;
      FCCHK(shifted_multidot_to(Z, j + 1, Z.KV.p, w, h1, true, nullptr));
      hipLaunchKernelGGL(fc_cgs_update, dim3(g), dim3(256), 0, st, n, j + 1, reinterpret_cast<const double2*>(Z.KV.p),
                         reinterpret_cast<const double2*>(h1), reinterpret_cast<double2*>(w));
      FCCHK(shifted_multidot_to(Z, j + 1, Z.KV.p, w, h2, true, nullptr));
      hipLaunchKernelGGL(fc_cgs_update, dim3(g), dim3(256), 0, st, n, j + 1, reinterpret_cast<const double2*>(Z.KV.p),
                         reinterpret_cast<const double2*>(h2), reinterpret_cast<double2*>(w));
      FCCHK(shifted_multidot_to(Z, 1, w, w, nullptr, false, &gx));
      hipLaunchKernelGGL(fc_cgmres_givens, dim3(1), dim3(64), 0, st, j, m, j + 1 == jend ? 1 : 0, Z.gm.p, reinterpret_cast<const double2*>(h1),
                         reinterpret_cast<const double2*>(h2), (const double*)Z.part.p, gx, Z.k_rtol);
      hipLaunchKernelGGL(fc_cnormalize_store, dim3(g), dim3(256), 0, st, n, reinterpret_cast<const double2*>(w), L.rec,
                         reinterpret_cast<double2*>(w));
      HIPCHK(hipGetLastError());
      if ((j + 1) % kShiftedKrylovCheck == 0 && j + 1 < jend) {
        FCCHK(read_rec());
        if (rec[CG_STATE] != 0.0) break;
      }
    }
    FCCHK(read_rec());
    if (rec[CG_STATE] <= 0.0)
      return fail(FC_ERR_NOT_CONVERGED, "shifted GMRES: breakdown (state " + std::to_string((int)rec[CG_STATE]) + ")");
    const int used = (int)rec[CG_USED];
    *iters += used;
    // x += P^-1 (V y), then the TRUE residual decides (the next cycle starts from it)
    hipLaunchKernelGGL(fc_cbasis_combine, dim3(g, 1), dim3(256), 0, st, n, used, 1, reinterpret_cast<const double2*>(Z.KV.p),
                       reinterpret_cast<const double2*>(L.y), reinterpret_cast<double2*>(Z.kt.p));
    FCCHK(shifted_apply(Z, Z.kt.p, Z.kt.p));
    hipLaunchKernelGGL(fc_axpy, dim3(nblocks((int64_t)n2, 256)), dim3(256), 0, st, (int)n2, 1.0, Z.kt.p, x);
    FCCHK(shifted_spmv(h, Z, Z.s_re, shifted_sim(Z), 1.0, x, b, Z.rz.p, res2));
  }
}

// one column through whatever the solver is set to: the direct solve with its refinement steps; on lagged factors (the operator's
// shift differs from the factored one) GMRES from zero; with Krylov on, GMRES from the refined iterate when that misses kShiftedTol.
// |b - M x|^2, |b|^2 into Z.scal[0..1] (device); *iters = GMRES iterations taken (0: none).
int shifted_solve_col(fc_ctx* h, ShiftedSolver& Z, const double* b, double* x, int* iters) {
  *iters = 0;
  if (Z.s_re != Z.f_re || Z.s_im != Z.f_im) {
    ++Z.n_gmres;
    return shifted_gmres(h, Z, b, x, false, Z.scal.p, iters);
  }
  FCCHK(shifted_solve_dev(h, Z, b, x, Z.scal.p));
  if (Z.k_max_iter <= 0) return FC_OK;
  double r2[2];
  HIPCHK(hipMemcpyAsync(r2, Z.scal.p, sizeof r2, hipMemcpyDeviceToHost, Z.in->stream));
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  const double rel = std::sqrt(r2[0] / (r2[1] > 0.0 ? r2[1] : 1.0));
  if (rel <= kShiftedTol) return FC_OK;
  ++Z.n_gmres;
  ++Z.n_rescue;
  return shifted_gmres(h, Z, b, x, std::isfinite(rel), Z.scal.p, iters);
}

// hd[off .. off + nv) = V[0 .. nv)^H w (complex), fixed reduction order
int shifted_multidot(ShiftedSolver& Z, int nv, const double* Vp, const double* w, int off) {
  return shifted_multidot_to(Z, nv, Vp, w, Z.hd.p + 2 * (size_t)off, true, nullptr);
}

// ── block solves ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
// everything fc_shifted_set_block holds: the inner context's batched-apply tables, tiled factor copy and work buffer, the block vectors
void shifted_block_release(ShiftedSolver& Z) {
  if (Z.in) {
    (void)hipStreamSynchronize(Z.in->stream);
    fc_ctx::Batch& T = Z.in->bat;
    batch_release_apply(T);
    T.ring.release();
    T.buf = fc_ctx::BufView{};
    T.KB = 0;
  }
  for (DevBuf<double>* d : {&Z.BB, &Z.BX, &Z.BR, &Z.BT, &Z.BZ, &Z.BKV, &Z.Bgm, &Z.Bh, &Z.Bsh, &Z.Bres2, &Z.Bpart, &Z.Bst}) d->release();
  Z.blk_k = Z.blk_KB = 0;
}

// out (+)= (held factors)^-1 src for all columns (block vectors; out may be src): ONE pass over the factors.  rec != nullptr: out +=,
// for the columns a cycle's end updates.
int shifted_apply_block(ShiftedSolver& Z, const double* src, double* out, const double* rec) {
  fc_ctx* in = Z.in;
  const int n2 = 2 * Z.n, KB = Z.blk_KB;
  const int g = nblocks((int64_t)n2 * KB, 256);
  hipStream_t st = in->stream;
  double* buf = in->bat.buf.p;
  pick_width(KB, [&](auto K) { hipLaunchKernelGGL(fc_cblock_perm<K>, dim3(g), dim3(256), 0, st, n2, in->perm.p, src, buf, 0, (const double*)nullptr); });
  FCCHK(batch_apply(in, 0));
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL(fc_cblock_perm<K>, dim3(g), dim3(256), 0, st, n2, in->perm.p, (const double*)(buf + (size_t)n2 * KB), out, rec ? 2 : 1, rec);
  });
  HIPCHK(hipGetLastError());
  ++Z.n_apply;
  return FC_OK;
}

// Y_c = (s_c E - t_c A') X_c or B_c - that, shifts from Z.Bsh; (|y_c|^2, |b_c|^2) into res2 [KB][2] when res2 != nullptr; columns
// frozen under (rec, mode) keep their y and res2
int shifted_spmv_block(fc_ctx* h, ShiftedSolver& Z, const double* x, const double* b, double* y, double* res2, const double* rec, int mode) {
  const int n = Z.n, KB = Z.blk_KB, grid = nblocks(n, 4);
  if (res2 && (size_t)2 * KB * grid > Z.Bpart.n) return fail(FC_ERR_INVALID, "shifted_spmv_block: reduction buffer too small");
  double* part = res2 ? Z.Bpart.p : nullptr;
  hipStream_t st = Z.in->stream;
  ++Z.n_matvec;
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL((fc_shifted_spmv_b<K, 64 / K>), dim3(grid), dim3(256), 0, st, n, h->rowptr.p, h->col.p,
                       (const double*)(Z.adj_cur ? Z.a_t.p : Z.a.p), (const double*)(Z.adj_cur ? Z.e_t.p : Z.e.p), (const double*)Z.Bsh.p, x, b, y, part,
                       Z.pin_dof, Z.pin_shift, rec, mode);
  });
  if (res2) hipLaunchKernelGGL(fc_cnorm_reduce_b, dim3(KB), dim3(256), 0, st, grid, KB, (const double*)Z.Bpart.p, res2, rec, mode);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// hout[i][c] = V_{i,c}^H w_c for i < nv (fixed order); reduce = false leaves the gx partials per dot in Z.Bpart
int shifted_multidot_block(ShiftedSolver& Z, int nv, const double* Vp, const double* w, double* hout, bool reduce, int* gx_out) {
  const int n = Z.n, KB = Z.blk_KB;
  const int gx = std::min(64, nblocks(n, 256 / KB));
  if ((size_t)2 * gx * nv * KB > Z.Bpart.n) return fail(FC_ERR_INVALID, "shifted_multidot_block: reduction buffer too small");
  hipStream_t st = Z.in->stream;
  pick_width(KB, [&](auto K) { hipLaunchKernelGGL(fc_cmultidot_b<K>, dim3(gx, nv), dim3(256), 0, st, n, Vp, w, Z.Bpart.p); });
  if (reduce)
    hipLaunchKernelGGL(fc_cmultidot_reduce_b, dim3(nv), dim3(64), 0, st, gx, KB, (const double*)Z.Bpart.p, reinterpret_cast<double2*>(hout));
  if (gx_out) *gx_out = gx;
  HIPCHK(hipGetLastError());
  return FC_OK;
}

// shifted_gmres for the k columns of a block in lock step: column c solves (sigma_c E - A') x_c = b_c (Z.BB -> Z.BX, zero start) on the
// held factors; ONE apply, one mat-vec and one pass per Gram-Schmidt step over the basis per iteration for all columns.  A column
// stops on its own estimate and is frozen from then on; a cycle ends when every column has stopped or closed it, then every column it
// moved gets its update and its TRUE residual, which starts (or ends) its next cycle.  Apart from the end of the budget (the cycles
// are cut at max_iter lock-step iterations) a column's arithmetic does not depend on its neighbours.  The host reads the k records
// every kShiftedKrylovCheck iterations and at the cycle's ends.  (|r_c|^2, |b_c|^2) of the final iterates stay in Z.Bres2.
int shifted_gmres_block(fc_ctx* h, ShiftedSolver& Z, int k, std::vector<int>& iters) {
  const int n = Z.n, m = Z.k_restart, KB = Z.blk_KB;
  const size_t nb = 2 * (size_t)n * KB;  // doubles of a block vector
  const int g = nblocks((int64_t)n * KB, 256);
  hipStream_t st = Z.in->stream;
  if (Z.BKV.n != nb * (m + 1)) {
    FCCHK(Z.BKV.alloc(nb * (m + 1)));
    FCCHK(Z.BKV.zero(st));  // (frozen and padding columns of the basis are never written: they stay zero, nothing non-finite reaches the apply)
  }
  if (Z.Bgm.n != fc_cgm_size_b(m, KB)) FCCHK(Z.Bgm.alloc(fc_cgm_size_b(m, KB)));
  if (Z.Bh.n != 4 * (size_t)m * KB) FCCHK(Z.Bh.alloc(4 * (size_t)m * KB));
  const size_t part_need = std::max((size_t)2 * KB * nblocks(n, 4), (size_t)2 * 64 * (m + 1) * KB);
  if (Z.Bpart.n < part_need) FCCHK(Z.Bpart.alloc(part_need));
  double* rec_d = fc_cgm_layout_b(Z.Bgm.p, m, 0, KB).rec;
  double* h1 = Z.Bh.p;
  double* h2 = Z.Bh.p + 2 * (size_t)m * KB;
  std::vector<double> rec((size_t)KB * CG_REC);
  auto read_rec = [&]() -> int {
    HIPCHK(hipMemcpyAsync(rec.data(), rec_d, rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FC_OK;
  };
  auto state = [&](int c) { return rec[(size_t)c * CG_REC + CG_STATE]; };
  iters.assign((size_t)k, 0);
  Z.blk_launched = Z.blk_cycles = 0;
  int total = 0;  // lock-step iterations so far
  HIPCHK(hipMemsetAsync(Z.BX.p, 0, nb * sizeof(double), st));
  FCCHK(shifted_spmv_block(h, Z, Z.BX.p, Z.BB.p, Z.BR.p, Z.Bres2.p, nullptr, 0));
  for (int cycle = 0;; ++cycle) {
    hipLaunchKernelGGL(fc_cgmres_begin_b, dim3(KB), dim3(64), 0, st, m, k, KB, cycle == 0 ? 1 : 0, Z.Bgm.p, (const double*)Z.Bres2.p, Z.k_rtol);
    pick_width(KB, [&](auto K) {
      hipLaunchKernelGGL(fc_cnormalize_store_b<K>, dim3(g), dim3(256), 0, st, n, (const double*)Z.BR.p, (const double*)rec_d, Z.BKV.p);
    });
    FCCHK(read_rec());
    bool running = false;
    for (int c = 0; c < k; ++c) running = running || state(c) == 0.0;
    const int jend = std::min(m, Z.k_max_iter - total);
    if (!running || jend <= 0) return FC_OK;  // (the caller reads Z.Bres2: a column that misses rtol is its finding)
    ++Z.blk_cycles;
    for (int j = 0; j < jend; ++j) {
      ++Z.blk_launched;
      double* vj = Z.BKV.p + nb * j;
      double* w = Z.BKV.p + nb * (j + 1);
      FCCHK(shifted_apply_block(Z, vj, Z.BZ.p, nullptr));
      FCCHK(shifted_spmv_block(h, Z, Z.BZ.p, nullptr, w, nullptr, rec_d, 0));
      int gx = 0;
      for (double* hp : {h1, h2}) {  // classical Gram-Schmidt, twice
        FCCHK(shifted_multidot_block(Z, j + 1, Z.BKV.p, w, hp, true, nullptr));
        pick_width(KB, [&](auto K) {
          hipLaunchKernelGGL(fc_cgs_update_b<K>, dim3(g), dim3(256), 0, st, n, j + 1, (const double*)Z.BKV.p, reinterpret_cast<const double2*>(hp), w,
                             (const double*)rec_d);
        });
      }
      FCCHK(shifted_multidot_block(Z, 1, w, w, nullptr, false, &gx));
      hipLaunchKernelGGL(fc_cgmres_givens_b, dim3(KB), dim3(64), 0, st, j, m, KB, j + 1 == jend ? 1 : 0, Z.Bgm.p, reinterpret_cast<const double2*>(h1),
                         reinterpret_cast<const double2*>(h2), (const double*)Z.Bpart.p, gx, Z.k_rtol);
      pick_width(KB, [&](auto K) { hipLaunchKernelGGL(fc_cnormalize_store_b<K>, dim3(g), dim3(256), 0, st, n, (const double*)w, (const double*)rec_d, w); });
      HIPCHK(hipGetLastError());
      if ((j + 1) % kShiftedKrylovCheck == 0 && j + 1 < jend) {
        FCCHK(read_rec());
        bool any = false;
        for (int c = 0; c < k; ++c) any = any || state(c) == 0.0;
        if (!any) break;
      }
    }
    FCCHK(read_rec());
    int longest = 0;
    for (int c = 0; c < k; ++c)
      if (state(c) == 3.0 || state(c) == 4.0) {
        const int used = (int)rec[(size_t)c * CG_REC + CG_USED];
        iters[(size_t)c] += used;
        longest = std::max(longest, used);
      }
    if (longest == 0) return FC_OK;  // (every column that ran broke down: nothing to update)
    total += longest;
    // x_c += P^-1 (V_c y_c) for the columns this cycle moved, then their TRUE residuals
    pick_width(KB, [&](auto K) { hipLaunchKernelGGL(fc_cbasis_combine_b<K>, dim3(g), dim3(256), 0, st, n, m, (const double*)Z.BKV.p, Z.Bgm.p, Z.BT.p); });
    FCCHK(shifted_apply_block(Z, Z.BT.p, Z.BX.p, rec_d));
    FCCHK(shifted_spmv_block(h, Z, Z.BX.p, Z.BB.p, Z.BR.p, Z.Bres2.p, rec_d, 1));
  }
}

}  // namespace

extern "C" {

int fc_setup_shifted(fc_handle h, const double* a_vals, const double* e_vals, double sigma_re, double sigma_im, int32_t refine) {
  if (!h || refine < 0 || refine > 100 || !std::isfinite(sigma_re) || !std::isfinite(sigma_im))
    return fail(FC_ERR_INVALID, "fc_setup_shifted: bad argument");
  if (h->partitioned || exchanges(h))
    return fail(FC_ERR_INVALID, "fc_setup_shifted: partitioned (multi-GPU) handles are not supported: the shifted solver factorises on one device");
  if (h->pin_dof >= 0 && !(h->shf && h->shf->pin_dof >= 0))
    return fail(FC_ERR_INVALID, "fc_setup_shifted: the handle has a pressure pin (enclosed flow): sigma E - A is singular for every sigma there "
                                "(fc_shifted_set_pin registers a pin of the shifted operator)");
  if ((a_vals == nullptr) != (e_vals == nullptr)) return fail(FC_ERR_INVALID, "fc_setup_shifted: pass both value arrays or neither");
  if (!a_vals && !(h->shf && h->shf->in)) return fail(FC_ERR_NOT_READY, "fc_setup_shifted: the first call needs the values of A and E");
  HIPCHK(hipSetDevice(h->device));
  if (!h->shf || !h->shf->in) {
    ShiftedSolver& Z = shifted_get(h);
    int code = FC_OK;
    try {
      code = shifted_build(h, Z);
    } catch (const std::exception& e) {
      code = fail(FC_ERR_INVALID, std::string("fc_setup_shifted: ") + e.what());
    }
    if (code != FC_OK) {
      const std::string msg = g_err;
      shifted_free(h);
      g_err = msg;
      return code;
    }
  }
  ShiftedSolver& Z = *h->shf;
  if (a_vals) {
    for (int64_t k = 0; k < h->nnz; ++k)
      if (!std::isfinite(a_vals[k]) || !std::isfinite(e_vals[k])) return fail(FC_ERR_INVALID, "fc_setup_shifted: non-finite matrix value");
    FCCHK(Z.a.upload(a_vals, (size_t)h->nnz, Z.in->stream));
    FCCHK(Z.e.upload(e_vals, (size_t)h->nnz, Z.in->stream));
    if (Z.adj_avail) FCCHK(shifted_gather_transposed(Z));
  }
  Z.s_re = sigma_re;
  Z.s_im = sigma_im;
  Z.refine = refine;
  Z.factored = false;
  if (Z.pin_dirty) {
    FCCHK(shifted_upload_pin(Z));
    Z.pin_dirty = false;
  }
  return shifted_refactor(Z);
}

int fc_solve_shifted(fc_handle h, int32_t nrhs, const double* b_re, const double* b_im, double* x_re, double* x_im, double* info) {
  FCCHK(shifted_ready(h, "fc_solve_shifted"));
  if (nrhs <= 0 || nrhs > 4096 || !b_re || (x_re == nullptr) != (x_im == nullptr)) return fail(FC_ERR_INVALID, "fc_solve_shifted: bad argument");
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  hipStream_t st = Z.in->stream;
  const int n = Z.n, g = nblocks(n, 256);
  const size_t n2 = 2 * (size_t)n;
  if (Z.bz.n < n2 * nrhs) FCCHK(Z.bz.alloc(n2 * nrhs));
  if (Z.xz.n < n2 * nrhs) FCCHK(Z.xz.alloc(n2 * nrhs));
  std::vector<double> r2(2 * (size_t)nrhs);
  Z.last_iters.assign((size_t)nrhs, 0);
  for (int c = 0; c < nrhs; ++c) {
    double* bc = Z.bz.p + n2 * c;
    double* xc = Z.xz.p + n2 * c;
    HIPCHK(hipMemcpyAsync(Z.st.p, b_re + (size_t)n * c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    if (b_im) HIPCHK(hipMemcpyAsync(Z.st.p + n, b_im + (size_t)n * c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fc_cinterleave, dim3(g), dim3(256), 0, st, n, Z.st.p, b_im ? Z.st.p + n : nullptr, reinterpret_cast<double2*>(bc));
    FCCHK(shifted_solve_col(h, Z, bc, xc, &Z.last_iters[(size_t)c]));
    HIPCHK(hipMemcpyAsync(r2.data() + 2 * c, Z.scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (x_re) {
      hipLaunchKernelGGL(fc_csplit, dim3(g), dim3(256), 0, st, n, reinterpret_cast<const double2*>(xc), Z.st.p, Z.st.p + n);
      HIPCHK(hipMemcpyAsync(x_re + (size_t)n * c, Z.st.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(x_im + (size_t)n * c, Z.st.p + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (the staging buffer is reused by the next column)
  }
  HIPCHK(hipGetLastError());
  Z.nrhs_last = nrhs;
  Z.last_res.assign((size_t)nrhs, 0.0);
  double worst = 0.0;
  for (int c = 0; c < nrhs; ++c) {
    const double b2 = r2[2 * (size_t)c + 1];
    const double rel = b2 > 0.0 ? std::sqrt(r2[2 * (size_t)c] / b2) : std::sqrt(r2[2 * (size_t)c]);
    Z.last_res[(size_t)c] = rel;
    if (info) info[c] = rel;
    if (Z.last_iters[(size_t)c] > 0 && rel <= Z.k_rtol) continue;  // (GMRES answers for its own tolerance)
    worst = std::max(worst, std::isfinite(rel) ? rel : INFINITY);
  }
  if (!(worst <= kShiftedTol))
    return fail(FC_ERR_NOT_CONVERGED, "fc_solve_shifted: relative residual " + sci(worst) + " after " + std::to_string(Z.refine) +
                                          " refinement steps (sigma = " + sci(Z.s_re) + " + " + sci(Z.s_im) + "i)");
  return FC_OK;
}

int fc_shifted_project(fc_handle h, int32_t nrhs, int32_t nrow, const int32_t* rowptr, const int32_t* idx, const double* w, double* y_re,
                       double* y_im) {
  FCCHK(shifted_ready(h, "fc_shifted_project"));
  ShiftedSolver& Z = *h->shf;
  if (nrhs <= 0 || nrhs > Z.nrhs_last || nrow <= 0 || !rowptr || !y_re || !y_im || rowptr[0] != 0)
    return fail(FC_ERR_INVALID, "fc_shifted_project: bad argument (nrhs must not exceed the last fc_solve_shifted's)");
  for (int r = 0; r < nrow; ++r)
    if (rowptr[r + 1] < rowptr[r]) return fail(FC_ERR_INVALID, "fc_shifted_project: row pointers not increasing");
  const int nz = rowptr[nrow];
  if (nz > 0 && (!idx || !w)) return fail(FC_ERR_INVALID, "fc_shifted_project: null index / weight array");
  for (int k = 0; k < nz; ++k)
    if (idx[k] < 0 || idx[k] >= Z.n) return fail(FC_ERR_INVALID, "fc_shifted_project: column index out of range");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const int zero_i = 0;
  const double zero_d = 0.0;
  DevBuf<int> drp, didx;
  DevBuf<double> dw, dy;
  FCCHK(drp.upload(rowptr, (size_t)nrow + 1, st));
  FCCHK(didx.upload(nz > 0 ? idx : &zero_i, (size_t)std::max(1, nz), st));
  FCCHK(dw.upload(nz > 0 ? w : &zero_d, (size_t)std::max(1, nz), st));
  FCCHK(dy.alloc(2 * (size_t)nrow * nrhs));
  hipLaunchKernelGGL(fc_cproject, dim3(nblocks((int64_t)nrow * nrhs, 64)), dim3(64), 0, st, nrow, nrhs, Z.n, drp.p, didx.p, dw.p,
                     reinterpret_cast<const double2*>(Z.xz.p), reinterpret_cast<double2*>(dy.p));
  HIPCHK(hipGetLastError());
  std::vector<double> y(2 * (size_t)nrow * nrhs);
  HIPCHK(hipMemcpyAsync(y.data(), dy.p, y.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t q = 0; q < (size_t)nrow * nrhs; ++q) y_re[q] = y[2 * q], y_im[q] = y[2 * q + 1];
  return FC_OK;
}

int fc_shifted_spmv(fc_handle h, double s_re, double s_im, double t, const double* x, double* y) {
  FCCHK(shifted_ready(h, "fc_shifted_spmv"));
  if (!x || !y) return fail(FC_ERR_INVALID, "fc_shifted_spmv: null argument");
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  hipStream_t st = Z.in->stream;
  const size_t n2 = 2 * (size_t)Z.n;
  HIPCHK(hipMemcpyAsync(Z.st.p, x, n2 * sizeof(double), hipMemcpyHostToDevice, st));
  FCCHK(shifted_spmv(h, Z, s_re, s_im, t, Z.st.p, nullptr, Z.rz.p, nullptr));
  HIPCHK(hipMemcpyAsync(y, Z.rz.p, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FC_OK;
}

int fc_shifted_info(fc_handle h, int64_t* info, double* dinfo, double* last_res) {
  if (!h) return fail(FC_ERR_INVALID, "fc_shifted_info: null handle");
  const ShiftedSolver* Z = h->shf;
  if (info) {
    info[0] = Z ? 8 * Z->factor_values : 0;
    info[1] = Z ? shifted_bytes(*Z) : 0;
    info[2] = Z ? 2 * (int64_t)Z->n : 0;
    info[3] = Z ? Z->nrhs_last : 0;
  }
  if (dinfo) {
    dinfo[0] = Z ? Z->refactor_ms : 0.0;
    dinfo[1] = Z ? Z->refactor_flops : 0.0;
    dinfo[2] = Z ? Z->s_re : 0.0;
    dinfo[3] = Z ? Z->s_im : 0.0;
  }
  if (last_res && Z)
    for (int c = 0; c < Z->nrhs_last; ++c) last_res[c] = Z->last_res[(size_t)c];
  return FC_OK;
}

int fc_shifted_set_pin(fc_handle h, int32_t dof, double shift) {
  if (!h || dof >= h->N || (dof >= 0 && dof < 2 * h->nn) || dof < -1)
    return fail(FC_ERR_INVALID, "fc_shifted_set_pin: the pinned dof must be a pressure dof (or -1)");
  if (dof >= 0 && (!std::isfinite(shift) || shift == 0.0)) return fail(FC_ERR_INVALID, "fc_shifted_set_pin: the shift must be finite and nonzero");
  if (dof < 0 && !h->shf) return FC_OK;
  ShiftedSolver& Z = shifted_get(h);
  if (dof >= 0 && Z.in && dof != Z.pin_slot_dof)
    return fail(FC_ERR_INVALID, "fc_shifted_set_pin: register the pin before the first fc_setup_shifted (its front slots are looked up in the "
                                "symbolic phase; fc_release_shifted starts over)");
  Z.pin_dof = dof;
  Z.pin_shift = dof >= 0 ? shift : 0.0;
  Z.pin_dirty = true;
  Z.factored = false;  // the held factors belong to another operator: fc_setup_shifted next
  return FC_OK;
}

int fc_shifted_set_krylov(fc_handle h, int32_t max_iter, int32_t restart, double rtol) {
  if (!h || max_iter < 0 || max_iter > 100000) return fail(FC_ERR_INVALID, "fc_shifted_set_krylov: bad argument");
  if (max_iter > 0 && (restart < 1 || restart > kCgmMaxRestart || !(rtol > 0.0) || !(rtol < 1.0)))
    return fail(FC_ERR_INVALID, "fc_shifted_set_krylov: need 1 <= restart <= " + std::to_string(kCgmMaxRestart) + " and 0 < rtol < 1");
  if (max_iter == 0 && !h->shf) return FC_OK;
  ShiftedSolver& Z = shifted_get(h);
  Z.k_max_iter = max_iter;
  Z.k_restart = max_iter > 0 ? restart : 0;
  Z.k_rtol = max_iter > 0 ? rtol : 0.0;
  if (max_iter == 0) Z.s_re = Z.f_re, Z.s_im = Z.f_im;  // no solves on lagged factors without Krylov
  return FC_OK;
}

int fc_shifted_set_shift(fc_handle h, double sigma_re, double sigma_im) {
  FCCHK(shifted_ready(h, "fc_shifted_set_shift"));
  ShiftedSolver& Z = *h->shf;
  if (!std::isfinite(sigma_re) || !std::isfinite(sigma_im)) return fail(FC_ERR_INVALID, "fc_shifted_set_shift: bad argument");
  if (Z.k_max_iter <= 0)
    return fail(FC_ERR_INVALID, "fc_shifted_set_shift: solves on lagged factors need the Krylov solver (fc_shifted_set_krylov)");
  Z.s_re = sigma_re;
  Z.s_im = sigma_im;
  return FC_OK;
}

int fc_shifted_krylov_info(fc_handle h, int32_t* iters, int64_t* counters) {
  if (!h) return fail(FC_ERR_INVALID, "fc_shifted_krylov_info: null handle");
  const ShiftedSolver* Z = h->shf;
  if (iters && Z)
    for (int c = 0; c < Z->nrhs_last && c < (int)Z->last_iters.size(); ++c) iters[c] = Z->last_iters[(size_t)c];
  if (counters) {
    counters[0] = Z ? Z->n_refactor : 0;
    counters[1] = Z ? Z->n_apply : 0;
    counters[2] = Z ? Z->n_matvec : 0;
    counters[3] = Z ? Z->n_gmres : 0;
    counters[4] = Z ? Z->n_rescue : 0;
  }
  return FC_OK;
}

int fc_shifted_set_block(fc_handle h, int32_t k) {
  if (!h || k < 0 || k > 32) return fail(FC_ERR_INVALID, "fc_shifted_set_block: k must be in [0, 32]");
  if (k == 0 && !h->shf) return FC_OK;
  HIPCHK(hipSetDevice(h->device));
  if (k == 0) {
    shifted_block_release(*h->shf);
    return FC_OK;
  }
  if (!h->shf || !h->shf->in) return fail(FC_ERR_NOT_READY, "fc_shifted_set_block: call fc_setup_shifted first (the block is built on its structure)");
  ShiftedSolver& Z = *h->shf;
  fc_ctx* in = Z.in;
  fc_ctx::Batch& T = in->bat;
  HIPCHK(hipStreamSynchronize(in->stream));
  try {
    FCCHK(build_batch_tables(in, Z.sym_fac, Z.sym_tree));
  } catch (const std::exception& e) {
    return fail(FC_ERR_INVALID, std::string("fc_shifted_set_block: ") + e.what());
  }
  const int KB = batch_width(k);
  const size_t n2 = 2 * (size_t)Z.n, nb = n2 * KB;
  if (KB != Z.blk_KB) {
    T.slot_doubles = batch_slot_doubles(T, n2, KB);  // one work buffer (fc_set_batch keeps a ring of four)
    FCCHK(T.ring.alloc(T.slot_doubles));
    FCCHK(T.ring.zero(in->stream));
    T.buf.p = T.ring.p;
    T.buf.n = T.slot_doubles;
    T.KB = KB;
    for (DevBuf<double>* d : {&Z.BB, &Z.BX, &Z.BR, &Z.BT, &Z.BZ}) FCCHK(d->alloc(nb));
    FCCHK(Z.Bsh.alloc(3 * (size_t)KB));
    FCCHK(Z.Bres2.alloc(2 * (size_t)KB));
    FCCHK(Z.Bst.alloc(n2 * KB));  // staging of split host arrays: re [KB][n] | im [KB][n]
    FCCHK(Z.Bpart.alloc(2 * (size_t)KB * nblocks(Z.n, 4)));
    Z.BKV.release(), Z.Bgm.release(), Z.Bh.release();  // (sized by the restart length at the first solve)
  }
  Z.blk_k = k;
  Z.blk_KB = KB;
  if (in->sys[0].ready && !T.ftile_ok[0]) FCCHK(batch_repack(in, 0));
  HIPCHK(hipStreamSynchronize(in->stream));
  return FC_OK;
}

int fc_solve_shifted_block(fc_handle h, int32_t k, const double* sigma_re, const double* sigma_im, const double* b_re, const double* b_im,
                           double* x_re, double* x_im, double* info) {
  FCCHK(shifted_ready(h, "fc_solve_shifted_block"));
  ShiftedSolver& Z = *h->shf;
  if (Z.blk_k == 0) return fail(FC_ERR_NOT_READY, "fc_solve_shifted_block: fc_shifted_set_block not called");
  if (k != Z.blk_k) return fail(FC_ERR_INVALID, "fc_solve_shifted_block: k differs from fc_shifted_set_block");
  if (Z.k_max_iter <= 0) return fail(FC_ERR_INVALID, "fc_solve_shifted_block: block solves run the Krylov solver (fc_shifted_set_krylov)");
  if (!sigma_re || !sigma_im || !b_re || (x_re == nullptr) != (x_im == nullptr)) return fail(FC_ERR_INVALID, "fc_solve_shifted_block: null argument");
  for (int c = 0; c < k; ++c)
    if (!std::isfinite(sigma_re[c]) || !std::isfinite(sigma_im[c])) return fail(FC_ERR_INVALID, "fc_solve_shifted_block: non-finite shift");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const int n = Z.n, KB = Z.blk_KB, g = nblocks((int64_t)n * KB, 256);
  const size_t nk = (size_t)n * k;
  std::vector<double> sh(3 * (size_t)KB, 0.0);  // (padding columns: the zero operator on a zero right-hand side)
  const double cj = Z.adj_cur ? -1.0 : 1.0;  // adjoint mode: column c solves (conj(sigma_c) E^T - A^T) x_c = b_c
  for (int c = 0; c < k; ++c) sh[3 * (size_t)c] = sigma_re[c], sh[3 * (size_t)c + 1] = cj * sigma_im[c], sh[3 * (size_t)c + 2] = 1.0;
  FCCHK(Z.Bsh.upload(sh, st));
  if (!Z.in->bat.ftile_ok[0]) FCCHK(batch_repack(Z.in, 0));  // (the mode was switched since the tiled copy was made)
  HIPCHK(hipMemcpyAsync(Z.Bst.p, b_re, nk * sizeof(double), hipMemcpyHostToDevice, st));
  if (b_im) HIPCHK(hipMemcpyAsync(Z.Bst.p + nk, b_im, nk * sizeof(double), hipMemcpyHostToDevice, st));
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL(fc_cblock_load<K>, dim3(g), dim3(256), 0, st, n, k, (const double*)Z.Bst.p,
                       b_im ? (const double*)(Z.Bst.p + nk) : (const double*)nullptr, Z.BB.p);
  });
  HIPCHK(hipGetLastError());
  Z.n_gmres += k;
  FCCHK(shifted_gmres_block(h, Z, k, Z.last_iters));
  if (Z.xz.n < 2 * nk) FCCHK(Z.xz.alloc(2 * nk));
  pick_width(KB, [&](auto K) {
    hipLaunchKernelGGL(fc_cblock_store<K>, dim3(g), dim3(256), 0, st, n, k, (const double*)Z.BX.p, reinterpret_cast<double2*>(Z.xz.p),
                       x_re ? Z.Bst.p : (double*)nullptr, x_re ? Z.Bst.p + nk : (double*)nullptr);
  });
  HIPCHK(hipGetLastError());
  std::vector<double> r2(2 * (size_t)KB);
  HIPCHK(hipMemcpyAsync(r2.data(), Z.Bres2.p, r2.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (x_re) {
    HIPCHK(hipMemcpyAsync(x_re, Z.Bst.p, nk * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(x_im, Z.Bst.p + nk, nk * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  Z.nrhs_last = k;
  Z.last_res.assign((size_t)k, 0.0);
  int worst_c = -1;
  double worst = 0.0;
  for (int c = 0; c < k; ++c) {
    const double b2 = r2[2 * (size_t)c + 1];
    double rel = b2 > 0.0 ? std::sqrt(r2[2 * (size_t)c] / b2) : std::sqrt(r2[2 * (size_t)c]);
    if (!std::isfinite(rel)) rel = INFINITY;
    Z.last_res[(size_t)c] = rel;
    if (info) info[c] = rel;
    if (rel > Z.k_rtol && rel > worst) worst = rel, worst_c = c;
  }
  if (worst_c >= 0)
    return fail(FC_ERR_NOT_CONVERGED, "fc_solve_shifted_block: column " + std::to_string(worst_c) + " has relative residual " + sci(worst) + " after " +
                                          std::to_string(Z.last_iters[(size_t)worst_c]) + " iterations (rtol " + sci(Z.k_rtol) +
                                          ", factors of sigma = " + sci(Z.f_re) + " + " + sci(Z.f_im) + "i)");
  return FC_OK;
}

int fc_shifted_block_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_shifted_block_info: null argument");
  const ShiftedSolver* Z = h->shf;
  info[0] = Z ? Z->blk_k : 0;
  info[1] = Z ? Z->blk_KB : 0;
  info[2] = Z ? Z->blk_launched : 0;
  info[3] = Z ? Z->blk_cycles : 0;
  return FC_OK;
}

int fc_bench_shifted_block(fc_handle h, int reps, double* ms, double* bytes) {
  FCCHK(shifted_ready(h, "fc_bench_shifted_block"));
  ShiftedSolver& Z = *h->shf;
  if (reps <= 0 || !ms || !bytes) return fail(FC_ERR_INVALID, "fc_bench_shifted_block: bad argument");
  if (Z.blk_k == 0) return fail(FC_ERR_NOT_READY, "fc_bench_shifted_block: fc_shifted_set_block not called");
  HIPCHK(hipSetDevice(h->device));
  fc_ctx* in = Z.in;
  hipStream_t st = in->stream;
  const int KB = Z.blk_KB;
  const size_t n2 = 2 * (size_t)Z.n;
  // zero operands (the time of a sweep does not depend on the values), unit shifts
  std::vector<double> sh(3 * (size_t)KB, 1.0);
  FCCHK(Z.Bsh.upload(sh, st));
  FCCHK(Z.BZ.zero(st));
  FCCHK(Z.wz.zero(st));
  HIPCHK(hipMemsetAsync(in->bat.buf.p, 0, in->bat.buf.n * sizeof(double), st));
  HIPCHK(hipMemsetAsync(in->buf.p, 0, in->buf.n * sizeof(double), st));
  const int64_t n_apply = Z.n_apply, n_matvec = Z.n_matvec;
  auto timed = [&](int which, auto&& body) -> int {
    for (int i = 0; i < 2; ++i) FCCHK(body());
    HIPCHK(hipEventRecord(in->ev0, st));
    for (int i = 0; i < reps; ++i) FCCHK(body());
    HIPCHK(hipEventRecord(in->ev1, st));
    HIPCHK(hipEventSynchronize(in->ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, in->ev0, in->ev1));
    ms[which] = (double)t / reps;
    return FC_OK;
  };
  FCCHK(timed(0, [&] { return batch_apply(in, 0); }));
  FCCHK(timed(1, [&] { return shifted_spmv_block(h, Z, Z.BZ.p, nullptr, Z.BT.p, nullptr, nullptr, 0); }));
  FCCHK(timed(2, [&] { return apply_factors(in, in->sys[0]); }));
  FCCHK(timed(3, [&] { return shifted_spmv(h, Z, 1.0, 1.0, 1.0, Z.wz.p, nullptr, Z.rz.p, nullptr); }));
  Z.n_apply = n_apply, Z.n_matvec = n_matvec;  // (a measurement is not a solve)
  const double N = (double)Z.n, nnz = (double)Z.nnz;
  bytes[0] = 8.0 * (double)in->bat.factor_values + 8.0 * in->bat.vec_rows * KB;
  bytes[1] = 4.0 * (N + 1.0) + 20.0 * nnz + 32.0 * N * KB;
  bytes[2] = in->sys[0].sweep_bytes;
  bytes[3] = 4.0 * (N + 1.0) + 20.0 * nnz + 32.0 * N;  // (the same terms as the block figure, one column)
  return FC_OK;
}

int fc_debug_scale_shifted_factors(fc_handle h, double scale) {
  FCCHK(shifted_ready(h, "fc_debug_scale_shifted_factors"));
  if (!std::isfinite(scale)) return fail(FC_ERR_INVALID, "fc_debug_scale_shifted_factors: bad argument");
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  DevBuf<double>& fv = Z.in->sys[0].f_val;
  for (double* base : {fv.p, Z.f_other.p}) {  // (both arrays when the adjoint one exists)
    if (!base) continue;
    for (size_t o = 0; o < fv.n; o += (size_t)1 << 30) {
      const int cnt = (int)std::min<size_t>((size_t)1 << 30, fv.n - o);
      hipLaunchKernelGGL(fc_scale_inplace, dim3(nblocks(cnt, 256)), dim3(256), 0, Z.in->stream, cnt, scale, base + o);
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  return FC_OK;
}

int fc_debug_get_shifted_factors(fc_handle h, int32_t adjoint, int64_t n, double* out) {
  FCCHK(shifted_ready(h, "fc_debug_get_shifted_factors"));
  ShiftedSolver& Z = *h->shf;
  if ((adjoint != 0 && adjoint != 1) || !out || n != Z.factor_values) return fail(FC_ERR_INVALID, "fc_debug_get_shifted_factors: bad argument");
  if (adjoint && !Z.adj_avail) return fail(FC_ERR_NOT_READY, "fc_debug_get_shifted_factors: no adjoint factors (fc_shifted_set_adjoint)");
  HIPCHK(hipSetDevice(h->device));
  const double* src = ((adjoint != 0) == Z.adj_cur) ? Z.in->sys[0].f_val.p : Z.f_other.p;
  HIPCHK(hipMemcpyAsync(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, Z.in->stream));
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  return FC_OK;
}

int fc_shifted_set_adjoint(fc_handle h, int32_t on) {
  if (h && (on < -1 || on > 1)) return fail(FC_ERR_INVALID, "fc_shifted_set_adjoint: on must be 1 (adjoint), 0 (direct) or -1 (direct, free the adjoint side)");
  FCCHK(shifted_ready(h, "fc_shifted_set_adjoint"));
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  fc_ctx* in = Z.in;
  if (on == 1 && !Z.adj_avail) {
    // the adjoint side, built on the structure and the fronts of the last factorisation: the map of the transposed values, the
    // export's work list, the second value array
    std::vector<int> tpos;
    std::vector<FcExpTItem> items;
    try {
      FCCHK(shifted_transpose_map(h->h_rowptr, h->h_col, tpos));
      items = export_t_items(in);
    } catch (const std::exception& e) {
      return fail(FC_ERR_INVALID, std::string("fc_shifted_set_adjoint: ") + e.what());
    }
    HIPCHK(hipStreamSynchronize(in->stream));
    int code = FC_OK;
    auto build = [&]() -> int {
      Z.texp_n = (int64_t)items.size();
      if (items.empty()) items.push_back(FcExpTItem{0, 0, 0, 0});
      FCCHK(Z.texp.upload(items, in->stream));
      FCCHK(Z.tpos.upload(tpos, in->stream));
      FCCHK(Z.a_t.alloc((size_t)Z.nnz));
      FCCHK(Z.e_t.alloc((size_t)Z.nnz));
      FCCHK(Z.f_other.alloc(in->sys[0].f_val.n));
      FCCHK(Z.f_other.zero(in->stream));
      FCCHK(shifted_gather_transposed(Z));
      FCCHK(shifted_export_adjoint(Z));
      return FC_OK;
    };
    code = build();
    HIPCHK(hipStreamSynchronize(in->stream));  // (the host lists go out of scope)
    if (code != FC_OK) {
      const std::string msg = g_err;
      shifted_release_adjoint(Z);
      g_err = msg;
      return code;
    }
    Z.adj_avail = true;
  }
  const bool want = on == 1;
  if (want != Z.adj_on) {
    Z.adj_on = want;
    shifted_use(Z, want);
    Z.arn_started = false;  // the basis belongs to the other operator
    ++Z.n_switch;
  }
  if (on == -1 && Z.adj_avail) {
    HIPCHK(hipStreamSynchronize(in->stream));
    shifted_release_adjoint(Z);
  }
  return FC_OK;
}

int fc_shifted_adjoint_info(fc_handle h, int64_t* info, double* dinfo) {
  if (!h) return fail(FC_ERR_INVALID, "fc_shifted_adjoint_info: null handle");
  const ShiftedSolver* Z = h->shf;
  if (info) {
    info[0] = Z ? (Z->adj_on ? 1 : 0) : 0;
    info[1] = Z ? shifted_adjoint_bytes(*Z) : 0;
    info[2] = Z ? Z->n_texport : 0;
    info[3] = Z ? Z->n_switch : 0;
  }
  if (dinfo) {
    dinfo[0] = Z ? Z->texp_ms : 0.0;
    dinfo[1] = Z ? Z->texp_bytes : 0.0;
  }
  return FC_OK;
}

int fc_shifted_arnoldi_set_op(fc_handle h, int32_t kind) {
  if (!h || (kind != 0 && kind != 1)) return fail(FC_ERR_INVALID, "fc_shifted_arnoldi_set_op: kind must be 0 (shift-invert) or 1 (resolvent)");
  if (kind == 0 && !h->shf) return FC_OK;
  if (kind == 1 && !(h->shf && h->shf->factored && h->shf->adj_avail))
    return fail(FC_ERR_NOT_READY, "fc_shifted_arnoldi_set_op: the resolvent operator needs the adjoint factors (fc_shifted_set_adjoint first)");
  ShiftedSolver& Z = *h->shf;
  if (kind != Z.arn_kind) Z.arn_started = false;
  Z.arn_kind = kind;
  return FC_OK;
}

int fc_release_shifted(fc_handle h) {
  if (!h) return fail(FC_ERR_INVALID, "fc_release_shifted: null handle");
  (void)hipSetDevice(h->device);
  shifted_free(h);
  return FC_OK;
}

int fc_shifted_arnoldi_start(fc_handle h, int32_t m, const double* v0) {
  FCCHK(shifted_ready(h, "fc_shifted_arnoldi_start"));
  if (m < 2 || m > 1024 || !v0) return fail(FC_ERR_INVALID, "fc_shifted_arnoldi_start: bad argument");
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  Z.arn_started = false;
  hipStream_t st = Z.in->stream;
  const size_t n2 = 2 * (size_t)Z.n;
  if (Z.m != m || Z.V.n != n2 * (m + 1)) {
    FCCHK(Z.V.alloc(n2 * (m + 1)));
    FCCHK(Z.T.alloc(n2 * m));
    FCCHK(Z.Q.alloc(2 * (size_t)m * m));
    FCCHK(Z.hd.alloc(2 * (3 * (size_t)m + 4)));
    if (Z.part.n < 2 * 64 * (size_t)(m + 1)) FCCHK(Z.part.alloc(2 * 64 * (size_t)(m + 1)));
    Z.m = m;
  }
  // V_0 = Op v0 / |Op v0|: the start vector is purged of the (infinite-eigenvalue) directions outside the range of Op
  HIPCHK(hipMemcpyAsync(Z.T.p, v0, n2 * sizeof(double), hipMemcpyHostToDevice, st));
  double rel = 0.0;
  FCCHK(shifted_op(h, Z, Z.T.p, Z.V.p, &rel));
  FCCHK(shifted_multidot(Z, 1, Z.V.p, Z.V.p, 0));
  double nrm[2];
  HIPCHK(hipMemcpyAsync(nrm, Z.hd.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (!(nrm[0] > 0.0) || !std::isfinite(nrm[0])) return fail(FC_ERR_INVALID, "fc_shifted_arnoldi_start: Op v0 vanishes");
  hipLaunchKernelGGL(fc_scale, dim3(nblocks((int64_t)n2, 256)), dim3(256), 0, st, (int)n2, 1.0 / std::sqrt(nrm[0]), Z.V.p, Z.V.p);
  HIPCHK(hipGetLastError());
  Z.arn_started = true;
  return FC_OK;
}

int fc_shifted_arnoldi_step(fc_handle h, int32_t j, double* hcol, double* beta) {
  FCCHK(shifted_ready(h, "fc_shifted_arnoldi_step"));
  ShiftedSolver& Z = *h->shf;
  if (j < 0 || j >= Z.m || !hcol || !beta) return fail(FC_ERR_INVALID, "fc_shifted_arnoldi_step: bad argument (fc_shifted_arnoldi_start first)");
  if (!Z.arn_started)
    return fail(FC_ERR_NOT_READY, "fc_shifted_arnoldi_step: the basis was dropped by fc_shifted_set_adjoint / fc_shifted_arnoldi_set_op "
                                  "(fc_shifted_arnoldi_start first)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const size_t n2 = 2 * (size_t)Z.n;
  const int nv = j + 1;
  double* w = Z.V.p + n2 * (j + 1);
  double rel = 0.0;
  FCCHK(shifted_op(h, Z, Z.V.p + n2 * j, w, &rel));
  // classical Gram-Schmidt, twice: h1 = V^H w, w -= V h1; h2 = V^H w, w -= V h2; then |w|^2
  for (int pass = 0; pass < 2; ++pass) {
    FCCHK(shifted_multidot(Z, nv, Z.V.p, w, pass * (Z.m + 1)));
    hipLaunchKernelGGL(fc_cgs_update, dim3(nblocks(Z.n, 256)), dim3(256), 0, st, Z.n, nv, reinterpret_cast<const double2*>(Z.V.p),
                       reinterpret_cast<const double2*>(Z.hd.p) + pass * (Z.m + 1), reinterpret_cast<double2*>(w));
  }
  FCCHK(shifted_multidot(Z, 1, w, w, 2 * (Z.m + 1)));
  std::vector<double> hh(2 * (3 * (size_t)Z.m + 3));
  HIPCHK(hipMemcpyAsync(hh.data(), Z.hd.p, hh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < nv; ++i) {
    hcol[2 * i] = hh[2 * (size_t)i] + hh[2 * ((size_t)Z.m + 1 + i)];
    hcol[2 * i + 1] = hh[2 * (size_t)i + 1] + hh[2 * ((size_t)Z.m + 1 + i) + 1];
  }
  *beta = std::sqrt(std::max(0.0, hh[2 * (2 * (size_t)Z.m + 2)]));
  if (*beta > 0.0) hipLaunchKernelGGL(fc_scale, dim3(nblocks((int64_t)n2, 256)), dim3(256), 0, st, (int)n2, 1.0 / *beta, w, w);
  HIPCHK(hipGetLastError());
  return FC_OK;
}

int fc_shifted_arnoldi_restart(fc_handle h, int32_t m, int32_t k, const double* Q) {
  FCCHK(shifted_ready(h, "fc_shifted_arnoldi_restart"));
  ShiftedSolver& Z = *h->shf;
  if (m != Z.m || k < 1 || k >= m || !Q) return fail(FC_ERR_INVALID, "fc_shifted_arnoldi_restart: bad argument");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const size_t n2 = 2 * (size_t)Z.n;
  HIPCHK(hipMemcpyAsync(Z.Q.p, Q, 2 * (size_t)m * k * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fc_cbasis_combine, dim3(nblocks(Z.n, 256), k), dim3(256), 0, st, Z.n, m, k, reinterpret_cast<const double2*>(Z.V.p),
                     reinterpret_cast<const double2*>(Z.Q.p), reinterpret_cast<double2*>(Z.T.p));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(Z.V.p, Z.T.p, n2 * k * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(Z.V.p + n2 * k, Z.V.p + n2 * m, n2 * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return FC_OK;
}

int fc_shifted_ritz(fc_handle h, int32_t m, int32_t k, const double* Y, const double* lam, double* res, double* X) {
  FCCHK(shifted_ready(h, "fc_shifted_ritz"));
  ShiftedSolver& Z = *h->shf;
  if (m != Z.m || k < 1 || k > m || !Y || !lam || !res) return fail(FC_ERR_INVALID, "fc_shifted_ritz: bad argument");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const size_t n2 = 2 * (size_t)Z.n;
  if (Z.hd.n < 6 * (size_t)k) FCCHK(Z.hd.alloc(6 * (size_t)k));
  HIPCHK(hipMemcpyAsync(Z.Q.p, Y, 2 * (size_t)m * k * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(fc_cbasis_combine, dim3(nblocks(Z.n, 256), k), dim3(256), 0, st, Z.n, m, k, reinterpret_cast<const double2*>(Z.V.p),
                     reinterpret_cast<const double2*>(Z.Q.p), reinterpret_cast<double2*>(Z.T.p));
  HIPCHK(hipGetLastError());
  if (Z.arn_kind == 1) {
    // resolvent: |Op_R x - lam x|, |Op_R x|, |x| per Ritz vector; hd: per column three complex dots, then lam [k]
    if (Z.hd.n < 8 * (size_t)k) FCCHK(Z.hd.alloc(8 * (size_t)k));
    double* lam_d = Z.hd.p + 6 * (size_t)k;
    HIPCHK(hipMemcpyAsync(lam_d, lam, 2 * (size_t)k * sizeof(double), hipMemcpyHostToDevice, st));
    for (int c = 0; c < k; ++c) {
      const double* x = Z.T.p + n2 * c;
      double rel = 0.0;
      FCCHK(shifted_op(h, Z, x, Z.st.p, &rel));
      FCCHK(shifted_multidot_to(Z, 1, Z.st.p, Z.st.p, Z.hd.p + 6 * (size_t)c + 2, true, nullptr));
      FCCHK(shifted_multidot_to(Z, 1, x, x, Z.hd.p + 6 * (size_t)c + 4, true, nullptr));
      hipLaunchKernelGGL(fc_cgs_update, dim3(nblocks(Z.n, 256)), dim3(256), 0, st, Z.n, 1, reinterpret_cast<const double2*>(x),
                         reinterpret_cast<const double2*>(lam_d) + c, reinterpret_cast<double2*>(Z.st.p));
      FCCHK(shifted_multidot_to(Z, 1, Z.st.p, Z.st.p, Z.hd.p + 6 * (size_t)c, true, nullptr));
    }
    HIPCHK(hipGetLastError());
    std::vector<double> d2(6 * (size_t)k);
    HIPCHK(hipMemcpyAsync(d2.data(), Z.hd.p, d2.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (X) HIPCHK(hipMemcpyAsync(X, Z.T.p, n2 * k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t q = 0; q < 3 * (size_t)k; ++q) res[q] = std::sqrt(std::max(0.0, d2[2 * q]));
    return FC_OK;
  }
  // |A x - lam E x|, |A x|, |E x| per Ritz vector, all through the shifted SpMV (the adjoint mode: A^T and E^T)
  for (int c = 0; c < k; ++c) {
    const double* x = Z.T.p + n2 * c;
    FCCHK(shifted_spmv(h, Z, lam[2 * c], lam[2 * c + 1], 1.0, x, nullptr, Z.rz.p, Z.hd.p + 3 * c));
    FCCHK(shifted_spmv(h, Z, 0.0, 0.0, -1.0, x, nullptr, Z.rz.p, Z.hd.p + 3 * c + 1));
    FCCHK(shifted_spmv(h, Z, 1.0, 0.0, 0.0, x, nullptr, Z.rz.p, Z.hd.p + 3 * c + 2));
  }
  std::vector<double> r2(3 * (size_t)k);
  HIPCHK(hipMemcpyAsync(r2.data(), Z.hd.p, r2.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (X) HIPCHK(hipMemcpyAsync(X, Z.T.p, n2 * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t q = 0; q < r2.size(); ++q) res[q] = std::sqrt(std::max(0.0, r2[q]));
  return FC_OK;
}

int fc_sym_build_shifted(int32_t nv, int32_t ne, int32_t nc, const double* coords, const int32_t* cells, const int32_t* cell_edges, int32_t depth,
                         int32_t merge, void** out) {
  if (!out || !coords || !cells || !cell_edges || nv <= 0 || ne <= 0 || nc <= 0 || merge < 1 || depth < 0)
    return fail(FC_ERR_INVALID, "fc_sym_build_shifted: bad argument");
  *out = nullptr;
  try {
    std::vector<int> cd, rp, col, rp2, col2;
    std::vector<double> cent;
    std::vector<int64_t> code;
    sym_mesh_tables(nv, ne, nc, coords, cells, cell_edges, cd, cent, rp, col);
    doubled_pattern(rp, col, rp2, col2, code);
    ShiftedSym y = shifted_symbolic(cd, cent, nc, rp2, col2, depth, merge);
    fc_sym* sy = new fc_sym();
    auto put = [&](const char* name, auto const& vec) { sy->v[name].assign(vec.begin(), vec.end()); };
    put("perm", y.t.perm);
    put("plan_nodes", y.pl.nodes);
    put("node_i0", y.pl.node_i0);
    put("level_ptr", y.pl.level_ptr);
    sy->v["n_val"] = {y.fac.n_val};
    sy->v["front_size"] = {y.pl.front_size};
    *out = sy;
  } catch (const std::exception& e) {
    return fail(FC_ERR_INVALID, std::string("fc_sym_build_shifted: ") + e.what());
  }
  return FC_OK;
}

// ── snapshot sets: balanced reduced models from frequency snapshots ("Reduced models") ──────────────────────────────
namespace {
constexpr int kSnapChunk = 32;  // right-hand columns per operator pass = one 64-column tile of fc_snap_gram

int snap_ready(fc_ctx* h, int32_t set, const char* who) {
  if (!h) return fail(FC_ERR_INVALID, std::string(who) + ": null handle");
  if (!h->shf || !h->shf->in) return fail(FC_ERR_NOT_READY, std::string(who) + ": call fc_setup_shifted first");
  if (set < 0 || set > 2) return fail(FC_ERR_INVALID, std::string(who) + ": the set must be 0 (direct), 1 (adjoint) or 2 (loaded)");
  return FC_OK;
}
}  // namespace

int fc_shifted_snap_reserve(fc_handle h, int32_t set, int32_t ncol) {
  FCCHK(snap_ready(h, set, "fc_shifted_snap_reserve"));
  if (ncol < 0 || ncol > 65536) return fail(FC_ERR_INVALID, "fc_shifted_snap_reserve: ncol must be in [0, 65536]");
  HIPCHK(hipSetDevice(h->device));
  ShiftedSolver& Z = *h->shf;
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  if (ncol != Z.snap_cap[set]) {
    Z.snap[set].release();
    Z.snap_cap[set] = Z.snap_cnt[set] = 0;
    if (ncol > 0) {
      FCCHK(Z.snap[set].alloc(2 * (size_t)Z.n * ncol));
      Z.snap_cap[set] = ncol;
    }
  }
  if (Z.snap_cap[0] + Z.snap_cap[1] + Z.snap_cap[2] == 0) Z.snap_w.release(), Z.snap_part.release(), Z.snap_out.release();
  return FC_OK;
}

int fc_shifted_snap_clear(fc_handle h, int32_t set) {
  FCCHK(snap_ready(h, set, "fc_shifted_snap_clear"));
  h->shf->snap_cnt[set] = 0;
  return FC_OK;
}

int fc_shifted_snap_push(fc_handle h, int32_t set, int32_t ncol, double scale) {
  FCCHK(snap_ready(h, set, "fc_shifted_snap_push"));
  ShiftedSolver& Z = *h->shf;
  if (ncol <= 0 || ncol > Z.nrhs_last || !std::isfinite(scale))
    return fail(FC_ERR_INVALID, "fc_shifted_snap_push: ncol must be in 1 .. the columns of the last solve, the scale finite");
  if (Z.snap_cnt[set] + ncol > Z.snap_cap[set])
    return fail(FC_ERR_INVALID, "fc_shifted_snap_push: set " + std::to_string(set) + " holds " + std::to_string(Z.snap_cnt[set]) + " of " +
                                    std::to_string(Z.snap_cap[set]) + " columns: no room for " + std::to_string(ncol) + " more");
  HIPCHK(hipSetDevice(h->device));
  const int64_t cnt = 2 * (int64_t)Z.n * ncol;
  hipLaunchKernelGGL(fc_snap_push, dim3(nblocks(cnt, 256)), dim3(256), 0, Z.in->stream, cnt, scale, (const double*)Z.xz.p,
                     Z.snap[set].p + 2 * (size_t)Z.n * Z.snap_cnt[set]);
  HIPCHK(hipGetLastError());
  Z.snap_cnt[set] += ncol;
  return FC_OK;
}

int fc_shifted_snap_load(fc_handle h, int32_t set, int32_t ncol, const double* re, const double* im, double scale) {
  FCCHK(snap_ready(h, set, "fc_shifted_snap_load"));
  ShiftedSolver& Z = *h->shf;
  if (ncol <= 0 || !re || !std::isfinite(scale)) return fail(FC_ERR_INVALID, "fc_shifted_snap_load: bad argument");
  if (Z.snap_cnt[set] + ncol > Z.snap_cap[set])
    return fail(FC_ERR_INVALID, "fc_shifted_snap_load: set " + std::to_string(set) + " holds " + std::to_string(Z.snap_cnt[set]) + " of " +
                                    std::to_string(Z.snap_cap[set]) + " columns: no room for " + std::to_string(ncol) + " more");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  const int n = Z.n;
  for (int c = 0; c < ncol; ++c) {
    HIPCHK(hipMemcpyAsync(Z.st.p, re + (size_t)n * c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    if (im) HIPCHK(hipMemcpyAsync(Z.st.p + n, im + (size_t)n * c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fc_snap_load, dim3(nblocks(n, 256)), dim3(256), 0, st, n, scale, (const double*)Z.st.p,
                       im ? (const double*)(Z.st.p + n) : (const double*)nullptr,
                       reinterpret_cast<double2*>(Z.snap[set].p + 2 * (size_t)n * (Z.snap_cnt[set] + c)));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));  // (the staging buffer is reused by the next column)
  }
  Z.snap_cnt[set] += ncol;
  return FC_OK;
}

int fc_shifted_snap_gram(fc_handle h, int32_t left, int32_t right, int32_t kind, double* out) {
  FCCHK(snap_ready(h, left, "fc_shifted_snap_gram"));
  FCCHK(snap_ready(h, right, "fc_shifted_snap_gram"));
  ShiftedSolver& Z = *h->shf;
  if (kind < 0 || kind > 2 || !out) return fail(FC_ERR_INVALID, "fc_shifted_snap_gram: kind must be 0 (identity), 1 (E) or 2 (A), out not null");
  const int ncl = Z.snap_cnt[left], ncr = Z.snap_cnt[right];
  if (ncl == 0 || ncr == 0) return fail(FC_ERR_INVALID, "fc_shifted_snap_gram: an empty set");
  HIPCHK(hipSetDevice(h->device));
  fc_ctx* in = Z.in;
  hipStream_t st = in->stream;
  const int n = Z.n, ld = 2 * ncr;
  const size_t n2 = 2 * (size_t)n;
  // slices of N: enough workgroups to fill the device, slices of at least 256 rows, a multiple of the kernel's chunk
  const int ti = nblocks(ncl, 32);
  const int ns0 = std::max(1, std::min(nblocks(n, 256), nblocks(512, ti)));
  const int slice = kSnapKC * nblocks(nblocks(n, ns0), kSnapKC);
  const int ns = nblocks(n, slice);
  const size_t cnt = 2 * (size_t)ncl * ld;
  if (kind != 0 && Z.snap_w.n < n2 * kSnapChunk) FCCHK(Z.snap_w.alloc(n2 * kSnapChunk));
  if (Z.snap_part.n < cnt * ns) FCCHK(Z.snap_part.alloc(cnt * ns));
  if (Z.snap_out.n < cnt) FCCHK(Z.snap_out.alloc(cnt));
  const double mean = (double)Z.nnz / std::max(1, n);
  const int L = mean <= 24 ? 8 : (mean <= 64 ? 16 : 32);
  const int g = nblocks(n, 256 / L);
  const double s_re = kind == 1 ? 1.0 : 0.0, t = kind == 2 ? -1.0 : 0.0;  // (s E - t A): E, or A -- the held direct values, no pin
  HIPCHK(hipEventRecord(in->ev0, st));
  for (int b0 = 0; b0 < ncr; b0 += kSnapChunk) {
    const int nb = std::min(kSnapChunk, ncr - b0);
    const double* R = Z.snap[right].p + n2 * b0;
    const double* W = R;
    if (kind != 0) {
      for (int c = 0; c < nb; ++c) {
        const double2* x2 = reinterpret_cast<const double2*>(R + n2 * c);
        double2* y2 = reinterpret_cast<double2*>(Z.snap_w.p + n2 * c);
        auto launch = [&](auto LANES) {
          hipLaunchKernelGGL(fc_shifted_spmv<LANES>, dim3(g), dim3(256), 0, st, n, h->rowptr.p, h->col.p, Z.a.p, Z.e.p, s_re, 0.0, t, x2,
                             (const double2*)nullptr, y2, (double*)nullptr, -1, 0.0);
        };
        if (!pick(fc_dispatch::ShiftedSpmvLanes{}, L, launch)) launch(int_c<32>{});
      }
      HIPCHK(hipGetLastError());
      W = Z.snap_w.p;
    }
    hipLaunchKernelGGL(fc_snap_gram, dim3(ti, 1, ns), dim3(256), 0, st, n, slice, ncl, nb, reinterpret_cast<const double2*>(Z.snap[left].p),
                       reinterpret_cast<const double2*>(W), ld, 2 * b0, Z.snap_part.p);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(fc_snap_gram_reduce, dim3(nblocks((int64_t)cnt, 256)), dim3(256), 0, st, (int64_t)cnt, ns, (const double*)Z.snap_part.p, Z.snap_out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(in->ev1, st));
  HIPCHK(hipMemcpyAsync(out, Z.snap_out.p, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, in->ev0, in->ev1));
  Z.gram_ms = (double)ms;
  // each set read once; the operator pass reads the pattern and both value arrays per column and writes + re-reads W
  Z.gram_bytes = 16.0 * n * ((double)ncl + ncr) + (kind != 0 ? (double)ncr * (4.0 * (n + 1.0) + 20.0 * (double)Z.nnz + 32.0 * n) : 0.0);
  Z.gram_flops = 2.0 * n * (2.0 * ncl) * (2.0 * ncr);
  ++Z.n_gram;
  return FC_OK;
}

int fc_shifted_snap_combine(fc_handle h, int32_t set, int32_t k, const double* Q, double* out) {
  FCCHK(snap_ready(h, set, "fc_shifted_snap_combine"));
  ShiftedSolver& Z = *h->shf;
  const int nc = Z.snap_cnt[set];
  if (k <= 0 || k > 65535 || !Q || !out) return fail(FC_ERR_INVALID, "fc_shifted_snap_combine: bad argument");
  if (nc == 0) return fail(FC_ERR_INVALID, "fc_shifted_snap_combine: an empty set");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = Z.in->stream;
  DevBuf<double> dq, dout;
  FCCHK(dq.upload(Q, 2 * (size_t)nc * k, st));
  FCCHK(dout.alloc((size_t)Z.n * k));
  hipLaunchKernelGGL(fc_snap_combine, dim3(nblocks(Z.n, 256), k), dim3(256), 0, st, Z.n, nc, k, reinterpret_cast<const double2*>(Z.snap[set].p),
                     (const double*)dq.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)Z.n * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FC_OK;
}

int fc_shifted_snap_info(fc_handle h, int64_t* info) {
  if (!h || !info) return fail(FC_ERR_INVALID, "fc_shifted_snap_info: null argument");
  const ShiftedSolver* Z = h->shf;
  for (int s = 0; s < 3; ++s) info[2 * s] = Z ? Z->snap_cnt[s] : 0, info[2 * s + 1] = Z ? Z->snap_cap[s] : 0;
  info[6] = Z ? shifted_snap_bytes(*Z) : 0;
  info[7] = Z ? Z->n_gram : 0;
  return FC_OK;
}

int fc_bench_snap_gram_last(fc_handle h, double* out) {
  if (!h || !out) return fail(FC_ERR_INVALID, "fc_bench_snap_gram_last: null argument");
  const ShiftedSolver* Z = h->shf;
  out[0] = Z ? Z->gram_ms : 0.0;
  out[1] = Z ? Z->gram_bytes : 0.0;
  out[2] = Z ? Z->gram_flops : 0.0;
  return FC_OK;
}

int fc_debug_get_snapshots(fc_handle h, int32_t set, int32_t first, int32_t ncol, double* out) {
  FCCHK(snap_ready(h, set, "fc_debug_get_snapshots"));
  ShiftedSolver& Z = *h->shf;
  if (first < 0 || ncol <= 0 || first + ncol > Z.snap_cnt[set] || !out) return fail(FC_ERR_INVALID, "fc_debug_get_snapshots: bad argument");
  HIPCHK(hipSetDevice(h->device));
  const size_t n2 = 2 * (size_t)Z.n;
  HIPCHK(hipMemcpyAsync(out, Z.snap[set].p + n2 * first, n2 * ncol * sizeof(double), hipMemcpyDeviceToHost, Z.in->stream));
  HIPCHK(hipStreamSynchronize(Z.in->stream));
  return FC_OK;
}

}  // extern "C"
