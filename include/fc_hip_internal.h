/*
 * fc_hip_internal.h — entry points of libfc_hip.so that are NOT the drop-in boundary (include/fc_hip.h is):
 *   - array-level setup for callers that bring their own symbolic analysis (flowcontrol_amd/ndsolver.py is the readable
 *     specification of the in-library one; tests compare the two table by table),
 *   - the symbolic phase on its own (fc_sym_*),
 *   - bench / profiling / debug hooks used by bench.py, scripts/ and the tests.
 * Same conventions as fc_hip.h (plain C, int status, opaque handle).  Nothing here is needed to drive a simulation.
 */
#ifndef FC_HIP_INTERNAL_H
#define FC_HIP_INTERNAL_H

#include "fc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* time `reps` back-to-back launches of the CSR SpMV kernel with HIP events on the handle's
 * stream; returns the mean milliseconds per launch */
int fc_bench_spmv(fc_handle h, int slot, int reps, double* ms_per_launch);
/* ── solver setup: replaces LUSolver.set_operator(A) + the factorisation MUMPS performs at the
 *    first solve (flowsolver.py:697,729).  The host side (flowcontrol_amd/ndsolver.py) supplies
 *    the nested-dissection permutation and the level-wise selected-inverse factors. ---------- */
int fc_set_permutation(fc_handle h, const int32_t* perm /* [N] new -> old */);
int fc_solver_setup(fc_handle h, int slot, const int32_t* Ap_rowptr, const int32_t* Ap_col,
                    const double* Ap_val, /* permuted system matrix (N rows) */
                    int32_t n_stages, const int64_t* stage_begin /* [n_stages] first row in seg_ptr */,
                    const int32_t* stage_row0 /* [n_stages] first destination row */,
                    const int32_t* stage_nrows /* [n_stages] */,
                    const int32_t* stage_kind /* [n_stages] 0 = up (y += ..), 1 = down (x = ..), 2 = diagonal (x = dscale y) */,
                    const int64_t* seg_ptr /* [total_rows + 1] */, int64_t n_seg,
                    const int64_t* seg_val /* [n_seg] offset into vals */,
                    const int32_t* seg_col /* [n_seg] >=0: first buffer index; <0: -(offset into idx)-1 */,
                    const int32_t* seg_len /* [n_seg] */, int64_t n_idx, const int32_t* idx,
                    int64_t n_val, const double* vals,
                    /* multi-GPU: after stage `ar_stage` (-1: none) the rows [ar_row0, ar_row0+ar_n) of the
                     * work buffer are summed over the ranks (RCCL all-reduce) */
                    int32_t ar_stage, int32_t ar_row0, int32_t ar_n,
                    /* and the rows x[ar_row0 .. +ar_n) after stage `ar2_stage` (-1: none): the root's down stage, in which
                     * every rank fills its own block of the root's rows (the others are zeroed before the launch) */
                    int32_t ar2_stage);
/* Truncated factors (memory-lean preconditioner): stages of kind 2 stand for tree levels whose pivot blocks are NOT
 * stored; on their rows x = dscale * y (dscale [N], permuted numbering: a diagonal stand-in for the Schur complement).
 * Such a slot is a preconditioner only: fc_solve / fc_step need FC_METHOD_GMRES or FC_METHOD_BICGSTAB. */
int fc_set_stage_diag(fc_handle h, int slot, const double* dscale /* [N] */);
/* optional: hand the down-sweep stages to the LDS-tiled block kernel.  Every block is up to 32
 * consecutive rows of ONE tree node, whose rows all read the same operand
 * [ y[i0..i0+ni) | x[idx[idx_off..+nb)] ] and whose values lie row-major (stride ni+nb) at blk_val.
 * stage_* arrays have one entry per stage of fc_solver_setup (count 0 = keep the segment kernel). */
int fc_solver_set_blocks(fc_handle h, int slot, int32_t n_stages, const int64_t* stage_blk_begin,
                         const int32_t* stage_blk_count, const int32_t* stage_lpr, int64_t n_blk,
                         const int64_t* blk_val, const int32_t* blk_row0, const int32_t* blk_nrows,
                         const int32_t* blk_i0, const int32_t* blk_ni, const int32_t* blk_idx,
                         const int32_t* blk_nb, int64_t n_idx, int64_t n_val);
/* the symbolic phase on its own, no device involved: every table fc_setup_solver derives, by name, widened to int64
 * (tests compare them with flowcontrol_amd/ndsolver.py entry by entry) */
int fc_sym_build(int32_t nv, int32_t ne, int32_t nc, const double* coords, const int32_t* cells, const int32_t* cell_edges,
                 int32_t n_bc, const int32_t* bc_dofs, int32_t depth, int32_t merge, int32_t world, int32_t rank, int32_t truncate,
                 void** out);
/* the symbolic phase of the complex-shifted solver (fc_setup_shifted) on its own: the real-equivalent system of order 2 N (dof i -> 2 i,
 * 2 i + 1; 30 dofs per cell), no skipped dofs; tables "perm", "plan_nodes", "node_i0", "level_ptr", "n_val", "front_size" */
int fc_sym_build_shifted(int32_t nv, int32_t ne, int32_t nc, const double* coords, const int32_t* cells, const int32_t* cell_edges, int32_t depth,
                         int32_t merge, void** out);
int fc_sym_size(void* sym, const char* name, int64_t* n);
int fc_sym_get(void* sym, const char* name, int64_t* out);
int fc_sym_free(void* sym);
/* Numeric factorisation ON THE DEVICE (what `solver.set_operator(A)` costs in the reference,
 * flowsolver.py:697,812-814 -> PETSc/MUMPS numeric phase; also every Newton/Picard iteration of
 * steadystate.py:60-159).  fc_factor_plan uploads the symbolic side once per (tree, pattern): all
 * fronts of the elimination tree live in one row-major buffer; `nodes` has 7 int64 per tree node in
 * elimination order (level, front offset, front order nf, pivot order ni, offset of the node's
 * [D^-1 | -U] rows in the factor values or -1, parent row or -1, child slot), `level_ptr`/`a_ptr` give
 * node and matrix-entry ranges per level (deepest first), (a_src, a_dst) scatter the CSR values of a slot
 * into the fronts, ext_p[ext_off[g] ...] are the positions of child g's update block in its parent's
 * front, ap_src maps the permuted matrix of the residual monitor to CSR value indices.
 * fc_refactor(slot) then recomputes the factor values and the permuted matrix of `slot` from the
 * slot's current CSR values (after fc_assemble_matrix + fc_apply_bc): scatter, per level extend-add of
 * the children's Schur complements, then the in-place elimination of all fronts of the level together by blocked
 * Gauss-Jordan steps of 32 pivot columns (pivot block inverted in LDS with partial pivoting inside the block, panels,
 * trailing update on the fp64 matrix cores, v_mfma_f64_16x16x4_f64: csrc/fc_front.hip.h), exported straight into the
 * layout the sweeps read.  No vendor BLAS / LAPACK is involved.
 * The structure (fc_solver_setup / fc_solver_set_blocks) must have been uploaded before, with any
 * values.  ms_out (optional): device time of the numeric phase.  On a partitioned handle every rank factorises its own
 * sub-tree and the root (plan built with keep=); the root front is summed over the ranks once (exchange). */
int fc_factor_plan(fc_handle h, int32_t n_nodes, const int64_t* nodes, int32_t n_levels, const int64_t* level_ptr,
                   int64_t front_size, int64_t n_a, const int64_t* a_src, const int64_t* a_dst,
                   const int64_t* a_ptr, const int64_t* ext_off, int64_t n_ext, const int32_t* ext_p,
                   int64_t n_ap, const int64_t* ap_src, int32_t max_slots);
/* Multi-GPU layouts made outside fc_setup_solver: of the ROOT's pivot-block inverse (the last plan node; every rank
 * eliminates the whole root front) this handle stores only the pivot rows [first, first + count) (0-based inside the
 * root's block) -- the rows it applies in the root's down stage -- at the root's value offset, row `first` first.
 * first = -1: all rows (single GPU).  Call before fc_refactor; fc_setup_solver does it itself. */
int fc_set_root_rows(fc_handle h, int32_t first, int32_t count);
/* values added to front entries (offsets into the front buffer of fc_factor_plan) after the matrix has
 * been scattered, in every later fc_refactor: a positive shift on ONE pressure diagonal selects the
 * solution with that pressure = 0 of an enclosed flow's singular system (lid-driven cavity; the reference
 * leaves that system to MUMPS, examples/lidcavity/lidcavityflowsolver.py:57-72).  n = 0 clears. */
int fc_set_front_shifts(fc_handle h, int32_t n, const int64_t* slots, const double* values);
/* download the factor values of a slot (n = the n_val given to fc_solver_setup): parity checks */
int fc_get_factor_values(fc_handle h, int slot, int64_t n, double* out);
/* velocity mass matrix (u,v) in the solver's permuted numbering, CSR with N rows (pressure rows
 * empty): the matrix behind compute_perturbation_energy (flowsolver.py:827-829), used by the
 * fused step tail */
int fc_set_energy_matrix(fc_handle h, const int32_t* rowptr, const int32_t* col, const double* val);
/* info[8]: k, KB, scratch rows of the up-sweep, block launches and fold launches per apply, factor bytes of one
 * batched apply (they serve KB simulated steps), vector (operand / result / fold) bytes of one batched apply, tasks */
int fc_get_batch_info(fc_handle h, double* info /* [8] */);
/* HIP-event timing of `reps` back-to-back batched factor applies; mean milliseconds per apply */
int fc_bench_batch_apply(fc_handle h, int slot, int reps, double* ms_per_apply);
/* the shifted solver's block (fc_shifted_set_block) against its single-column path, HIP-event timing of `reps` back-to-back launches on
 * zero operands: ms[4] / bytes[4] = mean milliseconds / algorithmic bytes of one batched factor apply at the block's padded width, one
 * fc_shifted_spmv_b, one single-column factor apply, one fc_shifted_spmv */
int fc_bench_shifted_block(fc_handle h, int reps, double* ms /* [4] */, double* bytes /* [4] */);
/* time `reps` back-to-back factor applies (all sweep launches of one M^-1 application) with HIP
 * events on the handle's stream; mean milliseconds per apply and launches per apply */
int fc_bench_sweeps(fc_handle h, int slot, int reps, double* ms_per_apply, int32_t* launches_per_apply);
/* HIP-event timing inside fc_step / fc_run: when on, the back-to-back factor-sweep launches of
 * every apply are bracketed by ONE event pair on the handle's stream (sweep_ms / sweep_launches =
 * mean launch duration including the inter-launch gap) and every in-step CSR SpMV launch by its own
 * pair; totals are accumulated after the step's synchronisation.  fc_set_timing resets them. */
int fc_set_timing(fc_handle h, int on);
int fc_get_timing(fc_handle h, double* sweep_ms, int64_t* sweep_launches, double* spmv_ms,
                  int64_t* spmv_launches);
/* algorithmic bytes of one factor apply (sum over sweep launches) and of one CSR SpMV */
int fc_algorithmic_bytes(fc_handle h, int slot, double* sweep_bytes, double* spmv_bytes);

/* shape of the handle's elimination tree: bits_out[<= 16] = bisections fused per tree level, root first (fc_setup_solver's tree, or the
 * default shape of this mesh before it ran); nnz_min_tree (optional, one host symbolic pass): factor values of the all-binary-pairs tree
 * [2, 2, ...] of the same depth -- the fixed denominator of bench.py's roofline.frac_min_tree */
int fc_get_tree_info(fc_handle h, int32_t* bits_out /* [16] */, int32_t* n_bits, int64_t* nnz_min_tree);

/* the multi-GPU partition as arrays (fc_setup_solver derives and applies it itself on a handle with an exchange): this rank's
 * cells and rowkind[N] (W numbering): 0 = other rank's dof, 1 = owned, 2 = root separator (replicated) */
int fc_set_partition(fc_handle h, int32_t n_local_cells, const int32_t* local_cells,
                     const uint8_t* rowkind /* [N] */, int lead);

/* trailing-update flops of the handle's last fc_refactor (each level priced by its widest front): as run, and what they would be if
 * every row of a multi-GPU root front were swept on every rank (the scheme up to round 3; FC_ROOT_SKIP=0 runs it): the eliminated
 * rows of the root front that a rank does not export are dead and skipped -- (1 + 1 / world) n^3 instead of 2 n^3 per rank */
int fc_get_refactor_flops(fc_handle h, double* run, double* full);

/* out = M^-1 in with the factor-free preconditioner of the slot (fc_setup_krylov), W layout (test aid).  On a partitioned handle a
 * collective: every rank passes the same `in` and gets the merged result. */
int fc_debug_apply_pc(fc_handle h, int slot, const double* in /* [N] */, double* out /* [N] */);
/* multiply the held factor values of the shifted solver by `scale` (test aid: inexact factors for the GMRES rescue of
 * fc_shifted_set_krylov; the adjoint array too when it exists); the next fc_setup_shifted recomputes them */
int fc_debug_scale_shifted_factors(fc_handle h, double scale);
/* download of the shifted solver's factor values (n = the n_val of fc_sym_build_shifted): adjoint = 0 the direct array, 1 the adjoint
 * one (fc_shifted_set_adjoint; FC_ERR_NOT_READY without it) -- test aid for the layout of the transposed export */
int fc_debug_get_shifted_factors(fc_handle h, int32_t adjoint, int64_t n, double* out);
/* download of the transposed factor values of a stepping slot (fc_set_adjoint_factors; n = the slot's factor values as for
 * fc_get_factor_values; FC_ERR_NOT_READY without them or while they are stale) -- test aid for the layout of the transposed export */
int fc_debug_get_adjoint_factors(fc_handle h, int slot, int64_t n, double* out);
/* download of ncol columns of the adjoint state tape from column col0 (fc_adjoint_tape_reserve / _begin; column 0 = x_{-1}, column
 * j + 1 = x_j; at most count + 2 columns exist): out [ncol][N] in the solver's PERMUTED numbering, as the tape holds them -- test aid */
int fc_debug_get_adjoint_tape(fc_handle h, int32_t col0, int32_t ncol, double* out);
/* download of ncol columns of the CHECKPOINTED tape's segment buffer from buffer column col0 (fc_adjoint_tape_reserve_sparse / _begin;
 * every + 2 columns exist): out [ncol][N] in the solver's PERMUTED numbering; *segment (may be NULL) = the segment j the buffer holds:
 * column 0 = x_{jc-1}, column i + 1 = x_{jc+i}.  Behind a march that is segment 0, recomputed if the run had more than one -- test aid */
int fc_debug_get_adjoint_segment(fc_handle h, int32_t col0, int32_t ncol, double* out, int32_t* segment);
/* the same for the checkpointed batched tape (fc_adjoint_tape_reserve_sparse_batch): out [ncol][k][N] in the W layout -- test aid */
int fc_debug_get_adjoint_segment_batch(fc_handle h, int32_t col0, int32_t ncol, int32_t k, double* out, int32_t* segment);
/* the handle's step counters: steps enqueued by fc_step / fc_run / fc_run_closed_loop, and batched steps (either may be NULL) -- test
 * aid: a march over a checkpointed tape recomputes forward steps and must count none of them */
int fc_debug_get_step_count(fc_handle h, int64_t* single, int64_t* batched);
/* the same for the batched state tape (fc_adjoint_tape_reserve_batch / _begin_batch): out [ncol][k][N] in the W layout -- test aid */
int fc_debug_get_adjoint_tape_batch(fc_handle h, int32_t col0, int32_t ncol, int32_t k, double* out);
/* download of ncol columns of a snapshot set from column `first` (fc_shifted_snap_*): out [ncol][N] complex interleaved -- test aid */
int fc_debug_get_snapshots(fc_handle h, int32_t set, int32_t first, int32_t ncol, double* out);
/* the last fc_shifted_snap_gram: out[3] = device ms between HIP events (operator pass, product, reduction), algorithmic bytes, flops */
int fc_bench_snap_gram_last(fc_handle h, double* out /* [3] */);
/* the last fc_state_snap_gram, in the same terms */
int fc_bench_state_snap_gram_last(fc_handle h, double* out /* [3] */);

/* What the handle's last time step launched (fc_step, fc_step_begin, the last step of fc_run): FC_STEP_ROUTE_COLS int32, written by the
 * launch sites themselves while the step was enqueued -- the record a test compares with its host model of the dispatch conditions, so
 * that a route that silently did not run fails.  No launch, no synchronisation, nothing in a step depends on it.
 *   [0] element kernel of the right-hand side: 0 = none, the element vectors speculated behind the previous step were reused;
 *       1 = fc_rhs_elem (eight lanes per cell); 2 = fc_rhs_elem_reg (a thread per cell)
 *   [1] order slot whose element loop was enqueued behind this step for the next one, -1: none
 *   [2] solver: 0 = one factor apply, 1 = the refinement driver (its sweeps, or none of them when the fused tail is off),
 *       2 = BiCGStab, 3 = GMRES
 *   [3] tail: 0 = fc_tail + fc_final, 1 = fc_tail with the fused final (FC_FUSED_FINAL=1), 2 = fc_finish + fc_final,
 *       3 = overlapped: fc_early on the main stream, fc_tail + fc_final_late on the side stream
 *   [4] 1 if this step formed the residual norms
 *   [5] row workgroups (tail 2: the workgroups of fc_finish)   [6] check workgroups   [7] cell workgroups (tail 2: workgroups of
 *       fc_finish that leave an energy partial)   [8] row / cell groups per workgroup (FC_TAIL_REPS)
 * FC_ERR_NOT_READY before the first step, FC_ERR_INVALID for a null handle / buffer or n < FC_STEP_ROUTE_COLS; nothing is written then. */
#define FC_STEP_ROUTE_COLS 9
int fc_get_step_route(fc_handle h, int32_t n, int32_t* out);

/* What the handle's last BATCHED time step launched (fc_step_batch, fc_step_batch_begin, the last step of fc_run_closed_loop_batch):
 * FC_BATCH_ROUTE_COLS int32, written by batch_enqueue / batch_launches / batch_launches_side where they decide -- a few ints in a host
 * struct: no launch, no synchronisation, nothing in a step depends on it.  A step replayed as a captured graph (FC_BATCH_GRAPH=1)
 * enqueues nothing: its record is the one written while that graph was captured.
 *   [0] lead: 2 = the step began with its element loop and the full gather, 1 = with the full gather (element vectors left by the
 *       previous step), 0 = with fc_rhs_ctrl_b only (the previous step gathered the control-independent right-hand side too)
 *   [1] element kernel this step launched, for itself or ahead for the next step: 0 none, FC_BATCH_ELEM_LDS fc_rhs_elem_b,
 *       _BREG fc_rhs_elem_breg<KB, false>, _BREG_FORCE fc_rhs_elem_breg<KB, true>
 *   [2] order slot + 1 whose element loop was enqueued behind this step for the next one, 0: none
 *   [3] 1 if the control-independent gather of the next step ran behind that loop
 *   [4] 1 = overlapped (fc_early_b on the main stream; fc_wait_solved_b, fc_tail_b, fc_final_late_b on the side stream), 0 = one stream
 *   [5] 1 if the gather that runs ahead opened the side stream's gate instead of fc_early_b
 *   [6] 1 if this step formed the residual norms
 *   [7] row blocks and [8] cell workgroups of fc_tail_b (both 0: it was not launched)   [9] tb_cols, the column width of a row block
 *   [10] KB, the padded batch width   [11] control rows of the step's slot (fc_rhs_ctrl_b), -1: not tabulated yet
 *   [12] 1 = replayed / captured as a HIP graph, 0 = plain launches
 * FC_ERR_NOT_READY before the first batched step (and after fc_set_batch), FC_ERR_INVALID for a null handle / buffer or
 * n < FC_BATCH_ROUTE_COLS; nothing is written then. */
#define FC_BATCH_ROUTE_COLS 13
#define FC_BATCH_ELEM_LDS 1
#define FC_BATCH_ELEM_BREG 2
#define FC_BATCH_ELEM_BREG_FORCE 3
int fc_get_batch_step_route(fc_handle h, int32_t n, int32_t* out);
/* The right-hand side the batched solve consumed (test aid).  on = 1: every batched step from here on copies its right-hand side,
 * device to device on the step's own stream, behind the gather / control-row launch and in front of the factor apply -- in the
 * one-stream form the gather that runs ahead overwrites the buffer with the next step's control-independent part before the host could
 * look.  on = 0 frees the copy.  The flag is part of the captured graphs' signature.  Never switched on: nothing is allocated and no
 * launch is added.  FC_ERR_INVALID while a step is in flight. */
int fc_debug_capture_batch_rhs(fc_handle h, int32_t on);
/* ... of the last batched step: out [k][N], W layout.  FC_ERR_NOT_READY without fc_set_batch, without capture or before the first
 * captured step; FC_ERR_INVALID for a null buffer or another k. */
int fc_debug_get_batch_rhs(fc_handle h, int32_t k, double* out);

/* What the handle's last backward (adjoint) step launched -- fc_step_adjoint, the last step of fc_run_adjoint / fc_run_adjoint_batch and of
 * the closed-loop marches built on them: FC_ADJ_ROUTE_COLS int32, written by the launch sites themselves while the step was enqueued (a few
 * ints in a host struct: no launch, no synchronisation, no allocation, nothing on the device reads them).
 *   [0] element kernel: FC_ADJ_ELEM_LANES fc_rhs_elem, _REG fc_rhs_elem_reg, _BREG fc_rhs_elem_breg<KB> (the forward loops on the two masked
 *       levels, linearised handles); _NL fc_adj_elem_nl, _NL_REG fc_adj_elem_nl_reg, _NL_B fc_adj_elem_nl_b<KB> (nonlinear handles)
 *   [1] its workgroups   [2] workgroups of fc_adj_rhs_gather / fc_adj_rhs_gather_b<KB>
 *   [3] 1 if sensor weights w were handed to the gather   [4] 1 if a terminal vector was
 *   [5] KB, the padded width of a batched step; 0: the single march   [6] k, its columns (0: the single march)
 *   [7] workgroups of fc_adj_tail / fc_adj_tail_b<KB> = partials per (actuator, column)   [8] the tail's passes ceil(n_act / 4), at least 1
 *   [9] 1 if fc_adj_reduce / fc_adj_reduce_b ran (not without actuators, not when the closed-loop march folds the partials itself)
 *   [10] its gx (0 if it did not run)
 *   [11] which fc_adj_tape_copy<NT> the last copy into the state tape of that march's kind used: 1 nontemporal, 0 plain (FC_ADJ_TAPE_NT=0),
 *        -1 no copy yet
 * FC_ERR_NOT_READY before the first backward step, FC_ERR_INVALID for a null handle / buffer or n < FC_ADJ_ROUTE_COLS. */
#define FC_ADJ_ROUTE_COLS 12
#define FC_ADJ_ELEM_LANES 1
#define FC_ADJ_ELEM_REG 2
#define FC_ADJ_ELEM_BREG 3
#define FC_ADJ_ELEM_NL 4
#define FC_ADJ_ELEM_NL_REG 5
#define FC_ADJ_ELEM_NL_B 6
/* ... while energy weights are held (fc_set_adjoint_energy), and only then: the three-level loops of linearised handles fc_adj_elem_en,
 * fc_adj_elem_en_reg, fc_adj_elem_en_b<KB>, and the EN = true instantiations of the nonlinear loops.  The state gradients at the end of a
 * run carry no energy term and report the codes above. */
#define FC_ADJ_ELEM_EN 7
#define FC_ADJ_ELEM_EN_REG 8
#define FC_ADJ_ELEM_EN_B 9
#define FC_ADJ_ELEM_NL_EN 10
#define FC_ADJ_ELEM_NL_REG_EN 11
#define FC_ADJ_ELEM_NL_B_EN 12
/* ... and while the energy source is the tangent tape (fc_set_adjoint_energy_source(1), single marches only): the same kernels of the
 * linearised scheme handed the tangent tape's column, and the <EN, SRC> = <true, true> instantiations of fc_adj_elem_nl / _reg */
#define FC_ADJ_ELEM_EN_SRC 13
#define FC_ADJ_ELEM_EN_REG_SRC 14
#define FC_ADJ_ELEM_NL_EN_SRC 15
#define FC_ADJ_ELEM_NL_REG_EN_SRC 16
int fc_get_adjoint_route(fc_handle h, int32_t n, int32_t* out);
/* Download of that step's buffers as the march holds them, in the solver's PERMUTED numbering (test aid; quiesces like the other
 * fc_debug_get_* calls).  kb / gx: entries [5] and [7] of fc_get_adjoint_route, which size the arrays (FC_ERR_INVALID if they are not the
 * last step's).  With W = max(1, kb) every vector is [N][W] (the single march: [N]):
 *   b the right-hand side; x, dx: the tail formed mu = x + dx when *has_dx, mu = x otherwise (dx is then left alone); zm_new the masked
 *   copy the tail wrote, zm_prev the one before it; partial [n_act][W][gx] the tail's workgroup shares; bt [n_act][N] the slot's control
 *   columns; lift [n_act][N] the slot's lifting and, when *has_fvec, fvec [n_act][N] the load vectors of the body-force profiles (left
 *   alone otherwise): the two operands fc_adj_control_columns adds off the Dirichlet rows, bt = -lift + fvec.  Any output may be null.
 *   FC_ERR_NOT_READY before a backward step, after its buffers were released or laid out again, and for b once a mass product
 *   (fc_adjoint_mass_product, the state gradients of a run) has overwritten it.
 * Call it straight after the backward step: b is guarded, the other buffers are not.  After a step with refinement sweeps x is the
 * handle's shared solution buffer, which any later fc_solve / fc_step / fc_solve_transposed of the handle overwrites; zm, partial and
 * the work buffer are the next backward step's as soon as one is enqueued. */
int fc_debug_get_adjoint_stage(fc_handle h, int32_t kb, int32_t gx, double* b, double* x, double* dx, int32_t* has_dx, double* zm_new,
                               double* zm_prev, double* partial, double* bt, double* lift, double* fvec, int32_t* has_fvec);

/* What the handle's last TANGENT step launched -- the last step of fc_run_tangent / fc_run_tangent_batch: FC_TAN_ROUTE_COLS int32, written
 * by the launch sites tan_enqueue_step / tanb_enqueue_step while they enqueue (a few ints in a host struct: no launch, no synchronisation,
 * no allocation, nothing on the device reads them).
 *   [0] element kernel, the code of fc_tangent_info: 1 fc_tan_elem_nl, 2 fc_tan_elem_nl_reg, 3 fc_tan_elem_nl_b<KB, false>,
 *       4 fc_tan_elem_nl_b<KB, true>   [1] its workgroups   [2] workgroups of fc_rhs_gather / fc_rhs_gather_b<KB>
 *   [3] KB, the padded width of a batched step; 0: the single march   [4] k, its columns (0: the single march)
 *   [5] ref_col, -1 when every column perturbs its own trajectory (and for the single march)
 *   [6] 1 if fc_tan_force_b<KB> ran   [7] 1 if the single gather was handed the load vectors fvec
 *   [8] 1 if the solve returned a correction dx (refinement sweeps): the tail then formed x + dx
 *   [9] workgroups of fc_tan_tail / fc_tan_tail_b<KB>
 *   [10] l1, [11] l2, [12] t2: the level gating the step's coefficients imply (cc_n != 0; cc_nn != 0; cc_nn != 0 or cm_nn != 0)
 *   [13] the order slot
 * FC_ERR_NOT_READY before the first tangent step and after fc_tangent_reserve has laid the buffers out again, FC_ERR_INVALID for a null
 * handle / buffer or n < FC_TAN_ROUTE_COLS; nothing is written then. */
#define FC_TAN_ROUTE_COLS 14
int fc_get_tangent_route(fc_handle h, int32_t n, int32_t* out);
/* Download of that step's buffers as the march holds them, in the solver's PERMUTED numbering (test aid; quiesces like the other
 * fc_debug_get_* calls).  kb: entry [3] of fc_get_tangent_route (FC_ERR_INVALID if it is not the last step's).  With W = max(1, kb) every
 * vector is [N][W] (the single march: [N]):
 *   ev [12][nc][W] the element vectors; b the right-hand side; x, dx: the tail formed the new level x + dx when *has_dx, x otherwise (dx
 *   is then left alone); lev_new the level the tail wrote, lev_other the other one (the step's d1); du [W][n_act] the step's control row
 *   as it lies on the device, padding columns included (the single march: [n_act]); dy [max(1, k)][n_sens] its sensor row (padding
 *   columns have none); flags [32] int32 the finiteness flags of the march; lift [n_act][N] the slot's lifting and, when *has_fvec, fvec
 *   [n_act][N] the load vectors of the body-force profiles (left alone otherwise).  Any output may be null.
 *   FC_ERR_NOT_READY before a tangent step and after its buffers were released or laid out again (fc_tangent_reserve, fc_set_batch, a
 *   new permutation).
 * Call it straight after the march, nothing here is guarded: x of a refined single solve is the handle's SHARED solution buffer, which
 * any later fc_solve / fc_step / fc_step_adjoint of the handle overwrites; ev, b, the work buffer behind x / dx of an unrefined or
 * batched solve, both levels, du, dy and the flags are the next tangent march's as soon as one is enqueued; lift and fvec are the slot's
 * and the handle's, replaced by fc_apply_bc / fc_set_force. */
int fc_debug_get_tangent_stage(fc_handle h, int32_t kb, double* ev, double* b, double* x, double* dx, int32_t* has_dx, double* lev_new,
                               double* lev_other, double* du, double* dy, int32_t* flags, double* lift, double* fvec, int32_t* has_fvec);

/* Columns first_col .. first_col + ncol - 1 of the tangent tape (fc_tangent_tape_reserve) as they lie on the device: out [ncol][N] in
 * the solver's PERMUTED numbering, column m - 1 = dx_m of the march the tape holds (test aid; quiesces).  FC_ERR_INVALID for columns
 * outside that march. */
int fc_debug_get_tangent_tape(fc_handle h, int32_t first_col, int32_t ncol, double* out);

/* A resident block of the optimal-perturbation driver (fc_optpert_reserve; FC_OPTPERT_U ..) as it lies on the device: out [N][kb] in
 * the solver's permuted numbering, the padding columns k .. kb - 1 included (test aid: fc_optpert_get hands out k columns).  kb: the
 * padded width (fc_optpert_info [3]), FC_ERR_INVALID otherwise. */
int fc_debug_get_optpert_block(fc_handle h, int32_t block, int32_t kb, double* out);

/* What the last apply of the slot's factor-free preconditioner launched (fc_setup_krylov; the applies inside fc_solve / fc_step and
 * fc_debug_apply_pc alike), written by the launch sites themselves while they enqueue -- the record a test compares with its host
 * model of the launch sequence, so that a kernel, a lane count or an AMG level that silently did not run fails.  A few ints in a fixed
 * host array per launch: no launch, no synchronisation, no allocation, nothing on the device.  (An Arnoldi step replayed as a captured
 * graph enqueues nothing: the record then stays that of the capture.)
 *   out[0] = n, the number of launches; then FC_PC_ROUTE_COLS int32 per launch, in launch order:
 *   [0] kernel: FC_PC_KERNEL_CSR fc_pc_csr, _DENSE fc_pc_dense, _FINAL fc_pc_final, _BSHARE fc_pc_bshare, _FINAL_SHARE
 *       fc_pc_final_share, _FILL a device fill (the two of the partitioned apply: the output vector, the Schur right-hand side)
 *   [1] rows (fill: doubles)   [2] lanes per row (fc_pc_csr without a matrix: 1; fc_pc_dense: 64; fill: 0)
 *   [3] AMG level of a V-cycle launch (the dense solve: the number of sparse levels), -1 outside the V-cycle
 * cap: int32 entries `out` holds.  FC_ERR_NOT_READY before fc_setup_krylov or the slot's first apply, FC_ERR_INVALID for a null handle /
 * buffer or cap < 1 + FC_PC_ROUTE_COLS * n; nothing is written then. */
#define FC_PC_ROUTE_COLS 4
#define FC_PC_ROUTE_MAX 48 /* launches of one apply: at most 15 velocity launches + 3 + 2 * 12 AMG levels */
#define FC_PC_KERNEL_CSR 0
#define FC_PC_KERNEL_DENSE 1
#define FC_PC_KERNEL_FINAL 2
#define FC_PC_KERNEL_BSHARE 3
#define FC_PC_KERNEL_FINAL_SHARE 4
#define FC_PC_KERNEL_FILL 5
int fc_get_pc_route(fc_handle h, int slot, int32_t* out, int cap);

/* Per-phase HIP-event timing of fc_step on the handle's stream (an instrumented replay: the marks cost ~1-2 us each and the
 * host polls less eagerly, so use it for the SPLIT of a step, not for its total).  When on, every fc_step records event marks at
 * its phase boundaries; fc_get_phase_timing returns the accumulated microseconds per phase and the number of steps since the
 * last fc_set_phase_timing.  Phases: 0 rhs (element loop + gather), 1 up-sweeps (local, to the first exchange), 2 exchange 1
 * (root right-hand side), 3 root stage, 4 exchange 2 (root solution), 5 down-sweeps, 6 tail kernels (residual rows, shift,
 * energy, sensors), 7 exchange 3 (80-double record), 8 publish.  On a single-GPU handle phases 2, 4, 7 stay zero and the whole
 * apply is reported under 1 (up to the root) and 5.  With a host exchange the exchange phases include the stream
 * synchronisation, the callback and the copies. */
int fc_set_phase_timing(fc_handle h, int on);
int fc_get_phase_timing(fc_handle h, double* us /* [9] */, int64_t* steps);

#ifdef __cplusplus
}
#endif
#endif /* FC_HIP_INTERNAL_H */
