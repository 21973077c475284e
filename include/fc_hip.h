/*
 * fc_hip.h — C ABI of libfc_hip.so: the MI355X (gfx950) implementation of FlowControl's
 * per-timestep hot path (FEM assembly of the semi-implicit Navier–Stokes forms + the linear
 * solve that advances (v, p) by one Δt).
 *
 * The reference (williamjussiau/FlowControl) has no FFI of its own: its hot path is
 * `FlowSolver.step` (src/flowcontrol/flowsolver.py:703-799) driving two third-party dolfin
 * objects, `dolfin.SystemAssembler` (:693-696, :728) and `dolfin.LUSolver("mumps")`
 * (:697, :729, :812-814).  Every entry point below names the reference interface it replaces.
 * The binding a reference maintainer would add is the ctypes stub in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch / C++ types in any signature; caller owns all host buffers, the library
 *     owns all device memory; one opaque handle per solver, one HIP stream per handle,
 *     not re-entrant per handle.
 *   - every function returns an int status: 0 = ok, <0 = error class (FC_ERR_*); nothing throws
 *     across the boundary.  fc_last_error() returns a message for the calling thread.
 *   - all floating point data is IEEE fp64 (the reference computes in fp64 throughout);
 *     all index data is int32 unless stated.
 *   - mixed-space vector layout "W": [ux(nn) | uy(nn) | p(nv)], nn = nv + ne P2 scalar nodes
 *     (vertex v → v, edge e → nv + e); N = 2 nn + nv.
 */
#ifndef FC_HIP_H
#define FC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fc_ctx* fc_handle;

enum {
  FC_OK = 0,
  FC_ERR_INVALID = -1,     /* bad argument / call order */
  FC_ERR_HIP = -2,         /* HIP runtime error (no device, OOM, launch failure) */
  FC_ERR_DIVERGED = -3,    /* non-finite velocity after the solve (flowsolver.py:731,816-819) */
  FC_ERR_NOT_CONVERGED = -4, /* Krylov / refinement did not reach the requested tolerance */
  FC_ERR_NOT_READY = -5    /* a required setup call is missing */
};

/* matrix slots: independent value arrays on the shared Taylor–Hood CSR pattern */
enum { FC_SLOT_BDF1 = 0, FC_SLOT_BDF2 = 1, FC_SLOT_MASS = 2, FC_SLOT_SCRATCH = 3, FC_NUM_SLOTS = 4 };

/* Krylov / refinement method of fc_solve / fc_step */
enum { FC_METHOD_REFINE = 0, FC_METHOD_BICGSTAB = 1, FC_METHOD_GMRES = 2 };

const char* fc_last_error(void);
int fc_device_count(int* count);

/* ── construction: replaces FlowSolver._make_mesh / _make_function_spaces
 *    (flowsolver.py:233-250) on the device side.  cells are CCW vertex triples,
 *    cell_edges[c][k] is the edge opposite local vertex k. ------------------------------------ */
int fc_create(fc_handle* out, int device, int32_t nv, int32_t ne, int32_t nc,
              const double* coords /* [nv][2] */, const int32_t* cells /* [nc][3] */,
              const int32_t* cell_edges /* [nc][3] */);
int fc_destroy(fc_handle h);

/* sizes of the mixed space and of the CSR pattern (full 15x15 element coupling minus the
 * pressure-pressure block) */
int fc_get_sizes(fc_handle h, int64_t* N, int64_t* nnz, int64_t* nn);
int fc_get_pattern(fc_handle h, int32_t* rowptr /* [N+1] */, int32_t* colidx /* [nnz] */);

/* ── bilinear-form assembly: replaces dolfin.SystemAssembler.assemble(A) (flowsolver.py:693-696),
 *    dolfin.assemble(a) in SteadyStateSolver.picard (steadystate.py:137) and the Jacobian
 *    assembly of OperatorGetter.get_A (operatorgetter.py:79-80).  Element loop on the device:
 *      mass (u,v) + adv_scale ((adv.grad)u, v) + lin_scale ((u.grad)lin, v) + nu (grad u, grad v)
 *      + pressure (p, div v) + divergence (q, div u)
 *    adv / lin are host velocity fields [2 nn] or NULL.  No boundary conditions. ------------- */
int fc_assemble_matrix(fc_handle h, int slot, double mass, double nu, const double* adv,
                       double adv_scale, const double* lin, double lin_scale, double pressure,
                       double divergence);
int fc_get_matrix_values(fc_handle h, int slot, double* vals /* [nnz] */);
int fc_set_matrix_values(fc_handle h, int slot, const double* vals /* [nnz] */);

/* y = A_slot x on the device (original numbering); parity hook + SpMV roofline probe */
int fc_spmv(fc_handle h, int slot, const double* x /* [N] */, double* y /* [N] */);

/* ── Dirichlet data: replaces the DirichletBC list handed to SystemAssembler
 *    (flowsolver.py:693; case files' _make_bcs).  Every actuator expression is linear in u_ctrl
 *    (actuator.py:190-199,241-251,269-276), so the value on BC dof i is
 *    sum_k profiles[i][k] * u_ctrl[k]. -------------------------------------------------------- */
int fc_set_bc(fc_handle h, int32_t n_bc, const int32_t* bc_dofs /* [n_bc] W indices */,
              int32_t n_act /* <= 32 for fc_step */, const double* profiles /* [n_bc][n_act] */);
/* body force of FORCE-type actuators (actuator.py:297-313): nodal P2 values per unit u_ctrl */
int fc_set_force(fc_handle h, int32_t n_act, const double* profiles /* [n_act][2 nn] or NULL */);
/* sensors as sparse rows of the functional up -> y (sensor.py:96-98,166-197; utils/mpi.py:22-37) */
int fc_set_sensors(fc_handle h, int32_t n_sens, const int32_t* rowptr /* [n_sens+1] */,
                   const int32_t* idx, const double* w);
/* time scheme constants (flowsolverparameters.py ParamTime.dt, ParamSolver.is_eq_nonlinear) */
int fc_set_time_scheme(fc_handle h, double dt, int nonlinear);

/* SystemAssembler's symmetric Dirichlet elimination on a slot: stores the lifting vectors
 * A[:, D] * profile_k for `order_slot`, then zeroes BC rows and columns and puts 1 on the
 * diagonal. */
int fc_apply_bc(fc_handle h, int slot);

/* COMPRESSED factors, the memory-lean Krylov mode (reference plug-in point flowsolver.py:812-814; north_star: "HIP
 * BiCGStab/GMRES ... preconditioning"): the selected inverse is computed in fp64 front by front as always, but its values are
 * STORED rounded to fp32 (bits = 32: 50 % of the memory) or bfloat16 (bits = 16: 25 %) — the fp64 array never exists — and
 * applied with fp64 accumulation as right preconditioner of the device GMRES / BiCGStab (cylinder operator: 2 / ~9 GMRES
 * iterations to 1e-12).  Call before fc_setup_solver; a change lays the slots out anew.  fc_setup_solver then accepts the
 * factors through a GMRES probe (<= 40 iterations); fc_solve / fc_step need FC_METHOD_GMRES or FC_METHOD_BICGSTAB. */
int fc_set_factor_precision(fc_handle h, int bits /* 64 (default, exact), 32, 16 */);
int fc_get_factor_storage(fc_handle h, int slot, int32_t* bits, int64_t* bytes /* bytes of factor values held for the slot */);
/* THE solver setup in one call (what LUSolver.set_operator + the first solve cost the reference, flowsolver.py:697,729):
 * symbolic analysis inside the library from the mesh the handle holds (element-based nested-dissection tree of
 * `depth` bisections — 0: leaves of ~12 cells — fused `merge` at a time; on a handle with a communicator / host exchange
 * the root is nranks-ary and this rank lays out its own sub-tree and the root), permutation, segment tables, workgroup
 * tiles, factorisation plan, task dependencies, then the numeric factorisation of the slot's current matrix on the
 * device and the acceptance solve of fc_accept_factors (below).  truncate = d > 0: only the tree levels >= d
 * are factorised (memory-lean preconditioner; use FC_METHOD_GMRES / FC_METHOD_BICGSTAB afterwards).  A later call for the
 * same slot redoes only the numeric phase.  Needs: fc_set_bc, fc_assemble_matrix(slot), fc_apply_bc(slot).  (The
 * array-level entry points a caller with an analysis of its own would use -- fc_set_permutation, fc_solver_setup,
 * fc_factor_plan ... -- are declared in fc_hip_internal.h with the bench / debug hooks; the boundary is this file.) */
int fc_setup_solver(fc_handle h, int slot, int32_t depth, int32_t merge, int32_t truncate, int32_t refine, int32_t check_residual);
int fc_get_permutation(fc_handle h, int32_t* perm /* [N] new -> old */);
/* info[10]: factor values stored on this rank, of the whole tree, swept by this rank per solve; stages; tree depth;
 * exchanged rows, the two exchange stages; cells assembled by this rank; truncate */
int fc_get_solver_info(fc_handle h, int slot, int64_t* info /* [10] */);
/* enclosed flows (velocity prescribed on the whole boundary: pressure defined up to a constant): a positive shift on the
 * diagonal of ONE pressure dof inside the factorisation of fc_setup_solver (dof = -1: none); cf. fc_set_front_shifts */
int fc_set_pressure_pin(fc_handle h, int32_t dof, double shift);
/* device milliseconds of the slot's last numeric factorisation (fc_refactor, also inside fc_setup_solver) */
int fc_get_refactor_ms(fc_handle h, int slot, double* ms);
/* block-step width every level of the elimination plan took in the handle's last numeric factorisation, deepest level first: 32, 64 or
 * 128 pivot columns per step (csrc/fc_front.hip.h), 0 for a level without fronts.  n: entries of out, at least the plan's levels (tree
 * depth + 1; the first of them are written).  Read-only: which kernels ran -- FC_FE_WIDE_NF / FC_FE_HUGE_NF / FC_FE_HUGE_MB and a refused
 * LDS size all show here.  FC_ERR_NOT_READY before the first fc_refactor. */
int fc_get_refactor_steps(fc_handle h, int32_t n, int32_t* out);
int fc_get_local_cells(fc_handle h, int32_t* cells /* [info[8] of fc_get_solver_info] */);
/* out[4]: cells of this rank (right-hand side, energy), cells whose element matrices fc_assemble_matrix computes on this handle (its own
 * and the other ranks' cells that touch a root dof: the rows a rank owns and the root's rows are complete, the other ranks' rows are
 * never read), lead rank (0 / 1), ranks.  A single-GPU handle: all cells, all cells, 1, 1. */
int fc_get_partition_info(fc_handle h, int32_t* out);
/* (On a partitioned handle fc_get_matrix_values returns this rank's view -- complete rows for the dofs it owns and the root's, partial
 * rows elsewhere -- and fc_spmv is a collective: every rank calls it with the same x and receives the whole product.) */
int fc_get_rowkind(fc_handle h, uint8_t* rowkind /* [N]: 0 other rank, 1 owned, 2 root (all 1 on a single-GPU handle) */);
/* Numeric factorisation ON THE DEVICE of the slot's current matrix values (after fc_assemble_matrix + fc_apply_bc) with the
 * structure of the first fc_setup_solver: what `solver.set_operator(A)` costs in the reference (flowsolver.py:697,812-814 ->
 * PETSc/MUMPS numeric phase; every Newton / Picard iteration of steadystate.py:60-159).  Multifrontal, all fronts of a tree
 * level together, blocked Gauss-Jordan steps with threshold partial pivoting, trailing updates on the fp64 matrix cores
 * (csrc/fc_front.hip.h); no vendor BLAS / LAPACK.  ms_out (optional): device time.  On a partitioned handle every rank
 * factorises its own sub-tree; the root front is summed over the ranks once (exchange). */
int fc_refactor(fc_handle h, int slot, double* ms_out);
/* Acceptance solve of a slot's freshly computed factors (fc_setup_solver runs it itself; call it after a bare fc_refactor): a fixed
 * right-hand side, residual against the matrix.  < 1e-10 by the direct apply: exact factors (time-step operators give <= 1e-12).
 * Between 1e-10 and 1e-2 (pivoting confined to the pivot blocks lost digits on an ill-conditioned operator, e.g. a steady Oseen
 * operator far beyond the Reynolds number the mesh resolves, where sparse LU with partial pivoting still reaches 1e-12): the factors
 * are kept as a PRECONDITIONER if GMRES reaches 1e-8 -- or, on a single-device handle, a normwise backward error
 * |r| / (|A|_F |x| + |b|) < 1e-13 -- within 40 iterations; fc_solve / fc_step on this slot then run GMRES(60, 1e-12, restarted on
 * the true residual until it stagnates) by themselves whenever FC_METHOD_REFINE is selected (*inexact_out = 1; the batched calls
 * refuse such a slot).  Anything else is FC_ERR_HIP.  residual_out: the direct apply's relative residual.  A collective on a
 * partitioned handle.  fc_refactor clears the flag. */
int fc_accept_factors(fc_handle h, int slot, double* residual_out, int32_t* inexact_out);
int fc_get_factors_inexact(fc_handle h, int slot, int32_t* inexact /* 1: the slot's factors serve as GMRES preconditioner */);
/* optional explicit operator C of the right-hand side, b -= C u_n (rows in the solver's permuted
 * numbering, columns = velocity dofs in W numbering): the explicit half of the linear terms of the
 * Crank-Nicolson form (NSForms._cn, nsforms.py:191-236).  rowptr == NULL removes it. */
int fc_set_rhs_operator(fc_handle h, int slot, const int32_t* rowptr, const int32_t* col, const double* val);
/* the slot's matrix changed (fc_assemble_matrix + fc_apply_bc) but its factors are kept as they are: only the
 * permuted copy that SpMV / residuals use is refreshed.  With FC_METHOD_BICGSTAB the old factors then act as
 * preconditioner of the new operator (Picard / Newton iterations of steadystate.py:60-159 between two
 * refactorisations; the reference re-factorises with MUMPS at every iteration). */
int fc_update_operator(fc_handle h, int slot);
/* method: FC_METHOD_*; max_iter: refinement sweeps (REFINE) or the Krylov iteration cap; rtol: Krylov target;
 * check_residual: 0 = no residual monitor, n >= 1 = fc_step / fc_run form |b - A x| / |b| on every n-th step of the handle (info[1];
 * NaN on the steps in between) -- the reference never forms it (flowsolver.py:728-737 tests finiteness only), n > 1 amortises the
 * pass over the system matrix it costs; -1 = auto: every step while the slot's factors stay in the 256 MiB Infinity Cache (the pass
 * hides beside the next step), every 8th step where they stream from HBM (there it costs ~10 % of a step).  The non-finite test
 * runs on every step regardless. */
int fc_set_solver_options(fc_handle h, int method, int max_iter, double rtol, int check_residual);

/* FACTORISATION-FREE Krylov mode (reference plug-in point FlowSolver._make_solver, flowsolver.py:812-814: "any object with
 * set_operator / solve"; BASELINE.json north_star: "HIP BiCGStab/GMRES with CSR SpMV and block-Jacobi/ILU(0) preconditioning").
 * Instead of fc_setup_solver: NOTHING is factorised.  The slot's solves and time steps run the device GMRES / BiCGStab on the
 * permuted system matrix, right-preconditioned by a SIMPLE-type block preconditioner built from the assembled values alone:
 *     u  = `sweeps` damped-Jacobi sweeps on the velocity block F         (the time-step operators are mass dominated)
 *     zp = one smoothed-aggregation AMG V(1,1)-cycle on S zp = B u - r_p,  S = B diag(F)^-1 Bt  (pressure Schur complement)
 *     zu = u - diag(F)^-1 Bt zp
 * Memory is O(nnz) (matrix blocks + an AMG hierarchy of ~1.3 nnz(S)), nothing grows like the fill of a factorisation.
 * Cylinder O1 BDF2 operator, sweeps = 3: ~20 GMRES iterations to 1e-10 from a zero guess, fewer inside time steps (which start
 * from the previous solution).  method: FC_METHOD_GMRES or FC_METHOD_BICGSTAB; max_iter / rtol / check_residual as in
 * fc_set_solver_options.  Needs fc_set_bc, fc_assemble_matrix(slot), fc_apply_bc(slot); after the slot's matrix changed call
 * it again (fc_update_operator alone keeps the old preconditioner for the new operator).  fc_setup_solver on the same slot later
 * replaces the mode.  Batched stepping needs factors.
 * Partitioned handles (fc_comm_init / fc_set_host_exchange; a COLLECTIVE, every rank calls it): the rows are split by the tree
 * fc_setup_solver builds (a world-ary root, the default shape), each rank computes its own rows and the root's, and every
 * preconditioner apply takes ONE exchange of (root velocity rows + pressure dofs) doubles; the pressure hierarchy is built from the
 * matrix gathered once at setup and replicated on every rank.  sweeps <= 2 there.  A slot set up for one permutation is dropped
 * when fc_set_permutation installs another one. */
int fc_setup_krylov(fc_handle h, int slot, int32_t sweeps, int method, int32_t max_iter, double rtol, int32_t check_residual);
/* info[8]: device bytes held for the slot's Krylov mode (permuted matrix + blocks + AMG hierarchy), velocity dofs, pressure dofs, AMG
 * levels (the dense coarsest one included), rows of the coarsest level, kernel launches per preconditioner apply, Jacobi sweeps, host
 * milliseconds of the setup; omega_out (optional): the Jacobi damping chosen from the spectral radius of diag(F)^-1 F */
int fc_get_krylov_info(fc_handle h, int slot, int64_t* info /* [8] */, double* omega_out);
/* info[8] of a factor-free slot on this rank: velocity rows it computes, pressure rows it holds, rows of the root block, exchanges
 * per preconditioner apply (0 on a single GPU, 1 on a partitioned handle), doubles exchanged per apply, device bytes of the
 * velocity-side matrices it holds (K_F, B, Bt; on a partitioned handle its share), device bytes of the pressure AMG hierarchy
 * (replicated on every rank), exchanges of the last time step's Krylov solve (its right-hand side's root sum included) */
int fc_get_krylov_partition_info(fc_handle h, int slot, int64_t* info /* [8] */);

/* ── state: FlowFieldCollection u_n, u_nn, p_n (flowfield.py:67-105; flowsolver.py:487-491) ─ */
int fc_set_state(fc_handle h, const double* u_n /* [2 nn] */, const double* u_nn /* [2 nn] */,
                 const double* p_n /* [nv] */);
/* Withdraw the last fc_step: (u_n, u_nn, p_n) as they were before it (the step's tail keeps what its shift overwrites).
 * The reference leaves its state untouched when a step fails (a non-finite velocity is detected BEFORE the fields are
 * shifted, flowsolver.py:727-751); a host program gets the same by calling this after FC_ERR_DIVERGED -- FlowSolver.step does.
 * Valid once after a single fc_step / fc_step_end (not after fc_run, fc_set_state or a batched step). */
int fc_undo_step(fc_handle h);
int fc_get_state(fc_handle h, double* u_n, double* u_nn, double* p_n);
int fc_get_solution(fc_handle h, double* up /* [N] last solve, W layout */);

/* ── THE per-step crossing: replaces assemblers[order].assemble(rhs); solvers[order].solve(...);
 *    split; _solver_diverged; field shift; make_measurement; compute_perturbation_energy
 *    (flowsolver.py:724-779).  order_slot is FC_SLOT_BDF1 or FC_SLOT_BDF2.
 *    y_out[n_sens], dE_out (1/2 |u|^2_L2, NaN if compute_energy == 0), info_out[4] =
 *    {iterations, relative residual of the first refinement residual, |b|, flags}. ------------- */
int fc_step(fc_handle h, int order_slot, const double* u_ctrl /* [n_act] */,
            const double* u_force /* [n_act] body-force amplitudes, NULL = u_ctrl (CN passes the
                                     mean of the new and the previous control, nsforms.py:224-226) */,
            double* y_out, double* dE_out, int compute_energy, double* info_out);
/* the same step in two halves: fc_step_begin writes the controls and enqueues the launches (the GPU works from here),
 * fc_step_end waits for the record -- the caller's own per-step bookkeeping fits in between (flowsolver.py:775-799: the
 * reference's exporter.log / progress / checkpoint work of the previous step).  fc_step = begin + end. */
int fc_step_begin(fc_handle h, int order_slot, const double* u_ctrl, const double* u_force, int compute_energy);
int fc_step_end(fc_handle h, double* y_out, double* dE_out, double* info_out);
/* What the controller of a closed loop waits for is y: on a single-GPU handle with the direct factor apply the step publishes the sensors
 * and the non-finite flag right behind the last sweep launch and computes residual monitor and energy on a second stream, overlapped with
 * the host's work and the next step's sweeps.  fc_step_end with dE_out == NULL and info_out == NULL returns as soon as y (and the flag:
 * FC_ERR_DIVERGED) is there; fc_step_collect hands over (dE, info) of that step later -- it blocks until they exist; the next
 * fc_step_begin keeps them if nobody asked.  With non-NULL dE_out / info_out fc_step_end (and fc_step) wait for everything, as before.
 * The reference's loop wants exactly this order: y_meas back to the controller at once, dE into the log (flowsolver.py:760-799). */
int fc_step_collect(fc_handle h, double* dE_out, double* info_out);
/* n_steps open-loop steps without host synchronisation in between (u_ctrl constant or a
 * sequence [n_steps][n_act]); y_seq [n_steps][n_sens], dE_seq [n_steps] (may be NULL). */
int fc_run(fc_handle h, int first_order_slot, int32_t n_steps, const double* u_ctrl,
           int u_ctrl_is_sequence, double* y_seq, double* dE_seq, int compute_energy);

/* ── closed loops on the device: a bank of discrete LTI controllers advanced by a kernel between two steps (csrc/fc_ctrl.hip.h), so that
 *    a closed loop is as enqueueable as an open one.  Replaces the per-step host work of the reference's closed loops
 *    (Controller.step, controller.py:136-159, between two FlowSolver.step calls: examples/cylinder/run_cylinder_example.py; one such
 *    loop per candidate in utils/optim.py).  For each of k simulations (k = 1: the single-simulation state; k = the batch of fc_set_batch):
 *        yc = G y_meas + g0 ;  uc = C x + D yc (state BEFORE the update) ;  x <- Ad x + Bd yc ;  u = S uc
 *    y_meas is the measurement of the previous step.  Host arrays are simulation-major, every matrix row-major:
 *    Ad [k][nx][nx], Bd [k][nx][nyc], C [k][nuc][nx], D [k][nuc][nyc], x0 [k][nx] (NULL: zero), G [k][nyc][n_sens], g0 [k][nyc] (NULL: zero),
 *    S [k][n_act][nuc]; a smaller controller is zero-padded to nx.  nx <= 256 (nx = 0: static gain, Ad / Bd / C / x0 may be NULL),
 *    1 <= nyc <= 8, 1 <= nuc <= 32; n_sens (1 .. 64) and n_act (1 .. 32) are the handle's; k <= max(1, batch size).  k = 0 frees the bank.
 *    With no bank set every other entry point enqueues exactly what it enqueued before. */
int fc_set_controllers(fc_handle h, int32_t k, int32_t nx, int32_t nyc, int32_t nuc, const double* Ad, const double* Bd, const double* C,
                       const double* D, const double* x0, const double* G, const double* g0, const double* S);
int fc_get_controller_state(fc_handle h, int32_t k, double* x_out /* [k][nx] */);
/* (a new state starts a new run: simulations that a batched closed-loop run had ended are live again) */
int fc_set_controller_state(fc_handle h, int32_t k, const double* x /* [k][nx] */);
/* advance the bank once from host-given measurements: what a host loop that keeps its own stepping calls, and the kernel's parity hook */
int fc_ctrl_apply(fc_handle h, int32_t k, const double* y /* [k][n_sens] */, double* u_out /* [k][n_act] */);
/* Signals added to the loop from outside and limits on the actuators; step by step the bank then forms
 *        yc = G y_meas + g0 + w_y[row] ;  uc = C x + D yc ;  x <- Ad x + Bd yc ;  v = S uc + w_u[row] ;  u = min(max(v, u_lo), u_hi)
 *    (a plain clamp: the controller state is not corrected; u, and with it u_seq, is the clamped value the plant saw; an ended simulation
 *    keeps u = 0).  w_y: reference or sensor noise at the controller input; w_u: excitation or disturbance at the plant input.  The arrays are
 *    copied to the device before the call returns.  A cursor on the handle starts at row 0 with every fc_set_loop_signals; step s of an
 *    fc_run_closed_loop, fc_run_closed_loop_batch or fc_ctrl_apply call reads row cursor + s, and the call advances the cursor by its steps:
 *    a run cut into several calls reads on where the previous call stopped.  FC_ERR_INVALID, with nothing enqueued: k is not the bank's, a call
 *    would read past n_rows, u_lo > u_hi, a NaN limit, a step in flight.  +-infinity = no limit on that side.  fc_set_controllers (a new
 *    bank, or k = 0) drops signals and limits.  With none set every entry point enqueues exactly what it enqueued before. */
int fc_set_loop_signals(fc_handle h, int32_t k, int32_t n_rows, const double* w_y /* [n_rows][k][nyc] or NULL */,
                        const double* w_u /* [n_rows][k][n_act] or NULL */); /* n_rows = 0 (or both NULL) frees */
int fc_set_control_limits(fc_handle h, int32_t k, const double* u_lo /* [k][n_act] */, const double* u_hi); /* both NULL: no limits */
int fc_get_loop_cursor(fc_handle h, int64_t* row);
/* The closed-loop counterpart of fc_run: per step fc_ctrl_step, then the launches of fc_run's step, which reads u from device memory;
 * one synchronisation at the end.  y0 [n_sens]: the measurement the first controller step sees (of the step before the run, or of the
 * initial condition).  y_seq [n_steps][n_sens], u_seq [n_steps][n_act] (the control each step actually used), dE_seq [n_steps]; any may
 * be NULL.  From the step after a non-finite velocity on, u = 0 and the controller state is frozen; FC_ERR_DIVERGED then.  The residual
 * monitor keeps the handle's cadence (fc_set_solver_options); what it saw is read with fc_get_run_monitor.
 * FC_ERR_INVALID on partitioned handles and Crank-Nicolson slots (fc_set_rhs_operator: their forcing averages two controls). */
int fc_run_closed_loop(fc_handle h, int first_order_slot, int32_t n_steps, const double* y0, double* y_seq, double* u_seq, double* dE_seq,
                       int compute_energy);
/* ... on the batched state (accepted wherever fc_step_batch is): y0 [k][n_sens]; y_seq [n_steps][k][n_sens], u_seq [n_steps][k][n_act],
 * dE_seq [n_steps][k]; first_bad_step [k]: first step (0-based) whose velocity was non-finite, -1 = finite to the end; info [k][4] of the
 * last step as fc_step_batch gives it.  The columns are independent: the other simulations run to the end; FC_ERR_DIVERGED when any
 * first_bad_step >= 0.  The bank remembers the simulations that ended (u = 0 in later calls) until fc_set_controller_state. */
int fc_run_closed_loop_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, const double* y0, double* y_seq, double* u_seq,
                             double* dE_seq, int compute_energy, int32_t* first_bad_step, double* info);
/* the residual monitor's findings over the last closed-loop run (steps up to a simulation's first non-finite one): largest relative
 * residual |b - A x| / |b| (0 if the monitor never ran), the step it was seen at (-1), the run's first non-finite step (-1: none) */
int fc_get_run_monitor(fc_handle h, double* max_residual, int32_t* residual_step, int32_t* first_bad_step);

/* ── base-flow (steady-state) iterations: replace SteadyStateSolver.picard / .newton (steadystate.py:60-159:
 *    dolfin.solve(F == 0, ...) :95 and the assemble / bc.apply / LUSolver.solve loop :137-145).  A host program drives the
 *    loop and its stopping rule (picard: relative change < tol, steadystate.py:150-156; newton: dolfin's residual criterion
 *    rel 1e-9 / abs 1e-10); every iteration's assembly, Dirichlet elimination, factorisation and solve run on the device.
 *    fc_set_baseflow_bc: the FULL-field Dirichlet data (FlowSolver._make_BCs, flowsolver.py:329-337) — it replaces the
 *    fc_set_bc tables (call fc_set_bc again before time stepping).  up: mixed vector [N], W layout, in = iterate, out = next
 *    iterate; load: (f, v) of a body force or NULL; nu = 1 / Re.  Enclosed flows: fc_set_pressure_pin first.
 *    fc_newton_step returns |F(up_in)| over the free rows in res_norm; update = 0 evaluates the residual only. */
int fc_set_baseflow_bc(fc_handle h, int32_t n_bc, const int32_t* bc_dofs, const double* bc_values);
int fc_picard_step(fc_handle h, double nu, double* up, const double* load, double* rel_change);
int fc_newton_step(fc_handle h, double nu, double* up, const double* load, double* res_norm, int update);

/* ── shared-operator batched stepping: k <= 32 lock-step simulations on ONE handle ────────────
 *    Replaces k independent FlowSolver instances that step the SAME operator with different initial
 *    conditions / controls / controllers — the reference's outer workloads: IC sweeps
 *    (examples/lidcavity/batch_run_lidcavity.py:197-215), controller optimisation (utils/optim.py:95-102),
 *    each of which runs FlowSolver.step (flowsolver.py:703-799) once per simulation and time step.
 *    All k simulations share the handle's operators, factors, BC / force / sensor tables and time scheme and are
 *    advanced together: every vector is a matrix [row][KB] on the device (KB = 4, 8, 16 or 32 >= k), every level
 *    of the factor sweep a dense block product on the fp64 matrix cores, so the factors are read once per
 *    step for all of them.  Needs fc_setup_solver (full factors, single GPU, no refinement sweeps).
 *    fc_set_batch(h, k) allocates the batched state (all zero; k = 0 frees it).  Host arrays are [k][...]
 *    (simulation-major).  The single-simulation state of the handle is independent of the batched one. */
/*    (fc_set_solver_options' check_residual = n applies to the batched steps too: the residual monitor runs on every n-th batched step of
 *    the handle, info_out[s][1], [2] are NaN in between; the non-finite test runs on every step.) */
int fc_set_batch(fc_handle h, int32_t k);
int fc_set_state_batch(fc_handle h, int32_t k, const double* u_n /* [k][2 nn] */, const double* u_nn /* [k][2 nn] */,
                       const double* p_n /* [k][nv] or NULL */);
int fc_get_state_batch(fc_handle h, int32_t k, double* u_n, double* u_nn, double* p_n /* any may be NULL */);
int fc_get_solution_batch(fc_handle h, int32_t k, double* up /* [k][N] last solve, W layout */);
/* fc_step for k simulations: u_ctrl [k][n_act], u_force [k][n_act] or NULL (= u_ctrl), y_out [k][n_sens], dE_out [k],
 * info_out [k][4] = {0, relative residual, |b|, flags}.  FC_ERR_DIVERGED when any simulation produced a non-finite
 * velocity (info_out[s][3] marks which; the others are unaffected: the columns are independent). */
int fc_step_batch(fc_handle h, int order_slot, int32_t k, const double* u_ctrl, const double* u_force, double* y_out,
                  double* dE_out, int compute_energy, double* info_out);
/* (the flags are per step: after FC_ERR_DIVERGED the other simulations simply go on; fc_reset_sim_batch(h, s) takes a diverged
 * run out of the dynamics -- its state becomes zero, so that its column stops producing non-finite values -- the host then ignores
 * its outputs.  The reference's per-run equivalent: FlowSolver.step returns None / raises and that run ends, flowsolver.py:727-737.) */
int fc_reset_sim_batch(fc_handle h, int32_t s);
int fc_step_batch_begin(fc_handle h, int order_slot, int32_t k, const double* u_ctrl, const double* u_force, int compute_energy);
int fc_step_batch_end(fc_handle h, int32_t k, double* y_out, double* dE_out, double* info_out);
/* fc_step_end(early) / fc_step_collect for k simulations (cache-resident factors: residual monitor and energy of a batched step run on a
 * second stream while the host and the next step go on): the early end hands over y [k][n_sens] and flags [k] (1: that simulation's
 * velocity became non-finite; FC_ERR_DIVERGED if any) as soon as the solve is done; fc_step_batch_collect returns (dE [k], info [k][4]) of
 * that step and blocks until they exist.  fc_step_batch_end with dE_out / info_out, and fc_step_batch, wait for everything as before. */
int fc_step_batch_end_early(fc_handle h, int32_t k, double* y_out, int32_t* flags_out);
int fc_step_batch_collect(fc_handle h, int32_t k, double* dE_out, double* info_out);
/* parity hook: X = A_bc^{-1} B for k right-hand sides through the batched factor apply; b, x: [k][N] */
int fc_solve_batch(fc_handle h, int slot, int32_t k, const double* b, double* x);
/* what the batched factor apply (fc_step_batch, fc_solve_batch, the closed loops) launches for `slot` with the handle's current tables and
 * batch width, in launch order: FC_BATCH_LAUNCH_COLS int32 per launch (their number: block + fold launches of the internal fc_get_batch_info),
 *   block launch {0, tasks, column-group waves per task (cg) at this batch width, fewest and most 32-column chunks of a task,
 *                 1 if a task is a part of a split tile, most parts of a tile (1: none is split), 1 if the slot's factors are streamed
 *                 with nontemporal loads}
 *   fold launch  {1, destination rows, 0, fewest and most source rows of a destination row, 0, 0, 0}
 * n: entries of out.  Read-only: which branches of the block and fold kernels ran -- FC_BATCH_CG / FC_BATCH_CPW / FC_BATCH_SPLIT /
 * FC_NT_BYTES all show here.  FC_ERR_NOT_READY without a batch (fc_set_batch), FC_ERR_INVALID for a null handle or a short buffer;
 * nothing is written on an error. */
#define FC_BATCH_LAUNCH_COLS 8
int fc_get_batch_launches(fc_handle h, int slot, int32_t n, int32_t* out);
/* what one whole single-vector factor apply of `slot` (fc_solve, the time step, fc_bench_sweeps) launches, in launch order: the record the
 * launchers themselves switch on, FC_SWEEP_LAUNCH_COLS int32 per launch --
 *   {kernel (0 fc_nd_sweep, 1 fc_nd_down_block, 2 fc_nd_flat_block, 3 fc_nd_fold1, 4 fc_diag_stage), direction (0 up, 1 down),
 *    first parameter (LANES / LPR / loads per thread / 0), second parameter (SUB / RPS / 0), workgroups, 1 if the values are read with
 *    nontemporal loads, storage bits of the values (64, 32, 16), rows written}
 * The column-form up-sweep is reported where the apply takes it (its tables are built by this call if no apply has tried yet).
 * n: entries of out.  n = 0 (out may be null): returns the NUMBER of launches (>= 0) and writes nothing -- the count to size out with.
 * Read-only otherwise: FC_SWEEP_GEOM, FC_BLOCK_*, FC_FLAT_*, FC_UP_FORM, FC_UPC_*, FC_NT_BYTES, FC_RESIDENT_BYTES and the factor precision
 * all show here.  FC_ERR_NOT_READY for a slot without factors, FC_ERR_INVALID for a null handle, a bad slot or a short buffer; nothing is
 * written on an error. */
#define FC_SWEEP_LAUNCH_COLS 8
int fc_get_sweep_launches(fc_handle h, int slot, int32_t n, int32_t* out);

/* ── parity hooks (tests) ------------------------------------------------------------------- */
/* RHS of `order_slot` for the current state and u_ctrl, in W layout, BCs lifted and imposed:
 * what SystemAssembler.assemble(rhs) returns (flowsolver.py:728) */
int fc_assemble_rhs(fc_handle h, int order_slot, const double* u_ctrl, double* b_out /* [N] */);
/* x = A_bc^{-1} b with the device solver of `slot` */
int fc_solve(fc_handle h, int slot, const double* b /* [N] */, double* x /* [N] */,
             double* info_out /* [4] */);
/* 1/2 u^T M u for a host velocity field (flowsolver.py:827-829); needs FC_SLOT_MASS assembled */
int fc_energy(fc_handle h, const double* u /* [2 nn] */, double* E);
int fc_measure(fc_handle h, const double* up /* [N] */, double* y /* [n_sens] */);

/* ── complex-shifted direct solver: replaces the reference's linear analysis (utils/linalg.py: the block splu of get_frequency_response_*
 *    and get_field_response, SLEPc's shift-invert in get_mat_vp_slepc).  M = sigma E - A for complex sigma, factorised on the device in
 *    its real-equivalent form (every complex dof a (re, im) pair, every entry a real 2x2 block) by the multifrontal kernels of the
 *    real solver, in a structure of its OWN inside the handle: own tree, permutation, plan, fronts, factor values and work vectors.
 *    The handle's slots, factors, permutation and time-stepping state are neither read nor written (a time step after a shifted solve
 *    is bit-identical to one without).  Single-GPU handles without a pressure pin only (FC_ERR_INVALID otherwise: on an enclosed flow
 *    sigma E - A is singular for every sigma).
 *    fc_setup_shifted: a_vals / e_vals [nnz] are A and E on the handle's CSR pattern (fc_get_pattern), copied into buffers of the
 *    solver; general matrices (no boundary-condition elimination, no skipped dofs).  The first call runs the symbolic phase, every
 *    call the numeric one; NULL value pointers keep the held values (a new sigma only).  refine: iterative-refinement steps of
 *    every solve, against M.
 *    fc_solve_shifted: x = M^-1 b for nrhs columns ([nrhs][N] each; b_im NULL = real right-hand sides; x_re / x_im NULL = keep the
 *    solutions on the device only, for fc_shifted_project).  info[nrhs] (optional): relative residual |b - M x| / |b| per column;
 *    FC_ERR_NOT_CONVERGED when one is above 1e-8.
 *    fc_shifted_project: y[r][c] = sum_k w[k] x_c[idx[k]] over the sparse rows (rowptr[nrow + 1], idx, w) of C, for the first nrhs
 *    solutions of the last fc_solve_shifted (y_re, y_im [nrow][nrhs]): only C X crosses to the host.
 *    fc_shifted_spmv: y = (s E - t A) x, s complex, t real; x, y [N] complex interleaved (re, im per dof).
 *    fc_shifted_info: info[4] = factor bytes, device bytes held, order of the real-equivalent system, columns of the last solve;
 *    dinfo[4] = device milliseconds and trailing-update flops of the last numeric factorisation, sigma (re, im); last_res (optional,
 *    [info[3]]): the residuals of the last solve.  All zero after fc_release_shifted.  fc_destroy frees the solver too. ---------- */
int fc_setup_shifted(fc_handle h, const double* a_vals, const double* e_vals, double sigma_re, double sigma_im, int32_t refine);
int fc_solve_shifted(fc_handle h, int32_t nrhs, const double* b_re, const double* b_im, double* x_re, double* x_im, double* info);
int fc_shifted_project(fc_handle h, int32_t nrhs, int32_t nrow, const int32_t* rowptr, const int32_t* idx, const double* w, double* y_re,
                       double* y_im);
int fc_shifted_spmv(fc_handle h, double s_re, double s_im, double t, const double* x, double* y);
int fc_shifted_info(fc_handle h, int64_t* info /* [4] */, double* dinfo /* [4] */, double* last_res);
int fc_release_shifted(fc_handle h);
/* Arnoldi on Op = (A - sigma E)^-1 E with the shifted factors (shift-invert eigenvalues: theta of Op <-> lambda = sigma + 1 / theta).
 * The basis V (m + 1 complex vectors of N) stays on the device; the host drives the restarts (flowcontrol_amd/linalg.py: Krylov-Schur).
 *    fc_shifted_arnoldi_start: V_0 = Op v0 / |Op v0| (v0 [N] complex interleaved).
 *    fc_shifted_arnoldi_step: V_{j+1} beta = Op V_j - V_{0..j} hcol (classical Gram-Schmidt with one re-orthogonalisation);
 *    hcol [j + 1] complex interleaved.  FC_ERR_NOT_CONVERGED if the inner solve misses 1e-8.
 *    fc_shifted_arnoldi_restart: V_{0..k} = V_{0..m} Q (Q [m][k] complex, row-major), then V_k = V_m.
 *    fc_shifted_ritz: X = V_{0..m} Y (Y [m][k]); res[k][3] = |A x - lam E x|, |A x|, |E x| per column (lam [k] complex) through
 *    the shifted SpMV; X [k][N] complex interleaved (optional). */
int fc_shifted_arnoldi_start(fc_handle h, int32_t m, const double* v0);
int fc_shifted_arnoldi_step(fc_handle h, int32_t j, double* hcol, double* beta);
int fc_shifted_arnoldi_restart(fc_handle h, int32_t m, int32_t k, const double* Q);
int fc_shifted_ritz(fc_handle h, int32_t m, int32_t k, const double* Y, const double* lam, double* res, double* X);
/* Opt-in extensions of the shifted solver; with none of them called everything above behaves as described there.
 *    fc_shifted_set_pin: enclosed flows.  Registers the pressure dof `dof` (W numbering; -1 clears) whose diagonal gets `shift`
 *    inside the shifted factorisation: M' = sigma E - A + shift e_k e_k^T (det M' = shift adj(M)_kk: the finite eigenvalues do not
 *    depend on the shift; for a right-hand side compatible with the constant-pressure null space the solution is M's with p_k = 0).
 *    Call before fc_setup_shifted, which then accepts the handle with or without fc_set_pressure_pin.  Residuals, refinement and
 *    fc_shifted_spmv (where t != 0: A' = A - shift e_k e_k^T) are those of M'.  The handle's own pin and factors are not touched.
 *    fc_shifted_set_krylov: right-preconditioned complex GMRES(restart) on the device, preconditioned by the held factors.
 *    max_iter = 0 (the default) is off.  When on, a solve whose refinement steps leave the relative residual above 1e-8 continues
 *    with GMRES from that iterate and fails with FC_ERR_NOT_CONVERGED only if rtol is missed within max_iter iterations.
 *    fc_shifted_set_shift: a new sigma for the operator WITHOUT refactorising (needs Krylov on, FC_ERR_INVALID otherwise): later
 *    fc_solve_shifted / fc_shifted_project / Arnoldi calls solve at the new sigma by GMRES on the lagged factors, from a zero start
 *    iterate.  fc_setup_shifted sets both shifts to its sigma again.
 *    fc_shifted_krylov_info: iters [columns of the last fc_solve_shifted] GMRES iterations per column (0: none was needed);
 *    counters[5] = numeric factorisations, factor applies, mat-vecs, solves that ran GMRES (fc_solve_shifted columns and Arnoldi
 *    steps alike) and, of those, rescues (solves at the factored sigma whose refinement missed 1e-8), all since the solver's
 *    structure was created (fc_release_shifted ends it).  Either pointer may be NULL.
 *    fc_shifted_set_pin with a new dof must come before the first fc_setup_shifted (the slots are looked up in its symbolic phase;
 *    fc_release_shifted starts over); the shift of the registered dof may change, and -1 clears, at any time. */
int fc_shifted_set_pin(fc_handle h, int32_t dof, double shift);
int fc_shifted_set_krylov(fc_handle h, int32_t max_iter, int32_t restart, double rtol);
int fc_shifted_set_shift(fc_handle h, double sigma_re, double sigma_im);
int fc_shifted_krylov_info(fc_handle h, int32_t* iters, int64_t* counters /* [5] */);
/* Block solves: k <= 32 columns, each at a shift of its own, on the factors the solver holds -- the frequencies of a sweep between two
 * factorisations.  The factors are read ONCE per GMRES iteration for all columns (the batched factor apply of fc_set_batch on the shifted
 * solver's own structure); every column runs the GMRES of fc_shifted_set_krylov (which must be on: its max_iter, restart, rtol) from a
 * zero start iterate, in lock step with the others, and stops on its own true residual.
 *    fc_shifted_set_block: builds (k > 0) or frees (k = 0) the block of width k: a tiled copy of the factor values (at least the factor
 *    size, redone by every fc_setup_shifted) and the block vectors; fc_shifted_info counts them.  After the first fc_setup_shifted.
 *    fc_solve_shifted_block: column c solves (sigma_c E - A) x_c = b_c (b_re, b_im, x_re, x_im [k][N]; b_im NULL = real right-hand sides;
 *    x_re / x_im NULL = keep the solutions on the device for fc_shifted_project).  info[k] (optional): relative true residual per column;
 *    iterations per column through fc_shifted_krylov_info.  FC_ERR_NOT_CONVERGED when a column misses rtol, with every info[c] and
 *    every solution filled.  k must be the block's width.  The operator's shift (fc_shifted_set_shift) is neither read nor moved.
 *    fc_shifted_block_info: info[4] = the block's width k, its padded width KB, and of the last fc_solve_shifted_block the lock-step
 *    iterations launched (each ONE factor apply for all columns) and the cycles that ran any (each one more apply for the update). */
int fc_shifted_set_block(fc_handle h, int32_t k);
int fc_shifted_block_info(fc_handle h, int64_t* info /* [4] */);
int fc_solve_shifted_block(fc_handle h, int32_t k, const double* sigma_re, const double* sigma_im, const double* b_re, const double* b_im,
                           double* x_re, double* x_im, double* info);
/* Adjoint solves on the held factors (opt-in; with fc_shifted_set_adjoint never called nothing is allocated and nothing above changes).
 * The factor values of the transposed system in the same layout are a per-front transposition of the values the factorisation left in
 * its fronts: a second value array, written by one more export pass, not a second factorisation.  In the adjoint mode the solver
 * behaves as the solver of M^H = conj(sigma) E^T - A^T, with sigma as given to fc_setup_shifted / fc_shifted_set_shift / per column:
 * fc_solve_shifted and fc_solve_shifted_block solve with M^H (refinement, GMRES rescue and lagged factors included: mat-vec at the
 * operator's shift, preconditioner = the transposed factors of the factored shift); fc_shifted_spmv(s, t) gives (s E^T - t A^T) x with
 * s as given; the Arnoldi runs on -(M^H)^-1 E^T, the shift-invert of (A^T, E^T) at conj(sigma), and fc_shifted_ritz forms its residuals
 * with A^T and E^T; fc_shifted_project is unchanged.
 *    fc_shifted_set_adjoint: on = 1 switches the mode on (the adjoint array, the values of A^T and E^T on the handle's pattern and their
 *    map are built now if missing: factor size + 20 bytes per pattern entry; from then on every fc_setup_shifted ends with the
 *    transposed export); 0 goes back to direct, the array stays; -1 goes to direct and frees the adjoint side.  FC_ERR_NOT_READY
 *    before the first fc_setup_shifted, FC_ERR_INVALID for other values and for a pattern that is not structurally symmetric.  A
 *    switch drops a started Arnoldi (fc_shifted_arnoldi_step: FC_ERR_NOT_READY until the next start) and the block's tiled copy of
 *    the factors is redone by the next block solve.
 *    fc_shifted_adjoint_info: info[4] = mode, device bytes held for the adjoint side, transposed exports since the structure was built,
 *    mode switches; dinfo[2] = device milliseconds and algorithmic bytes of the last transposed export.
 *    fc_shifted_arnoldi_set_op: the operator of fc_shifted_arnoldi_* / fc_shifted_ritz: 0 the shift-invert above (default), 1 the
 *    resolvent Op_R v = M^-H E^T M^-1 E v, both solves at the operator's shift, each with its refinement or GMRES, on the two arrays
 *    whatever the mode is (FC_ERR_NOT_READY without the adjoint array).  For symmetric positive semidefinite E its eigenvalues are
 *    the squared gains max q^H E q / g^H E g of q = M^-1 E g.  fc_shifted_ritz then returns |Op_R x - lam x|, |Op_R x|, |x| per column.
 *    A change of operator drops a started Arnoldi. */
int fc_shifted_set_adjoint(fc_handle h, int32_t on);
int fc_shifted_adjoint_info(fc_handle h, int64_t* info /* [4] */, double* dinfo /* [2] */);
int fc_shifted_arnoldi_set_op(fc_handle h, int32_t kind);
/* Snapshot sets: balanced reduced models from frequency snapshots (opt-in; with none of these called nothing is allocated and no new
 * kernel runs).  The solver keeps up to three sets of complex columns on the device, in the layout of its solutions ([col][N]
 * interleaved): set 0 for direct solutions, 1 for adjoint solutions, 2 for vectors loaded from the host (B, test data).
 *    fc_shifted_snap_reserve: room for ncol columns in `set` (ncol = 0 frees it; another capacity drops the set's columns).  After the
 *    first fc_setup_shifted (FC_ERR_NOT_READY before).  fc_shifted_info counts the bytes.
 *    fc_shifted_snap_push: appends scale * the first ncol solutions of the last fc_solve_shifted / fc_solve_shifted_block.
 *    FC_ERR_INVALID past the capacity or past the columns of that solve; nothing is written then.
 *    fc_shifted_snap_load: appends scale * (re + i im) for ncol host vectors ([ncol][N]; im NULL = real).
 *    fc_shifted_snap_gram: out[2 a + p][2 b + q] = part_p(l_a)^T Op part_q(r_b), p, q in {re, im}, a / b the columns of the sets `left` /
 *    `right`: a real row-major matrix of 2 ncol_left x 2 ncol_right.  kind 0: Op = identity, 1: E, 2: A -- the held direct values
 *    whatever the adjoint mode is, without the pin's shift.  No floating-point atomics: a repeated call returns the same bits.
 *    FC_ERR_INVALID for an empty set, an unknown set or kind.
 *    fc_shifted_snap_combine: out[c][:] = sum_J Q[J][c] part_J (Q [2 ncol][k] real, row-major; part_{2 a + p} = part p of column a): k real
 *    N-vectors (out [k][N]), the modes of a reduced model -- the only N-long data that cross, and only on request.
 *    fc_shifted_snap_info: info[8] = columns, capacity of set 0, of set 1, of set 2, device bytes held by the sets and their work
 *    buffers, Gram calls since the structure was built.
 *    fc_shifted_snap_clear: the set's column count back to 0, the memory stays.
 * fc_release_shifted and fc_destroy free all sets. */
int fc_shifted_snap_reserve(fc_handle h, int32_t set, int32_t ncol);
int fc_shifted_snap_push(fc_handle h, int32_t set, int32_t ncol, double scale);
int fc_shifted_snap_load(fc_handle h, int32_t set, int32_t ncol, const double* re, const double* im, double scale);
int fc_shifted_snap_gram(fc_handle h, int32_t left, int32_t right, int32_t kind, double* out);
int fc_shifted_snap_combine(fc_handle h, int32_t set, int32_t k, const double* Q, double* out);
int fc_shifted_snap_info(fc_handle h, int64_t* info /* [8] */);
int fc_shifted_snap_clear(fc_handle h, int32_t set);

/* ── state snapshots on the device: the history of a run without host round trips, POD / DMD from it (opt-in; with no bank reserved
 *    nothing is allocated, nothing new is launched and every trajectory is bit-identical).  Replaces cutting a run into pieces and
 *    downloading the field after each (the reference's per-step exporter, flowsolver.py:775-799, as the source of modal analysis).
 *    The bank holds two sets of real columns [col][N], W layout, original numbering, `capacity` columns each: set 0 the captured
 *    states (u_n, p_n), set 1 vectors loaded from the host or combined on the device (allocated on first use).
 *    fc_state_snap_reserve: a new, empty bank (capacity = 0 frees everything).  From then on the handle counts every step whose
 *    solution becomes the state -- fc_step, fc_step_begin / _end, fc_run, fc_run_closed_loop -- and after step number s of the count
 *    (1-based) with s > first and (s - first) % every == 0 it enqueues ONE launch on the step's stream that gathers the new state into
 *    the next column of set 0; when set 0 is full the step is counted as dropped and nothing is launched.  fc_undo_step takes the count
 *    back, and the column if the withdrawn step was captured; fc_set_state captures nothing.  A non-finite step is captured like any
 *    other: after a diverged fc_run the columns from that step on are non-finite.  FC_ERR_INVALID, with nothing touched: partitioned
 *    handles, handles with a batch set (their steps never reach the capture), every < 1, first < 0, a step in flight.  FC_ERR_HIP when
 *    the allocation fails; the handle is then as it was.
 *    fc_state_snap_push: the current state into the next column of set 0, now.
 *    fc_state_snap_load / _get: ncol host columns X [ncol][N] into / out of `set` from column col0 (load: col0 <= the set's count,
 *    col0 + ncol <= capacity; the count becomes at least col0 + ncol).  fc_state_snap_clear: the set's count back to 0.
 *    fc_state_snap_info: info[8] = capacity, columns of set 0, of set 1, every, first, steps counted, steps dropped, device bytes held.
 *    fc_state_snap_mean: out [N] (may be NULL; the mean stays on the device either way) = mean of columns [c0, c1) of `set`, summed in
 *    column order; subtract = 1 subtracts it from those columns in place.
 *    fc_state_snap_gram: out [(a1 - a0)][(b1 - b0)] row-major = L[:, a0:a1]^T Wt R[:, b0:b1], L / R the sets lset / rset;
 *    weight_slot = -1: Wt = I, >= 0: the values now in that matrix slot (FC_SLOT_MASS: the energy inner product; FC_ERR_NOT_READY for
 *    a slot that is not assembled).  Exactly (a1 - a0)(b1 - b0) doubles are written.  fp64 matrix cores, no floating-point atomics:
 *    a repeated call returns the same bits.
 *    fc_state_snap_combine: out [k][N] = sum_j Q[j][c] X_j over the columns j = c0 .. c1 - 1 of `set` in that order (Q [(c1 - c0)][k]
 *    row-major); keep = 1 also appends the k vectors to set 1 (FC_ERR_INVALID past its capacity, nothing written), so that a later Gram
 *    projects onto them; out may be NULL then.
 *    Every call but _info waits for the handle's outstanding work first.  fc_destroy frees the bank. ------------------------------ */
int fc_state_snap_reserve(fc_handle h, int32_t capacity, int32_t every, int32_t first);
int fc_state_snap_push(fc_handle h);
int fc_state_snap_load(fc_handle h, int32_t set, int32_t col0, int32_t ncol, const double* X);
int fc_state_snap_get(fc_handle h, int32_t set, int32_t col0, int32_t ncol, double* out);
int fc_state_snap_clear(fc_handle h, int32_t set);
int fc_state_snap_info(fc_handle h, int64_t* info /* [8] */);
int fc_state_snap_mean(fc_handle h, int32_t set, int32_t c0, int32_t c1, int32_t subtract, double* out);
int fc_state_snap_gram(fc_handle h, int32_t lset, int32_t a0, int32_t a1, int32_t rset, int32_t b0, int32_t b1, int32_t weight_slot,
                       double* out);
int fc_state_snap_combine(fc_handle h, int32_t set, int32_t c0, int32_t c1, int32_t k, const double* Q, int32_t keep, double* out);

/* ── adjoint time stepping: gradients of a run's cost (csrc/fc_adjoint.hip.h).  Opt-in: with fc_set_adjoint_factors never
 *    called nothing is allocated and nothing above changes.  The linearised stepper (fc_set_time_scheme(dt, 0)) is the recurrence
 *        A_s x_{m+1} = Z M (cm_n x_m + cm_nn x_{m-1}) + B~ u_{m+1},   y_m = C x_m
 *    (Z zeroes the Dirichlet rows, M is the velocity mass of the element loop, B~ the control columns of fc_rhs_gather, C the sensor
 *    rows); for J = sum_m w_m . y_m + z . x_n its exact discrete adjoint is the same recurrence run backwards on A^T:
 *        mu_m = A_s^-T [C^T w_m (+ z at m = n) + M Z (cm_n mu_{m+1} + cm_nn mu_{m+2})],   dJ/du_m = B~^T mu_m.
 *    No forward trajectory is stored.
 *    fc_set_adjoint_factors: on = 1 builds, for `slot`, the factor values of the transposed system in the layout of the direct ones
 *    (a second fp64 array, exported from the fronts: the call re-runs the slot's elimination on the slot's present matrix, which
 *    reproduces the direct values bit for bit) and the values of the transposed permuted matrix (refinement, residual monitor);
 *    on = 0 keeps them but refuses adjoint calls (FC_ERR_NOT_READY); on = -1 frees them (and, with the last slot, every buffer of the
 *    march).  A later fc_refactor of the slot rebuilds them; fc_update_operator, fc_apply_bc or a new permutation mark them stale
 *    (adjoint calls: FC_ERR_NOT_READY until on = 1 again); a new solver structure drops them.  FC_ERR_INVALID, with the reason, for:
 *    a partitioned handle, compressed (bits != 64), truncated or inexact factors, a factor-free slot, a Krylov method selected
 *    (fc_set_solver_options), a slot with an explicit right-hand-side operator (Crank-Nicolson), a pattern without a partner entry.
 *    fc_adjoint_info: info[8] = available, stale, in use, device bytes of the slot's arrays, device bytes of the march's buffers and
 *    tables (shared by both slots), transposed exports so far; dinfo[2] = milliseconds of the slot's last export (HIP events, the
 *    matrix-value gather included), milliseconds of the handle's last fc_run_adjoint (HIP events around its launches and copies).
 *    fc_solve_transposed: fc_solve's contract for A_slot^T x = b (same sweeps on the transposed values, same refinement count on the
 *    transposed matrix, same info_out); the direct arrays are back in place on return.
 *    fc_run_adjoint: n_steps backward steps for a forward run that started with `first_order_slot` (BDF2 afterwards), enqueued without
 *    host synchronisation in between.  w_seq [n_steps][n_sens] (row m - 1 weights y_m, the output of forward step m) or NULL;
 *    z_terminal [N] (W layout) or NULL; g_seq [n_steps][n_act] (row m - 1 = dJ/du_m); dx0, dxm1 [N] (W layout; either may be NULL):
 *    dJ/dx_0 and dJ/dx_{-1}.  FC_ERR_DIVERGED for a non-finite mu; FC_ERR_INVALID with a nonlinear time scheme and no state tape of the run (below).  State, step counter,
 *    snapshot bank, loop cursor and fc_undo_step are untouched.
 *    fc_adjoint_reset / fc_step_adjoint / fc_adjoint_mass_product: the same march one step at a time.  reset: mu_{m+1} = mu_{m+2} = 0
 *    and z (or NULL) to be added by the next step; step: one backward step on `slot` with the coefficients cm_n, cm_nn_next of the
 *    forward steps that consumed x_m (w [n_sens] or NULL, g_out [n_act]); mass_product: out [N] (W layout) =
 *    M Z (cm_n mu_last + cm_nn mu_before), which is dJ/dx_0 (cm_n of step 1, cm_nn of step 2) or dJ/dx_{-1} (cm_nn of step 1, 0).
 *    Both are refused (FC_ERR_INVALID) with a nonlinear time scheme: their signatures carry no state.
 *
 *    The NONLINEAR stepper (fc_set_time_scheme(dt, 1)): the adjoint reads the forward trajectory from a state tape on the device.
 *    fc_adjoint_tape_reserve: capacity + 2 columns of N doubles (8 N bytes per step) in the solver's numbering; 0 frees the tape.
 *    Refused on partitioned handles, with a batch set, before a permutation exists and (FC_ERR_INVALID, the bytes needed and free
 *    named, the handle as it was) when the tape does not fit into free device memory.  Without a tape no step enqueues anything for
 *    it.  fc_adjoint_tape_begin: the count back to 0, the present (u_nn, u_n) levels into columns 0 and 1; every state advance from
 *    here on (fc_step, fc_run, fc_run_closed_loop) appends the new state with one device copy and the host notes the step's order
 *    slot; fc_undo_step withdraws the last column.  A step beyond the capacity marks the tape overflowed and writes nothing.
 *    fc_set_state, fc_set_state_batch, a new permutation or solver structure end the tape until the next _begin.
 *    fc_run_adjoint on a nonlinear handle needs a tape that holds exactly its run: n_steps steps, not overflowed, the first on
 *    first_order_slot, the others on BDF2 -- else FC_ERR_INVALID with the reason.  Backward step m reads column m + 1.
 *    fc_adjoint_tape_info: info[8] = capacity, steps held, overflowed, device bytes (also part of fc_adjoint_info's shared bytes),
 *    begun, steps lost to the overflow.
 *
 *    The CHECKPOINTED form of that tape, for horizons whose dense tape does not fit (DESIGN §5.4 "Checkpointed tape").
 *    fc_adjoint_tape_reserve_sparse(capacity, every = c): the pair (x_{jc-1}, x_{jc}) for every j < ceil(capacity / c), ONE dense
 *    segment buffer of c + 2 columns and a control tape of the (u_ctrl, u_force) rows every taped step read: (2 ceil(capacity / c) +
 *    c + 2) 8 N + capacity 16 n_act bytes instead of (capacity + 2) 8 N.  every = 0 or capacity = 0 frees the reserve.  A handle
 *    holds the dense or the checkpointed tape, never both: reserving one frees the other.  Refused (FC_ERR_INVALID, the reason, nothing
 *    enqueued) for every < 0, a capacity outside [0, 2^24], a step in flight, partitioned handles, a batch set, and when the reserve
 *    does not fit into free device memory.  _begin and _info serve both forms; of the checkpointed one info[3] counts buffer, pairs and
 *    control tape, info[6] = every, info[7] = forward steps the last march recomputed.  A taped step costs what it costs on the dense
 *    tape and, where it opens a segment, two copies of a pair; its control row is one small launch in front of an fc_step, and one
 *    launch for all rows behind an fc_run / fc_run_closed_loop.  fc_undo_step withdraws the last
 *    column inside a segment; withdrawing the step that opened one ends the tape.
 *    fc_run_adjoint / fc_run_adjoint_closed_loop take the checkpointed tape wherever they take the dense one (energy weights
 *    included), signatures unchanged: the march runs segment by segment from the last to the first and, in front of every segment but
 *    the one the forward run left in the buffer, enqueues -- same stream, no host synchronisation -- the restore of its pair and its
 *    forward steps again: the taped step's own launches on the taped controls (no controller, no residual monitor, no energy, nothing
 *    counted or taped).  The gradients equal the dense tape's in every bit.  On return the state ring, step counter, snapshot bank,
 *    loop cursor and fc_undo_step are as on entry.  FC_ERR_HIP if a replay went non-finite where the taped run did not.  A march that
 *    recomputed leaves segment 0 in the buffer: the same run can be marched again (every segment is then recomputed), a further
 *    forward step ends the tape.
 *    fc_step_adjoint and the optimal perturbations (fc_optpert_*) do not read it.  Batched: fc_adjoint_tape_reserve_sparse_batch. */
int fc_adjoint_tape_reserve(fc_handle h, int32_t capacity);
int fc_adjoint_tape_reserve_sparse(fc_handle h, int32_t capacity, int32_t every);
int fc_adjoint_tape_begin(fc_handle h);
int fc_adjoint_tape_info(fc_handle h, int64_t* info /* [8] */);
int fc_set_adjoint_factors(fc_handle h, int slot, int32_t on);
int fc_adjoint_info(fc_handle h, int slot, int64_t* info /* [8] */, double* dinfo /* [2] */);
int fc_solve_transposed(fc_handle h, int slot, const double* b, double* x, double* info_out /* [4] */);
int fc_run_adjoint(fc_handle h, int first_order_slot, int32_t n_steps, const double* w_seq, const double* z_terminal, double* g_seq,
                   double* dx0, double* dxm1);
int fc_adjoint_reset(fc_handle h, const double* z_terminal);
int fc_step_adjoint(fc_handle h, int slot, double cm_n, double cm_nn_next, const double* w, double* g_out);
int fc_adjoint_mass_product(fc_handle h, double cm_n, double cm_nn, double* out);

/* ── adjoint of a closed loop: gradients of the controller (csrc/fc_adjoint_loop.hip.h).  For a single closed loop (k = 1;
 *    xi = controller state, y_0 = the y0 argument of fc_run_closed_loop, m = 1 .. n)
 *        yc_m = G y_{m-1} + g0 + w_y[m]     uc_m = C xi_{m-1} + D yc_m     xi_m = Ad xi_{m-1} + Bd yc_m
 *        v_m  = S uc_m + w_u[m]             u_m  = min(max(v_m, lo), hi)   plant step m with u_m,  y_m = C_s x_m
 *    and J = sum_m (w_m . y_m + r_m . u_m) + z . x_n, the backward march of fc_run_adjoint carries the controller with it
 *    (lambda = adjoint of xi, eta = adjoint of yc, lambda_n = 0, eta_{n+1} = 0; sigma_m = 1 where lo < v_m < hi, else 0):
 *        mu_m  = A_s^-T [C_s^T (w_m + G^T eta_{m+1}) (+ z at m = n) + the mass / Jacobian terms of fc_run_adjoint]
 *        ub_m  = B~^T mu_m + r_m     vb_m = sigma_m o ub_m     ucb_m = S^T vb_m
 *        eta_m = D^T ucb_m + Bd^T lambda_m                     lambda_{m-1} = Ad^T lambda_m + C^T ucb_m
 *        dJ/dAd = sum lambda_m xi_{m-1}^T   dJ/dBd = sum lambda_m yc_m^T   dJ/dC = sum ucb_m xi_{m-1}^T   dJ/dD = sum ucb_m yc_m^T
 *        dJ/dG = sum eta_m y_{m-1}^T   dJ/dg0 = sum eta_m   dJ/dS = sum vb_m uc_m^T   dJ/dw_y[m] = eta_m   dJ/dw_u[m] = vb_m
 *        dJ/dxi_0 = lambda_0           dJ/dy_0 = G^T eta_1
 *    The forward run is read from the LOOP TAPE: one row [xi_{m-1} (nx) | y_{m-1} (n_sens) | v_m (n_act)] per step, stored by the
 *    controller launch of fc_run_closed_loop.
 *    fc_adjoint_loop_reserve: a tape of `capacity` steps laid out for the present bank, and an untransposed copy of the bank for the
 *    transposed products; 0 frees both.  FC_ERR_NOT_READY without a bank; FC_ERR_INVALID on partitioned handles, with a batch set and
 *    for a bank of k > 1.  Without a reserve nothing is allocated or launched and fc_run_closed_loop forms exactly what it formed
 *    before.  fc_set_controllers with a reserve lays the tape out again for the new bank (k = 0 or k > 1: the reserve is dropped).
 *    fc_adjoint_loop_begin: the count back to 0; from here on every step of every fc_run_closed_loop call appends its row, so a run
 *    cut into several calls (each call's y0 = the last measurement of the one before) is one tape.  fc_ctrl_apply does not tape;
 *    fc_run_closed_loop_batch has a tape of its own (fc_adjoint_loop_reserve_batch, below), never this one.  The tape ends -- until the next _begin -- on fc_set_controllers, fc_set_controller_state,
 *    fc_set_loop_signals, fc_set_control_limits, fc_set_state, fc_undo_step, a time step taken outside fc_run_closed_loop, a new
 *    permutation or solver structure; a step beyond the capacity marks it overflowed and writes nothing.
 *    fc_adjoint_loop_info: info[8] = capacity, steps held, overflowed, device bytes, begun, steps lost, the taped run went
 *    non-finite, doubles per tape row.
 *    fc_run_adjoint_closed_loop: the march for a taped run of n_steps steps that started on `first_order_slot`; one controller launch
 *    per backward step more than fc_run_adjoint, one launch for the parameter gradients, one synchronisation at the end.  w_seq
 *    [n_steps][n_sens], r_seq [n_steps][n_act], z_terminal [N]: the cost's weights, each may be NULL.  Outputs, each may be NULL:
 *    gAd [nx][nx], gBd [nx][nyc], gC [nuc][nx], gD [nuc][nyc], gG [nyc][n_sens], gg0 [nyc], gS [n_act][nuc] (row-major, the shapes
 *    fc_set_controllers takes), dxc0 [nx] = dJ/dxi_0, dy0 [n_sens], dwy [n_steps][nyc], dwu [n_steps][n_act], ubar_seq
 *    [n_steps][n_act] (row m - 1 = ub_m, the gradient with respect to the clamped control), dx0, dxm1 [N] as fc_run_adjoint.  Works
 *    on linearised handles and, with the state tape of the same run, on nonlinear ones.  FC_ERR_NOT_READY without a reserve;
 *    FC_ERR_INVALID, with the reason and nothing enqueued, for a loop tape that does not hold exactly this run (step count, first
 *    slot, overflowed, ended, not begun), a forward run that went non-finite, k != 1, and everything fc_run_adjoint refuses.  Every
 *    sum is formed by one thread in index order: two marches are bit-identical.  fc_run_adjoint, the state, the step counter, the
 *    snapshot bank and the loop cursor are untouched (fc_adjoint_info's run time reports the last march of either kind). */
int fc_adjoint_loop_reserve(fc_handle h, int32_t capacity);
int fc_adjoint_loop_begin(fc_handle h);
int fc_adjoint_loop_info(fc_handle h, int64_t* info /* [8] */);
int fc_run_adjoint_closed_loop(fc_handle h, int first_order_slot, int32_t n_steps, const double* w_seq, const double* r_seq,
                               const double* z_terminal, double* gAd, double* gBd, double* gC, double* gD, double* gG, double* gg0, double* gS,
                               double* dxc0, double* dy0, double* dwy, double* dwu, double* ubar_seq, double* dx0, double* dxm1);

/* ── batched adjoint march: gradients of k lock-step runs in one backward sweep (csrc/fc_adjoint_batch.hip.h).  Opt-in:
 *    a handle that never calls these allocates nothing and launches nothing for them, and every other entry point forms what it formed.
 *    Open-loop marches, linearised and nonlinear, under the conditions of fc_set_batch (single GPU, full fp64 factors, refine = 0);
 *    partitioned handles, compressed / truncated / inexact factors and the factor-free mode are refused with FC_ERR_INVALID and the
 *    reason.  Host arrays are simulation-major, as in the rest of the batch API.  Column s of every array follows exactly the
 *    recurrence of fc_run_adjoint; the transposed solves of all columns are block products on the matrix cores (fc_nd_block_b on a
 *    tiled copy of the slot's transposed factor values), which reads the factors once per backward step for all columns.
 *    fc_set_adjoint_batch: on = 1 needs fc_set_batch and current, switched-on fc_set_adjoint_factors(slot, 1).  It packs the tiled copy
 *    of the transposed values (an array of its own, the size of the batch's tiled copy; forward batched steps never read it) and
 *    allocates the march's [row][KB] buffers.  on = -1 frees the slot's copy and, with the last slot, the buffers.  The copy goes stale
 *    with the transposed values (fc_refactor, fc_update_operator, fc_apply_bc, fc_set_bc, a new permutation or structure) and with
 *    fc_set_batch: the next march repacks it if the transposed values are current again (fc_refactor rebuilds them), and fails with
 *    FC_ERR_NOT_READY otherwise (fc_set_adjoint_factors(slot, 1) again).  fc_set_batch(0), and fc_set_bc with another set of Dirichlet dofs (which drops
 *    the batch), free everything, the tape included.
 *    fc_solve_transposed_batch: parity hook, fc_solve_batch's contract for A_slot^T X = B (b, x: [k][N]).
 *    fc_run_adjoint_batch: w_seq [n_steps][k][n_sens] or NULL, z_terminal [k][N] or NULL, g_seq [n_steps][k][n_act], dx0 / dxm1 [k][N] or
 *    NULL, flags_out [k] or NULL.  All steps are enqueued behind one quiesce, one synchronisation at the end.  A column that goes
 *    non-finite is marked in flags_out and the call returns FC_ERR_DIVERGED; the columns are independent, so the others are valid.
 *    Columns k .. KB - 1 are padding: zero throughout, they reach no output.  The march never touches the batch's state ring, its tiled
 *    factors, its graphs or its step counter.  Sums run in a fixed order: two marches are bit-identical, equal columns bit-equal.
 *    fc_adjoint_tape_reserve_batch / _begin_batch / _info_batch: the state tape of batched steps, which a nonlinear handle's march
 *    reads: capacity + 2 columns of N x KB doubles (the batch's state as it stands, solver's numbering).  8 N KB bytes per step -- KB,
 *    the padded width, not k: 14.4 MB per step on the cylinder's O1 mesh at KB = 32.  A reserve that does not fit in the free device
 *    memory is refused.  fc_step_batch / fc_step_batch_begin append behind the step (one contiguous copy on the main stream);
 *    fc_run_closed_loop_batch appends behind every step while a batched LOOP tape is begun (fc_adjoint_loop_begin_batch, below) and ends
 *    a begun state tape otherwise.  The tape ends with fc_set_state_batch, fc_reset_sim_batch,
 *    fc_set_batch and a new permutation or structure; a step past the capacity marks it overflowed and writes nothing.  On a
 *    nonlinear handle fc_run_adjoint_batch needs a tape that holds exactly its run; the refusals are fc_run_adjoint's.  The single
 *    run's tape (fc_adjoint_tape_reserve) is still refused with a batch set.  info[8] as fc_adjoint_tape_info, info[6] = KB.
 *    fc_adjoint_batch_info: info[8] = set up, stale, bytes of the slot's tiled transposed copy, bytes of the march's buffers, bytes of
 *    the batched tape, repacks so far, KB of the buffers, 0; dinfo[2] = milliseconds of the last fc_run_adjoint_batch (HIP events), 0. */
int fc_set_adjoint_batch(fc_handle h, int slot, int32_t on);
int fc_adjoint_batch_info(fc_handle h, int slot, int64_t* info /* [8] */, double* dinfo /* [2] */);
int fc_solve_transposed_batch(fc_handle h, int slot, int32_t k, const double* b, double* x);
int fc_run_adjoint_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, const double* w_seq, const double* z_terminal,
                         double* g_seq, double* dx0, double* dxm1, int32_t* flags_out);
int fc_adjoint_tape_reserve_batch(fc_handle h, int32_t capacity);
/* The checkpointed form of the batched tape (fc_adjoint_tape_reserve_sparse, above, with columns of N KB doubles and KB control rows per
 * step): (2 ceil(capacity / every) + every + 2) 8 N KB + capacity 16 KB n_act bytes.  Same refusals; FC_ERR_NOT_READY without a batch
 * set.  fc_step_batch, fc_step_batch_begin and fc_run_closed_loop_batch tape onto it wherever they tape onto the dense one;
 * fc_run_adjoint_batch and fc_run_adjoint_closed_loop_batch march over it segment by segment, recomputing every segment but the one
 * the forward run left in the buffer with the batched step's plain launches (element loop, full gather, apply, tail; no residual
 * monitor, no energy, nothing run ahead) on the taped control rows; gradients equal the dense tape's in every bit.  _begin_batch and
 * _info_batch serve both forms: of the checkpointed one info[3] counts buffer, pairs and control tape and info[7] = every (its one free
 * slot); the forward steps the last march recomputed are fc_adjoint_batch_info's info[7]. */
int fc_adjoint_tape_reserve_sparse_batch(fc_handle h, int32_t capacity, int32_t every);
int fc_adjoint_tape_begin_batch(fc_handle h);
int fc_adjoint_tape_info_batch(fc_handle h, int64_t* info /* [8] */);

/* ── adjoint of k lock-step closed loops: gradients of a bank of k controllers in one backward sweep (csrc/fc_adjoint_loop_batch.hip.h,
 *    DESIGN §5.4 "Batched closed loops").  Opt-in, beside the single loop's entry points above, which keep every refusal they have.
 *    Column s of the batch runs the recurrence of fc_run_adjoint_closed_loop with ITS controller (block s of the bank), signals, limits
 *    and weights; the transposed solves of all columns are fc_run_adjoint_batch's block products.
 *    fc_adjoint_loop_reserve_batch: a tape [capacity][k][nx + n_sens + n_act] (row of simulation s at step m: [xi_{m-1,s} | y_{m-1,s} |
 *    v_{m,s}], as in the single tape) and an untransposed copy [k][stride] of all k blocks of the bank; 0 frees both.  Needs fc_set_batch
 *    and a bank of exactly the batch's k (FC_ERR_NOT_READY without either, FC_ERR_INVALID for k that differ); FC_ERR_INVALID on
 *    partitioned handles, with a step in flight and for a capacity outside [0, 2^24].  Without a reserve nothing is allocated or
 *    launched and fc_run_closed_loop_batch forms exactly what it formed before.  fc_set_controllers with a reserve lays the tape out
 *    again for a new bank of the batch's k and drops the reserve for any other.
 *    fc_adjoint_loop_begin_batch: zeroes the tape (a column whose run ends early is read as zeros) and sets the count to 0; from here on
 *    every step of every fc_run_closed_loop_batch call appends one row per simulation (a dead simulation writes nothing), so a run cut
 *    into several calls is one tape, and appends the new state to a begun batched state tape (fc_adjoint_tape_begin_batch) instead of
 *    ending it: a nonlinear handle then holds the state tape of the same run.  The tape ends -- until the next _begin_batch -- on
 *    fc_set_controllers, fc_set_controller_state, fc_set_loop_signals, fc_set_control_limits, fc_set_state_batch, fc_reset_sim_batch,
 *    fc_step_batch / fc_step_batch_begin, a new permutation or solver structure; fc_set_batch frees everything.  A step beyond the
 *    capacity marks it overflowed and writes nothing.
 *    fc_adjoint_loop_info_batch: info[8] = capacity, steps held, overflowed, device bytes, begun, steps lost, bit mask of the columns
 *    whose taped forward run went non-finite, doubles per tape row.
 *    fc_run_adjoint_closed_loop_batch: fc_run_adjoint_closed_loop's arguments with a leading k on every array: w_seq [n][k][n_sens],
 *    r_seq [n][k][n_act], z_terminal [k][N] (each may be NULL); gAd [k][nx][nx], gBd, gC, gD, gG, gg0, gS per column, dxc0 [k][nx], dy0
 *    [k][n_sens], dwy [n][k][nyc], dwu / ubar_seq [n][k][n_act], dx0 / dxm1 [k][N], flags_out [k] (each may be NULL).  Per backward step
 *    the launches of fc_run_adjoint_batch and one more, fc_ctrl_adj_step_b (grid k, one wave per column); one fc_ctrl_adj_grads_b
 *    launch behind the last; one synchronisation at the end; device time in fc_adjoint_batch_info's dinfo[0].  A column whose forward run went non-finite, or whose adjoint goes
 *    non-finite, is marked in flags_out, its outputs are NaN and the call returns FC_ERR_DIVERGED; the other columns are valid.
 *    FC_ERR_NOT_READY without a reserve; FC_ERR_INVALID, with the reason and nothing enqueued, for a loop tape that does not hold
 *    exactly this run (step count, first slot, overflowed, ended, not begun), a bank whose k differs from the batch's, a nonlinear
 *    handle without the batched state tape of the same run, and everything fc_run_adjoint_batch refuses.  No atomics, no cross-lane
 *    sums beyond the fixed tree of the g reduction: equal columns come out bit-equal, two marches are bit-identical.  The state ring,
 *    the step counter, the loop cursor, the snapshot bank and the single run's tapes are untouched. */
int fc_adjoint_loop_reserve_batch(fc_handle h, int32_t capacity);
int fc_adjoint_loop_begin_batch(fc_handle h);
int fc_adjoint_loop_info_batch(fc_handle h, int64_t* info /* [8] */);
int fc_run_adjoint_closed_loop_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, const double* w_seq, const double* r_seq,
                                     const double* z_terminal, double* gAd, double* gBd, double* gC, double* gD, double* gG, double* gg0, double* gS,
                                     double* dxc0, double* dy0, double* dwy, double* dwu, double* ubar_seq, double* dx0, double* dxm1,
                                     int32_t* flags_out);

/* ── energy term in the cost of the adjoint marches (csrc/fc_adjoint_energy.hip.h, DESIGN §5.4 "Energy term").  Opt-in: a handle that
 *    holds no rows allocates nothing and launches nothing for them, and every march forms what it formed, bit for bit.
 *    With dE_m = 1/2 x_m^T M x_m (velocity mass matrix, the full state x_m: actuated Dirichlet values included -- the energy every step
 *    logs), a cost term  sum_m e_m dE_m  adds  e_m M x_m  to the right-hand side of backward step m, on every row, unmasked:
 *        mu_m = A_s^-T [C^T w_m (+ z at m = n) + M (Z (cm_n mu_{m+1} + cm_nn mu_{m+2}) + e_m x_m) (+ the Jacobian term)]
 *    x_m is read from the state tape, on linearised handles too (8 N bytes per step; batched: 8 N KB).
 *    fc_set_adjoint_energy: k = 0: e_seq [n_steps] for fc_run_adjoint and fc_run_adjoint_closed_loop; k >= 1: e_seq [n_steps][k] for
 *    fc_run_adjoint_batch and fc_run_adjoint_closed_loop_batch (k = the batch's, FC_ERR_NOT_READY without fc_set_batch; padded to KB on
 *    the device).  Row m - 1 weights dE_m.  The rows are uploaded once and held until they are replaced or cleared; n_steps = 0 or
 *    e_seq = NULL clears and frees.  FC_ERR_INVALID on partitioned handles and for a non-finite weight.
 *    While rows are held each of the four marches uses them on every backward step -- not for dx0 / dxm1, whose products carry no
 *    energy term because dE_0 is not in the sum -- and refuses with FC_ERR_INVALID and the reason: rows of the other kind (k = 0 rows in
 *    a batched march and the reverse), another n_steps or k than the call's, and a state tape (of the march's kind) that does not hold
 *    exactly the run, on linearised handles as on nonlinear ones.  fc_step_adjoint carries no state and refuses held rows.
 *    fc_adjoint_energy_info: info[8] = rows held (n_steps), k, device bytes, backward steps of the last march that ran an energy
 *    kernel, KB of the rows (0: single), 0, 0, 0. */
int fc_set_adjoint_energy(fc_handle h, int32_t n_steps, int32_t k, const double* e_seq);
int fc_adjoint_energy_info(fc_handle h, int64_t* info /* [8] */);

/* ── optimal perturbations: transient growth by batched direct-adjoint loops (csrc/fc_optpert.hip.h).  Opt-in: a handle
 *    that never calls these entry points allocates nothing and launches nothing for them, and every other call returns the bits it
 *    returned.  Notation of "adjoint time stepping" above.  f: the free velocity rows (W-layout velocity dofs not in fc_set_bc's list),
 *    P_f the mask onto them, M_ff FC_SLOT_MASS restricted to f x f.  A run of n steps with u = 0 from x_0 = U[:, c], x_{-1} = 0, p_0 = 0
 *    (first step on first_order_slot, the rest on BDF2) is x_n = Phi x_0; the operator of the eigenproblem  K v = theta M_ff v  is
 *        K U = P_f Phi^T M Phi U:   z = M_ff x_n as the terminal weight of the batched march (w = NULL), K U = its dx0 masked to f.
 *    All blocks are [k][N] on the host (W layout, original numbering) and [N][KB] on the device (the batch's layout and numbering).
 *    Every entry point needs fc_set_batch and an assembled FC_SLOT_MASS (FC_ERR_NOT_READY) and refuses partitioned handles and a step
 *    in flight (FC_ERR_INVALID).  The compacted M_ff, its Jacobi diagonal and the mask are built on first use and again after the mass
 *    slot's values changed (fc_assemble_matrix, fc_set_matrix_values, fc_apply_bc on FC_SLOT_MASS) or the permutation did.
 *    fc_mass_solve_batch: x = M_ff^-1 b_f on f, exactly zero elsewhere; whatever b holds outside f is ignored.  Block Jacobi-
 *    preconditioned CG, all columns in lock step, stopped per column on |r_c|_2 <= rtol |b_f,c|_2; a converged column, a column with
 *    b_f = 0 and the padding columns freeze (a zero column returns exact zeros after 0 iterations).  info [k][2] = iterations, final
 *    |r| / |b| per column.  FC_ERR_NOT_CONVERGED when max_iter ran out (info filled, x the last iterate).  Needs nothing else: no
 *    adjoint factors, no time scheme.  The host synchronises once per chunk of 8 iterations (it reads the per-column scalars there) and
 *    nowhere else inside the solve: ceil(iterations / 8) times; the entry point's own download of x is one more.
 *    fc_optpert_reserve(on = 1): the resident blocks FC_OPTPERT_U .. FC_OPTPERT_RESPONSE for the present batch width, zeroed; on = 0
 *    frees everything these entry points hold.  FC_ERR_NOT_READY without fc_set_adjoint_batch on a slot, or with a batched adjoint
 *    setup that is not current; FC_ERR_INVALID with the reason on a nonlinear time scheme and on everything fc_set_adjoint_batch
 *    refuses.  Dropped by whatever drops the batch (fc_set_batch, fc_set_bc with other dofs) and by a new permutation.
 *    fc_optpert_load / _get: host <-> a block; load zeroes every row outside f.
 *    fc_optpert_apply: G = K U from block U into block G, H_out [k][k] = U^T G (not symmetrised), E_out [k] = 1/2 x_n,c^T M x_n,c, the
 *    response block = x_n.  n_steps batched steps with zero controls and the backward march are enqueued back to back; one
 *    synchronisation at the end.  It OVERWRITES the batch's state ring, which afterwards holds the run's last two states, and ends
 *    batched state and loop tapes exactly as fc_set_state_batch does.  FC_ERR_INVALID with nothing enqueued: energy weights held
 *    (fc_set_adjoint_energy; the march would add them), n_steps < 1, k other than the batch's, a nonlinear scheme, and whatever
 *    fc_step_batch and fc_run_adjoint_batch refuse on the slots of the run.  A column that went non-finite is marked in flags_out
 *    [k] and the call returns FC_ERR_DIVERGED; the other columns are valid.
 *    fc_optpert_mass_solve: the block CG between two resident blocks (dst != src).  fc_optpert_gram: out [k][k] = A^T B (weighted = 0)
 *    or A^T M B; fixed summation order, a repeated call returns the same bits.  fc_optpert_combine: dst = src Q diag(scale) for a
 *    k x k Q (scale NULL: none), dst != src, padding columns stay zero; accumulate = 1 adds the product onto dst (the residual
 *    block R = V S - U S Theta is two calls, so it is formed as a block and not from Gram entries).
 *    fc_optpert_info: info[8] = reserved, tables stale, device bytes, KB, applies so far, CG iterations of the last solve (max over the
 *    columns), forward steps and backward steps enqueued by the last apply; dinfo[2] = HIP-event ms of the last apply, of the last
 *    mass solve. */
#define FC_OPTPERT_U 0
#define FC_OPTPERT_G 1
#define FC_OPTPERT_V 2
#define FC_OPTPERT_R 3
#define FC_OPTPERT_SCRATCH 4
#define FC_OPTPERT_RESPONSE 5
int fc_mass_solve_batch(fc_handle h, int32_t k, const double* b, double* x, double rtol, int32_t max_iter, double* info /* [k][2] */);
int fc_optpert_reserve(fc_handle h, int32_t on);
int fc_optpert_load(fc_handle h, int32_t block, int32_t k, const double* X);
int fc_optpert_get(fc_handle h, int32_t block, int32_t k, double* out);
int fc_optpert_apply(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, double* H_out, double* E_out, int32_t* flags_out);
int fc_optpert_mass_solve(fc_handle h, int32_t dst_block, int32_t src_block, double rtol, int32_t max_iter, double* info /* [k][2] */);
int fc_optpert_gram(fc_handle h, int32_t a_block, int32_t b_block, int32_t weighted, double* out);
int fc_optpert_combine(fc_handle h, int32_t dst_block, int32_t src_block, const double* Q, const double* scale, int32_t accumulate);
int fc_optpert_info(fc_handle h, int64_t* info /* [8] */, double* dinfo /* [2] */);

/* ── tangent-linear march: Jacobian-vector products of a NONLINEAR run (csrc/fc_tangent.hip.h, csrc/fc_tangent_run.hpp).
 *    The exact tangent of the taped forward run (fc_adjoint_tape_reserve / _begin, then fc_run; batched: fc_adjoint_tape_reserve_batch /
 *    _begin_batch, then fc_step_batch), step j on the order slot and with the coefficients of forward step j:
 *        A_s dx_j = Z [ M (cm_n dx_{j-1} + cm_nn dx_{j-2}) + cc_n J(x_{j-1}) dx_{j-1} + cc_nn J(x_{j-2}) dx_{j-2} ] + B~ du_j,   dy_j = C dx_j
 *    J(x) d = the directional derivative of the convective load vector, both halves ((d.grad)u + (u.grad)d), taken at the state the
 *    forward step READ (tape columns j and j - 1); dx is read unmasked, Z sits on the output rows; B~ du is what a forward step adds
 *    for u = du (Dirichlet profiles, lifting, body-force load vectors).  The sweeps run on the slot's DIRECT factors with the
 *    handle's refinement sweeps, as in a forward step: no transposed export is needed.
 *    fc_tangent_reserve(on = 1): the march's own buffers for the present mode -- single, or the batch's width KB (two tangent levels,
 *    work buffer, right-hand side, element vectors; the du / dy sequences grow with the longest march); on = 0 frees them.  The march
 *    leaves the state ring, the step counter, the snapshot bank, the loop cursor, the tapes, the batch's ring and its record pages
 *    untouched; a handle that never reserves allocates nothing, launches nothing more and returns the bits it returned before.
 *    Dropped by fc_set_batch (the mode ends), by fc_set_bc with other dofs (a new structure) and by a new permutation.  The single
 *    march stages its state vectors through the handle's scratch vectors, like every call behind a quiesce.
 *    fc_run_tangent: du_seq [n][n_act], dx0 / dxm1 [N] in the W layout (NULL: zero; their pressure rows are never read), dy_seq
 *    [n][n_sens], dxn / dxnm1 [N] = dx_n, dx_{n-1} (any may be NULL).  All steps are enqueued behind one quiesce, one synchronisation
 *    at the end.  fc_run_tangent_batch: the same for the k columns of fc_set_batch, du_seq [n][k][n_act], dx0 / dxm1 / dxn / dxnm1
 *    [k][N], dy_seq [n][k][n_sens]; ref_col = -1: column s perturbs trajectory s of the batched tape; ref_col = c in [0, k): every
 *    column perturbs trajectory c (k directions about one base flow).  Columns never mix; padding columns reach no output.
 *    A partitioned handle is refused first (FC_ERR_INVALID), by the reserve too.  FC_ERR_NOT_READY without a reserve (or a reserve
 *    for another mode / width).  FC_ERR_INVALID with the reason and nothing enqueued:
 *    a linearised time scheme (its forward run is its own tangent); no dense state tape, or one that does not hold exactly this run
 *    (step count, first slot, overflowed, ended, not begun); a checkpointed tape (a tangent over it is not built); ref_col outside
 *    [-1, k); k other than the batch's; a step in flight; partitioned handles; Crank-Nicolson slots; a Krylov method, factor-free,
 *    truncated or inexact slots (the march applies the direct factors); whatever fc_run (single) or fc_step_batch (batched) refuse on
 *    the slots of the run.  FC_ERR_DIVERGED for a non-finite tangent state: the batched march marks the column in flags_out [k], the
 *    other columns are valid.
 *    fc_tangent_info: info[8] = reserved, KB (0: single), device bytes, steps of the last march, its element kernel (1 fc_tan_elem_nl,
 *    2 fc_tan_elem_nl_reg, 3 fc_tan_elem_nl_b, 4 fc_tan_elem_nl_b with a shared reference column), marches so far, 0, 0;
 *    dinfo[2] = HIP-event ms of the last march's steps, 0. */
int fc_tangent_reserve(fc_handle h, int32_t on);
int fc_run_tangent(fc_handle h, int first_order_slot, int32_t n_steps, const double* du_seq, const double* dx0, const double* dxm1,
                   double* dy_seq, double* dxn, double* dxnm1);
int fc_run_tangent_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, int32_t ref_col, const double* du_seq,
                         const double* dx0, const double* dxm1, double* dy_seq, double* dxn, double* dxnm1, int32_t* flags_out /* [k] */);
int fc_tangent_info(fc_handle h, int64_t* info /* [8] */, double* dinfo /* [2] */);

/* ── tangent of a CLOSED loop: Jacobian-vector products of the controller problem (csrc/fc_tangent_loop.hip.h,
 *    csrc/fc_tangent_loop_run.hpp; DESIGN §5.6 "Closed loop").  The exact tangent of the taped closed-loop run (fc_adjoint_loop_reserve /
 *    _begin, then fc_run_closed_loop; batched: the _batch calls) along a direction
 *        (dAd, dBd, dC, dD, dG, dg0, dS, dxi_0, dy_0, dw_y[n], dw_u[n], dx_0, dx_{-1}),
 *    step m = 1 .. n, ahead of the plant's tangent step m (fc_run_tangent's, unchanged, on the control row du_m):
 *        dyc_m = G dy_{m-1} + dG y_{m-1} + dg0 + dw_y[m]              duc_m = C dxi_{m-1} + dC xi_{m-1} + D dyc_m + dD yc_m
 *        dxi_m = Ad dxi_{m-1} + dAd xi_{m-1} + Bd dyc_m + dBd yc_m    dv_m = S duc_m + dS uc_m + dw_u[m]      du_m = sigma_m o dv_m
 *    sigma_m = 1 where u_lo < v_m < u_hi (the taped unclamped control; the mask of fc_run_adjoint_closed_loop), else 0; all 1 without
 *    limits.  xi_{m-1}, y_{m-1}, v_m come from the loop tape; yc_m, uc_m are formed again from them with the forward kernel's sums.
 *    The matrices are row-major in the shapes fc_set_controllers takes, dxi0 [nx], dy0 [n_sens], dw_y [n][nyc], dw_u [n][n_act], dx0 /
 *    dxm1 [N] (W layout); any input may be NULL (zero).  Outputs, any may be NULL: dy_seq [n][n_sens], du_seq [n][n_act] (exactly 0
 *    where a limit holds the control), dxi_n [nx], dxn / dxnm1 [N].  fc_tangent_reserve comes first; the direction's device copies are
 *    sized inside the call and freed with the reserve (fc_tangent_info's bytes count them).  The march writes none of: state ring,
 *    controller state, loop cursor, tapes, step counter.
 *    fc_run_tangent_closed_loop_batch: the same for the k loops of fc_run_closed_loop_batch, every array with a leading k behind the
 *    step index (dAd [k][nx][nx] .. dw_u [n][k][n_act], dx0 [k][N]); ref_col = -1: column s is the tangent of loop s; ref_col = c:
 *    every column is a tangent of loop c (its bank block, tape rows, signal rows, limits and trajectory) along its own direction.
 *    A LINEARISED time scheme is accepted (with clamps, affine terms and parameter directions the loop's tangent is not its forward
 *    run): the march then reads the loop tape alone.  A nonlinear scheme needs the dense state tape of the same run as well.
 *    FC_ERR_NOT_READY without tangent buffers or without a loop tape.  FC_ERR_INVALID with the reason and nothing enqueued: a loop
 *    tape that does not hold exactly this run (its own reason: step count, first slot, overflowed, ended, not begun, non-finite); a
 *    bank whose k is not the call's; on a nonlinear scheme a missing, checkpointed or other state tape; partitioned handles; a step
 *    in flight; Crank-Nicolson slots; a Krylov method, factor-free, truncated or inexact slots.  FC_ERR_DIVERGED for a non-finite
 *    tangent state; the batched march marks in flags_out [k] every column whose forward run or tangent went non-finite and fills its
 *    outputs with NaN -- the other columns are valid. */
int fc_run_tangent_closed_loop(fc_handle h, int first_order_slot, int32_t n_steps, const double* dAd, const double* dBd, const double* dC,
                               const double* dD, const double* dG, const double* dg0, const double* dS, const double* dxi0, const double* dy0,
                               const double* dw_y, const double* dw_u, const double* dx0, const double* dxm1, double* dy_seq, double* du_seq,
                               double* dxi_n, double* dxn, double* dxnm1);
int fc_run_tangent_closed_loop_batch(fc_handle h, int first_order_slot, int32_t k, int32_t n_steps, int32_t ref_col, const double* dAd,
                                     const double* dBd, const double* dC, const double* dD, const double* dG, const double* dg0, const double* dS,
                                     const double* dxi0, const double* dy0, const double* dw_y, const double* dw_u, const double* dx0,
                                     const double* dxm1, double* dy_seq, double* du_seq, double* dxi_n, double* dxn, double* dxnm1,
                                     int32_t* flags_out /* [k] */);

/* ── tangent of the ENERGY: d(dE_m) = x_m^T M_s dx_m, the directional derivative of the perturbation kinetic energy every forward step
 *    logs, for m = 1 .. n (csrc/fc_tangent_energy.hip.h, csrc/fc_tangent_energy_run.hpp; DESIGN §5.6 "Energy").  M_s: the symmetric
 *    velocity mass matrix, evaluated by the quadrature of the step tail's energy cells on the taped state x_m and the tangent level the
 *    step has just written -- neither masked: dE integrates the whole velocity field, actuated Dirichlet values included.
 *    fc_tangent_set_energy(on = 1): every later tangent march of the handle (fc_run_tangent, _batch, fc_run_tangent_closed_loop, _batch)
 *    enqueues one energy launch behind each step's tail and one fold behind the last step; on = 0 frees the rows.  Needs
 *    fc_tangent_reserve (FC_ERR_NOT_READY) and goes with the reserve when it is freed or laid out again.  The partials
 *    [n][G][max(1, KB)] and the rows [n][max(1, k)] are sized inside the marches and counted in fc_tangent_info's bytes.  A handle that
 *    never sets the option allocates nothing and its marches enqueue what they enqueued before.  With the option a LINEARISED closed-loop
 *    march reads the dense state tape too (x_m): without a tape that holds the run it is refused with the reason, nothing enqueued.
 *    fc_get_tangent_energy: the rows of the last march, dde [n] (k = 0: a single march) or [n][k].  FC_ERR_NOT_READY if the last march
 *    ran without the option or failed, FC_ERR_INVALID if n_steps / k are not the last march's.  A column of a batched march that
 *    FC_ERR_DIVERGED marks holds whatever its non-finite states gave; the other columns are valid.  No device work.
 *    fc_tangent_energy_info: info[8] = option on, the last march ran the energy launches, its kernel (1 fc_tan_energy,
 *    2 fc_tan_energy_b<KB, false>, 3 fc_tan_energy_b<KB, true>), workgroups per launch G, n_steps, k, energy launches of the march,
 *    device bytes of the partials and the rows.  FC_ERR_INVALID on partitioned handles (fc_tangent_set_energy), null arguments. */
int fc_tangent_set_energy(fc_handle h, int32_t on);
int fc_get_tangent_energy(fc_handle h, int32_t n_steps, int32_t k, double* dde);
int fc_tangent_energy_info(fc_handle h, int64_t* info /* [8] */);

/* ── Gauss-Newton products of the energy cost sum_m e_m dE_m:  H_E v = sum_m e_m X_m^T M_s X_m v,  X_m = d x_m / d theta  (DESIGN §5.6
 *    "Energy").  One tangent march that KEEPS dx_m, then one adjoint march whose energy forcing of backward step m is e_m M_s dx_m
 *    instead of e_m M_s x_m.
 *    fc_tangent_tape_reserve(n_steps): the tangent tape, n_steps columns of N doubles (0 frees).  Single marches only: FC_ERR_INVALID on
 *    a handle with a batch set and on partitioned handles; it goes with fc_set_batch, a new permutation or structure, not with
 *    fc_tangent_reserve.  Every later fc_run_tangent / fc_run_tangent_closed_loop of n <= n_steps steps copies each new level into
 *    column m - 1 (the solver's numbering, 8 N bytes per step) and records its step count and first slot; a longer or failed march
 *    leaves the tape empty.  A refused reserve leaves an existing tape and the source as they are.  The tape records the step count
 *    and the first slot of its march, nothing else: a tape left from an EARLIER run of the same length and order is not told apart --
 *    march the tangent over the state tape's run before marching back with source 1.  fc_tangent_tape_info: info[8] = capacity, steps held, first slot of that march (-1: none), device bytes.
 *    fc_set_adjoint_energy_source(source): 0 (default) the weights of fc_set_adjoint_energy multiply the state tape's x_m; 1 they
 *    multiply the tangent tape's dx_m, in fc_run_adjoint and fc_run_adjoint_closed_loop, while J(x_m)^T still reads the state tape.
 *    A march with rows held and source 1 is refused (FC_ERR_INVALID, the reason, nothing enqueued) unless the tangent tape holds a
 *    march of exactly its n_steps and first slot; the batched marches, fc_step_adjoint and checkpointed state tapes refuse source 1.
 *    The source falls back to 0 when the rows are cleared (fc_set_adjoint_energy(h, 0, 0, NULL)) and when the tangent tape is freed;
 *    fc_adjoint_energy_info [5] reports it. */
int fc_tangent_tape_reserve(fc_handle h, int32_t n_steps);
int fc_tangent_tape_info(fc_handle h, int64_t* info /* [8] */);
int fc_set_adjoint_energy_source(fc_handle h, int32_t source);

/* ── multi-GPU (one process per GPU): replaces dolfin's MPI mesh partitioning
 *    (flowsolver.py:236-238) and PETSc/MUMPS' internal MPI.  Each rank holds the whole (small)
 *    discretisation but assembles only its cells and sweeps only its sub-tree of the elimination
 *    tree; rowkind[N] (W numbering): 0 = other rank's dof, 1 = owned, 2 = root separator (replicated).
 *    Exchange steps per step (all-reduces over RCCL/xGMI, or fc_set_host_exchange): the root right-hand side and the
 *    root solution (every rank applies its block of the root's rows) inside the solve, and the 80-double step
 *    tail (sensor partials, energy, residual norms, divergence flag). */
int fc_comm_unique_id(char* out128 /* ncclUniqueId bytes, made on rank 0 and broadcast by the host */);
int fc_comm_init(fc_handle h, int nranks, int rank, const char* id128);
/* fc_comm_probe: can this rank load RCCL at all?  Every rank calls it BEFORE fc_comm_init and the ranks agree on the outcome over
 * their own process group: ncclCommInitRank is a collective, so a rank that cannot load RCCL must not leave the others waiting in it.
 * fc_comm_destroy: give the communicator back (mixed outcome of fc_comm_init: everybody then uses fc_set_host_exchange). */
int fc_comm_probe(int rank);
int fc_comm_destroy(fc_handle h);
/* Exchange through the host for a partitioned handle that has NO RCCL communicator (several ranks on one GPU,
 * CPU-only collectives such as gloo): `fn(buf, n, user)` must sum the n doubles of `buf` over the ranks, in place.
 * The launch sequence of a step is the one of the RCCL path; only the exchange itself differs (device -> pinned
 * host buffer -> fn -> device instead of an in-stream ncclAllReduce).  Three exchanges per step: the root
 * right-hand side, the root solution (row blocks), the 80-double step record. */
/* what the handle's exchange is: transport 0 = none, 1 = RCCL (nranks / rank READ BACK from the communicator with
 * ncclCommCount / ncclCommUserRank), 2 = host callback */
int fc_comm_info(fc_handle h, int32_t* nranks, int32_t* rank, int32_t* transport);
typedef void (*fc_exchange_fn)(double* buf, int64_t n, void* user);
int fc_set_host_exchange(fc_handle h, int nranks, int rank, fc_exchange_fn fn, void* user);
/* Pre-flight of the handle's exchange (call on EVERY rank after fc_comm_init / fc_set_host_exchange, before any setup): one
 * all-reduce of a known vector (entry i of rank r = (r + 1) * (i + 1), 256 doubles) through the very path the time steps use
 * (in-stream ncclAllReduce, or the host callback), checked entry by entry against nranks (nranks + 1) / 2 * (i + 1).
 * FC_ERR_HIP with the first wrong entry in fc_last_error() on a mismatch: a communicator that connects the wrong ranks, a
 * callback that does not sum, a second HIP runtime in the process.  max_err_out (optional): largest deviation seen.
 * Replaces nothing in the reference (MPI_Init's own checks, src/utils/mpi.py:22-37). */
int fc_comm_selftest(fc_handle h, double* max_err_out);


#ifdef __cplusplus
}
#endif
#endif /* FC_HIP_H */
