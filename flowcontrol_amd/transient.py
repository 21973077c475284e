"""Optimal initial perturbations and transient growth ``G(T) = max |x(T)|^2_M / |x(0)|^2_M`` of the linearised stepper by batched
direct-adjoint loops (csrc/fc_optpert.hip.h; device extension, not in the reference).

With ``x_n = Phi x_0`` the run of n steps with zero controls from ``x_0`` (``x_{-1} = 0``, first step on ``first_order``, the rest BDF2),
f the free velocity rows and M the velocity mass matrix, the k leading optimal perturbations are the leading eigenpairs of

    K v = theta M_ff v,        K = P_f Phi^T M Phi P_f

and come from one subspace iteration on an M-orthonormal block U (N x k).  One iteration:

    G = K U  (one batched forward run, one batched backward march),   H = sym(U^T G) = S Theta S^T  (theta descending)
    V = M_ff^-1 G  (block CG),   R = V S - U S Theta,   res_i = |R_i|_M / theta_0
    stop when max_{i < n_modes} res_i <= tol, else  U <- cholqr_M(cholqr_M(V S Theta^-1))

The modes returned are ``U S`` of the last iteration and theta their exact Rayleigh quotients: ``theta_i = dE_n / dE_0`` of a forward
run from mode i holds at every iteration.  Only k x k matrices and k-vectors cross to the host inside an iteration.

The iteration (:func:`subspace_iteration`) is written once against a block backend -- ``load, get, apply, mass_solve, gram, combine``
on the named blocks U, G, V, R, S, Y; :class:`DeviceBlocks` is the device's (``fc_optpert_*``), the tests run it on a numpy model.

A plain subspace iteration converges at the rate ``theta_k / theta_i``: short horizons with clustered gains need many iterations (no
block Krylov acceleration here).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS

#: block-CG iterations allowed per mass solve (Jacobi-preconditioned P2 mass matrices need a few dozen)
MASS_MAX_ITER = 500


@dataclass
class OptimalPerturbations:
    gains: np.ndarray        # [n_modes] energy gains theta_i = dE_n / dE_0, descending
    modes: np.ndarray        # [n_modes, N] optimal initial perturbations, v^T M v = 1
    responses: np.ndarray    # [n_modes, N] Phi v_i
    residuals: np.ndarray    # [n_modes] |R_i|_M / theta_0 of the last iteration
    iterations: int
    history: list = field(default_factory=list)  # theta [k] of every iteration
    converged: bool = False
    block: np.ndarray | None = None  # [k, N] all k Ritz vectors of the last iteration (a warm start for a neighbouring horizon)
    n_steps: int = 0


def default_width(n_modes: int) -> int:
    """``max(4, 2 n_modes)`` rounded up to 4, 8, 16 or 32."""
    want = max(4, 2 * int(n_modes))
    return next(w for w in (4, 8, 16, 32) if w >= min(want, 32))


def check_arguments(n_steps, n_modes, k, tol, max_iter, first_order) -> int:
    """The argument checks of :func:`optimal_perturbations`; returns the block width."""
    if int(n_steps) < 1:
        raise ValueError(f"n_steps must be at least 1, got {n_steps!r}")
    if not 1 <= int(n_modes) <= 16:
        raise ValueError(f"n_modes must be in [1, 16], got {n_modes!r}")
    k = default_width(n_modes) if k is None else int(k)
    if not int(n_modes) <= k <= 32:
        raise ValueError(f"k must be in [n_modes, 32] = [{int(n_modes)}, 32], got {k}")
    if not tol > 0.0:
        raise ValueError(f"tol must be positive, got {tol!r}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter!r}")
    if first_order not in (None, 1, 2):
        raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
    return k


def _cholqr(be, dst: str, src: str, what: str) -> None:
    """``dst = src L^-T`` with ``L L^T = sym(src^T M src)``."""
    W = be.gram(src, src, True)
    W = 0.5 * (W + W.T)
    try:
        L = np.linalg.cholesky(W)
    except np.linalg.LinAlgError as e:
        raise RuntimeError(f"optimal_perturbations: the Gram matrix of the block is not positive definite ({what}): {e}") from None
    be.combine(dst, src, np.linalg.inv(L).T)


def orthonormalise_start(be, X0) -> None:
    """Block U <- two M-Cholesky-QR passes over ``X0`` (k, N) masked to the free rows."""
    be.load("S", X0)
    _cholqr(be, "R", "S", "start block")
    _cholqr(be, "U", "R", "start block")


def subspace_iteration(be, n_steps: int, n_modes: int = 1, tol: float = 1e-6, max_iter: int = 50, first_order: int = 1,
                       mass_rtol: float = 1e-12) -> OptimalPerturbations:
    """The iteration of the module docstring on the backend's M-orthonormal block U."""
    k = be.k
    history, res, theta, S = [], None, None, None
    converged = False
    for it in range(1, int(max_iter) + 1):
        H, _ = be.apply(int(n_steps), int(first_order))
        H = 0.5 * (H + H.T)
        if not np.all(np.isfinite(H)):
            raise RuntimeError(f"optimal_perturbations: non-finite Rayleigh matrix in iteration {it}")
        theta, S = np.linalg.eigh(H)
        theta, S = theta[::-1].copy(), np.ascontiguousarray(S[:, ::-1])
        history.append(theta.copy())
        if theta[-1] <= 0.0:
            raise RuntimeError(f"optimal_perturbations: non-positive gain {theta[-1]:.3e} in the block in iteration {it} "
                               "(the block has lost rank, or the run does not reach every direction of it)")
        be.mass_solve("V", "G", mass_rtol)
        be.combine("R", "V", S)
        be.combine("R", "U", -S * theta[None, :], accumulate=True)
        res = np.sqrt(np.maximum(np.diag(be.gram("R", "R", True)), 0.0)) / theta[0]
        converged = bool(np.max(res[:n_modes]) <= tol)
        if converged or it == int(max_iter):
            break
        be.combine("S", "V", S, scale=1.0 / theta)
        _cholqr(be, "R", "S", f"iteration {it}")
        _cholqr(be, "U", "R", f"iteration {it}")
    be.combine("V", "U", S)  # the Ritz vectors ...
    be.combine("G", "Y", S)  # ... and their responses (Y = Phi U of the last apply)
    modes, resp = be.get("V"), be.get("G")
    return OptimalPerturbations(gains=theta[:n_modes].copy(), modes=modes[:n_modes].copy(), responses=resp[:n_modes].copy(), residuals=res[:n_modes].copy(),
                                iterations=it, history=history, converged=converged, block=modes, n_steps=int(n_steps))


class DeviceBlocks:
    """The block backend on a device handle with :meth:`DeviceSolver.optpert_reserve` done."""

    def __init__(self, dev):
        self.dev, self.k, self.N = dev, dev.batch_k, dev.N
        #: the free velocity rows f (W layout): velocity dofs outside the handle's Dirichlet list
        self.free = np.setdiff1d(np.arange(2 * dev.nn), np.asarray(dev.bc_dofs, dtype=np.int64))

    def load(self, block, X):
        self.dev.optpert_load(block, X)

    def get(self, block):
        return self.dev.optpert_get(block)

    def apply(self, n_steps, first_order):
        return self.dev.optpert_apply(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n_steps)

    def mass_solve(self, dst, src, rtol):
        return self.dev.optpert_mass_solve(dst, src, rtol, MASS_MAX_ITER)

    def gram(self, a, b, weighted=False):
        return self.dev.optpert_gram(a, b, weighted)

    def combine(self, dst, src, Q, scale=None, accumulate=False):
        self.dev.optpert_combine(dst, src, Q, scale, accumulate)


def _refuse_nonlinear(fs) -> None:
    if fs is not None and fs.params_solver.is_eq_nonlinear:
        raise ValueError("optimal_perturbations: is_eq_nonlinear=True -- optimal perturbations are those of the linearised stepper: build the "
                         "solver with is_eq_nonlinear=False")


class _Setup:
    """What :func:`optimal_perturbations` needs on the solver it is given -- batch, transposed factors, batched adjoint, mass slot,
    resident blocks -- and its release, as :class:`flowcontrol_amd.adjoint.AdjointRun`."""

    def __init__(self, fs_or_bfs, k: int):
        from .adjoint import AdjointRun, _is_batched
        from .batch import BatchedFlowSolver

        self.own_batch = None
        _refuse_nonlinear(fs_or_bfs.fs if _is_batched(fs_or_bfs) else fs_or_bfs)  # (first: nothing is set up on a solver that is refused)
        if _is_batched(fs_or_bfs):
            bfs = fs_or_bfs
            if bfs.k != k:
                raise ValueError(f"optimal_perturbations: the BatchedFlowSolver has k = {bfs.k}, the block k = {k}")
        else:
            bfs = self.own_batch = BatchedFlowSolver(fs_or_bfs, k)
        self.bfs = bfs
        self.adj = None
        try:
            self.adj = AdjointRun(bfs)
            self.dev = dev = self.adj.dev
            dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
            dev.optpert_reserve(True)
        except Exception:
            self.close()
            raise

    def close(self) -> None:
        try:
            if getattr(self, "dev", None) is not None:
                self.dev.optpert_reserve(False)
        finally:
            try:
                if self.adj is not None:
                    self.adj.close()
            finally:
                if self.own_batch is not None:
                    self._release_batch()

    def _release_batch(self) -> None:
        # the batch this call set up goes, and the handle's solver options go back to the single run's (fc_set_solver_options)
        bfs, fs = self.own_batch, self.own_batch.fs
        bfs.close()
        dev = fs.th.device()
        every = -1 if fs.check_residual_every is None else fs.check_residual_every
        dev.set_solver_options(refine=fs.refine_steps, check_residual=every)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def optimal_perturbations(fs_or_bfs, n_steps: int, n_modes: int = 1, k: int | None = None, tol: float = 1e-6, max_iter: int = 50, x0=None, seed: int = 0,
                          first_order: int | None = None, mass_rtol: float = 1e-12) -> OptimalPerturbations:
    """The ``n_modes`` leading optimal initial perturbations of the linearised ``FlowSolver`` (or of the solver a
    ``BatchedFlowSolver`` shares) over ``n_steps`` steps and their energy gains, by subspace iteration on a block of ``k`` columns
    (default ``max(4, 2 n_modes)`` rounded up to 4, 8, 16 or 32).  ``x0`` (k, N): start block (masked to the free velocity rows and
    M-orthonormalised); default: seeded random.  ``first_order``: order of the first step (default 1: a run from ``x_{-1} = 0`` starts
    on the first-order step, as ``FlowSolver.initialize_time_stepping`` does).  Everything set up on the solver is released before it returns."""
    from .adjoint import _is_batched

    if _is_batched(fs_or_bfs) and k is None:
        k = fs_or_bfs.k
    k = check_arguments(n_steps, n_modes, k, tol, max_iter, first_order)
    with _Setup(fs_or_bfs, k) as st:
        be = DeviceBlocks(st.dev)
        X0 = start_block(k, be.N, x0, seed, be.free)
        orthonormalise_start(be, X0)
        return subspace_iteration(be, n_steps, n_modes, tol, max_iter, first_order or 1, mass_rtol)


def start_block(k: int, N: int, x0, seed: int, free) -> np.ndarray:
    """The start block (k, N): ``x0``, or seeded random on the free velocity rows ``free`` (drawn as the |f| x k matrix U_f)."""
    if x0 is None:
        free = np.asarray(free)
        X0 = np.zeros((k, N))
        X0[:, free] = np.random.default_rng(seed).standard_normal((free.size, k)).T
        return X0
    X0 = np.asarray(x0, dtype=np.float64)
    if X0.shape != (k, N):
        raise ValueError(f"x0 must be ({k}, {N}), got {X0.shape}")
    return X0


def transient_growth(fs, horizons, n_modes: int = 1, k: int | None = None, tol: float = 1e-6, max_iter: int = 50, seed: int = 0,
                     first_order: int | None = None, mass_rtol: float = 1e-12):
    """The gain curve ``G(T)``: ``(gains [len(horizons), n_modes], results)`` for the step counts ``horizons``; every horizon is
    warm-started from the previous horizon's block.  One setup serves all horizons."""
    from .adjoint import _is_batched

    horizons = [int(n) for n in horizons]
    if not horizons:
        raise ValueError("transient_growth: no horizons")
    if _is_batched(fs) and k is None:
        k = fs.k
    k = check_arguments(min(horizons), n_modes, k, tol, max_iter, first_order)
    results = []
    with _Setup(fs, k) as st:
        be = DeviceBlocks(st.dev)
        block = None
        for n in horizons:
            orthonormalise_start(be, start_block(k, be.N, block, seed, be.free))
            results.append(subspace_iteration(be, n, n_modes, tol, max_iter, first_order or 1, mass_rtol))
            block = results[-1].block
    return np.array([r.gains for r in results]), results


def mass_solve(fs_or_dev, b, rtol: float = 1e-12, max_iter: int = MASS_MAX_ITER) -> np.ndarray:
    """``M_ff^-1 b_f`` on the free velocity rows, zero elsewhere, for one vector (N,) or a block (k <= 32, N) on the device
    (``fc_mass_solve_batch``): the L2 projection of the reference's ``projectm`` (``utils/fem.py``) for right-hand sides already
    assembled against the velocity test functions.  ``fs_or_dev``: a ``FlowSolver`` or a ``DeviceSolver`` with a solver set up; a
    batch set on the handle is replaced and released."""
    fs = fs_or_dev if hasattr(fs_or_dev, "params_solver") else None
    if fs is not None:
        fs._begin_stepping()
        fs._flush_log()
        dev = fs.th.device()
    else:
        dev = fs_or_dev
    B = np.asarray(b, dtype=np.float64)
    single = B.ndim == 1
    B = np.atleast_2d(B)
    if B.shape[0] > 32 or B.shape[1] != dev.N:
        raise ValueError(f"mass_solve: b must be ({dev.N},) or (k <= 32, {dev.N}), got {np.shape(b)}")
    dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
    dev.set_batch(B.shape[0])
    try:
        x, _ = dev.mass_solve_batch(B, rtol, max_iter)
    finally:
        dev.optpert_reserve(False)
        dev.set_batch(0)
    return x[0] if single else x
