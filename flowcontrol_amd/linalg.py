"""Linear analysis of the state-space operators ``E dq/dt = A q + B u, y = C q`` on the device: frequency responses and
shift-invert eigenvalues.  Mirror of the reference's ``src/utils/linalg.py`` (``get_frequency_response_sequential`` /
``_parallel`` / ``_mpi``, ``get_field_response``, ``get_mat_vp_slepc``): same names, same argument order, same return shapes, so
that ``examples/operators/compute_frequency_response.py`` and ``compute_eigenvalues.py`` port by changing their imports.  The one
addition is the keyword ``flowsolver=``: the solver whose handle hosts the computation (its CSR pattern is the one A and E live on).

Every complex-shifted operator ``sigma E - A`` is factorised on the MI355X by the complex-shifted direct solver of the handle
(``fc_setup_shifted``: the real-equivalent system through the multifrontal kernels of the real solver), in a structure
of its own: the handle's time-stepping operators, factors and state are not touched.  There is no host fall-back.

    H(i w) = C (i w E - A)^-1 B          one numeric factorisation per frequency, nu solves, C X formed on the device
    A v = lambda E v, lambda near sigma   Krylov-Schur on Op = (A - sigma E)^-1 E, basis on the device, m x m work in numpy

Opt-in: ``pressure_pin=`` runs the same analysis on enclosed flows (lid-driven cavity; a diagonal shift on one pressure dof inside
the shifted factorisation), ``krylov=`` turns on the device's complex GMRES preconditioned by the held factors (rescue of a solve
whose refinement stalls), and ``refactor_every=n`` factorises only every n-th frequency of a sweep and solves the ones in between
by that GMRES on the lagged factors.
"""

from __future__ import annotations

import ctypes as C
import logging
import time
from typing import Any

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from . import _lib
from ._lib import check

logger = logging.getLogger(__name__)

#: keyword arguments of the reference's get_mat_vp_slepc that only configure SLEPc / PETSc: accepted, logged, ignored
_SLEPC_ONLY = ("eps_type", "precond_type", "ksp_type", "mpd")


# ── matrices onto the handle's pattern ──────────────────────────────────────────────────────────────────────────────────────────
def _as_csr(M, name: str, n: int | None = None) -> sp.csr_matrix:
    if not sp.issparse(M):
        raise TypeError(f"{name} must be a scipy sparse matrix, got {type(M).__name__}")
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sum_duplicates()
    if M.shape[0] != M.shape[1]:
        raise ValueError(f"{name} must be square, got shape {M.shape}")
    if n is not None and M.shape[0] != n:
        raise ValueError(f"{name} has order {M.shape[0]}, the flowsolver's mixed space has {n} dofs")
    return M


def values_on_pattern(M: sp.csr_matrix, rowptr: np.ndarray, colidx: np.ndarray, name: str = "matrix") -> np.ndarray:
    """Values of ``M`` on the CSR pattern (rowptr, colidx); ValueError if a nonzero of ``M`` lies outside it."""
    n = rowptr.size - 1
    M = _as_csr(M, name, n).tocoo()
    keep = M.data != 0.0
    r, c, v = M.row[keep].astype(np.int64), M.col[keep].astype(np.int64), M.data[keep]
    pkeys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + colidx.astype(np.int64)
    keys = r * n + c
    pos = np.searchsorted(pkeys, keys)
    pos_c = np.minimum(pos, pkeys.size - 1)
    bad = (pos >= pkeys.size) | (pkeys[pos_c] != keys)
    if np.any(bad):
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{name} has {int(bad.sum())} nonzero(s) outside the flowsolver's CSR pattern (first at ({r[i]}, {c[i]}))")
    vals = np.zeros(pkeys.size)
    np.add.at(vals, pos, v)
    return vals


def _sparse_rows(Cm: np.ndarray):
    """Rows of a dense / sparse output matrix as CSR arrays (rowptr, idx, w) of their nonzeros."""
    Cs = sp.csr_matrix(Cm, dtype=np.float64)
    Cs.eliminate_zeros()
    rp = np.ascontiguousarray(Cs.indptr, dtype=np.int32)
    idx = np.ascontiguousarray(Cs.indices if Cs.nnz else np.zeros(1), dtype=np.int32)
    w = np.ascontiguousarray(Cs.data if Cs.nnz else np.zeros(1), dtype=np.float64)
    return rp, idx, w


#: GMRES settings of ``krylov=True``
KRYLOV_DEFAULTS = {"max_iter": 200, "restart": 60, "rtol": 1e-10}


def _krylov_settings(krylov) -> dict | None:
    if krylov is None or krylov is False:
        return None
    kw = dict(KRYLOV_DEFAULTS)
    if krylov is not True:
        extra = set(krylov) - set(kw)
        if extra:
            raise TypeError(f"krylov=: unexpected keys {sorted(extra)} (known: {sorted(kw)})")
        kw.update(krylov)
    return kw


class ShiftedOperator:
    """``sigma E - A`` on the device of ``flowsolver`` (``fc_setup_shifted`` and friends).  ``A`` and ``E`` are copied onto the
    handle's CSR pattern once; :meth:`factor` redoes the numeric factorisation for a new sigma.

    ``pressure_pin``: ``None`` refuses enclosed flows (sigma E - A is singular there); ``"auto"`` pins the pressure dof the
    flowsolver's own time stepping pins (``fem.boundary.pressure_pin``), an int names one: the operator is then
    ``sigma E - A + pin_shift e_k e_k^T``, whose finite eigenvalues do not depend on ``pin_shift``.
    ``krylov``: ``None`` off; ``True`` or a dict of ``max_iter``, ``restart``, ``rtol`` turns the device GMRES on
    (``fc_shifted_set_krylov``); :meth:`shift` then moves sigma without refactorising.  ``last_iterations``: GMRES iterations of
    the columns of the last solve (zeros when none was needed)."""

    def __init__(self, flowsolver, A, E, refine: int = 2, pressure_pin=None, krylov=None, pin_shift: float = 1.0):
        dev = flowsolver.th.device()
        self.dev, self.lib, self.n = dev, dev.lib, dev.N
        if getattr(dev, "world", 1) > 1:
            raise ValueError("the shifted solver runs on single-GPU handles only (this flowsolver is partitioned over ranks)")
        enclosed = getattr(dev, "_pin", None) is not None or _enclosed(flowsolver)
        if pressure_pin is None:
            if enclosed:
                raise ValueError("enclosed flow (velocity prescribed on the whole boundary): sigma E - A is singular for every sigma "
                                 "(pressure_pin='auto' pins one pressure dof inside the shifted factorisation)")
            self.pin = None
        elif isinstance(pressure_pin, str):
            if pressure_pin != "auto":
                raise ValueError(f"pressure_pin must be None, 'auto' or a pressure dof, got {pressure_pin!r}")
            self.pin = _auto_pin(flowsolver, dev)  # (None on an open flow: nothing to pin)
        else:
            self.pin = int(pressure_pin)
            if not 2 * dev.nn <= self.pin < dev.N:
                raise ValueError(f"pressure_pin={self.pin} is not a pressure dof ({2 * dev.nn} <= dof < {dev.N})")
        self.pin_shift = float(pin_shift)
        self.krylov = _krylov_settings(krylov)
        self.a_vals = values_on_pattern(A, dev.rowptr, dev.colidx, "A")
        self.e_vals = values_on_pattern(E, dev.rowptr, dev.colidx, "E")
        self.refine = int(refine)
        self.sigma: complex | None = None
        self.factored_sigma: complex | None = None
        self.last_iterations = np.zeros(0, dtype=np.int32)
        self._first = True

    @property
    def _h(self):
        return self.dev._h

    def factor(self, sigma: complex) -> None:
        sigma = complex(sigma)
        if self._first:
            a, e = self.a_vals.ctypes.data_as(C.c_void_p), self.e_vals.ctypes.data_as(C.c_void_p)
            if self.pin is not None:
                check(self.lib.fc_shifted_set_pin(self._h, self.pin, self.pin_shift))
            if self.krylov is not None:
                check(self.lib.fc_shifted_set_krylov(self._h, int(self.krylov["max_iter"]), int(self.krylov["restart"]),
                                                     float(self.krylov["rtol"])))
        else:
            a = e = None
        check(self.lib.fc_setup_shifted(self._h, a, e, sigma.real, sigma.imag, self.refine))
        self._first = False
        self.sigma = self.factored_sigma = sigma

    def shift(self, sigma: complex) -> None:
        """Move the operator to ``sigma`` WITHOUT refactorising: later solves run GMRES on the factors of the last :meth:`factor`
        (needs ``krylov=``)."""
        if self.krylov is None:
            raise ValueError("shift() solves on lagged factors and needs the Krylov solver: ShiftedOperator(..., krylov=True)")
        sigma = complex(sigma)
        check(self.lib.fc_shifted_set_shift(self._h, sigma.real, sigma.imag))
        self.sigma = sigma

    def krylov_info(self) -> dict:
        """GMRES iterations per column of the last solve; numeric factorisations, factor applies, mat-vecs, solves that ran GMRES
        and rescues among them (solves and Arnoldi steps alike) since the first :meth:`factor`."""
        nrhs = self.info()["nrhs"]
        it, cnt = np.zeros(max(nrhs, 1), dtype=np.int32), np.zeros(5, dtype=np.int64)
        check(self.lib.fc_shifted_krylov_info(self._h, _lib.ptr(it), _lib.ptr(cnt)))
        return {"iterations": it[:nrhs].copy(), "refactorisations": int(cnt[0]), "applies": int(cnt[1]), "matvecs": int(cnt[2]),
                "gmres_solves": int(cnt[3]), "rescues": int(cnt[4])}

    @property
    def rescued(self) -> bool:
        """A solve at the factored sigma -- a column of :meth:`solve` or an Arnoldi step of the eigen solver -- went through the
        GMRES rescue since the first :meth:`factor` (counted by the library)."""
        return (not self._first) and self.krylov_info()["rescues"] > 0

    def _after_solve(self, info: np.ndarray) -> None:
        self.last_residuals = info
        if self.krylov is not None:
            self.last_iterations = self.krylov_info()["iterations"]
        else:
            self.last_iterations = np.zeros(info.size, dtype=np.int32)

    def solve(self, b: np.ndarray, download: bool = True) -> np.ndarray | None:
        """x = (sigma E - A)^-1 b for the columns of b ([n] or [n, nrhs], real or complex)."""
        b = np.asarray(b)
        cols = b.reshape(self.n, -1)
        nrhs = cols.shape[1]
        bre = np.ascontiguousarray(cols.real.T, dtype=np.float64)
        bim = np.ascontiguousarray(cols.imag.T, dtype=np.float64) if np.iscomplexobj(cols) else None
        info = np.zeros(nrhs)
        if download:
            xre, xim = np.empty((nrhs, self.n)), np.empty((nrhs, self.n))
            check(self.lib.fc_solve_shifted(self._h, nrhs, bre, _lib.ptr(bim), _lib.ptr(xre), _lib.ptr(xim), _lib.ptr(info)))
            self._after_solve(info)
            x = (xre + 1j * xim).T
            return x.reshape(b.shape) if b.ndim == 1 else x
        check(self.lib.fc_solve_shifted(self._h, nrhs, bre, _lib.ptr(bim), None, None, _lib.ptr(info)))
        self._after_solve(info)
        return None

    def transfer(self, B: np.ndarray, Cm: np.ndarray) -> np.ndarray:
        """C (sigma E - A)^-1 B at the current sigma: nu solves, C X on the device, only (ny, nu) comes back."""
        self.solve(B, download=False)
        rp, idx, w = _sparse_rows(Cm)
        ny, nu = Cm.shape[0], B.shape[1]
        yre, yim = np.empty(ny * nu), np.empty(ny * nu)
        check(self.lib.fc_shifted_project(self._h, nu, ny, rp, idx, w, yre, yim))
        return (yre + 1j * yim).reshape(ny, nu)

    def spmv(self, s: complex, t: float, x: np.ndarray) -> np.ndarray:
        """(s E - t A) x on the device (x complex [n])."""
        xz = np.ascontiguousarray(x, dtype=np.complex128)
        y = np.empty(self.n, dtype=np.complex128)
        check(self.lib.fc_shifted_spmv(self._h, complex(s).real, complex(s).imag, float(t), xz.view(np.float64), y.view(np.float64)))
        return y

    def info(self) -> dict:
        iv, dv = np.zeros(4, dtype=np.int64), np.zeros(4)
        check(self.lib.fc_shifted_info(self._h, _lib.ptr(iv), _lib.ptr(dv), None))
        return {"factor_bytes": int(iv[0]), "device_bytes": int(iv[1]), "order": int(iv[2]), "nrhs": int(iv[3]),
                "refactor_ms": float(dv[0]), "refactor_flops": float(dv[1]), "sigma": complex(dv[2], dv[3])}

    def release(self) -> None:
        if getattr(self.dev, "_h", None):
            check(self.lib.fc_release_shifted(self._h))
        self._first = True
        self.sigma = self.factored_sigma = None


def _auto_pin(flowsolver, dev) -> int | None:
    """The pressure dof the flowsolver's own time stepping pins (None on an open flow)."""
    if getattr(dev, "_pin", None) is not None:
        return int(dev._pin)
    try:
        from .fem.boundary import pressure_pin

        dofs, _ = flowsolver._bc_tables()
        return pressure_pin(flowsolver.th, dofs)
    except (AttributeError, NotImplementedError):
        return None


def _enclosed(flowsolver) -> bool:
    try:
        from .fem.boundary import pressure_pin

        dofs, _ = flowsolver._bc_tables()
        return pressure_pin(flowsolver.th, dofs) is not None
    except (AttributeError, NotImplementedError):
        return False  # (the handle's own pressure pin is refused by fc_setup_shifted)


# ── frequency response ──────────────────────────────────────────────────────────────────────────────────────────────────────────
def _freqresp_sizes(A, B, C, ww) -> tuple[int, int, int, int]:
    """(n, nu, ny, nw) with the reference's checks (``_get_freqresp_sizes``)."""
    B, C = np.asarray(B), np.asarray(C)
    n, m = A.shape
    nu = B.shape[1] if B.ndim == 2 else 1
    ny = C.shape[0] if C.ndim == 2 else 1
    nw = len(np.atleast_1d(ww))
    if n != m:
        raise ValueError(f"A must be square, got shape ({n}, {m}).")
    if nw < 1:
        raise ValueError(f"ww must be non-empty, got length {nw}.")
    if B.shape[0] != n or (C.ndim == 2 and C.shape[1] != n) or (C.ndim == 1 and C.shape[0] != n):
        raise ValueError(f"B {B.shape} / C {C.shape} do not match A of order {n}")
    return n, nu, ny, nw


def _lagged(op, sigma: complex, solve):
    """``solve()`` at sigma on the factors ``op`` holds (GMRES); a GMRES that does not converge falls back to refactorising at
    sigma, logged."""
    op.shift(sigma)
    try:
        return solve()
    except _lib.FcError as exc:
        if exc.code != _lib.FC_ERR_NOT_CONVERGED:
            raise
        logger.warning("lagged factors of sigma = %s did not converge at sigma = %s: refactorising there (%s)", op.factored_sigma, sigma, exc)
        op.factor(sigma)
        return solve()


def _check_refactor_every(op, refactor_every: int) -> int:
    n = int(refactor_every)
    if n < 1:
        raise ValueError(f"refactor_every must be >= 1, got {refactor_every}")
    if n > 1 and getattr(op, "krylov", None) is None:
        raise ValueError("refactor_every > 1 solves on lagged factors and needs the Krylov solver (krylov=)")
    return n


def frequency_response(op, B, C, ww, verbose: bool = True, refactor_every: int = 1) -> tuple[np.ndarray, np.ndarray]:
    """H[:, :, i] = C (i ww[i] E - A)^-1 B through a shifted-operator backend ``op`` (``factor(sigma)``, ``transfer(B, C)``):
    the loop the three public variants share.  ``refactor_every=n > 1``: only every n-th frequency is factorised, the ones in
    between are solved by GMRES on those factors (``op.shift``)."""
    refactor_every = _check_refactor_every(op, refactor_every)
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    B = np.asarray(B, dtype=float)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    C = np.asarray(C, dtype=float)
    C = C.reshape(1, -1) if C.ndim == 1 else C
    H = np.zeros((C.shape[0], B.shape[1], ww.size), dtype=complex)
    t0 = time.time()
    for ii, w in enumerate(ww):
        t1 = time.time()
        if ii % refactor_every == 0:
            op.factor(1j * w)
            H[:, :, ii] = op.transfer(B, C)
        else:
            H[:, :, ii] = _lagged(op, 1j * w, lambda: op.transfer(B, C))
        if verbose:
            logger.info("  [%d/%d] w=%.4e | max|H|=%.4e | elapsed: %.3fs", ii + 1, ww.size, w, np.max(np.abs(H[:, :, ii])), time.time() - t1)
    if verbose:
        logger.info("Frequency response computed in %.3fs total.", time.time() - t0)
    return H, ww


def _need_flowsolver(flowsolver) -> None:
    if flowsolver is None:
        raise ValueError("flowsolver= is required: the computation runs on that solver's device handle")


def _sweep_krylov(krylov, refactor_every: int):
    """Lagged-factor sweeps need the GMRES: on by default settings when ``refactor_every > 1`` and ``krylov`` was not given."""
    return True if (krylov is None and int(refactor_every) > 1) else krylov


def get_frequency_response_sequential(A, B, C, Q, ww, verbose: bool = True, *, flowsolver=None, refine: int = 2, pressure_pin=None,
                                      refactor_every: int = 1, krylov=None):
    """H(w) = C (jwQ - A)^-1 B for every w of ww (reference ``utils/linalg.py:192-232``).  Returns (H [ny, nu, nw] complex, ww).
    One numeric factorisation of jwQ - A per frequency on the device, nu solves, C X formed on the device.
    ``pressure_pin="auto"`` (or a pressure dof): enclosed flows, see :class:`ShiftedOperator`.  ``refactor_every=n > 1``: one
    factorisation per n frequencies, GMRES on the lagged factors in between (``krylov=`` sets its max_iter / restart / rtol)."""
    _need_flowsolver(flowsolver)
    n, nu, ny, nw = _freqresp_sizes(A, B, C, ww)
    if verbose:
        ww_ = np.atleast_1d(ww)
        logger.info("System dimensions: n=%d, nu=%d, ny=%d | Frequency points: nw=%d, w in [1e%g, 1e%g]", n, nu, ny, nw,
                    np.log10(ww_[0]), np.log10(ww_[-1]))
    op = ShiftedOperator(flowsolver, A, Q, refine=refine, pressure_pin=pressure_pin, krylov=_sweep_krylov(krylov, refactor_every))
    try:
        return frequency_response(op, B, C, ww, verbose, refactor_every)
    finally:
        op.release()


def get_frequency_response_parallel(A, B, C, Q, ww, verbose: bool = True, n_jobs: int = 1, *, flowsolver=None, refine: int = 2, **kw):
    """Same result as :func:`get_frequency_response_sequential`.  ``n_jobs`` is accepted for the reference's signature and has no
    meaning here: the frequencies are factorised one after the other on one device, each factorisation using all of it."""
    return get_frequency_response_sequential(A, B, C, Q, ww, verbose, flowsolver=flowsolver, refine=refine, **kw)


def get_frequency_response_mpi(A, B, C, Q, ww, verbose: bool = True, *, flowsolver=None, refine: int = 2, **kw):
    """Same result as :func:`get_frequency_response_sequential` (the reference's MPI/MUMPS variant; one device here)."""
    return get_frequency_response_sequential(A, B, C, Q, ww, verbose, flowsolver=flowsolver, refine=refine, **kw)


def get_field_response(A, B, Q, ww, verbose: bool = True, *, flowsolver=None, refine: int = 2, pressure_pin=None, refactor_every: int = 1,
                       krylov=None) -> np.ndarray:
    """X(w) = (jwQ - A)^-1 B for each w of ww (reference ``utils/linalg.py:331``).  Returns X [n, nu, nw] complex.
    ``pressure_pin``, ``refactor_every``, ``krylov``: as :func:`get_frequency_response_sequential`."""
    _need_flowsolver(flowsolver)
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    B = np.asarray(B, dtype=float)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    n = A.shape[0]
    if B.shape[0] != n:
        raise ValueError(f"B {B.shape} does not match A of order {n}")
    op = ShiftedOperator(flowsolver, A, Q, refine=refine, pressure_pin=pressure_pin, krylov=_sweep_krylov(krylov, refactor_every))
    refactor_every = _check_refactor_every(op, refactor_every)
    X = np.zeros((n, B.shape[1], ww.size), dtype=complex)
    try:
        for ii, w in enumerate(ww):
            if ii % refactor_every == 0:
                op.factor(1j * w)
                X[:, :, ii] = op.solve(B)
            else:
                X[:, :, ii] = _lagged(op, 1j * w, lambda: op.solve(B))
            if verbose:
                logger.info("  [%d/%d] w=%.4e | max|X|=%.4e", ii + 1, ww.size, w, np.max(np.abs(X[:, :, ii])))
    finally:
        op.release()
    return X


# ── shift-invert eigenvalues: Krylov-Schur ──────────────────────────────────────────────────────────────────────────────────────
def krylov_schur(backend, nev: int, ncv: int, sigma: complex, tol: float = 1e-5, maxit: int = 1000, v0: np.ndarray | None = None,
                 verbose: bool = False) -> tuple[np.ndarray, np.ndarray, dict]:
    """Krylov-Schur iteration (Stewart 2001) for the ``nev`` eigenvalues of Op = (A - sigma E)^-1 E of largest modulus, i.e. the
    eigenvalues lambda = sigma + 1 / theta of the pencil (A, E) nearest ``sigma``.  Only the (ncv x ncv) Schur work runs here; the
    vectors live with ``backend``:

        backend.start(m, v0)          V_0 = Op v0 / |Op v0|, room for m + 1 basis vectors
        backend.step(j) -> (h, beta)  V_{j+1} beta = Op V_j - V_{0..j} h   (h complex [j + 1])
        backend.restart(Q)            V_{0..k} = V_{0..m} Q (Q [m, k]), V_k = V_m
        backend.ritz(Y, lam, vectors) -> (res [k, 3], X [n, k] or None): res = |A x - lam E x|, |A x|, |E x| of x = V_{0..m} Y

    A pair has converged when |A x - lam E x| / (|lam| |E x| + |A x|) <= tol.  Returns (lam [nev], X [n, nev], stats); the
    eigenvalues nearest sigma first, X with unit 2-norm columns."""
    m = int(ncv)
    if not 1 <= nev < m:
        raise ValueError(f"need 1 <= n < ncv, got n={nev}, ncv={m}")
    keep = min(m - 1, max(nev + 1, (nev + m) // 2))
    if v0 is None:
        rng = np.random.default_rng(0)
        v0 = rng.standard_normal(backend.n) + 1j * rng.standard_normal(backend.n)
    backend.start(m, np.ascontiguousarray(v0, dtype=np.complex128))
    H = np.zeros((m + 1, m), dtype=complex)
    k = 0
    steps = 0
    rel = np.full(nev, np.inf)
    for it in range(1, int(maxit) + 1):
        for j in range(k, m):
            h, beta = backend.step(j)
            H[: j + 1, j] = h
            H[j + 1, j] = beta
            steps += 1
        Hm = H[:m, :m]
        mags = np.sort(np.abs(np.linalg.eigvals(Hm)))[::-1]
        thr = 0.5 * (mags[keep - 1] + mags[keep])
        T, Z, sdim = sla.schur(Hm, output="complex", sort=lambda x: abs(x) > thr)
        k = int(min(max(sdim, nev), m - 1))
        w, S = np.linalg.eig(T[:k, :k])
        sel = np.argsort(-np.abs(w))[:nev]
        Y = Z[:, :k] @ S[:, sel]
        Y /= np.linalg.norm(Y, axis=0)
        lam = sigma + 1.0 / w[sel]
        res, _ = backend.ritz(Y, lam, vectors=False)
        rel = res[:, 0] / (np.abs(lam) * res[:, 2] + res[:, 1])
        if verbose:
            logger.info("Krylov-Schur restart %d: %d Arnoldi steps, residuals %s", it, steps, np.array2string(rel, precision=2))
        if np.all(rel <= tol):
            res, X = backend.ritz(Y, lam, vectors=True)
            X = X / np.linalg.norm(X, axis=0)
            return lam, X, {"restarts": it, "steps": steps, "residuals": rel}
        beta = H[m, m - 1]
        H[:] = 0.0
        H[:k, :k] = T[:k, :k]
        H[k, :k] = beta * Z[m - 1, :k]
        backend.restart(np.ascontiguousarray(Z[:, :k]))
    raise RuntimeError(f"Krylov-Schur: {int(np.sum(rel <= tol))} of {nev} eigenpairs converged to {tol:g} in {maxit} restarts "
                       f"(residuals {rel})")


class DeviceKrylov:
    """The vector side of :func:`krylov_schur` on the device: basis, Gram-Schmidt, restarts and Ritz residuals in the handle's
    shifted solver (``fc_shifted_arnoldi_*``, ``fc_shifted_ritz``)."""

    def __init__(self, op: ShiftedOperator):
        self.op, self.lib, self.n = op, op.lib, op.n
        self.m = 0

    def start(self, m: int, v0: np.ndarray) -> None:
        self.m = m
        check(self.lib.fc_shifted_arnoldi_start(self.op._h, m, v0.view(np.float64)))

    def step(self, j: int):
        h = np.empty(j + 1, dtype=np.complex128)
        beta = C.c_double()
        check(self.lib.fc_shifted_arnoldi_step(self.op._h, j, h.view(np.float64), C.byref(beta)))
        return h, beta.value

    def restart(self, Q: np.ndarray) -> None:
        Q = np.ascontiguousarray(Q, dtype=np.complex128)
        check(self.lib.fc_shifted_arnoldi_restart(self.op._h, self.m, Q.shape[1], Q.view(np.float64).reshape(-1)))

    def ritz(self, Y: np.ndarray, lam: np.ndarray, vectors: bool):
        Y = np.ascontiguousarray(Y, dtype=np.complex128)
        lam = np.ascontiguousarray(lam, dtype=np.complex128)
        k = Y.shape[1]
        res = np.empty((k, 3))
        X = np.empty((k, self.n), dtype=np.complex128) if vectors else None
        check(self.lib.fc_shifted_ritz(self.op._h, self.m, k, Y.view(np.float64).reshape(-1), lam.view(np.float64), res,
                                       None if X is None else X.ctypes.data_as(C.c_void_p)))
        return res, (None if X is None else X.T)


def get_mat_vp(A, B=None, n: int = 10, target: complex = 0.0, tol: float = 1e-5, niter: int = 1000, ncv: int | None = None, *,
               flowsolver=None, verbose: bool = False, return_eigensolver: bool = False, refine: int = 2, pressure_pin=None, krylov=None,
               pin_shift: float = 1.0, operator: ShiftedOperator | None = None, **slepc_options: Any):
    """The ``n`` eigenvalues of the pencil (A, B) nearest ``target`` and their eigenvectors (reference ``get_mat_vp_slepc``,
    ``utils/linalg.py:52-131``): shift-invert Krylov-Schur with the device's direct solver of A - target B.  Returns
    (valp [n] complex, vecp [N, n] complex in the W layout, unit 2-norm columns), nearest ``target`` first.  ``B`` is the mass
    matrix (E); it must lie on the flowsolver's CSR pattern like ``A`` (``B=None``, the standard problem, needs an identity on it,
    which the pressure block of the pattern does not have).  SLEPc-only options (eps_type, precond_type, ksp_type, mpd) are
    accepted and ignored.  ``pressure_pin="auto"`` (or a pressure dof): enclosed flows, the eigenvalues of the pencil
    (A - pin_shift e_k e_k^T, B), whose finite ones do not depend on ``pin_shift``.  ``krylov``: the GMRES rescue of
    :class:`ShiftedOperator`.  ``operator``: a :class:`ShiftedOperator` of (A, B) to reuse (one symbolic phase for several
    targets); it is not released."""
    if operator is None:
        _need_flowsolver(flowsolver)
    for key in list(slepc_options):
        if key in _SLEPC_ONLY:
            logger.info("get_mat_vp: %s=%r ignored (SLEPc option; the device runs Krylov-Schur with its own direct solver)", key,
                        slepc_options.pop(key))
    if slepc_options:
        raise TypeError(f"get_mat_vp: unexpected keyword arguments {sorted(slepc_options)}")
    N = A.shape[0]
    if B is None:
        B = sp.identity(N, format="csr")
    n = int(n)
    if ncv is None or ncv <= 0:
        ncv = max(2 * n + 1, 20)
    ncv = int(min(ncv, N - 1))
    op = operator if operator is not None else ShiftedOperator(flowsolver, A, B, refine=refine, pressure_pin=pressure_pin, krylov=krylov,
                                                               pin_shift=pin_shift)
    try:
        op.factor(complex(target))
        t0 = time.time()
        lam, X, stats = krylov_schur(DeviceKrylov(op), n, ncv, complex(target), tol, niter, verbose=verbose)
        if verbose:
            logger.info("get_mat_vp: %d eigenpairs in %.3fs (%d restarts, %d Arnoldi steps)", n, time.time() - t0, stats["restarts"],
                        stats["steps"])
            for i, v in enumerate(lam):
                logger.info("Eigenvalue %2d: %+.6f %+.6fj", i + 1, v.real, v.imag)
    finally:
        if operator is None:
            op.release()
    if return_eigensolver:
        return (lam, X), stats
    return lam, X


#: the reference's name
get_mat_vp_slepc = get_mat_vp

__all__ = ["get_frequency_response_sequential", "get_frequency_response_parallel", "get_frequency_response_mpi", "get_field_response",
           "get_mat_vp", "get_mat_vp_slepc", "krylov_schur", "frequency_response", "ShiftedOperator", "DeviceKrylov", "values_on_pattern"]
