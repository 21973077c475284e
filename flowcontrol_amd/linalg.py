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
by that GMRES on the lagged factors.  ``block=`` solves the frequencies of such a group side by side (``fc_solve_shifted_block``: up
to 32 columns, each at its own shift, one pass over the factors per GMRES iteration for all of them).

Adjoint side, on the SAME factors (``fc_shifted_set_adjoint``: the factors of the transposed system are a per-front transposition of
the values the factorisation leaves behind, one more export pass instead of a second factorisation):

    (sigma E - A)^H y = c                 ``ShiftedOperator.solve(c, adjoint=True)``, ``solve_block(..., adjoint=True)``
    y^H A = lambda y^H E                  ``get_mat_vp(..., left=True)``: a second Krylov-Schur in the adjoint mode
    max |q|_E / |g|_E, q = (iwE - A)^-1 E g   ``resolvent_gains``: Arnoldi on M^-H E^T M^-1 E, direct and adjoint solves alternating
"""

from __future__ import annotations

import contextlib
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


#: widest block of ``fc_shifted_set_block``
MAX_BLOCK = 32


def expand_block_columns(b, sigmas, k: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """Columns and shifts of a block solve as (cols [n, k] complex, sig [k] complex).  ``b`` [n, k] with k shifts: column c at shift c.
    ``b`` [n, nu] with ``len(sigmas) * nu == k``: every input at every shift, shift-major (column ``s * nu + i`` is input i at shift
    s).  ``k`` (the block's width) decides between the two readings; ``None``: the first where it fits, else the second."""
    b = np.asarray(b)
    if b.ndim == 1:
        b = b.reshape(-1, 1)
    if b.ndim != 2:
        raise ValueError(f"b must be [n] or [n, columns], got shape {b.shape}")
    sig = np.atleast_1d(np.asarray(sigmas, dtype=complex)).ravel()
    if sig.size < 1:
        raise ValueError("sigmas must not be empty")
    if not np.all(np.isfinite(sig)):
        raise ValueError("sigmas must be finite")
    nu = b.shape[1]
    if sig.size == nu and (k is None or k == nu):
        cols = b
    elif k is None or sig.size * nu == k:
        cols, sig = np.tile(b, (1, sig.size)), np.repeat(sig, nu)
    else:
        raise ValueError(f"b has {nu} column(s) and there are {sig.size} shift(s): neither {nu} == {sig.size} == k nor "
                         f"{sig.size} * {nu} == k for the block width k = {k}")
    if not 1 <= cols.shape[1] <= MAX_BLOCK:
        raise ValueError(f"a block has 1 .. {MAX_BLOCK} columns, got {cols.shape[1]}")
    return np.asarray(cols, dtype=complex), sig


def sweep_groups(ww, refactor_every: int, nu: int) -> list[dict]:
    """The plan of a block sweep: ``ww`` cut into groups of ``refactor_every`` consecutive frequencies (the last one may be shorter),
    each factorised ONCE at ``mid`` -- the geometric middle sqrt(first * last) of the group, the arithmetic one when a frequency of
    it is not positive -- and its frequencies cut into ``blocks`` [j0, j1) of at most ``MAX_BLOCK // nu`` frequencies, so that a
    block's (j1 - j0) * nu columns fit one block solve.  Returns [{"start", "stop", "mid", "blocks"}]."""
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    n, nu = int(refactor_every), int(nu)
    if n < 1:
        raise ValueError(f"refactor_every must be >= 1, got {refactor_every}")
    if not 1 <= nu <= MAX_BLOCK:
        raise ValueError(f"a block sweep takes 1 .. {MAX_BLOCK} inputs, got {nu}")
    per_block = MAX_BLOCK // nu
    groups = []
    for i0 in range(0, ww.size, n):
        i1 = min(i0 + n, ww.size)
        lo, hi = float(ww[i0]), float(ww[i1 - 1])
        mid = float(np.sqrt(lo * hi)) if np.all(ww[i0:i1] > 0.0) else 0.5 * (lo + hi)
        blocks = [(j0, min(j0 + per_block, i1)) for j0 in range(i0, i1, per_block)]
        groups.append({"start": i0, "stop": i1, "mid": mid, "blocks": blocks})
    return groups


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
    the columns of the last solve (zeros when none was needed).
    ``block``: ``None`` off; k in 1 .. 32 builds the block of ``fc_shifted_set_block`` with the first :meth:`factor` (needs
    ``krylov=``): :meth:`solve_block` then solves k columns at k shifts on the held factors in one lock-step GMRES."""

    def __init__(self, flowsolver, A, E, refine: int = 2, pressure_pin=None, krylov=None, pin_shift: float = 1.0, block: int | None = None):
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
        self.block = None if block is None else int(block)
        if self.block is not None:
            if not 1 <= self.block <= MAX_BLOCK:
                raise ValueError(f"block must be in 1 .. {MAX_BLOCK}, got {block}")
            if self.krylov is None:
                raise ValueError("block= solves on the held factors by GMRES and needs the Krylov solver (krylov=)")
        self._block_set = 0
        self.a_vals = values_on_pattern(A, dev.rowptr, dev.colidx, "A")
        self.e_vals = values_on_pattern(E, dev.rowptr, dev.colidx, "E")
        self.refine = int(refine)
        self.sigma: complex | None = None
        self.factored_sigma: complex | None = None
        self.last_iterations = np.zeros(0, dtype=np.int32)
        self._first = True
        self._adjoint = False

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
        if self.block is not None and self._block_set != self.block:
            self.set_block(self.block)

    def set_block(self, k: int) -> None:
        """Build the block of width ``k`` (0 frees it) on the structure of the first :meth:`factor`."""
        k = int(k)
        if not 0 <= k <= MAX_BLOCK:
            raise ValueError(f"block width must be in 0 .. {MAX_BLOCK}, got {k}")
        if k > 0 and self.krylov is None:
            raise ValueError("block solves run the Krylov solver: ShiftedOperator(..., krylov=True)")
        if self._first:
            raise ValueError("set_block() builds on the solver's structure: factor() first")
        check(self.lib.fc_shifted_set_block(self._h, k))
        self._block_set = k

    def shift(self, sigma: complex) -> None:
        """Move the operator to ``sigma`` WITHOUT refactorising: later solves run GMRES on the factors of the last :meth:`factor`
        (needs ``krylov=``)."""
        if self.krylov is None:
            raise ValueError("shift() solves on lagged factors and needs the Krylov solver: ShiftedOperator(..., krylov=True)")
        sigma = complex(sigma)
        check(self.lib.fc_shifted_set_shift(self._h, sigma.real, sigma.imag))
        self.sigma = sigma

    def set_adjoint(self, on) -> None:
        """Adjoint mode (``fc_shifted_set_adjoint``): ``True`` / 1 -- the operator behaves as ``(sigma E - A)^H = conj(sigma) E^T - A^T``
        in :meth:`solve`, :meth:`solve_block`, :meth:`spmv` (``(s E^T - t A^T) x``) and the eigen solver, on the factors it holds (the
        adjoint factor array is built by the first call: the factor size again, no second factorisation); ``False`` / 0 back to
        direct, the array stays; -1 back to direct and the adjoint side freed.  After the first :meth:`factor`."""
        on = -1 if on == -1 else int(bool(on))
        check(self.lib.fc_shifted_set_adjoint(self._h, on))
        self._adjoint = on == 1

    @contextlib.contextmanager
    def adjoint(self, on: bool = True):
        """``with op.adjoint(): ...`` -- the adjoint mode inside the block, the previous mode after it."""
        prev = self._adjoint
        self.set_adjoint(on)
        try:
            yield self
        finally:
            if getattr(self.dev, "_h", None) and not self._first:
                self.set_adjoint(prev)

    def adjoint_info(self) -> dict:
        """Mode, device bytes of the adjoint side, transposed exports and mode switches since the structure was built; device time and
        algorithmic bytes of the last transposed export."""
        iv, dv = np.zeros(4, dtype=np.int64), np.zeros(2)
        check(self.lib.fc_shifted_adjoint_info(self._h, _lib.ptr(iv), _lib.ptr(dv)))
        return {"adjoint": bool(iv[0]), "bytes": int(iv[1]), "exports": int(iv[2]), "switches": int(iv[3]), "export_ms": float(dv[0]),
                "export_bytes": float(dv[1]), "export_TBps": float(dv[1] / (1e9 * dv[0])) if dv[0] > 0 else 0.0}

    def krylov_info(self) -> dict:
        """GMRES iterations per column of the last solve; numeric factorisations, factor applies, mat-vecs, solves that ran GMRES
        and rescues among them (solves and Arnoldi steps alike) since the first :meth:`factor`."""
        nrhs = self.info()["nrhs"]
        it, cnt = np.zeros(max(nrhs, 1), dtype=np.int32), np.zeros(5, dtype=np.int64)
        check(self.lib.fc_shifted_krylov_info(self._h, _lib.ptr(it), _lib.ptr(cnt)))
        return {"iterations": it[:nrhs].copy(), "refactorisations": int(cnt[0]), "applies": int(cnt[1]), "matvecs": int(cnt[2]),
                "gmres_solves": int(cnt[3]), "rescues": int(cnt[4])}

    def block_info(self) -> dict:
        """Width and padded width of the block; lock-step iterations launched and cycles run by the last :meth:`solve_block` (the
        factors were read ``lockstep_iterations + cycles`` times for all its columns together)."""
        iv = np.zeros(4, dtype=np.int64)
        check(self.lib.fc_shifted_block_info(self._h, _lib.ptr(iv)))
        return {"k": int(iv[0]), "KB": int(iv[1]), "lockstep_iterations": int(iv[2]), "cycles": int(iv[3])}

    def bench_block(self, reps: int = 20) -> dict:
        """Device time (HIP events, mean of ``reps``) and algorithmic bytes of one batched factor apply and one block SpMV at the
        block's padded width, and of their single-column counterparts."""
        ms, nbytes = np.zeros(4), np.zeros(4)
        check(self.lib.fc_bench_shifted_block(self._h, int(reps), ms, nbytes))
        names = ("apply_block", "spmv_block", "apply_single", "spmv_single")
        return {n: {"ms": float(t), "bytes": float(b), "TBps": float(b / (1e9 * t)) if t > 0 else 0.0} for n, t, b in zip(names, ms, nbytes)}

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

    def solve(self, b: np.ndarray, download: bool = True, adjoint: bool = False) -> np.ndarray | None:
        """x = (sigma E - A)^-1 b for the columns of b ([n] or [n, nrhs], real or complex).  ``adjoint=True``: x = (sigma E - A)^-H b,
        whatever the mode is, which is restored afterwards (``False``: the solve of the current mode, :meth:`set_adjoint`)."""
        if adjoint and not self._adjoint:
            with self.adjoint():
                return self.solve(b, download)
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

    def solve_block(self, b: np.ndarray, sigmas, download: bool = True, adjoint: bool = False) -> np.ndarray | None:
        """x_c = (sigma_c E - A)^-1 b_c for the k columns of the block, on the factors of the last :meth:`factor`, all columns in
        one lock-step GMRES (``fc_solve_shifted_block``).  ``b`` [n, k] with k shifts, or [n, nu] with ``len(sigmas) * nu == k``:
        every input at every shift (:func:`expand_block_columns`).  Returns x [n, k] (``download=False``: kept on the device for
        :meth:`project`).  A column that misses rtol raises ``FcError`` (FC_ERR_NOT_CONVERGED); ``last_residuals`` and
        ``last_iterations`` name it.  ``adjoint=True``: x_c = (sigma_c E - A)^-H b_c, as in :meth:`solve`."""
        if adjoint and not self._adjoint:
            with self.adjoint():
                return self.solve_block(b, sigmas, download)
        if self.krylov is None:
            raise ValueError("solve_block() runs the Krylov solver: ShiftedOperator(..., krylov=True)")
        if np.asarray(b).shape[0] != self.n:
            raise ValueError(f"b has {np.asarray(b).shape[0]} rows, the operator has order {self.n}")
        cols, sig = expand_block_columns(b, sigmas, self._block_set or self.block)
        k = cols.shape[1]
        if self._first or self._block_set == 0:
            raise ValueError("no block is set: ShiftedOperator(..., block=k) and factor(), or set_block(k)")
        if k != self._block_set:
            raise ValueError(f"{k} columns for a block of width {self._block_set}")
        bre = np.ascontiguousarray(cols.real.T, dtype=np.float64)
        bim = np.ascontiguousarray(cols.imag.T, dtype=np.float64)
        sre, sim = np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag)
        info = np.full(k, np.nan)
        xre, xim = (np.empty((k, self.n)), np.empty((k, self.n))) if download else (None, None)
        rc = self.lib.fc_solve_shifted_block(self._h, k, sre, sim, bre, _lib.ptr(bim), _lib.ptr(xre), _lib.ptr(xim), _lib.ptr(info))
        if rc in (0, _lib.FC_ERR_NOT_CONVERGED):
            self._after_solve(info)
        check(rc)
        return (xre + 1j * xim).T if download else None

    def project(self, Cm: np.ndarray, ncols: int) -> np.ndarray:
        """C X for the first ``ncols`` solutions the last solve left on the device: only (ny, ncols) comes back."""
        rp, idx, w = _sparse_rows(Cm)
        ny = Cm.shape[0]
        yre, yim = np.empty(ny * ncols), np.empty(ny * ncols)
        check(self.lib.fc_shifted_project(self._h, ncols, ny, rp, idx, w, yre, yim))
        return (yre + 1j * yim).reshape(ny, ncols)

    def transfer(self, B: np.ndarray, Cm: np.ndarray) -> np.ndarray:
        """C (sigma E - A)^-1 B at the current sigma: nu solves, C X on the device, only (ny, nu) comes back."""
        self.solve(B, download=False)
        return self.project(Cm, B.shape[1])

    def spmv(self, s: complex, t: float, x: np.ndarray) -> np.ndarray:
        """(s E - t A) x on the device (x complex [n])."""
        xz = np.ascontiguousarray(x, dtype=np.complex128)
        y = np.empty(self.n, dtype=np.complex128)
        check(self.lib.fc_shifted_spmv(self._h, complex(s).real, complex(s).imag, float(t), xz.view(np.float64), y.view(np.float64)))
        return y

    # snapshot sets (``fc_shifted_snap_*``): 0 direct solutions, 1 adjoint solutions, 2 vectors loaded from the host; see rom.py
    def snap_reserve(self, which: int, ncol: int) -> None:
        """Room for ``ncol`` complex columns in set ``which`` on the device (0 frees the set).  After the first :meth:`factor`."""
        check(self.lib.fc_shifted_snap_reserve(self._h, int(which), int(ncol)))

    def snap_push(self, which: int, ncol: int, scale: float = 1.0) -> None:
        """Append ``scale`` times the first ``ncol`` solutions of the last solve to set ``which`` (a device copy)."""
        check(self.lib.fc_shifted_snap_push(self._h, int(which), int(ncol), float(scale)))

    def snap_load(self, which: int, x: np.ndarray, scale: float = 1.0) -> None:
        """Append ``scale`` times the columns of the host array ``x`` ([n] or [n, ncol], real or complex) to set ``which``."""
        cols = np.asarray(x).reshape(self.n, -1)
        re = np.ascontiguousarray(cols.real.T, dtype=np.float64)
        im = np.ascontiguousarray(cols.imag.T, dtype=np.float64) if np.iscomplexobj(cols) else None
        check(self.lib.fc_shifted_snap_load(self._h, int(which), cols.shape[1], re, _lib.ptr(im), float(scale)))

    def snap_gram(self, left: int, right: int, kind: int = 0) -> np.ndarray:
        """G[2a + p, 2b + q] = part_p(l_a)^T Op part_q(r_b) over the columns of the sets ``left`` and ``right`` (p, q: re, im);
        ``kind`` 0: Op = I, 1: E, 2: A.  Formed on the device; only the small matrix comes back."""
        cnt = self.snap_info()["columns"]
        nl, nr = (cnt[w] if 0 <= w <= 2 else 0 for w in (int(left), int(right)))  # (an unknown or empty set is refused by the library)
        out = np.empty((max(2 * nl, 1), max(2 * nr, 1)))
        check(self.lib.fc_shifted_snap_gram(self._h, int(left), int(right), int(kind), out))
        return out

    def snap_combine(self, which: int, Q: np.ndarray) -> np.ndarray:
        """The real vectors sum_J Q[J, c] part_J of set ``which`` (Q [2 ncol, k]; part_{2a + p} = part p of column a): [n, k]."""
        Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).reshape(2 * self.snap_info()["columns"][int(which)], -1))
        out = np.empty((Q.shape[1], self.n))
        check(self.lib.fc_shifted_snap_combine(self._h, int(which), Q.shape[1], Q, out))
        return out.T

    def snap_info(self) -> dict:
        """Columns and capacity of the three sets, device bytes held by them, Gram calls since the structure was built."""
        iv = np.zeros(8, dtype=np.int64)
        check(self.lib.fc_shifted_snap_info(self._h, iv))
        return {"columns": [int(iv[0]), int(iv[2]), int(iv[4])], "capacity": [int(iv[1]), int(iv[3]), int(iv[5])], "bytes": int(iv[6]),
                "gram_calls": int(iv[7])}

    def snap_clear(self, which: int) -> None:
        """Column count of set ``which`` back to 0; the memory stays."""
        check(self.lib.fc_shifted_snap_clear(self._h, int(which)))

    def snap_gram_timing(self) -> dict:
        """Device time (HIP events), algorithmic bytes and flops of the last :meth:`snap_gram`."""
        dv = np.zeros(3)
        check(self.lib.fc_bench_snap_gram_last(self._h, dv))
        return {"ms": float(dv[0]), "bytes": float(dv[1]), "flops": float(dv[2]), "TBps": float(dv[1] / (1e9 * dv[0])) if dv[0] > 0 else 0.0,
                "TFLOPs": float(dv[2] / (1e9 * dv[0])) if dv[0] > 0 else 0.0}

    def info(self) -> dict:
        iv, dv = np.zeros(4, dtype=np.int64), np.zeros(4)
        check(self.lib.fc_shifted_info(self._h, _lib.ptr(iv), _lib.ptr(dv), None))
        return {"factor_bytes": int(iv[0]), "device_bytes": int(iv[1]), "order": int(iv[2]), "nrhs": int(iv[3]),
                "refactor_ms": float(dv[0]), "refactor_flops": float(dv[1]), "sigma": complex(dv[2], dv[3])}

    def release(self) -> None:
        if getattr(self.dev, "_h", None):
            check(self.lib.fc_release_shifted(self._h))
        self._first = True
        self._block_set = 0
        self._adjoint = False
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


def _check_block(op, block) -> bool:
    if not block:
        return False
    if getattr(op, "krylov", None) is None or not hasattr(op, "solve_block"):
        raise ValueError("block=True solves on the held factors by GMRES and needs a ShiftedOperator with the Krylov solver (krylov=)")
    return True


def _block_sweep(op, B, ww, refactor_every: int, solve_block, per_frequency, verbose: bool) -> None:
    """The block form of a sweep (:func:`sweep_groups`): every group is factorised once at its middle frequency and its blocks go
    through ``solve_block(j0, j1, sigmas)``; a block with a column that misses the tolerance sends its whole group through
    ``per_frequency(i)`` -- the path of ``block=None`` -- instead, logged."""
    nu = B.shape[1]
    for grp in sweep_groups(ww, refactor_every, nu):
        t1 = time.time()
        try:
            op.factor(1j * grp["mid"])
            for j0, j1 in grp["blocks"]:
                if op._block_set != (j1 - j0) * nu:
                    op.set_block((j1 - j0) * nu)
                solve_block(j0, j1, 1j * ww[j0:j1])
        except _lib.FcError as exc:
            if exc.code != _lib.FC_ERR_NOT_CONVERGED:
                raise
            logger.warning("block solve on the factors of sigma = %s did not converge for the frequencies %d .. %d: solving them one by "
                           "one (%s)", op.factored_sigma, grp["start"], grp["stop"] - 1, exc)
            for i in range(grp["start"], grp["stop"]):
                per_frequency(i)
        if verbose:
            logger.info("  [%d..%d/%d] factorised at w=%.4e | elapsed: %.3fs", grp["start"] + 1, grp["stop"], ww.size, grp["mid"], time.time() - t1)


def frequency_response(op, B, C, ww, verbose: bool = True, refactor_every: int = 1, block=None) -> tuple[np.ndarray, np.ndarray]:
    """H[:, :, i] = C (i ww[i] E - A)^-1 B through a shifted-operator backend ``op`` (``factor(sigma)``, ``transfer(B, C)``):
    the loop the three public variants share.  ``refactor_every=n > 1``: only every n-th frequency is factorised, the ones in
    between are solved by GMRES on those factors (``op.shift``).  ``block=True``: every group of n frequencies is factorised at its
    middle frequency and its n nu columns are solved side by side, at most 32 at a time (:meth:`ShiftedOperator.solve_block`)."""
    refactor_every = _check_refactor_every(op, refactor_every)
    block = _check_block(op, block)
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    B = np.asarray(B, dtype=float)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    C = np.asarray(C, dtype=float)
    C = C.reshape(1, -1) if C.ndim == 1 else C
    H = np.zeros((C.shape[0], B.shape[1], ww.size), dtype=complex)
    t0 = time.time()
    if block:
        ny, nu = C.shape[0], B.shape[1]

        def solve_block(j0, j1, sigmas):
            op.solve_block(B, sigmas, download=False)
            H[:, :, j0:j1] = op.project(C, (j1 - j0) * nu).reshape(ny, j1 - j0, nu).transpose(0, 2, 1)

        def per_frequency(ii):
            if ii % refactor_every == 0:
                op.factor(1j * ww[ii])
                H[:, :, ii] = op.transfer(B, C)
            else:
                H[:, :, ii] = _lagged(op, 1j * ww[ii], lambda: op.transfer(B, C))

        _block_sweep(op, B, ww, refactor_every, solve_block, per_frequency, verbose)
        if verbose:
            logger.info("Frequency response computed in %.3fs total.", time.time() - t0)
        return H, ww
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


def _sweep_krylov(krylov, refactor_every: int, block=None):
    """Lagged-factor and block sweeps need the GMRES: on by default settings when ``refactor_every > 1`` or ``block`` is set and
    ``krylov`` was not given."""
    return True if (krylov is None and (int(refactor_every) > 1 or block)) else krylov


def get_frequency_response_sequential(A, B, C, Q, ww, verbose: bool = True, *, flowsolver=None, refine: int = 2, pressure_pin=None,
                                      refactor_every: int = 1, krylov=None, block=None):
    """H(w) = C (jwQ - A)^-1 B for every w of ww (reference ``utils/linalg.py:192-232``).  Returns (H [ny, nu, nw] complex, ww).
    One numeric factorisation of jwQ - A per frequency on the device, nu solves, C X formed on the device.
    ``pressure_pin="auto"`` (or a pressure dof): enclosed flows, see :class:`ShiftedOperator`.  ``refactor_every=n > 1``: one
    factorisation per n frequencies, GMRES on the lagged factors in between (``krylov=`` sets its max_iter / restart / rtol).
    ``block=True``: the n frequencies of a group share the factors of its middle frequency and are solved side by side."""
    _need_flowsolver(flowsolver)
    n, nu, ny, nw = _freqresp_sizes(A, B, C, ww)
    if verbose:
        ww_ = np.atleast_1d(ww)
        logger.info("System dimensions: n=%d, nu=%d, ny=%d | Frequency points: nw=%d, w in [1e%g, 1e%g]", n, nu, ny, nw,
                    np.log10(ww_[0]), np.log10(ww_[-1]))
    op = ShiftedOperator(flowsolver, A, Q, refine=refine, pressure_pin=pressure_pin, krylov=_sweep_krylov(krylov, refactor_every, block))
    try:
        return frequency_response(op, B, C, ww, verbose, refactor_every, block)
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
                       krylov=None, block=None) -> np.ndarray:
    """X(w) = (jwQ - A)^-1 B for each w of ww (reference ``utils/linalg.py:331``).  Returns X [n, nu, nw] complex.
    ``pressure_pin``, ``refactor_every``, ``krylov``, ``block``: as :func:`get_frequency_response_sequential`."""
    _need_flowsolver(flowsolver)
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    B = np.asarray(B, dtype=float)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    n = A.shape[0]
    if B.shape[0] != n:
        raise ValueError(f"B {B.shape} does not match A of order {n}")
    op = ShiftedOperator(flowsolver, A, Q, refine=refine, pressure_pin=pressure_pin, krylov=_sweep_krylov(krylov, refactor_every, block))
    refactor_every = _check_refactor_every(op, refactor_every)
    X = np.zeros((n, B.shape[1], ww.size), dtype=complex)
    try:
        if _check_block(op, block):
            nu = B.shape[1]

            def solve_block(j0, j1, sigmas):
                X[:, :, j0:j1] = op.solve_block(B, sigmas).reshape(n, j1 - j0, nu).transpose(0, 2, 1)

            def per_frequency(ii):
                if ii % refactor_every == 0:
                    op.factor(1j * ww[ii])
                    X[:, :, ii] = op.solve(B)
                else:
                    X[:, :, ii] = _lagged(op, 1j * ww[ii], lambda: op.solve(B))

            _block_sweep(op, B, ww, refactor_every, solve_block, per_frequency, verbose)
            return X
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
                 verbose: bool = False, invert: bool = True) -> tuple[np.ndarray, np.ndarray, dict]:
    """Krylov-Schur iteration (Stewart 2001) for the ``nev`` eigenvalues of Op = (A - sigma E)^-1 E of largest modulus, i.e. the
    eigenvalues lambda = sigma + 1 / theta of the pencil (A, E) nearest ``sigma``.  Only the (ncv x ncv) Schur work runs here; the
    vectors live with ``backend``:

        backend.start(m, v0)          V_0 = Op v0 / |Op v0|, room for m + 1 basis vectors
        backend.step(j) -> (h, beta)  V_{j+1} beta = Op V_j - V_{0..j} h   (h complex [j + 1])
        backend.restart(Q)            V_{0..k} = V_{0..m} Q (Q [m, k]), V_k = V_m
        backend.ritz(Y, lam, vectors) -> (res [k, 3], X [n, k] or None): res = |A x - lam E x|, |A x|, |E x| of x = V_{0..m} Y

    A pair has converged when |A x - lam E x| / (|lam| |E x| + |A x|) <= tol.  Returns (lam [nev], X [n, nev], stats); the
    eigenvalues nearest sigma first, X with unit 2-norm columns.

    ``invert=False``: the eigenvalues theta of the backend's operator itself, largest modulus first (``sigma`` unused); the backend's
    ``ritz`` then returns res = |Op x - theta x|, |Op x|, |x| and the same test reads |Op x - theta x| / (|theta| |x| + |Op x|) <= tol
    (the resolvent operator of :func:`resolvent_gains`)."""
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
        lam = sigma + 1.0 / w[sel] if invert else w[sel]
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

    def set_op(self, kind: int) -> None:
        """0: the shift-invert operator (default); 1: the resolvent M^-H E^T M^-1 E (needs the adjoint factors)."""
        check(self.lib.fc_shifted_arnoldi_set_op(self.op._h, int(kind)))

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
               pin_shift: float = 1.0, operator: ShiftedOperator | None = None, left: bool = False, **slepc_options: Any):
    """The ``n`` eigenvalues of the pencil (A, B) nearest ``target`` and their eigenvectors (reference ``get_mat_vp_slepc``,
    ``utils/linalg.py:52-131``): shift-invert Krylov-Schur with the device's direct solver of A - target B.  Returns
    (valp [n] complex, vecp [N, n] complex in the W layout, unit 2-norm columns), nearest ``target`` first.  ``B`` is the mass
    matrix (E); it must lie on the flowsolver's CSR pattern like ``A`` (``B=None``, the standard problem, needs an identity on it,
    which the pressure block of the pattern does not have).  SLEPc-only options (eps_type, precond_type, ksp_type, mpd) are
    accepted and ignored.  ``pressure_pin="auto"`` (or a pressure dof): enclosed flows, the eigenvalues of the pencil
    (A - pin_shift e_k e_k^T, B), whose finite ones do not depend on ``pin_shift``.  ``krylov``: the GMRES rescue of
    :class:`ShiftedOperator`.  ``operator``: a :class:`ShiftedOperator` of (A, B) to reuse (one symbolic phase for several
    targets); it is not released.
    ``left=True``: returns (valp, vecp, vecl) with the left eigenvectors, ``vecl[:, i]^H A = valp[i] vecl[:, i]^H B``, scaled to
    ``vecl[:, i]^H B vecp[:, i] = 1``.  They come from a second Krylov-Schur in the adjoint mode of the operator -- the shift-invert
    of (A^T, B^T) at conj(target), on the SAME factors -- whose pairs (mu, z) are matched to valp = conj(mu)."""
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
        if left:
            Yl, lstats = _left_modes(op, lam, X, n, ncv, complex(target), tol, niter, verbose)
            stats = dict(stats, left=lstats)
    finally:
        if operator is None:
            op.release()
    if return_eigensolver:
        return ((lam, X, Yl) if left else (lam, X)), stats
    return (lam, X, Yl) if left else (lam, X)


def _left_modes(op: ShiftedOperator, lam: np.ndarray, X: np.ndarray, n: int, ncv: int, target: complex, tol: float, niter: int, verbose: bool):
    """Left eigenvectors for the right pairs (lam, X) on the factors ``op`` holds: Krylov-Schur in the adjoint mode with
    sigma = conj(target), pairs (mu, z) matched to lam = conj(mu), y = z scaled to y^H B x = 1 (B x through the device's SpMV)."""
    with op.adjoint():
        mu, Zl, lstats = krylov_schur(DeviceKrylov(op), n, ncv, np.conj(target), tol, niter, verbose=verbose)
    Yl = np.empty_like(X)
    free = list(range(mu.size))
    for i, v in enumerate(lam):
        j = min(free, key=lambda q: abs(np.conj(mu[q]) - v))
        if abs(np.conj(mu[j]) - v) > 1e3 * max(tol, 1e-12) * max(1.0, abs(v)):
            raise RuntimeError(f"get_mat_vp(left=True): no left pair for the eigenvalue {v} (adjoint eigenvalues {mu})")
        free.remove(j)
        Bx = op.spmv(1.0, 0.0, X[:, i])
        d = np.vdot(Zl[:, j], Bx)
        if d == 0.0:
            raise RuntimeError(f"get_mat_vp(left=True): the left and right vectors of {v} are B-orthogonal (defective eigenvalue?)")
        Yl[:, i] = Zl[:, j] / np.conj(d)
    return Yl, lstats


def resolvent_gains(A, E, ww, n: int = 1, *, flowsolver=None, ncv: int = 20, tol: float = 1e-10, vectors: bool = False, refine: int = 2,
                    pressure_pin=None, krylov=None, maxit: int = 100, verbose: bool = False):
    """The ``n`` largest resolvent gains gamma = max |q|_E / |g|_E of q = (i w E - A)^-1 E g at every w of ``ww`` (E symmetric
    positive semidefinite: |x|_E^2 = x^H E x).  Returns gains [n, nw], largest first; ``vectors=True``: (gains, G, Q) with the optimal
    forcings G [N, n, nw] (g^H E g = 1) and their responses Q [N, n, nw] = M^-1 E g (q^H E q = gamma^2).

    Per frequency ONE factorisation of M = i w E - A and one transposed export; then Arnoldi on Op_R = M^-H E^T M^-1 E on the device
    (``fc_shifted_arnoldi_set_op(1)``: a direct and an adjoint solve per step on the same factors), whose eigenvalues are gamma^2:
    ``ncv`` steps, and thick restarts (:func:`krylov_schur`, at most ``maxit``) while one of the ``n`` largest Ritz pairs misses
    |Op_R x - theta x| <= tol (|theta| |x| + |Op_R x|) (``fc_shifted_ritz``); RuntimeError when ``maxit`` restarts do not get there."""
    _need_flowsolver(flowsolver)
    ww = np.atleast_1d(np.asarray(ww, dtype=float))
    n, m = int(n), int(ncv)
    if not 1 <= n < m:
        raise ValueError(f"need 1 <= n < ncv, got n={n}, ncv={m}")
    N = A.shape[0]
    gains = np.zeros((n, ww.size))
    G = np.zeros((N, n, ww.size), dtype=complex) if vectors else None
    Q = np.zeros((N, n, ww.size), dtype=complex) if vectors else None
    op = ShiftedOperator(flowsolver, A, E, refine=refine, pressure_pin=pressure_pin, krylov=krylov)
    try:
        kry = DeviceKrylov(op)
        for iw, w in enumerate(ww):
            op.factor(1j * w)
            if iw == 0:  # the adjoint array: built once, re-exported by every later factor()
                op.set_adjoint(True)
                op.set_adjoint(False)
                kry.set_op(1)
            theta, X, stats = krylov_schur(kry, n, m, 0.0, tol, maxit, invert=False)
            if np.any(theta.real <= 0.0) or np.any(np.abs(theta.imag) > 1e-6 * np.abs(theta)):
                raise RuntimeError(f"resolvent_gains: w = {w:g}: Ritz values {theta} are not real positive (is E symmetric positive "
                                   "semidefinite?)")
            gains[:, iw] = np.sqrt(theta.real)
            if verbose:
                logger.info("  [%d/%d] w=%.4e | gains %s | %d restart(s)", iw + 1, ww.size, w, np.array2string(gains[:, iw], precision=6),
                            stats["restarts"])
            if vectors:
                for c in range(n):
                    g = X[:, c]
                    Eg = op.spmv(1.0, 0.0, g)
                    nrm = np.sqrt(np.vdot(g, Eg).real)
                    G[:, c, iw] = g / nrm
                    Q[:, c, iw] = op.solve(Eg / nrm)
    finally:
        op.release()
    return (gains, G, Q) if vectors else gains


#: the reference's name
get_mat_vp_slepc = get_mat_vp

__all__ = ["get_frequency_response_sequential", "get_frequency_response_parallel", "get_frequency_response_mpi", "get_field_response",
           "get_mat_vp", "get_mat_vp_slepc", "krylov_schur", "frequency_response", "ShiftedOperator", "DeviceKrylov", "values_on_pattern",
           "resolvent_gains"]
