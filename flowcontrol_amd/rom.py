"""Balanced reduced-order models from frequency snapshots kept on the device (balanced POD; DESIGN §4.2, "Reduced models").

For ``E dx/dt = A x + B u, y = C x`` (E singular: pressure rows) and quadrature nodes ``w_j > 0`` with weights ``d_j``:

    X_j = (i w_j E - A)^-1 B,   Z_j = (i w_j E - A)^-H C^T            direct and adjoint solves on ONE factorisation per frequency
    Xs = [s_j Re X_j, s_j Im X_j]_j,  Zs likewise,  s_j = sqrt(d_j / pi)      Xs Xs^T, Zs Zs^T: quadratures of the Gramians over the band
    G_E = Zs^T E Xs = U S V^T                                         the Hankel singular values S
    Phi = Xs V_r S_r^-1/2,  Psi = Zs U_r S_r^-1/2                     Psi^T E Phi = I
    A_r = S_r^-1/2 U_r^T (Zs^T A Xs) V_r S_r^-1/2,  B_r = S_r^-1/2 U_r^T (Zs^T B),  C_r = (C Xs) V_r S_r^-1/2,  D_r = 0

The snapshots never leave the device: the solver pushes every solution into a snapshot set (``fc_shifted_snap_push``), three Gram
products are formed there (``fc_shifted_snap_gram``: ``Zs^T E Xs``, ``Zs^T A Xs``, ``Zs^T B``), ``C Xs`` comes from the projection
that also gives the full-order response ``H(i w_j)``, and the SVD and the scaling are m x m work on the host.  The modes ``Phi``,
``Psi`` are formed on the device and cross only with ``modes=True``.  The construction is defined for an unstable plant too, as long
as no pole lies on the imaginary axis: the frequency-domain Gramians are then those of the stable / antistable splitting.
"""

from __future__ import annotations

import logging
import time
from dataclasses import dataclass

import numpy as np

from . import linalg

logger = logging.getLogger(__name__)


def log_quadrature(w_lo: float, w_hi: float, nq: int) -> tuple[np.ndarray, np.ndarray]:
    """Gauss-Legendre in log w on [w_lo, w_hi]: nodes ``ww`` [nq] and weights with ``sum f(ww) * weights ~ int f dw``."""
    w_lo, w_hi, nq = float(w_lo), float(w_hi), int(nq)
    if not (0.0 < w_lo < w_hi) or not np.isfinite(w_hi):
        raise ValueError(f"the band must satisfy 0 < w_lo < w_hi, got [{w_lo}, {w_hi}]")
    if nq < 1:
        raise ValueError(f"nq must be >= 1, got {nq}")
    x, g = np.polynomial.legendre.leggauss(nq)
    L = np.log(w_hi / w_lo)
    ww = w_lo * np.exp(0.5 * (x + 1.0) * L)
    return ww, 0.5 * L * g * ww


def _check_quadrature(ww, weights, band, nq) -> tuple[np.ndarray, np.ndarray]:
    if ww is None:
        if band is None or nq is None:
            raise ValueError("give the quadrature as (ww, weights) or as (band=(w_lo, w_hi), nq=)")
        return log_quadrature(band[0], band[1], nq)
    if weights is None:
        raise ValueError("ww needs its quadrature weights")
    ww = np.atleast_1d(np.asarray(ww, dtype=float)).ravel()
    weights = np.atleast_1d(np.asarray(weights, dtype=float)).ravel()
    if ww.size != weights.size or ww.size < 1:
        raise ValueError(f"ww has {ww.size} node(s), weights has {weights.size}")
    if not np.all(np.isfinite(ww)) or not np.all(ww > 0.0):
        raise ValueError("the quadrature frequencies must be positive and finite")
    if not np.all(np.isfinite(weights)) or not np.all(weights > 0.0):
        raise ValueError("the quadrature weights must be positive and finite")
    return ww, weights


def select_order(hsv: np.ndarray, tol: float) -> int:
    """The smallest r with ``2 * sum(hsv[r:]) <= tol * hsv[0]``."""
    hsv = np.asarray(hsv, dtype=float)
    tails = 2.0 * np.r_[np.cumsum(hsv[::-1])[::-1], 0.0]  # tails[r] = 2 sum_{i >= r} hsv_i
    return int(np.argmax(tails <= float(tol) * hsv[0]))


@dataclass
class ReducedModel:
    """``dx_r/dt = A x_r + B u, y = C x_r + D u`` of order ``r``; ``hsv``: all Hankel singular values of the quadrature; ``H``
    [nq, ny, nu]: the full-order response at the nodes ``ww``; ``error_bound = 2 * sum(hsv[r:])``; ``Phi``, ``Psi`` [n, r] with
    ``modes=True`` only."""

    A: np.ndarray
    B: np.ndarray
    C: np.ndarray
    D: np.ndarray
    hsv: np.ndarray
    r: int
    ww: np.ndarray
    weights: np.ndarray
    H: np.ndarray | None = None
    error_bound: float = 0.0
    Phi: np.ndarray | None = None
    Psi: np.ndarray | None = None
    TL: np.ndarray | None = None  # S_r^-1/2 U_r^T [r, mz] and V_r S_r^-1/2 [mx, r]: Psi = Zs TL^T, Phi = Xs TR
    TR: np.ndarray | None = None

    def frequency_response(self, ww) -> np.ndarray:
        """H_r(i w) = C (i w I - A)^-1 B + D for every w of ww: [nw, ny, nu] complex."""
        ww = np.atleast_1d(np.asarray(ww, dtype=float))
        eye = np.eye(self.r)
        return np.stack([self.C @ np.linalg.solve(1j * w * eye - self.A, self.B.astype(complex)) + self.D for w in ww])

    def eigenvalues(self) -> np.ndarray:
        return np.linalg.eigvals(self.A)

    def save(self, path) -> None:
        """A ``.mat`` file with the keys A, B, C, D (what ``Controller.from_file`` reads)."""
        import scipy.io as sio

        sio.savemat(str(path), {"A": self.A, "B": self.B, "C": self.C, "D": self.D})


def balancing_factors(GE: np.ndarray, r: int | None = None, tol: float | None = None):
    """SVD of the Hankel matrix ``GE = Zs^T E Xs`` and the two small factors of a model of order r: (hsv, r, TL [r, mz], TR [mx, r])
    with ``TL = S_r^-1/2 U_r^T`` and ``TR = V_r S_r^-1/2`` (``Psi = Zs TL^T``, ``Phi = Xs TR``).  ``r`` is given, or the smallest order
    with ``2 * sum(hsv[r:]) <= tol * hsv[0]``."""
    U, S, Vt = np.linalg.svd(np.asarray(GE, dtype=float), full_matrices=False)
    if S.size == 0 or not S[0] > 0.0:
        raise ValueError("the Hankel matrix is zero: no reduced model")
    rank = int(np.sum(S > S[0] * max(GE.shape) * np.finfo(float).eps))
    if r is None:
        if tol is None:
            raise ValueError("give the order r= or the tolerance tol=")
        r = max(1, min(select_order(S, tol), rank))
    r = int(r)
    if not 1 <= r <= rank:
        raise ValueError(f"r = {r} is outside 1 .. {rank}, the numerical rank of the Hankel matrix ({GE.shape[0]} x {GE.shape[1]})")
    isq = 1.0 / np.sqrt(S[:r])
    return S, r, isq[:, None] * U[:, :r].T, Vt[:r].T * isq[None, :]


def reduced_from_grams(GE, GA, ZtB, CXs, ww, weights, H=None, r: int | None = None, tol: float | None = None) -> ReducedModel:
    """The reduced model from the small matrices alone: ``GE = Zs^T E Xs``, ``GA = Zs^T A Xs``, ``ZtB = Zs^T B`` [mz, nu],
    ``CXs = C Xs`` [ny, mx]."""
    hsv, r, TL, TR = balancing_factors(GE, r, tol)
    ZtB, CXs = np.asarray(ZtB, dtype=float), np.asarray(CXs, dtype=float)
    return ReducedModel(A=TL @ np.asarray(GA, dtype=float) @ TR, B=TL @ ZtB, C=CXs @ TR, D=np.zeros((CXs.shape[0], ZtB.shape[1])), hsv=hsv, r=r,
                        ww=np.asarray(ww, dtype=float), weights=np.asarray(weights, dtype=float), H=H, error_bound=float(2.0 * np.sum(hsv[r:])),
                        TL=TL, TR=TR)


def snapshot_sweep(op, B: np.ndarray, Cm: np.ndarray, ww: np.ndarray, weights: np.ndarray, verbose: bool = True, on_factor=None):
    """The sweep of :func:`balanced_rom` on a :class:`linalg.ShiftedOperator`: per frequency one factorisation, the direct solves
    pushed into set 0, ``C X`` projected, the adjoint solves (a pointer swap away) pushed into set 1.  Returns (H [nq, ny, nu],
    CXs [ny, 2 nq nu]); the sets stay on the device.  ``on_factor(j, op)`` (optional) is called after the factorisation of node j."""
    nu, ny, nq = B.shape[1], Cm.shape[0], ww.size
    H = np.zeros((nq, ny, nu), dtype=complex)
    CXs = np.zeros((ny, 2 * nq * nu))
    Ct = np.ascontiguousarray(Cm.T)
    for j, (w, d) in enumerate(zip(ww, weights)):
        t1 = time.time()
        s = float(np.sqrt(d / np.pi))
        op.factor(1j * w)
        if on_factor is not None:
            on_factor(j, op)
        if j == 0:
            op.snap_reserve(0, nq * nu)
            op.snap_reserve(1, nq * ny)
            op.snap_clear(0)
            op.snap_clear(1)
        op.solve(B, download=False)
        op.snap_push(0, nu, s)
        H[j] = op.project(Cm, nu)
        CXs[:, 2 * j * nu:2 * (j + 1) * nu:2] = s * H[j].real
        CXs[:, 2 * j * nu + 1:2 * (j + 1) * nu:2] = s * H[j].imag
        op.set_adjoint(1)
        try:
            op.solve(Ct, download=False)
            op.snap_push(1, ny, s)
        finally:
            op.set_adjoint(0)
        if verbose:
            logger.info("  [%d/%d] w=%.4e | max|H|=%.4e | elapsed: %.3fs", j + 1, nq, w, np.max(np.abs(H[j])), time.time() - t1)
    return H, CXs


def balanced_rom(A, B, C, E, ww=None, weights=None, *, band=None, nq=None, r=None, tol=None, flowsolver=None, modes: bool = False,
                 refine: int = 2, pressure_pin=None, krylov=None, verbose: bool = True, operator=None) -> ReducedModel:
    """Balanced truncation of ``E dx/dt = A x + B u, y = C x`` from frequency snapshots on the device of ``flowsolver``.

    The quadrature is ``(ww, weights)`` or Gauss-Legendre in log w on ``band`` with ``nq`` nodes (:func:`log_quadrature`).  ``r``: the
    order, or ``tol``: the smallest order with ``2 * sum(hsv[r:]) <= tol * hsv[0]``.  ``modes=True`` also returns ``Phi`` and ``Psi``
    (formed on the device).  ``refine``, ``pressure_pin``, ``krylov``: as :class:`linalg.ShiftedOperator` (``krylov`` only rescues a
    solve whose refinement stalls; every frequency is factorised).  ``operator``: a :class:`linalg.ShiftedOperator` of (A, E) to run
    on instead of a new one (as in ``get_mat_vp``); it is not released and keeps the snapshot sets, for inspection."""
    ww, weights = _check_quadrature(ww, weights, band, nq)
    if r is None and tol is None:
        raise ValueError("give the order r= or the tolerance tol=")
    if r is not None and int(r) < 1:
        raise ValueError(f"r must be >= 1, got {r}")
    if operator is None:
        linalg._need_flowsolver(flowsolver)
    B = np.asarray(B, dtype=float)
    B = B.reshape(-1, 1) if B.ndim == 1 else B
    Cm = np.asarray(C.toarray() if hasattr(C, "toarray") else C, dtype=float)
    Cm = Cm.reshape(1, -1) if Cm.ndim == 1 else Cm
    n = A.shape[0]
    if B.shape[0] != n or Cm.shape[1] != n:
        raise ValueError(f"B {B.shape} / C {Cm.shape} do not match A of order {n}")
    nu = B.shape[1]
    op = operator if operator is not None else linalg.ShiftedOperator(flowsolver, A, E, refine=refine, pressure_pin=pressure_pin, krylov=krylov)
    t0 = time.time()
    try:
        H, CXs = snapshot_sweep(op, B, Cm, ww, weights, verbose)
        op.snap_reserve(2, nu)
        op.snap_clear(2)
        op.snap_load(2, B)
        GE = op.snap_gram(1, 0, 1)
        GA = op.snap_gram(1, 0, 2)
        ZtB = op.snap_gram(1, 2, 0)[:, 0::2]  # (B is real: its imaginary parts are zero columns)
        rom = reduced_from_grams(GE, GA, ZtB, CXs, ww, weights, H=H, r=r, tol=tol)
        if modes:
            rom.Phi = op.snap_combine(0, rom.TR)
            rom.Psi = op.snap_combine(1, rom.TL.T)
        if verbose:
            logger.info("Reduced model of order %d from %d frequencies in %.3fs (error bound %.3e).", rom.r, ww.size, time.time() - t0,
                        rom.error_bound)
        return rom
    finally:
        if operator is None:
            op.release()
