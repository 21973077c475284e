"""Continuous-time LTI controller with cached ZOH discretisation.

Mirror of the reference's ``src/flowcontrol/controller.py`` (``Controller(A, B, C, D, file, x0)``,
``from_file``, ``from_matrices``, ``step(y, dt)``, ``reset``, ``x`` and the ``+ * inv`` algebra).
The reference subclasses ``control.StateSpace`` and discretises with ``control.c2d(..., "zoh")``
(``controller.py:121-134``); python-control is not a dependency here — ZOH is the exact
augmented-matrix exponential, which is what ``c2d`` computes.
"""

from __future__ import annotations

import warnings
from pathlib import Path

import numpy as np
import scipy.io as sio
from numpy.typing import NDArray
from scipy.linalg import expm


def read_matfile(path):
    """Load a MATLAB v5 file without the duplicate-variable warning (``utils/lticontrol.py:20-24``)."""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", "Duplicate variable name*")
        return sio.loadmat(str(path))


class Controller:
    def __init__(self, A, B, C, D, file: Path | None = None, x0: NDArray[np.float64] | None = None):
        A = np.atleast_2d(np.array(A, dtype=np.float64))
        n = A.shape[0] if A.size else 0
        A = A.reshape(n, n)
        B = np.array(B, dtype=np.float64)
        B = B.reshape(n, -1) if n else np.zeros((0, max(1, B.size)))
        m = B.shape[1]
        C = np.array(C, dtype=np.float64)
        C = C.reshape(-1, n) if n else np.zeros((max(1, C.size), 0))
        p = C.shape[0]
        D = np.array(D, dtype=np.float64)
        D = np.full((p, m), float(D.reshape(-1)[0])) if D.size == 1 else D.reshape(p, m)
        self.A, self.B, self.C, self.D = A, B, C, D
        self.nstates, self.ninputs, self.noutputs = n, m, p
        self.file = file
        self.x = np.array(x0, dtype=np.float64) if x0 is not None else np.zeros((n,))

    @classmethod
    def from_file(cls, file: Path, x0=None) -> "Controller":
        m = read_matfile(file)
        return cls(m["A"], m["B"], m["C"], m["D"], x0=x0, file=file)

    @classmethod
    def from_matrices(cls, A, B, C, D, file: Path | None = None, x0=None) -> "Controller":
        return cls(A, B, C, D, x0=x0, file=file)

    def _discretize(self, dt: float) -> None:
        n, m = self.nstates, self.ninputs
        M = np.zeros((n + m, n + m))
        M[:n, :n] = self.A * dt
        M[:n, n:] = self.B * dt
        E = expm(M)
        self._Ad, self._Bd = E[:n, :n], E[:n, n:]
        self._Cd, self._Dd = self.C, self.D
        self._dt = dt

    def discrete(self, dt: float):
        """``(Ad, Bd, Cd, Dd)`` of the zero-order-hold discretisation at ``dt`` — the matrices :meth:`step` advances with (cached)."""
        if not hasattr(self, "_dt") or self._dt != dt:
            self._discretize(dt)
        return self._Ad, self._Bd, self._Cd, self._Dd

    def discrete_gradient(self, dt: float, gAd, gBd):
        """Pull a gradient with respect to the discrete ``(Ad, Bd)`` of :meth:`discrete` back through the zero-order hold:
        ``(gA, gB)`` with respect to the continuous-time ``(A, B)``.  With ``X = [[A, B], [0, 0]] dt`` and ``Gbar = [[gAd, gBd], [0, 0]]``
        the adjoint of the Frechet derivative of ``expm`` at ``X`` is the Frechet derivative at ``X^T``: the top blocks of
        ``expm_frechet(X^T, Gbar)`` times ``dt``.  ``C`` and ``D`` pass through the discretisation unchanged."""
        from scipy.linalg import expm_frechet

        n, m = self.nstates, self.ninputs
        X = np.zeros((n + m, n + m))
        X[:n, :n] = self.A * dt
        X[:n, n:] = self.B * dt
        Gbar = np.zeros((n + m, n + m))
        Gbar[:n, :n] = np.asarray(gAd, dtype=np.float64).reshape(n, n)
        Gbar[:n, n:] = np.asarray(gBd, dtype=np.float64).reshape(n, m)
        L = expm_frechet(X.T, Gbar, compute_expm=False)
        return L[:n, :n] * dt, L[:n, n:] * dt

    def discrete_tangent(self, dt: float, dA, dB):
        """Push a direction ``(dA, dB)`` of the continuous-time ``(A, B)`` forward through the zero-order hold: ``(dAd, dBd)``, the
        directional derivative of :meth:`discrete` -- the forward counterpart of :meth:`discrete_gradient`.  With
        ``X = [[A, B], [0, 0]] dt`` these are the top blocks of ``expm_frechet(X, [[dA, dB], [0, 0]] dt)``."""
        from scipy.linalg import expm_frechet

        n, m = self.nstates, self.ninputs
        X = np.zeros((n + m, n + m))
        X[:n, :n] = self.A * dt
        X[:n, n:] = self.B * dt
        E = np.zeros((n + m, n + m))
        E[:n, :n] = np.asarray(dA, dtype=np.float64).reshape(n, n) * dt
        E[:n, n:] = np.asarray(dB, dtype=np.float64).reshape(n, m) * dt
        L = expm_frechet(X, E, compute_expm=False)
        return L[:n, :n], L[:n, n:]

    def step(self, y, dt: float) -> NDArray[np.float64]:
        """u = Cd x + Dd y ; x ← Ad x + Bd y  (``controller.py:136-159``)."""
        if not hasattr(self, "_dt") or self._dt != dt:
            self._discretize(dt)
        y = np.atleast_1d(np.asarray(y, dtype=np.float64))
        u = self._Cd @ self.x + self._Dd @ y
        self.x = self._Ad @ self.x + self._Bd @ y
        return u

    def reset(self) -> None:
        self.x = np.zeros((self.nstates,))

    # ── algebra (parallel, series, inverse) preserving the Controller type ───
    def _coerce(self, other) -> "Controller":
        if isinstance(other, Controller):
            return other
        g = np.atleast_2d(np.asarray(other, dtype=np.float64))
        return Controller(np.zeros((0, 0)), np.zeros((0, g.shape[1])), np.zeros((g.shape[0], 0)), g)

    def _with_state(self, K: "Controller", other) -> "Controller":
        if isinstance(other, Controller):
            K.x = np.concatenate((self.x, other.x), axis=0)
        return K

    def __add__(self, other) -> "Controller":
        o = self._coerce(other)
        n1, n2 = self.nstates, o.nstates
        A = np.block([[self.A, np.zeros((n1, n2))], [np.zeros((n2, n1)), o.A]])
        return self._with_state(Controller(A, np.vstack([self.B, o.B]), np.hstack([self.C, o.C]), self.D + o.D), other)

    __radd__ = __add__

    def __mul__(self, other) -> "Controller":
        """Series connection ``self ∘ other`` (other acts first), states ordered [self, other]."""
        o = self._coerce(other)
        n1, n2 = self.nstates, o.nstates
        A = np.block([[self.A, self.B @ o.C], [np.zeros((n2, n1)), o.A]])
        B = np.vstack([self.B @ o.D, o.B])
        C = np.hstack([self.C, self.D @ o.C])
        return self._with_state(Controller(A, B, C, self.D @ o.D), other)

    def __rmul__(self, other) -> "Controller":
        return self._coerce(other) * self

    def inv(self) -> "Controller":
        Di = np.linalg.inv(self.D)
        return Controller(self.A - self.B @ Di @ self.C, self.B @ Di, -Di @ self.C, Di)


def pack_controllers(controllers, dt: float, n_sens: int, n_act: int, feedback=None) -> dict:
    """The arrays of a device controller bank (``fc_set_controllers``) for ``controllers`` stepped at ``dt``: simulation-major,
    every matrix row-major, each controller zero-padded to the bank's ``nx`` / ``nuc`` (padded states stay zero and feed nothing).

    ``feedback``: ``None`` — the reference loop, ``yc = -y_meas[0]`` — or a pair ``(G, g0)``, ``yc = G @ y_meas + g0`` with ``G`` of
    shape (nyc, n_sens), shared by all controllers or one per controller (k, nyc, n_sens).  ``S`` carries the controller's outputs to
    the actuators as the host loops do: one output goes to every actuator, ``n_act`` outputs go one to one.

    Returns ``{"k", "nx", "nyc", "nuc", "Ad", "Bd", "C", "D", "x0", "G", "g0", "S", "sizes"}``; ``sizes[i]`` = (nstates, noutputs) of
    controller i, which is what :func:`unpack_controllers` needs to undo the padding."""
    controllers = list(controllers)
    k = len(controllers)
    if k < 1:
        raise ValueError("at least one controller")
    for K in controllers:
        if not isinstance(K, Controller):
            raise TypeError(f"a device controller bank holds Controller instances (LTI), got {type(K).__name__}")
    if feedback is None:
        G = np.zeros((1, n_sens))
        G[0, 0] = -1.0
        g0 = np.zeros(1)
    elif callable(feedback):
        raise TypeError("a Python callable cannot run on the device: give feedback as None or as a pair (G, g0)")
    else:
        G, g0 = feedback
        G = np.asarray(G, dtype=np.float64)
        if G.ndim == 1:
            G = G.reshape(1, -1)
        g0 = np.zeros(G.shape[-2]) if g0 is None else np.asarray(g0, dtype=np.float64)
    nyc = G.shape[-2]
    if G.shape[-1] != n_sens:
        raise ValueError(f"G has {G.shape[-1]} columns, the solver has {n_sens} sensors")
    Gk = np.broadcast_to(G, (k, nyc, n_sens)).copy()
    g0k = np.broadcast_to(g0.reshape(-1, nyc), (k, nyc)).copy()
    nx = max(K.nstates for K in controllers)
    nuc = max(K.noutputs for K in controllers)
    Ad, Bd = np.zeros((k, nx, nx)), np.zeros((k, nx, nyc))
    Cd, Dd = np.zeros((k, nuc, nx)), np.zeros((k, nuc, nyc))
    x0, S = np.zeros((k, nx)), np.zeros((k, n_act, nuc))
    sizes = []
    for i, K in enumerate(controllers):
        n, p = K.nstates, K.noutputs
        if K.ninputs != nyc:
            raise ValueError(f"controller {i} takes {K.ninputs} inputs, the feedback map gives {nyc}")
        if p not in (1, n_act):
            raise ValueError(f"controller {i} has {p} outputs: expected 1 (applied to every actuator) or {n_act}")
        a, b, c, d = K.discrete(dt)
        Ad[i, :n, :n], Bd[i, :n], Cd[i, :p, :n], Dd[i, :p] = a, b, c, d
        x0[i, :n] = np.asarray(K.x, dtype=np.float64).reshape(-1)
        if p == n_act:
            S[i, :, :p] = np.eye(n_act)
        else:
            S[i, :, 0] = 1.0
        sizes.append((n, p))
    return {"k": k, "nx": nx, "nyc": nyc, "nuc": nuc, "Ad": Ad, "Bd": Bd, "C": Cd, "D": Dd, "x0": x0, "G": Gk, "g0": g0k, "S": S,
            "sizes": sizes}


def loop_signal_rows(w, n_steps: int, shape: tuple, name: str):
    """``w`` as a float64 array of shape ``(n_steps, *shape)`` (``None`` stays ``None``): the rows a closed-loop run adds step by step."""
    if w is None:
        return None
    w = np.asarray(w, dtype=np.float64)
    if shape[-1] == 1 and w.shape == (n_steps, *shape[:-1]):  # a bare series for a one-wide signal
        w = w.reshape((n_steps, *shape))
    if w.shape != (n_steps, *shape):
        raise ValueError(f"{name} must have shape {(n_steps, *shape)}, got {w.shape}")
    return np.ascontiguousarray(w)


def loop_signal_rows_batch(w, n_steps: int, k: int, width: int, name: str):
    """The same for k simulations, ``(n_steps, k, width)``; one row set ``(n_steps, width)`` is shared by all of them."""
    if w is None:
        return None
    w = np.asarray(w, dtype=np.float64)
    if w.ndim <= 2:
        w = np.broadcast_to(loop_signal_rows(w, n_steps, (width,), name)[:, None, :], (n_steps, k, width))
    return loop_signal_rows(w, n_steps, (k, width), name)


def loop_limits(u_limits, shape: tuple):
    """``u_limits = (lo, hi)`` — scalars, per actuator, or anything that broadcasts to ``shape`` — as two float64 arrays of ``shape``
    (``None`` stays ``None``; a ``None`` side is unlimited).  NaN and ``lo > hi`` are refused, as the device refuses them."""
    if u_limits is None:
        return None
    lo, hi = u_limits
    lo = np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), shape).copy()
    hi = np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), shape).copy()
    if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(lo > hi):
        raise ValueError("u_limits: NaN or lo > hi")
    return lo, hi


def unpack_controllers(bank: dict) -> list:
    """Per controller ``(Ad, Bd, Cd, Dd, x)`` without the padding of :func:`pack_controllers`."""
    out = []
    for i, (n, p) in enumerate(bank["sizes"]):
        out.append((bank["Ad"][i, :n, :n].copy(), bank["Bd"][i, :n].copy(), bank["C"][i, :p, :n].copy(), bank["D"][i, :p].copy(),
                    bank["x0"][i, :n].copy()))
    return out


def bank_transposed(bank: dict) -> np.ndarray:
    """The bank as the device holds it (``csrc/fc_ctrl.hip.h``): per controller one block
    ``[Ad^T | Bd^T | C^T | D^T | G^T | g0 | S^T]``, every matrix transposed so that consecutive lanes read consecutive rows."""
    return np.stack([np.concatenate([bank[m][i].T.ravel() if m != "g0" else bank[m][i].ravel() for m in ("Ad", "Bd", "C", "D", "G", "g0", "S")])
                     for i in range(bank["k"])])


def bank_step(bank: dict, x: np.ndarray, y_meas: np.ndarray, blocks: np.ndarray | None = None, *, w_y=None, w_u=None, u_lo=None, u_hi=None):
    """One step of the bank recursion in numpy, ``(u, x_new)``: the model of ``fc_ctrl_step``.  With ``blocks`` (from
    :func:`bank_transposed`) the matrices are read back from the device layout.

    ``w_y`` (k, nyc) is added to ``yc`` behind ``G y + g0`` (the state sees the disturbed ``yc``), ``w_u`` (k, n_act) behind ``S uc``,
    and ``u_lo`` / ``u_hi`` (k, n_act; scalars and rows broadcast; ±inf: no limit) clamp the sum: ``u = min(max(v, u_lo), u_hi)`` — the
    kernel's order.  The state is not corrected for saturation.  ``None`` skips a term: without keywords the result is the one of the
    plain recursion, bit for bit."""
    k, nx, nyc, nuc = bank["k"], bank["nx"], bank["nyc"], bank["nuc"]
    n_sens, n_act = bank["G"].shape[2], bank["S"].shape[1]
    w_y = None if w_y is None else np.broadcast_to(np.asarray(w_y, dtype=np.float64), (k, nyc))
    w_u = None if w_u is None else np.broadcast_to(np.asarray(w_u, dtype=np.float64), (k, n_act))
    if (u_lo is None) != (u_hi is None):
        raise ValueError("give both limits or neither")
    if u_lo is not None:
        u_lo = np.broadcast_to(np.asarray(u_lo, dtype=np.float64), (k, n_act))
        u_hi = np.broadcast_to(np.asarray(u_hi, dtype=np.float64), (k, n_act))
    u, xn = np.zeros((k, n_act)), np.zeros((k, nx))
    for i in range(k):
        if blocks is None:
            Ad, Bd, C, D, G, g0, S = (bank[m][i] for m in ("Ad", "Bd", "C", "D", "G", "g0", "S"))
        else:
            o, mats = 0, []
            for r, c in ((nx, nx), (nx, nyc), (nuc, nx), (nuc, nyc), (nyc, n_sens), (nyc, 1), (n_act, nuc)):
                mats.append(np.ascontiguousarray(blocks[i, o : o + r * c].reshape(c, r).T))
                o += r * c
            Ad, Bd, C, D, G, g0, S = mats
            g0 = g0.reshape(-1)
        yc = G @ y_meas[i] + g0
        if w_y is not None:
            yc = yc + w_y[i]
        v = S @ (C @ x[i] + D @ yc)
        if w_u is not None:
            v = v + w_u[i]
        if u_lo is not None:
            v = np.minimum(np.maximum(v, u_lo[i]), u_hi[i])
        u[i] = v
        xn[i] = Ad @ x[i] + Bd @ yc
    return u, xn
