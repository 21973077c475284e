"""State snapshots kept on the device, and POD / DMD from them.

A :class:`SnapshotBank` is the Python face of the ``fc_state_snap_*`` entry points: once reserved, the time-stepping handle gathers
the state of every ``every``-th step into a column ``x_j`` (W layout ``[ux | uy | p]``, original numbering) with one launch of the step
itself -- ``step``, ``run`` and ``run_closed_loop`` keep their rate, nothing is downloaded.  What is computed from the columns
``X = [x_0 .. x_{m-1}]`` is computed where they are:

    G = X^T M X                       mass-weighted Gram on the fp64 matrix cores (``weight="energy"``: the velocity mass matrix, so that
                                      ``G_jj / 2`` is the perturbation energy of snapshot j; ``weight=None``: M = I)
    POD:  G = V S^2 V^T,  Phi = X V_r S_r^-1            (method of snapshots; Phi^T M Phi = I)
    DMD:  X1 = x_0 .. x_{m-2},  X2 = x_1 .. x_{m-1}:  X1^T M X1 = V S^2 V^T,  Atilde = S_r^-1 V_r^T (X1^T M X2) V_r S_r^-1,
          Atilde w = mu w,  modes X2 V_r S_r^-1 w

Only m x m matrices cross to the host, where the eigenproblems are solved; N-long vectors (modes, the mean) cross on request.  The
snapshot spacing is ``every * dt``: ``lam = log(mu) / (every dt)`` is the continuous-time rate, and ``lam_bdf2`` the eigenvalue of the
pencil (A, E) that the BDF2 scheme maps onto ``mu`` -- exact for the linear equations, where every term is implicit: one step multiplies
an eigenvector by ``mu_1`` with ``(3 mu_1^2 - 4 mu_1 + 1) / (2 dt mu_1^2) = lambda``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import SLOT_MASS


def _weight_slot(weight) -> int:
    if weight is None or weight == "identity":
        return -1
    if weight == "energy":
        return SLOT_MASS
    if isinstance(weight, (int, np.integer)) and not isinstance(weight, bool):
        return int(weight)
    raise ValueError(f"weight must be 'energy', None / 'identity' or a matrix slot, got {weight!r}")


class SnapshotBank:
    """State history of one device handle: set 0 holds the captured states, set 1 vectors loaded from the host or combined on the
    device (kept POD / DMD modes).  Built by :meth:`FlowSolver.record_snapshots` (or from a ``DeviceSolver`` directly)."""

    def __init__(self, dev, capacity: int, every: int = 1, first: int = 0):
        if int(capacity) < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        if getattr(dev, "world", 1) > 1 or getattr(dev, "part", None) is not None:
            raise RuntimeError("snapshots are recorded on single-GPU handles: a rank of a partitioned run holds its own rows only")
        if getattr(dev, "batch_k", 0):
            raise RuntimeError("snapshots are recorded from single-simulation steps: this handle has a batch set (BatchedFlowSolver)")
        self.dev = dev
        dev.snap_reserve(capacity, every, first)
        self.capacity, self.every, self.first = int(capacity), int(every), int(first)
        self._closed = False
        self.mean_removed: np.ndarray | bool | None = None  # set 0 was centred in place: its mean (True: it stayed on the device)

    # ── bookkeeping ──────────────────────────────────────────────────────────
    def info(self) -> dict:
        return self.dev.snap_info()

    @property
    def count(self) -> int:
        """Captured states held (columns of set 0)."""
        return self.info()["count"]

    @property
    def kept(self) -> int:
        """Vectors held by set 1."""
        return self.info()["kept"]

    @property
    def dropped(self) -> int:
        """Steps that were due for capture when set 0 was full."""
        return self.info()["dropped"]

    def _cols(self, set_: int, c0, c1) -> tuple[int, int]:
        n = self.info()["count" if set_ == 0 else "kept"]
        return (0 if c0 is None else int(c0)), (n if c1 is None else int(c1))

    # ── data in and out ──────────────────────────────────────────────────────
    def push(self) -> None:
        """Capture the handle's current state now."""
        self.dev.snap_push()

    def load(self, X, set: int = 1, col0: int | None = None) -> None:  # noqa: A002
        """Upload host columns ``X`` [ncol][N] into a set (appended by default)."""
        self.dev.snap_load(set, self._cols(set, None, None)[1] if col0 is None else col0, X)

    def get(self, c0: int | None = None, c1: int | None = None, set: int = 0) -> np.ndarray:  # noqa: A002
        """Download the columns ``[c0, c1)`` of a set: [ncol][N]."""
        c0, c1 = self._cols(set, c0, c1)
        return self.dev.snap_get(set, c0, c1 - c0)

    def clear(self, set: int = 0) -> None:  # noqa: A002
        self.dev.snap_clear(set)
        if set == 0:
            self.mean_removed = None

    def close(self) -> None:
        """Free the bank; the handle steps as if it had never existed."""
        if not self._closed:
            self._closed = True
            if getattr(self.dev, "_h", None):
                self.dev.snap_reserve(0)

    # ── computed on the device ───────────────────────────────────────────────
    def mean(self, c0: int | None = None, c1: int | None = None, set: int = 0, subtract: bool = False,  # noqa: A002
             download: bool = True) -> np.ndarray | None:
        """Mean of the columns ``[c0, c1)``; ``subtract`` removes it from them in place."""
        c0, c1 = self._cols(set, c0, c1)
        return self.dev.snap_mean(set, c0, c1, subtract, download)

    def gram(self, a: tuple[int, int] | None = None, b: tuple[int, int] | None = None, weight="energy", lset: int = 0,
             rset: int = 0) -> np.ndarray:
        """``L[:, a]^T M R[:, b]`` for column ranges ``a = (a0, a1)``, ``b = (b0, b1)`` (default: all) of the sets ``lset``, ``rset``."""
        a0, a1 = self._cols(lset, *(a or (None, None)))
        b0, b1 = self._cols(rset, *(b or (None, None)))
        return self.dev.snap_gram(lset, a0, a1, rset, b0, b1, _weight_slot(weight))

    def combine(self, Q, c0: int | None = None, c1: int | None = None, set: int = 0, keep: bool = False,  # noqa: A002
                download: bool = True) -> np.ndarray | None:
        """``sum_j Q[j, c] x_j`` over the columns ``[c0, c1)``: [k][N]; ``keep`` appends the k vectors to set 1."""
        c0, c1 = self._cols(set, c0, c1)
        return self.dev.snap_combine(set, c0, c1, Q, keep, download)


@dataclass
class PODResult:
    sigma: np.ndarray          #: all m singular values of M^1/2 X, descending
    energy: np.ndarray         #: sigma_i^2 / sum sigma^2
    V: np.ndarray              #: [m][r] right singular vectors (temporal coefficients: X^T M Phi = V S)
    r: int
    modes: np.ndarray | None   #: [r][N] Phi = X V_r S_r^-1, or None
    mean: np.ndarray | None    #: [N] the mean that was removed (None: not centred, or not downloaded)
    kept_at: int | None        #: first column of set 1 that holds the modes (``keep=True``)


@dataclass
class DMDResult:
    mu: np.ndarray             #: [r] eigenvalues of the snapshot-to-snapshot map, by decreasing modulus
    lam: np.ndarray            #: log(mu) / (every dt)
    lam_bdf2: np.ndarray       #: the eigenvalue of (A, E) that BDF2 maps onto mu
    sigma: np.ndarray          #: singular values of M^1/2 X1
    W: np.ndarray              #: [r][r] eigenvectors of Atilde
    modes: np.ndarray | None   #: [r][N] complex exact-DMD modes X2 V_r S_r^-1 W, or None


def gram_eig(G: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Eigenpairs of a symmetric positive semidefinite Gram matrix, descending; sigma = sqrt(max(eigenvalue, 0))."""
    G = np.asarray(G, dtype=float)
    w, V = np.linalg.eigh(0.5 * (G + G.T))
    order = np.argsort(w)[::-1]
    return np.sqrt(np.maximum(w[order], 0.0)), V[:, order]


def numerical_rank(sigma: np.ndarray, tol: float | None = None) -> int:
    """Singular values the Gram route still resolves: the eigenvalues of G carry an error of about ``m eps sigma_0^2``, so sigma_i is
    meaningful above ``sqrt(m eps) sigma_0`` (the default ``tol``)."""
    sigma = np.asarray(sigma)
    if sigma.size == 0 or sigma[0] <= 0.0:
        return 0
    if tol is None:
        tol = np.sqrt(sigma.size * np.finfo(float).eps)
    return int(np.count_nonzero(sigma > tol * sigma[0]))


def bdf2_rate(mu, dt: float, every: int = 1) -> np.ndarray:
    """The lambda of ``E x' = A x`` whose BDF2 amplification over ``every`` steps of ``dt`` is ``mu`` (principal root)."""
    mu1 = np.asarray(mu, dtype=complex) ** (1.0 / int(every))
    return (3.0 * mu1 ** 2 - 4.0 * mu1 + 1.0) / (2.0 * float(dt) * mu1 ** 2)


def bdf2_amplification(lam, dt: float, every: int = 1) -> np.ndarray:
    """Inverse of :func:`bdf2_rate`: the physical root of ``(3 - 2 dt lam) mu_1^2 - 4 mu_1 + 1 = 0``, to the power ``every``."""
    z = float(dt) * np.asarray(lam, dtype=complex)
    mu1 = (2.0 + np.sqrt(1.0 + 2.0 * z)) / (3.0 - 2.0 * z)
    return mu1 ** int(every)


#: singular values below this fraction of sigma_0 are left to the second (deflated) pass of :func:`pod`
POD_SPLIT = 1e-4


def pod(bank: SnapshotBank, r: int | None = None, tol: float | None = None, center: bool = True, weight="energy", modes: bool = True,
        keep: bool = False, refine: bool | None = None) -> PODResult:
    """Method-of-snapshots POD of the captured states.

    ``center`` removes the mean from the bank's columns IN PLACE (once: a bank that is already centred is left alone); ``r`` modes are
    kept, or those with ``sigma_i > tol sigma_0`` (default: the numerical rank).  ``modes=True`` returns ``Phi`` [r][N] and the mean;
    otherwise nothing N-long crosses to the host.  ``keep`` appends Phi to set 1 for :func:`project`.

    One Gram matrix in fp64 resolves singular values down to ``sqrt(m eps) sigma_0`` only (its eigenvalues carry an error of
    ``m eps sigma_0^2``).  ``refine`` adds a deflated second pass on the device: with ``V_1`` the eigenvectors above
    ``POD_SPLIT sigma_0``, the residual columns ``R = X (I - V_1 V_1^T)`` are formed in set 1 (``combine``: their entries carry an
    error of ``m eps |X|``, not of ``sqrt(eps)``), ``R^T M R = W S_2^2 W^T`` gives the singular values below the split down to
    ``max(sqrt(m eps) sigma_split, m eps sigma_0)``, and their modes are ``R W S_2^-1``.  ``Phi S V^T`` with ``V = [V_1, W]`` reproduces X; each block of V is orthonormal
    and each block of Phi M-orthonormal, while across the blocks ``V_1^T w_i`` is of order ``m eps sigma_0 / sigma_i`` and
    ``Phi_1^T M Phi_2`` of order ``eps sigma_0^2 / (sigma_i sigma_j)``.  The pass needs set 1 empty (it is cleared afterwards); ``refine=None`` runs it when that holds and the modes asked
    for reach below the split, ``True`` insists (ValueError otherwise), ``False`` is the single pass.  Modes below the split cannot be
    kept (``keep``): set 1 holds the residual while they are formed."""
    m = bank.count
    if m < 1:
        raise ValueError("the bank holds no snapshots")
    mean = None
    if center:
        if bank.mean_removed is None:
            out = bank.mean(subtract=True, download=modes)
            bank.mean_removed = True if out is None else out
        mean = bank.mean_removed if isinstance(bank.mean_removed, np.ndarray) else None
        if modes and mean is None:
            raise RuntimeError("the bank was centred by a call that left its mean on the device: it cannot be returned with the modes")
    sigma, V = gram_eig(bank.gram(weight=weight))
    eps = np.finfo(float).eps
    floor = np.sqrt(m * eps) * sigma[0]  # what this Gram matrix resolves
    r1 = int(np.count_nonzero(sigma > POD_SPLIT * sigma[0]))
    below = (r is None and (tol is None or tol < POD_SPLIT)) or (r is not None and int(r) > r1)
    room = bank.kept == 0 and bank.capacity >= m
    if refine and not room:
        raise ValueError("pod(refine=True) forms the residual columns in set 1: it must be empty and the capacity at least the snapshot count")
    if refine and keep and below:
        raise ValueError("pod(refine=True, keep=True): modes below POD_SPLIT sigma_0 cannot be kept")
    if 0 < r1 < m and below and room and not keep and refine is not False:
        V1 = V[:, :r1]
        bank.combine(np.eye(m) - V1 @ V1.T, keep=True, download=False)  # R = X (I - V1 V1^T) into set 1
        try:
            s2, W = gram_eig(bank.gram(a=(0, m), b=(0, m), weight=weight, lset=1, rset=1))
            sigma = np.r_[sigma[:r1], s2[: m - r1]]
            V = np.c_[V1, W[:, : m - r1]]
            floor = max(np.sqrt(m * eps) * s2[0], 4.0 * m * eps * sigma[0])
            lam = sigma ** 2
            if r is None:
                r = int(np.count_nonzero(sigma > max(floor, (tol or 0.0) * sigma[0])))
            r = int(r)
            if not 1 <= r <= m or sigma[r - 1] <= 0.0:
                raise ValueError(f"r = {r}: the snapshots give {int(np.count_nonzero(sigma > floor))} usable singular values of {m}")
            Phi = None
            if modes:
                Phi = bank.combine(V1 / sigma[:r1], set=0)
                if r > r1:
                    Phi = np.vstack([Phi, bank.combine(W[:, : r - r1] / s2[: r - r1], set=1)])
                Phi = Phi[:r]
        finally:
            bank.clear(1)
        energy = lam / lam.sum()
        return PODResult(sigma=sigma, energy=energy, V=V[:, :r].copy(), r=r, modes=Phi, mean=mean, kept_at=None)
    lam = sigma ** 2
    energy = lam / lam.sum() if lam.sum() > 0 else np.zeros_like(lam)
    if r is None:
        r = int(np.count_nonzero(sigma > max(floor, (tol or 0.0) * sigma[0])))
    r = int(r)
    if not 1 <= r <= m or sigma[r - 1] <= 0.0:
        raise ValueError(f"r = {r}: the snapshots give {numerical_rank(sigma)} usable singular values of {m}")
    Phi, kept_at = None, None
    if modes or keep:
        kept_at = bank.kept if keep else None
        Phi = bank.combine(V[:, :r] / sigma[:r], keep=keep, download=modes)
    return PODResult(sigma=sigma, energy=energy, V=V[:, :r].copy(), r=r, modes=Phi, mean=mean, kept_at=kept_at)


def dmd(bank: SnapshotBank, r: int, dt: float, weight="energy", modes: bool = False) -> DMDResult:
    """Dynamic mode decomposition of the captured states in the ``weight`` inner product, projected on ``r`` POD modes of X1.

    Two Gram calls on column ranges of the bank (``X1^T M X1``, ``X1^T M X2``); the r x r eigenproblem is solved on the host."""
    m = bank.count
    if m < 2:
        raise ValueError("DMD needs at least two snapshots")
    G11 = bank.gram(a=(0, m - 1), b=(0, m - 1), weight=weight)
    G12 = bank.gram(a=(0, m - 1), b=(1, m), weight=weight)
    sigma, V = gram_eig(G11)
    r = int(r)
    if not 1 <= r <= m - 1 or sigma[r - 1] <= 0.0:
        raise ValueError(f"r = {r}: X1 gives {numerical_rank(sigma)} usable singular values of {m - 1}")
    T = V[:, :r] / sigma[:r]
    mu, W = np.linalg.eig(T.T @ G12 @ T)
    order = np.argsort(-np.abs(mu), kind="stable")
    mu, W = mu[order], W[:, order]
    every = bank.every
    Phi = None
    if modes:
        Q = T @ W  # complex [m - 1][r]: two real combinations of X2
        Phi = bank.combine(Q.real, c0=1, c1=m) + 1j * bank.combine(Q.imag, c0=1, c1=m)
    return DMDResult(mu=mu, lam=np.log(mu.astype(complex)) / (every * float(dt)), lam_bdf2=bdf2_rate(mu, dt, every), sigma=sigma, W=W, modes=Phi)


def project(bank: SnapshotBank, c0: int | None = None, c1: int | None = None, weight="energy", modes: tuple[int, int] | None = None) -> np.ndarray:
    """Coefficients ``Phi^T M x_j`` of the set-0 columns ``[c0, c1)`` on the modes kept in set 1 (``modes``: their column range there,
    default all): [n_modes][n_columns], one Gram call between set 1 and set 0."""
    if bank.kept < 1:
        raise ValueError("set 1 holds no modes: keep them first (pod(..., keep=True) or combine(..., keep=True))")
    return bank.gram(a=modes, b=(c0, c1) if (c0 is not None or c1 is not None) else None, weight=weight, lset=1, rset=0)


__all__ = ["SnapshotBank", "PODResult", "DMDResult", "pod", "dmd", "project", "gram_eig", "numerical_rank", "bdf2_rate", "bdf2_amplification"]
