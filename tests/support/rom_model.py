"""numpy / scipy model of the balanced reduced models of ``flowcontrol_amd.rom`` ("Reduced models"), and the small
fixture its tests share: the 10 x 10 open-square operator of test_shifted_adjoint_gpu.py (N = 1003), two Gaussian body forces as
inputs, three nodal velocities as outputs, the band [0.05, 200].

Everything here is dense host work on explicit N-long snapshots: ``splu`` per frequency (``trans="H"`` for the adjoint), the real
snapshot matrices, the three Grams, the SVD, and the reduced matrices formed twice -- from the Grams and from explicit modes."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

BAND = (0.05, 200.0)
SIGMA = 0.08
FORCES = ((0.3, 0.5, 1), (0.5, 0.3, 0))  # (x, y, velocity component the force acts on)
SENSORS = ((0.8, 0.5, 0), (0.8, 0.5, 1), (0.6, 0.7, 1))  # (x, y, velocity component read)
CHECK_WW = np.logspace(-1.0, 2.0, 40)  # where the 2 * tail bound is checked


def advection_field(node_xy: np.ndarray) -> np.ndarray:
    return np.r_[1.0 + 0.2 * np.sin(3 * node_xy[:, 1]), 0.3 * np.cos(2 * node_xy[:, 0])]


def wall_nodes(node_xy: np.ndarray) -> np.ndarray:
    return np.flatnonzero((node_xy[:, 0] < 1e-12) | (node_xy[:, 1] < 1e-12))


def with_wall_rows(A0: sp.spmatrix, node_xy: np.ndarray, nn: int) -> sp.csr_matrix:
    """Identity rows on the left / bottom velocity dofs (as ``_Open`` of test_shifted_adjoint_gpu.py)."""
    N = A0.shape[0]
    wall = wall_nodes(node_xy)
    keep = np.ones(N)
    keep[np.r_[wall, nn + wall]] = 0.0
    return (sp.diags(keep) @ sp.csr_matrix(A0) + sp.diags(1.0 - keep)).tocsr()


def inputs_outputs(E: sp.spmatrix, node_xy: np.ndarray, nn: int) -> tuple[np.ndarray, np.ndarray]:
    """B [N, 2] = E f with the wall rows zeroed (f: nodal Gaussians), C [3, N]: unit rows at the nodes nearest the sensor points."""
    N = E.shape[0]
    wall = wall_nodes(node_xy)
    F = np.zeros((N, len(FORCES)))
    for k, (x, y, comp) in enumerate(FORCES):
        F[comp * nn:(comp + 1) * nn, k] = np.exp(-((node_xy[:, 0] - x) ** 2 + (node_xy[:, 1] - y) ** 2) / (2.0 * SIGMA**2))
    B = np.asarray(sp.csr_matrix(E) @ F)
    B[np.r_[wall, nn + wall]] = 0.0
    C = np.zeros((len(SENSORS), N))
    for k, (x, y, comp) in enumerate(SENSORS):
        C[k, comp * nn + int(np.argmin((node_xy[:, 0] - x) ** 2 + (node_xy[:, 1] - y) ** 2))] = 1.0
    return B, C


def host_fixture():
    """(A, E, B, C) of the fixture, assembled on the CPU by the oracle."""
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from oracle import ns_oracle as O

    th = TaylorHood(Mesh.unit_square(10, 10))
    d = O.Disc.from_taylor_hood(th)
    xy = th.node_coords
    A0 = O.assemble_matrix(d, mass=0.0, nu=-0.02, adv=advection_field(xy), adv_scale=-1.0, pressure=1.0, divergence=1.0)
    E = O.assemble_matrix(d, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0).tocsr()
    A = with_wall_rows(A0, xy, th.nn)
    B, C = inputs_outputs(E, xy, th.nn)
    return A, E, B, C


def log_quadrature(w_lo: float, w_hi: float, nq: int):
    x, g = np.polynomial.legendre.leggauss(nq)
    L = np.log(w_hi / w_lo)
    ww = np.exp(np.log(w_lo) + 0.5 * (x + 1.0) * L)
    return ww, 0.5 * L * g * ww


def full_response(A, E, B, C, ww) -> np.ndarray:
    """H [nw, ny, nu] = C (i w E - A)^-1 B."""
    out = []
    for w in np.atleast_1d(ww):
        lu = spla.splu((1j * w * E - A).astype(complex).tocsc())
        out.append(C @ lu.solve(B.astype(complex)))
    return np.stack(out)


def snapshots(A, E, B, C, ww, weights, permc_spec: str = "COLAMD"):
    """Xs [N, 2 nq nu], Zs [N, 2 nq ny] (real column 2 (j n + i) + p = part p of column i at frequency j, scaled by sqrt(d_j / pi))
    and H [nq, ny, nu]."""
    nu, ny = B.shape[1], C.shape[0]
    Xs, Zs, H = [], [], []
    for w, d in zip(ww, weights):
        lu = spla.splu((1j * w * E - A).astype(complex).tocsc(), permc_spec=permc_spec)
        s = np.sqrt(d / np.pi)
        X = lu.solve(B.astype(complex))
        Z = lu.solve(C.T.astype(complex), "H")
        H.append(C @ X)
        for M, out, k in ((X, Xs, nu), (Z, Zs, ny)):
            for i in range(k):
                out += [s * M[:, i].real, s * M[:, i].imag]
    return np.array(Xs).T, np.array(Zs).T, np.stack(H)


class Model:
    """The whole construction on the host for one quadrature."""

    def __init__(self, A, E, B, C, ww, weights, permc_spec: str = "COLAMD"):
        self.A, self.E, self.B, self.C = A, E, B, C
        self.ww, self.weights = np.asarray(ww), np.asarray(weights)
        self.Xs, self.Zs, self.H = snapshots(A, E, B, C, ww, weights, permc_spec)
        self.GE = self.Zs.T @ (E @ self.Xs)
        self.GA = self.Zs.T @ (A @ self.Xs)
        self.ZtB = self.Zs.T @ B
        self.CXs = C @ self.Xs
        self.U, self.hsv, self.Vt = np.linalg.svd(self.GE, full_matrices=False)

    def tail(self, r: int) -> float:
        return float(2.0 * np.sum(self.hsv[r:]))

    def modes(self, r: int):
        isq = 1.0 / np.sqrt(self.hsv[:r])
        return self.Xs @ (self.Vt[:r].T * isq), self.Zs @ (self.U[:, :r] * isq)

    def from_grams(self, r: int):
        isq = 1.0 / np.sqrt(self.hsv[:r])
        TL, TR = isq[:, None] * self.U[:, :r].T, self.Vt[:r].T * isq
        return TL @ self.GA @ TR, TL @ self.ZtB, self.CXs @ TR

    def from_modes(self, r: int):
        Phi, Psi = self.modes(r)
        return Psi.T @ (self.A @ Phi), Psi.T @ self.B, self.C @ Phi


def response(Ar, Br, Cr, ww) -> np.ndarray:
    eye = np.eye(Ar.shape[0])
    return np.stack([Cr @ np.linalg.solve(1j * w * eye - Ar, Br.astype(complex)) for w in np.atleast_1d(ww)])


def worst_error(H, Hr) -> float:
    """max over frequencies of the spectral norm of H - Hr."""
    return float(max(np.linalg.norm(a - b, 2) for a, b in zip(H, Hr)))
