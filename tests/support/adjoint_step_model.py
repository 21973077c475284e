"""scipy model of the linearised time stepper and of its exact discrete adjoint (``fc_run`` / ``fc_run_adjoint``) -- TEST INFRASTRUCTURE.

Forward, n steps from ``(x0, xm1)``; step j = 1 .. n runs on the order ``s_j`` (``first_order`` for j = 1, 2 afterwards):

    A_s x_j = Z M (cm_n(s) x_{j-1} + cm_nn(s) x_{j-2}) + B_s u_j,        y_j = C x_j

``Z`` zeroes the Dirichlet rows, ``M`` is the velocity mass matrix (zero on the pressure block), ``B_s`` holds the actuator profiles on
the Dirichlet rows and ``-lift_s (+ F)`` on the others, ``cm_n, cm_nn = 1/dt, 0`` (order 1) or ``2/dt, -1/(2 dt)`` (order 2).

Backward, written out on its own (no transposed copy of the forward code): for ``J = sum_j w_j . y_j + z . x_n``

    mu_j = A_s^-T [C^T w_j (+ z at j = n) + M Z (cm_n(s_{j+1}) mu_{j+1} + cm_nn(s_{j+2}) mu_{j+2})],      g_j = B_s^T mu_j
    dx0 = M Z (cm_n(s_1) mu_1 + cm_nn(s_2) mu_2),        dxm1 = M Z cm_nn(s_1) mu_1

``wrong=`` switches one of the two classic mistakes on (the tests show that the inputs tell them apart): ``"ZM"`` masks the OUTPUT of
the mass product instead of its input; ``"bdf2_on_first"`` gives the first forward step BDF2's coefficients in the backward march.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def coeffs(order: int, dt: float) -> tuple[float, float]:
    return (1.0 / dt, 0.0) if order == 1 else (2.0 / dt, -0.5 / dt)


class StepModel:
    def __init__(self, A1, A2, M, bc_dofs, profiles, lift1, lift2, C, dt, F=None):
        """``A1, A2``: the BC-eliminated system matrices of order 1 / 2 (N x N); ``M``: N x N; ``profiles``: (n_bc, n_act) values on
        ``bc_dofs``; ``lift_s``: (N, n_act) = (A_s before the elimination) @ (profiles scattered to N); ``C``: (n_sens, N); ``F``:
        optional (N, n_act) load vectors of body-force actuators."""
        self.N = A1.shape[0]
        self.dt = float(dt)
        self.A = {1: sp.csc_matrix(A1), 2: sp.csc_matrix(A2)}
        self.lu = {s: spla.splu(self.A[s]) for s in (1, 2)}
        self.M = sp.csr_matrix(M)
        self.C = sp.csr_matrix(C)
        self.free = np.ones(self.N)
        self.free[np.asarray(bc_dofs)] = 0.0
        profiles = np.asarray(profiles, dtype=float).reshape(len(bc_dofs), -1)
        self.n_act = profiles.shape[1]
        self.B = {}
        for s, lift in ((1, lift1), (2, lift2)):
            B = -np.asarray(lift, dtype=float).reshape(self.N, self.n_act) * self.free[:, None]
            if F is not None:
                B = B + np.asarray(F).reshape(self.N, self.n_act) * self.free[:, None]
            B[np.asarray(bc_dofs)] = profiles
            self.B[s] = B

    def order_of(self, j: int, first_order: int) -> int:
        return first_order if j == 1 else 2

    # ── forward ──────────────────────────────────────────────────────────────
    def forward(self, first_order, u_seq, x0, xm1):
        """(X [n + 2, N] = x_{-1}, x_0, x_1 .. x_n;  y [n, n_sens] = C x_1 .. C x_n)."""
        u_seq = np.asarray(u_seq, dtype=float).reshape(-1, self.n_act)
        X = [np.asarray(xm1, dtype=float), np.asarray(x0, dtype=float)]
        for j in range(1, u_seq.shape[0] + 1):
            s = self.order_of(j, first_order)
            cn, cnn = coeffs(s, self.dt)
            rhs = self.free * (self.M @ (cn * X[-1] + cnn * X[-2])) + self.B[s] @ u_seq[j - 1]
            X.append(self.lu[s].solve(rhs))
        X = np.array(X)
        return X, (self.C @ X[2:].T).T

    # ── backward ─────────────────────────────────────────────────────────────
    def _mass_t(self, v, wrong):
        if wrong == "ZM":
            return self.free * (self.M.T @ v)
        return self.M.T @ (self.free * v)

    def adjoint(self, first_order, n, w=None, z=None, wrong=None):
        """(g [n, n_act], dx0 [N], dxm1 [N], mu [n, N])."""
        n = int(n)
        ns = self.C.shape[0]
        w = np.zeros((n, ns)) if w is None else np.asarray(w, dtype=float).reshape(n, ns)
        Ct = self.C.T.tocsr()

        def cf(j):  # coefficients of forward step j as the backward march sees them
            s = self.order_of(j, first_order)
            if wrong == "bdf2_on_first":
                s = 2
            return coeffs(s, self.dt)

        mu = {n + 1: np.zeros(self.N), n + 2: np.zeros(self.N)}
        g = np.zeros((n, self.n_act))
        for j in range(n, 0, -1):
            r = Ct @ w[j - 1]
            if j == n and z is not None:
                r = r + np.asarray(z, dtype=float)
            acc = np.zeros(self.N)
            if j + 1 <= n:
                acc += cf(j + 1)[0] * mu[j + 1]
            if j + 2 <= n:
                acc += cf(j + 2)[1] * mu[j + 2]
            r = r + self._mass_t(acc, wrong)
            s = self.order_of(j, first_order)
            mu[j] = self.lu[s].solve(r, trans="T")
            g[j - 1] = self.B[s].T @ mu[j]
        acc0 = cf(1)[0] * mu[1] + (cf(2)[1] * mu[2] if n >= 2 else 0.0)
        dx0 = self._mass_t(acc0, wrong)
        dxm1 = self._mass_t(cf(1)[1] * mu[1], wrong)
        return g, dx0, dxm1, np.array([mu[j] for j in range(1, n + 1)])

    # ── the identity ─────────────────────────────────────────────────────────
    @staticmethod
    def dot_defect(lhs_terms, rhs_terms) -> float:
        """|lhs - rhs| relative to the larger of the two sums of absolute terms (what round-off scales with)."""
        lhs, rhs = float(np.sum(lhs_terms)), float(np.sum(rhs_terms))
        scale = max(float(np.sum(np.abs(lhs_terms))), float(np.sum(np.abs(rhs_terms))), np.finfo(float).tiny)
        return abs(lhs - rhs) / scale


def identity_terms(w, y, z, xn, u, g, x0, dx0, xm1, dxm1):
    """The two sides of  sum w . y + z . x_n  =  sum u . g + x0 . dx0 + xm1 . dxm1  as lists of terms."""
    lhs = [float(np.sum(np.asarray(w) * np.asarray(y)))] + ([float(np.dot(z, xn))] if z is not None else [])
    rhs = [float(np.sum(np.asarray(u) * np.asarray(g))), float(np.dot(x0, dx0)), float(np.dot(xm1, dxm1))]
    return lhs, rhs


def random_problem(nx=4, ny=3, dt=0.05, seed=0):
    """A small stepping problem on the Taylor-Hood pattern of the nx x ny square with random operators of the right structure:
    A_s = cm(s) M + K (K unsymmetric), Dirichlet rows and columns eliminated, two actuators on the Dirichlet dofs, two sensors.
    Returns (model, dict of the raw pieces)."""
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    th = TaylorHood(Mesh.unit_square(nx, ny))
    N, nn2 = th.N, 2 * th.nn
    rng = np.random.default_rng(seed)
    cd = np.asarray(th.cell_dofs)
    rows, cols = np.repeat(cd, cd.shape[1], axis=1).ravel(), np.tile(cd, (1, cd.shape[1])).ravel()
    P = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(N, N))
    P.sum_duplicates()
    P.data[:] = 1.0
    vel = np.zeros(N)
    vel[:nn2] = 1.0
    S = P.copy()
    S.data = rng.standard_normal(S.nnz)
    M = (S + S.T) * 0.05 + sp.diags(np.full(N, 1.0))
    M = sp.diags(vel) @ M @ sp.diags(vel)  # velocity block only
    K = P.copy()
    K.data = rng.standard_normal(K.nnz)
    K = K + sp.diags(np.full(N, 30.0))
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    bc = np.sort(np.r_[nodes, nodes + th.nn])
    prof = rng.standard_normal((bc.size, 2))
    free = np.ones(N)
    free[bc] = 0.0
    Zf, Zd = sp.diags(free), sp.diags(1.0 - free)
    G = np.zeros((N, 2))
    G[bc] = prof
    raw, A, lift = {}, {}, {}
    for s, c in ((1, 1.0 / dt), (2, 1.5 / dt)):
        raw[s] = (c * M + K).tocsr()
        lift[s] = raw[s] @ G
        A[s] = (Zf @ raw[s] @ Zf + Zd).tocsr()
    C = sp.random(2, N, density=0.2, random_state=np.random.RandomState(seed), format="csr")
    C = C + sp.csr_matrix((np.ones(2), ([0, 1], [bc[0], bc[-1]])), shape=(2, N))  # the sensors see Dirichlet dofs too
    model = StepModel(A[1], A[2], M, bc, prof, lift[1], lift[2], C, dt)
    return model, dict(th=th, bc=bc, prof=prof, M=M, A=A, lift=lift, C=C)
