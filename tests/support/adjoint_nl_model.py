"""scipy model of the NONLINEAR time stepper and of its exact discrete adjoint (``fc_run`` / ``fc_run_adjoint`` with
``fc_set_time_scheme(dt, 1)`` and a state tape) -- TEST INFRASTRUCTURE.

Forward, step j = 1 .. n on the order ``s_j`` (``first_order`` for j = 1, 2 afterwards):

    A_s x_j = Z [ M (cm_n x_{j-1} + cm_nn x_{j-2}) + cc_n N(x_{j-1}) + cc_nn N(x_{j-2}) ] + B_s u_j,        y_j = C x_j

``N(x)[a,i] = ∫ φ_a ((u.∇)u)_i`` is the oracle's convective load vector, ``(cm_n, cm_nn, cc_n, cc_nn)`` = ``(1/dt, 0, -1, 0)`` (order 1) or
``(2/dt, -1/(2dt), -2, 1)`` (order 2).  Backward, written out on its own, for ``J = sum_j w_j . y_j + z . x_n``: with
``J(x) = dN/dx`` (the oracle's ``assemble_matrix(adv=x, lin=x)`` without mass, viscosity, pressure and divergence)

    r_m = C^T w_m (+ z at m = n) + M Z (cm_n(m+1) mu_{m+1} + cm_nn(m+2) mu_{m+2}) + J(x_m)^T Z (cc_n(m+1) mu_{m+1} + cc_nn(m+2) mu_{m+2})
    mu_m = A_s^-T r_m,   g_m = B_s^T mu_m,   dx0 = the two products at m = 0,   dxm1 = M Z cm_nn(1) mu_1 + J(x_{-1})^T Z cc_nn(1) mu_1

``wrong=`` switches one mistake on (the tests show that the inputs tell them apart): ``"linear"`` leaves the Jacobian term out,
``"J_next"`` takes J at x_{m+1} instead of x_m, ``"mask_out"`` puts the Dirichlet mask on the output of J^T instead of its input.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import ns_oracle as O
from tests.support.adjoint_step_model import StepModel


def coeffs(order: int, dt: float) -> tuple[float, float, float, float]:
    return (1.0 / dt, 0.0, -1.0, 0.0) if order == 1 else (2.0 / dt, -0.5 / dt, -2.0, 1.0)


class NonlinearStepModel(StepModel):
    """``StepModel``'s matrices (A_s, their LU, M, B_s, C, the Dirichlet mask) with the convective term ``N`` and its Jacobian from the
    oracle's discretisation ``disc``."""

    def __init__(self, disc, *args, **kw):
        super().__init__(*args, **kw)
        self.d = disc
        self.nn2 = 2 * disc.nn

    def conv(self, x):
        """N(x), an N-vector (zero on the pressure rows)."""
        u = np.asarray(x, dtype=float)[: self.nn2]
        return O._load(self.d, O.convective(self.d, u))

    def jac(self, x):
        """J(x) = dN/dx, N x N."""
        u = np.asarray(x, dtype=float)[: self.nn2]
        return O.assemble_matrix(self.d, adv=u, lin=u, pressure=0.0, divergence=0.0)

    # ── forward ──────────────────────────────────────────────────────────────
    def forward(self, first_order, u_seq, x0, xm1):
        """(X [n + 2, N] = x_{-1}, x_0, x_1 .. x_n;  y [n, n_sens])."""
        u_seq = np.asarray(u_seq, dtype=float).reshape(-1, self.n_act)
        X = [np.asarray(xm1, dtype=float), np.asarray(x0, dtype=float)]
        for j in range(1, u_seq.shape[0] + 1):
            s = self.order_of(j, first_order)
            cn, cnn, ccn, ccnn = coeffs(s, self.dt)
            inner = self.M @ (cn * X[-1] + cnn * X[-2]) + ccn * self.conv(X[-1])
            if ccnn != 0.0:
                inner = inner + ccnn * self.conv(X[-2])
            X.append(self.lu[s].solve(self.free * inner + self.B[s] @ u_seq[j - 1]))
        X = np.array(X)
        return X, (self.C @ X[2:].T).T

    def cost(self, first_order, u_seq, x0, xm1, w, z=None):
        X, y = self.forward(first_order, u_seq, x0, xm1)
        return float(np.sum(np.asarray(w) * y) + (0.0 if z is None else np.dot(z, X[-1])))

    # ── backward ─────────────────────────────────────────────────────────────
    def _products(self, X, col, am, ac, wrong):
        """M Z am + J(X[col])^T Z ac, with the mistake ``wrong`` switched on."""
        out = self.M.T @ (self.free * am)
        if wrong == "linear":
            return out
        if wrong == "J_next":
            col += 1
        Jt = self.jac(X[col]).T
        if wrong == "mask_out":
            return out + self.free * (Jt @ ac)
        return out + Jt @ (self.free * ac)

    def adjoint(self, first_order, X, w=None, z=None, wrong=None):
        """(g [n, n_act], dx0 [N], dxm1 [N], mu [n, N]) for the forward run ``X`` (n + 2 rows)."""
        X = np.asarray(X, dtype=float)
        n = X.shape[0] - 2
        ns = self.C.shape[0]
        w = np.zeros((n, ns)) if w is None else np.asarray(w, dtype=float).reshape(n, ns)
        Ct = self.C.T.tocsr()
        cf = lambda j: coeffs(self.order_of(j, first_order), self.dt)  # noqa: E731
        zero = np.zeros(self.N)
        mu = {n + 1: zero, n + 2: zero}

        def combined(m):  # what the forward steps m + 1 and m + 2 did with x_m, gated by the horizon
            am, ac = zero.copy(), zero.copy()
            if m + 1 <= n:
                c = cf(m + 1)
                am += c[0] * mu[m + 1]
                ac += c[2] * mu[m + 1]
            if m + 2 <= n:
                c = cf(m + 2)
                am += c[1] * mu[m + 2]
                ac += c[3] * mu[m + 2]
            return am, ac

        g = np.zeros((n, self.n_act))
        for m in range(n, 0, -1):
            r = Ct @ w[m - 1]
            if m == n and z is not None:
                r = r + np.asarray(z, dtype=float)
            if m < n:
                r = r + self._products(X, m + 1, *combined(m), wrong)
            s = self.order_of(m, first_order)
            mu[m] = self.lu[s].solve(r, trans="T")
            g[m - 1] = self.B[s].T @ mu[m]
        dx0 = self._products(X, 1, *combined(0), wrong)
        c1 = cf(1)
        dxm1 = self._products(X, 0, c1[1] * mu[1], c1[3] * mu[1], wrong)
        return g, dx0, dxm1, np.array([mu[j] for j in range(1, n + 1)])


# ── the 7 x 5 square of tests/test_adjoint_nl_host.py and tests/test_adjoint_nl_gpu.py ─────────────────────────────────────────────
DT, RE = 0.005, 100.0


def square_inputs(th, amplitude=1.0, seed=2):
    """(U0, bc dofs, profiles, sensor row, u_n, u_nn, p): the BC set, sensor and smooth states of tests/support/adjoint_step_child.py
    with the two time levels at ``amplitude``."""
    from tests.support.adjoint_step_child import bc_setup, smooth_velocity

    U0 = smooth_velocity(th)
    dofs, prof = bc_setup(th)
    row = th.point_eval_row((0.31, 0.42), 1)
    rng = np.random.default_rng(seed)
    u_n = amplitude * smooth_velocity(th, 2.0) + 0.01 * rng.standard_normal(2 * th.nn)
    u_nn = amplitude * smooth_velocity(th, 1.5)
    p = 0.01 * rng.standard_normal(th.nv)
    return U0, dofs, prof, row, u_n, u_nn, p


def model_from(th, raw, A, M, dofs, prof, row, dt=DT):
    """The model on given matrices (``raw``, ``A``: {1, 2} -> the operator before / after the elimination of the Dirichlet dofs)."""
    N = th.N
    G = np.zeros((N, prof.shape[1]))
    G[dofs] = prof
    C = sp.csr_matrix((row[1], (np.zeros(len(row[0]), dtype=int), row[0])), shape=(1, N))
    return NonlinearStepModel(O.Disc.from_taylor_hood(th), A[1], A[2], M, dofs, prof, raw[1] @ G, raw[2] @ G, C, dt)


def host_square(nx=7, ny=5, amplitude=1.0):
    """The whole problem from the oracle's operators (no device): (model, th, (u_n, u_nn, p))."""
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    th = TaylorHood(Mesh.unit_square(nx, ny))
    d = O.Disc.from_taylor_hood(th)
    U0, dofs, prof, row, u_n, u_nn, p = square_inputs(th, amplitude)
    free = np.ones(th.N)
    free[dofs] = 0.0
    Zf, Zd = sp.diags(free), sp.diags(1.0 - free)
    raw, A = {}, {}
    for order, c in ((1, 1.0 / DT), (2, 1.5 / DT)):
        raw[order] = O.assemble_matrix(d, mass=c, nu=1.0 / RE, adv=U0, lin=U0)
        A[order] = (Zf @ raw[order] @ Zf + Zd).tocsr()
    M = sp.block_diag([O.velocity_mass(d), sp.csr_matrix((th.nv, th.nv))]).tocsr()
    return model_from(th, raw, A, M, dofs, prof, row), th, (u_n, u_nn, p)


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(ref)) / np.linalg.norm(ref))
