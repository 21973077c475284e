"""The energy term of the adjoint marches' cost (fc_set_adjoint_energy; csrc/fc_adjoint_energy.hip.h) -- TEST INFRASTRUCTURE, no GPU import.

With ``dE_m = 1/2 x_m^T M x_m`` (velocity mass matrix, the FULL state: actuated Dirichlet values included) a cost term ``sum_m e_m dE_m``
adds ``e_m M x_m`` to the right-hand side of backward step m, on every row, unmasked; ``dE_0`` is not in the sum, so the state gradients
``dx0`` / ``dxm1`` carry no such term.

  EnergyStepModel / EnergyNonlinearStepModel / EnergyLoop   the host models of the three earlier test families with that term in the cost and
                                                            in the adjoint (subclasses: the forward runs are the parents')
  weights                                                   the e_m of the tests: distinct per step, one zero row (n >= 2)
  EnergyMarchModel                                          adjoint_march_cases.MarchModel with the third operand of the element loop: the
                                                            np.longdouble model of ONE right-hand side, M (cm_n z1 + cm_nn z2 + e x) (+ ..)
  route_with_energy                                         what fc_get_adjoint_route reports while weights are held

tests/test_adjoint_energy_host.py runs all of it on the host and asserts the constants below; tests/support/adjoint_energy_child.py runs
the device against it."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_march_cases as mc
from tests.support.adjoint_nl_model import NonlinearStepModel
from tests.support.adjoint_step_model import StepModel

L = np.longdouble

# ── central differences ────────────────────────────────────────────────────────────────────────────────────────────────────────────
# Steps of the GPU tests' central differences of the DEVICE's own cost: the sibling tests' (open loop: tests/support/adjoint_nl_child.py
# and adjoint_batch_cases.py, 1e-4; closed loop: adjoint_loop_cases.FD_EPS) and their bound, 1e-6 each.
FD_STEP_OPEN, FD_STEP_LOOP, FD_TOL_SIBLING = 1e-4, 2e-5, 1e-6
# Largest distance of the MODEL's gradient from central differences of the MODEL's own cost at those steps, along one random direction
# per group (open loop: u, x0, x_{-1}; closed loop: every group of adjoint_loop_model.GROUPS), relative to the difference quotient; over
# first order 1 and 2, n in {1, 2, 5}, the weights of weights(n), sensor and control weights and a terminal vector.  Measured by
# tests/test_adjoint_energy_host.py::test_model_gradient_matches_central_differences; test_fd_constants_are_tight asserts that each
# constant bounds what the twelve cases measure and exceeds it by less than a factor of two.
#   linearised plant (8 x 8 square), open loop, h = 1e-4: J is a quadratic form of (u, x0, x_{-1}), so central differences are exact up to
#     rounding, eps |J| / (h |J'|): measured 4.10e-9 (n = 2 from BDF2, x_{-1}).  Closed loop, h = 2e-5: J is a polynomial of degree up to
#     2 n in the controller's matrices, not a quadratic; truncation joins the rounding: measured 1.22e-8 (n = 5 from BDF2)
#   nonlinear plant (7 x 5 square): open loop 2.96e-8 (n = 2 from BDF2, x_{-1}), closed loop 4.17e-7 (n = 2 from BDF2, the feedback map G,
#     whose derivative along the test's direction is small against J: rounding; every other group and case is below 8e-8)
HOST_FD_DISTANCE = {("lin", "open"): 4.5e-9, ("lin", "loop"): 1.4e-8, ("nl", "open"): 3.3e-8, ("nl", "loop"): 4.6e-7}


def fd_tol(kind: str, march: str) -> float:
    """The GPU tests' bound of the device's gradient against central differences of the device's own cost: the sibling test's 1e-6, or
    ten times the host-measured distance where that is larger (the nonlinear closed loop: 4.6e-6)."""
    return max(FD_TOL_SIBLING, 10 * HOST_FD_DISTANCE[kind, march])


FD_TOL = FD_TOL_SIBLING

# ── the kernel model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────
# Largest relative distance of an fp64 numpy evaluation of EnergyMarchModel.rhs (the same expression, every table and operand rounded to
# fp64) from the np.longdouble one, 2-norm / max-norm over the velocity rows of a step whose two masked levels, taped state and weight
# are not zero; measured per mesh by tests/test_adjoint_energy_host.py::test_host_constants, which asserts that these constants bound what
# it measures and exceed it by less than a factor of two (the way adjoint_march_cases.HOST_ADJ_RHS_ERROR is stated and asserted).
#            linearised                nonlinear
#   5x3      1.38e-16 / 1.92e-16       1.44e-16 / 2.05e-16
#   9x9      1.28e-16 / 1.86e-16       1.32e-16 / 2.12e-16
#   12x7     1.25e-16 / 1.88e-16       1.33e-16 / 1.82e-16
# (about twice adjoint_march_cases.HOST_ADJ_RHS_ERROR: the three operands are combined at the nodes, one more rounding in front of the
# quadrature than the forward loop's sum at the points)
HOST_ADJ_EN_RHS_ERROR = (1.45e-16, 2.13e-16)
EN_MESHES = ("5x3", "9x9", "12x7")

ELEM_EN, ELEM_EN_REG, ELEM_EN_B, ELEM_NL_EN, ELEM_NL_REG_EN, ELEM_NL_B_EN = 7, 8, 9, 10, 11, 12  # FC_ADJ_ELEM_* in include/fc_hip_internal.h
ENERGY_OF = {mc.ELEM_LANES: ELEM_EN, mc.ELEM_REG: ELEM_EN_REG, mc.ELEM_BREG: ELEM_EN_B, mc.ELEM_NL: ELEM_NL_EN, mc.ELEM_NL_REG: ELEM_NL_REG_EN,
             mc.ELEM_NL_B: ELEM_NL_B_EN}


def route_with_energy(route: np.ndarray) -> np.ndarray:
    """adjoint_march_cases.predicted_route with the element kernel's code replaced by its energy form: the grids are the same."""
    out = np.array(route, dtype=np.int32)
    out[0] = ENERGY_OF[int(out[0])]
    return out


def weights(n: int, k: int = 0, seed: int = 5) -> np.ndarray:
    """e (n,) or (n, k): distinct per step (and column), positive and negative, row 1 zero (n >= 2); of a size at which the energy
    term moves the gradients of the tests' small states by more than 1e-3 of themselves."""
    rng = np.random.default_rng(seed + n + 7 * k)
    e = 10.0 * (0.5 + rng.random((n, max(k, 1))) * 2.0)
    e[::3] *= -0.6
    if n >= 2:
        e[1] = 0.0
    return e if k else e[:, 0]


def msym(M):
    return (0.5 * (sp.csr_matrix(M) + sp.csr_matrix(M).T)).tocsr()


def energy_cost(M, X, e) -> float:
    """sum_m e_m 1/2 x_m^T M x_m over X = x_{-1}, x_0, x_1 .. x_n (rows m + 1)."""
    return float(sum(e[m - 1] * 0.5 * (X[m + 1] @ (M @ X[m + 1])) for m in range(1, len(e) + 1)))


# ── host models of the three families ──────────────────────────────────────────────────────────────────────────────────────────────
class EnergyStepModel(StepModel):
    """The linearised stepper; ``J = sum w . y + z . x_n + sum e_m dE_m``.  The forcing e_m M x_m of backward step m is a sensor: n more
    rows (M x_m)^T of C, weighted e_m at step m and 0 elsewhere -- the parent's march then forms exactly C^T w_m + e_m M x_m."""

    def cost(self, first_order, u_seq, x0, xm1, w, z=None, e=None):
        X, y = self.forward(first_order, u_seq, x0, xm1)
        return float(np.sum(np.asarray(w) * y) + (0.0 if z is None else np.dot(z, X[-1])) + (0.0 if e is None else energy_cost(self.M, X, e)))

    def adjoint_energy(self, first_order, X, w, z, e):
        X = np.asarray(X, dtype=float)
        n = X.shape[0] - 2
        C0 = self.C
        try:
            self.C = sp.vstack([C0, sp.csr_matrix((msym(self.M) @ X[2:].T).T)]).tocsr()
            return self.adjoint(first_order, n, np.hstack([np.asarray(w, dtype=float).reshape(n, C0.shape[0]), np.diag(np.asarray(e, dtype=float))]), z)
        finally:
            self.C = C0


class EnergyNonlinearStepModel(NonlinearStepModel):
    """The nonlinear stepper with the same cost.  The parent forms the products of backward step m < n through ``_products(X, m + 1, ..)``:
    the forcing joins them there; the one of step n arrives with the terminal vector."""

    _e = None

    def cost(self, first_order, u_seq, x0, xm1, w, z=None, e=None):
        X, y = self.forward(first_order, u_seq, x0, xm1)
        return float(np.sum(np.asarray(w) * y) + (0.0 if z is None else np.dot(z, X[-1])) + (0.0 if e is None else energy_cost(self.M, X, e)))

    def _products(self, X, col, am, ac, wrong):
        out = super()._products(X, col, am, ac, wrong)
        if self._e is not None and col >= 2:
            out = out + self._e[col - 2] * (msym(self.M) @ X[col])
        return out

    def adjoint_energy(self, first_order, X, w, z, e):
        X = np.asarray(X, dtype=float)
        n = X.shape[0] - 2
        self._e = np.asarray(e, dtype=float)
        try:
            zz = (0.0 if z is None else np.asarray(z, dtype=float)) + self._e[n - 1] * (msym(self.M) @ X[n + 1])
            return self.adjoint(first_order, X, w, zz)
        finally:
            self._e = None


def with_energy(model):
    """The model's energy subclass on the same matrices (no copy: the class of the object is moved)."""
    model.__class__ = EnergyNonlinearStepModel if isinstance(model, NonlinearStepModel) else EnergyStepModel
    return model


class EnergyLoop(lm.Loop):
    """The closed loop with ``sum e_m dE_m`` in the cost (``e``: attribute, (n,))."""

    e = None

    def clone(self):
        q = EnergyLoop(self.plant, lm.copy_bank(self.bank), self.first_order, self.n, self.x0, self.xm1, self.y0, self.w_y, self.w_u, self.lo, self.hi)
        q.e = self.e
        return q

    @classmethod
    def of(cls, loop: lm.Loop, e):
        q = cls(loop.plant, lm.copy_bank(loop.bank), loop.first_order, loop.n, loop.x0, loop.xm1, loop.y0, loop.w_y, loop.w_u, loop.lo, loop.hi)
        q.e = np.asarray(e, dtype=float).reshape(loop.n)
        return q

    def cost(self, w, r, z=None):
        f = self.forward()
        J = float(np.sum(np.asarray(w) * f["y"][1:]) + np.sum(np.asarray(r) * f["u"]) + (0.0 if z is None else np.dot(z, f["X"][-1])))
        return J + (0.0 if self.e is None else energy_cost(self.plant.M, f["X"], self.e))

    def _products(self, X, col, a_m, a_c):
        out = super()._products(X, col, a_m, a_c)
        if self.e is not None and col >= 2:
            out = out + self.e[col - 2] * (msym(self.plant.M) @ X[col])
        return out

    def adjoint(self, f, w, r, z=None, wrong=None):
        if self.e is None:
            return super().adjoint(f, w, r, z, wrong)
        X, n = f["X"], self.n
        zz = (0.0 if z is None else np.asarray(z, dtype=float)) + self.e[n - 1] * (msym(self.plant.M) @ X[n + 1])
        return super().adjoint(f, w, r, zz, wrong)


# ── the kernel model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────
class EnergyMarchModel(mc.MarchModel):
    """MarchModel with the third operand of the element loop: ``e`` and the taped state ``x_state`` (W numbering, NOT masked) join the two
    masked levels at the nodes, in front of the quadrature -- M (cm_n Z z1 + cm_nn Z z2 + e x) -- as fc_adj_elem_en / _reg / _b and the
    EN instantiations of fc_adj_elem_nl / _reg / _b form it.  ``wrong="x_masked"``: the mask also on x (a mistake the inputs must tell:
    the actuated Dirichlet values carry energy); ``wrong="no_energy"``: the term left out."""

    def elem_part(self, zm1, zm2, coeffs, x_taped=None, T=L, wrong=None, e=None, x_state=None):
        if e is None or wrong == "no_energy":
            return super().elem_part(zm1, zm2, coeffs, x_taped, T, wrong if wrong == "mask_out" else None)
        hm = self.hm
        cm_n, cm_nn, cc_n, cc_nn = coeffs
        z1, z2 = (np.where(self.free, np.asarray(z, dtype=T), T(0)) for z in (zm1, zm2))
        x = np.asarray(x_state, dtype=T)
        if wrong == "x_masked":
            x = np.where(self.free, x, T(0))
        am = T(cm_n) * z1 + T(cm_nn) * z2 + T(e) * x
        Vm = self._at_q(am[: 2 * self.nn], T)[0]
        Le = np.einsum("cq,qb,cqj->cbj", hm.w.astype(T), hm.PHI2.astype(T), Vm)
        out = np.zeros(self.N, dtype=T)
        np.add.at(out, hm.cn.reshape(-1), Le[:, :, 0].reshape(-1))
        np.add.at(out, self.nn + hm.cn.reshape(-1), Le[:, :, 1].reshape(-1))
        if x_taped is not None and (cc_n != 0 or cc_nn != 0):
            out = out + super().elem_part(zm1, zm2, (0.0, 0.0, cc_n, cc_nn), x_taped, T)
        return out

    def rhs(self, zm1, zm2, coeffs, w, term, x_taped=None, T=L, wrong=None, e=None, x_state=None):
        """M (Z (cm_n zm1 + cm_nn zm2) + e x_state) (+ J(x_taped)^T Z (..)) + C^T w + term on every row.  Not masked."""
        b = self.elem_part(zm1, zm2, coeffs, x_taped, T, wrong, e, x_state) + self.ct_part(w, T)[0]
        return b if term is None else b + np.asarray(term, dtype=T)


def step_inputs(model: mc.MarchModel, seed: int):
    """(z1, z2, x, w, e): two levels with entries on the Dirichlet rows too (the mask must remove them), a state whose Dirichlet values
    are not zero, sensor weights, a weight of the energy."""
    rng = np.random.default_rng(seed)
    N = model.N
    z1, z2, x = rng.standard_normal(N), rng.standard_normal(N), 0.3 * rng.standard_normal(N)
    return z1, z2, x, rng.standard_normal(len(model.rows)), 1.7
