"""The tangent of the energy in the tangent marches (fc_tangent_set_energy; csrc/fc_tangent_energy.hip.h) and the Gauss-Newton product of
the energy cost built on it -- TEST INFRASTRUCTURE, no GPU import.

With ``dE_m = 1/2 x_m^T M x_m`` (velocity mass matrix, the FULL state: actuated Dirichlet values included) a tangent march that produces
``dx_1 .. dx_n`` gives ``d(dE_m) = x_m^T M_s dx_m`` for m = 1 .. n; ``d(dE_0)`` is not part of it.  Neither factor is masked.

  dde_rows                  the rows from the states X and the tangent states D of any of the models
  TangentEnergyModel        tangent_model.TangentModel with ``dde`` and with the energy product H_E v = sum_m e_m X_m^T M_s X_m v
  loop_dde / loop_energy    the same for adjoint_loop_model.Loop and tangent_loop_model.tangent
  wrong=                    the two mistakes DESIGN section 5.4 names: ``"x_masked"`` (the Dirichlet mask on x_m) and ``"mask_out"`` (the
                            mask on the tangent state)

tests/test_tangent_energy_host.py runs all of it on the host and asserts the constants below; the GPU tests run the device against it."""
from __future__ import annotations

import numpy as np

from tests.support import adjoint_energy_cases as ec
from tests.support import tangent_loop_model as tlm
from tests.support.adjoint_nl_child import EPS, TOL, TOL_FD  # noqa: F401  (1e-4, 1e-8, 1e-6: the sibling tests' step and bounds)
from tests.support.tangent_model import TangentModel

# ── central differences ────────────────────────────────────────────────────────────────────────────────────────────────────────────
# Largest distance of the MODEL's dde from central differences of the MODEL's own energy series dE_1 .. dE_n along one random direction
# (open loop: u, x0, x_{-1} together at h = EPS = 1e-4; closed loop: every group of adjoint_loop_model.GROUPS together at h =
# adjoint_loop_cases.FD_EPS = 2e-5), 2-norm over the n rows relative to the difference quotient; over first order 1 and 2 and n in
# {1, 2, 5}.  Measured by tests/test_tangent_energy_host.py::test_model_dde_matches_central_differences, which asserts that each constant
# bounds what the cases measure and exceeds it by less than a factor of two.
#   nonlinear open loop (7 x 5 square): measured 3.99e-10 (n = 2 from BDF2)
#   closed loops with a clamp (n = 1: without): linearised 8 x 8 square 8.13e-9 (n = 1 from BDF2; the smaller step leaves more rounding),
#   nonlinear 7 x 5 square 6.00e-8 (n = 2 from BDF2)
# Every one is under a tenth of the sibling tests' TOL_FD = 1e-6, so the GPU tests hold the device to TOL_FD itself (fd_tol).
HOST_FD_DISTANCE = {("nl", "open"): 4.4e-10, ("lin", "loop"): 9.0e-9, ("nl", "loop"): 6.6e-8}


def fd_tol(kind: str, march: str) -> float:
    """The GPU tests' bound of the device's dde against central differences of the device's own dE series: the sibling test's TOL_FD
    where the host distance is under a tenth of it, else 16 times the host distance."""
    d = HOST_FD_DISTANCE[kind, march]
    return TOL_FD if d < 0.1 * TOL_FD else 16 * d


# ── the rows ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def dde_rows(M, free, X, D, wrong=None):
    """d(dE_m) = x_m^T M_s dx_m, m = 1 .. n, from X = x_{-1}, x_0, x_1 .. x_n and D = dx_{-1}, dx_0, dx_1 .. dx_n (rows m + 1)."""
    Ms = ec.msym(M)
    X, D = np.asarray(X, dtype=float), np.asarray(D, dtype=float)
    if wrong == "x_masked":
        X = X * free
    if wrong == "mask_out":
        D = D * free
    return np.array([X[m + 1] @ (Ms @ D[m + 1]) for m in range(1, X.shape[0] - 1)])


def energy_series(M, X):
    """dE_m = 1/2 x_m^T M x_m, m = 1 .. n."""
    X = np.asarray(X, dtype=float)
    return np.array([0.5 * (X[m + 1] @ (M @ X[m + 1])) for m in range(1, X.shape[0] - 1)])


class TangentEnergyModel(TangentModel):
    """``TangentModel`` (on an ``adjoint_energy_cases.EnergyNonlinearStepModel``: ``with_energy``) with the rows and the product."""

    def tangent_energy(self, first_order, X, du=None, dx0=None, dxm1=None, wrong=None):
        """(D, dy, dde [n])."""
        D, dy = self.tangent(first_order, X, du, dx0, dxm1)
        return D, dy, dde_rows(self.m.M, self.m.free, X, D, wrong)

    def energy_product(self, first_order, X, e, v):
        """H_E v = sum_m e_m X_m^T M_s X_m v over the controls, (n, n_act): one tangent that keeps dx_m, then the adjoint whose energy
        forcing of backward step m is e_m M_s dx_m -- ``adjoint_energy`` on the tangent states in the place of the states, with J still
        at the states (the parent's ``_products`` reads the forcing column from ``_e_src``)."""
        m = self.m
        D, _ = self.tangent(first_order, X, v)
        return energy_adjoint_of(m, first_order, X, D, e)[0]


class _ForcedStep(ec.EnergyNonlinearStepModel):
    """The nonlinear model's adjoint with the forcing column of backward step m taken from ``_F`` (the tangent states) instead of X,
    while J(x_m)^T stays at the states: the second source of the device's energy forcing."""

    _F = None

    def _products(self, X, col, am, ac, wrong):
        out = super(ec.EnergyNonlinearStepModel, self)._products(X, col, am, ac, wrong)
        return out + self._e[col - 2] * (ec.msym(self.M) @ self._F[col]) if col >= 2 else out


def energy_adjoint_of(model, first_order, X, F, e):
    """(g, dx0, dxm1, mu) of the nonlinear model's adjoint with the energy forcing e_m M_s F[m + 1] (F = X: the gradient of
    sum e_m dE_m; F = D: the Gauss-Newton product).  The class of the object is moved for the call, as ``with_energy`` moves it."""
    X, F, e = np.asarray(X, dtype=float), np.asarray(F, dtype=float), np.asarray(e, dtype=float)
    n = X.shape[0] - 2
    cls = model.__class__
    model.__class__ = _ForcedStep
    model._e, model._F = e, F
    try:
        return model.adjoint(first_order, X, None, e[n - 1] * (ec.msym(model.M) @ F[n + 1]))
    finally:
        model.__class__ = cls
        del model._e, model._F


# ── closed loops ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def loop_dde(loop, f, t, wrong=None):
    """The rows of a closed loop from ``Loop.forward()`` and ``tangent_loop_model.tangent``."""
    return dde_rows(loop.plant.M, loop.plant.free, f["X"], t["dX"], wrong)


def loop_energy(loop):
    return energy_series(loop.plant.M, loop.forward()["X"])


class ForcedLoop(ec.EnergyLoop):
    """``EnergyLoop`` whose forcing column comes from ``F`` (n + 2, N) instead of the states: with F = dX of a tangent, ``adjoint(f, w, r)``
    is the closed-loop Gauss-Newton product's backward march."""

    F = None

    @classmethod
    def of(cls, loop, e, F):
        q = super().of(loop, e)
        q.F = np.asarray(F, dtype=float)
        return q

    def _products(self, X, col, a_m, a_c):
        out = super(ec.EnergyLoop, self)._products(X, col, a_m, a_c)
        return out + self.e[col - 2] * (ec.msym(self.plant.M) @ self.F[col]) if col >= 2 else out

    def adjoint(self, f, w, r, z=None, wrong=None):
        zz = (0.0 if z is None else np.asarray(z, dtype=float)) + self.e[self.n - 1] * (ec.msym(self.plant.M) @ self.F[self.n + 1])
        return super(ec.EnergyLoop, self).adjoint(f, w, r, zz, wrong)


__all__ = ["HOST_FD_DISTANCE", "fd_tol", "dde_rows", "energy_series", "TangentEnergyModel", "energy_adjoint_of", "loop_dde", "loop_energy",
           "ForcedLoop", "tlm"]
