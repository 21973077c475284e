"""A few gradient-descent steps on the matrices of the shipped cylinder controller, with the exact gradient of the closed loop's cost
from one forward and one backward run on the device (``flu.closed_loop_gradient``, ``fc_run_adjoint_closed_loop``).

The flow is the cylinder at Re = 100 about its base flow, started from the usual perturbation, in closed loop with
``Kopt_reduced13.mat`` (13 states: 13^2 + 2 * 13 + 1 = 196 parameters).  Over a horizon of ``n_steps`` steps the cost is the sensor
cost ``J(K) = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)``.  The reference's ``utils/optim.py`` gives such costs to a derivative-free
optimiser, one closed-loop run per candidate; here every descent step costs one forward and one backward run, whatever the number of
parameters.  The step along ``-grad`` over the continuous-time ``(A, B, C, D)`` starts from a size that moves the matrices by
``first_move`` of their norm and is halved (backtracking) until the cost goes down.

    python -m flowcontrol_amd.examples.cylinder.optimize_controller_gradient [--nonlinear] [--cost energy] [--gauss-newton] [out_dir [base_flow.npz]]

``--gauss-newton`` takes damped Gauss-Newton steps instead: the four matrices are scaled very differently, which is
where curvature pays.  Each outer iteration solves ``(H + lambda I) p = -grad`` by a few CG iterations whose products are
``flu.closed_loop_gauss_newton_product`` -- per product one taped closed-loop run, one closed-loop tangent march
(``fc_run_tangent_closed_loop``) and one backward march on the same tapes.

``--cost energy`` descends on the reference's own cost instead (``src/utils/optim.py``), the one ``optim.closed_loop_costs`` ranks
candidates by: ``J = Tnorm sum_m dE_m + u_penalty Tnorm sum_m |u_m|^2`` with ``dE`` the perturbation kinetic energy every step logs
(``optim.energy_cost_weights``; ``flu.closed_loop_gradient(..., energy=)``).  The forward run is then taped state by state on the
linearised solver too.  With ``--gauss-newton`` the CG products carry the same weights (``flu.closed_loop_gauss_newton_product(...,
energy=)``): the tangent march keeps its states and the backward march is forced with ``e_m M dx_m`` (DESIGN §5.6 "Energy").

``--nonlinear`` runs the same descent on the nonlinear perturbation equations: the forward run is then also taped state by state
(``AdjointRun(fs, tape=n_steps, loop=n_steps)``).  ``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the
steady-state computation.
"""
import argparse
import logging
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cylinder.compute_control_gradient import _solver
from flowcontrol_amd.examples.data import controller_file

logger = logging.getLogger(__name__)

NAMES = ("A", "B", "C", "D")


def descend(fs, K: Controller, n_steps: int = 200, n_iter: int = 5, r_weight: float = 1e-3, first_move: float = 1e-2, cost: str = "sensors",
            u_penalty: float = 1e-3) -> dict:
    """``n_iter`` descent steps with a backtracking line search on the horizon of ``n_steps`` steps; returns the costs and the last
    controller's matrices.  ``cost``: ``"sensors"`` (Q = I, R = r_weight I) or ``"energy"`` (the reference's J with ``u_penalty``)."""
    if cost not in ("sensors", "energy"):
        raise ValueError(f"cost must be 'sensors' or 'energy', got {cost!r}")
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    fs._begin_stepping()
    dev = fs.th.device()
    Q, R, energy = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act), None
    if cost == "energy":
        from flowcontrol_amd.optim import energy_cost_weights

        energy, Q, R, _, _ = energy_cost_weights(n_steps, fs.params_time.dt, dev.n_sens, dev.n_act, "integral", u_penalty)
    mats = {k: getattr(K, k).copy() for k in NAMES}
    x0 = np.array(K.x, copy=True)
    make = lambda m: Controller(m["A"], m["B"], m["C"], m["D"], x0=x0)  # noqa: E731
    costs = []
    with flu.AdjointRun(fs, tape=n_steps if (nonlinear or energy is not None) else None, loop=n_steps) as run:
        J, g = flu.closed_loop_gradient(fs, make(mats), n_steps, Q, R, adjoint=run, energy=energy)
        for it in range(n_iter):
            costs.append(J)
            gg = float(sum(np.sum(g[k] ** 2) for k in NAMES))
            logger.info("iteration %d: J = %.6e, |grad| = %.3e", it, J, np.sqrt(gg))
            if gg == 0.0:
                break
            size = float(np.sqrt(sum(np.sum(mats[k] ** 2) for k in NAMES)))
            alpha = first_move * size / np.sqrt(gg)
            for _ in range(12):
                trial = {k: mats[k] - alpha * g[k] for k in NAMES}
                J_new, g_new = flu.closed_loop_gradient(fs, make(trial), n_steps, Q, R, adjoint=run, energy=energy)
                if np.isfinite(J_new) and J_new < J:
                    break
                alpha *= 0.5
            else:
                break  # no decrease along -grad at any tried step
            mats, J, g = trial, J_new, g_new
        costs.append(J)
        logger.info("after %d steps: J = %.6e (from %.6e); adjoint setup %.1f MiB", len(costs) - 1, J, costs[0], run.info()["bytes"] / 2**20)
    return {"J": np.array(costs), **mats}


def descend_gauss_newton(fs, K: Controller, n_steps: int = 200, n_iter: int = 3, r_weight: float = 1e-3, cg_iter: int = 6, damping: float = 1e-3,
                         cost: str = "sensors", u_penalty: float = 1e-3) -> dict:
    """``n_iter`` damped Gauss-Newton steps on the cost ``cost`` (as :func:`descend`) over the continuous-time ``(A, B, C, D)``: each outer iteration solves
    ``(H + lambda I) p = -grad`` by ``cg_iter`` CG iterations whose products are ``flu.closed_loop_gauss_newton_product`` (a taped run,
    a tangent and a backward march on the device), ``lambda = damping * (g . H g) / (g . g)``, then backtracks along ``p``.  ``H`` is the
    Gauss-Newton matrix of the loop with its clamp pattern held.  Returns the costs and the last controller's matrices."""
    if cost not in ("sensors", "energy"):
        raise ValueError(f"cost must be 'sensors' or 'energy', got {cost!r}")
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    fs._begin_stepping()
    dev = fs.th.device()
    Q, R, energy = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act), None
    if cost == "energy":
        from flowcontrol_amd.optim import energy_cost_weights

        energy, Q, R, _, _ = energy_cost_weights(n_steps, fs.params_time.dt, dev.n_sens, dev.n_act, "integral", u_penalty)
    mats = {k: getattr(K, k).copy() for k in NAMES}
    x0 = np.array(K.x, copy=True)
    make = lambda m: Controller(m["A"], m["B"], m["C"], m["D"], x0=x0)  # noqa: E731
    dot = lambda a, b: float(sum(np.sum(a[k] * b[k]) for k in NAMES))  # noqa: E731
    axpy = lambda a, x, y: {k: a * x[k] + y[k] for k in NAMES}  # noqa: E731
    costs = []
    with flu.AdjointRun(fs, tape=n_steps if (nonlinear or energy is not None) else None, loop=n_steps) as run:
        J, g = flu.closed_loop_gradient(fs, make(mats), n_steps, Q, R, adjoint=run, energy=energy)
        for it in range(n_iter):
            costs.append(J)
            logger.info("iteration %d: J = %.6e, |grad| = %.3e", it, J, np.sqrt(dot(g, g)))
            if dot(g, g) == 0.0:
                break
            Kc = make(mats)
            product = lambda v: flu.closed_loop_gauss_newton_product(fs, Kc, n_steps, Q, R, {k: v[k] for k in NAMES}, adjoint=run, energy=energy)  # noqa: E731,B023
            lam = None
            p, r = {k: np.zeros_like(mats[k]) for k in NAMES}, {k: -g[k] for k in NAMES}
            d, rr = dict(r), dot(r, r)
            for _ in range(cg_iter):
                if rr == 0.0:
                    break
                Hd = product(d)
                if lam is None:  # (the first direction is -grad: its Rayleigh quotient scales the damping)
                    lam = damping * dot(d, Hd) / dot(d, d)
                Hd = axpy(lam, d, Hd)
                curv = dot(d, Hd)
                if not curv > 0.0:  # (H d = 0, e.g. every control value clamped: no curvature along d, CG ends with what it has)
                    break
                alpha = rr / curv
                p, r = axpy(alpha, d, p), axpy(-alpha, Hd, r)
                rr, rr0 = dot(r, r), rr
                d = axpy(rr / rr0, d, r)
            step = 1.0
            for _ in range(12):
                trial = axpy(step, p, mats)
                J_new, g_new = flu.closed_loop_gradient(fs, make(trial), n_steps, Q, R, adjoint=run, energy=energy)
                if np.isfinite(J_new) and J_new < J:
                    break
                step *= 0.5
            else:
                break  # no decrease along the Gauss-Newton direction at any tried step
            mats, J, g = trial, J_new, g_new
        costs.append(J)
        logger.info("after %d Gauss-Newton steps: J = %.6e (from %.6e)", len(costs) - 1, J, costs[0])
    return {"J": np.array(costs), **mats}


def main(out: Path, base_flow: Path | None = None, nonlinear: bool = False, cost: str = "sensors", gauss_newton: bool = False) -> dict:
    fs = _solver(out, base_flow, nonlinear)
    try:
        K = Controller.from_file(file=controller_file(), x0=None)
        res = descend_gauss_newton(fs, K, cost=cost) if gauss_newton else descend(fs, K, cost=cost)
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "controller_gradient.npz", **res)
        return res
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    ap = argparse.ArgumentParser(description="Gradient descent on the matrices of the shipped cylinder controller.")
    ap.add_argument("--nonlinear", action="store_true", help="descend on the nonlinear perturbation equations")
    ap.add_argument("--cost", choices=("sensors", "energy"), default="sensors", help="the sensor cost (default) or the reference's energy cost J")
    ap.add_argument("out_dir", nargs="?", type=Path, default=Path.cwd() / "data_output")
    ap.add_argument("base_flow", nargs="?", type=Path, default=None, help="npz with the key UP0: skips the steady-state computation")
    ap.add_argument("--gauss-newton", action="store_true", help="damped Gauss-Newton steps on the chosen cost (CG on flu.closed_loop_gauss_newton_product)")
    args = ap.parse_args()  # (a missing or unknown --cost value ends here, before any solver is built)
    main(args.out_dir, args.base_flow, nonlinear=args.nonlinear, cost=args.cost, gauss_newton=args.gauss_newton)
