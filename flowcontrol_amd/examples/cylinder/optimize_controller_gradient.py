"""A few gradient-descent steps on the matrices of the shipped cylinder controller, with the exact gradient of the closed loop's cost
from one forward and one backward run on the device (``flu.closed_loop_gradient``, ``fc_run_adjoint_closed_loop``).

The flow is the cylinder at Re = 100 about its base flow, started from the usual perturbation, in closed loop with
``Kopt_reduced13.mat`` (13 states: 13^2 + 2 * 13 + 1 = 196 parameters).  Over a horizon of ``n_steps`` steps the cost is the sensor
cost ``J(K) = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)``.  The reference's ``utils/optim.py`` gives such costs to a derivative-free
optimiser, one closed-loop run per candidate; here every descent step costs one forward and one backward run, whatever the number of
parameters.  The step along ``-grad`` over the continuous-time ``(A, B, C, D)`` starts from a size that moves the matrices by
``first_move`` of their norm and is halved (backtracking) until the cost goes down.

    python -m flowcontrol_amd.examples.cylinder.optimize_controller_gradient [--nonlinear] [out_dir [base_flow.npz]]

``--nonlinear`` runs the same descent on the nonlinear perturbation equations: the forward run is then also taped state by state
(``AdjointRun(fs, tape=n_steps, loop=n_steps)``).  ``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the
steady-state computation.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cylinder.compute_control_gradient import _solver
from flowcontrol_amd.examples.data import controller_file

logger = logging.getLogger(__name__)

NAMES = ("A", "B", "C", "D")


def descend(fs, K: Controller, n_steps: int = 200, n_iter: int = 5, r_weight: float = 1e-3, first_move: float = 1e-2) -> dict:
    """``n_iter`` descent steps with a backtracking line search on the horizon of ``n_steps`` steps; returns the costs and the last
    controller's matrices."""
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    fs._begin_stepping()
    dev = fs.th.device()
    Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
    mats = {k: getattr(K, k).copy() for k in NAMES}
    x0 = np.array(K.x, copy=True)
    make = lambda m: Controller(m["A"], m["B"], m["C"], m["D"], x0=x0)  # noqa: E731
    costs = []
    with flu.AdjointRun(fs, tape=n_steps if nonlinear else None, loop=n_steps) as run:
        J, g = flu.closed_loop_gradient(fs, make(mats), n_steps, Q, R, adjoint=run)
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
                J_new, g_new = flu.closed_loop_gradient(fs, make(trial), n_steps, Q, R, adjoint=run)
                if np.isfinite(J_new) and J_new < J:
                    break
                alpha *= 0.5
            else:
                break  # no decrease along -grad at any tried step
            mats, J, g = trial, J_new, g_new
        costs.append(J)
        logger.info("after %d steps: J = %.6e (from %.6e); adjoint setup %.1f MiB", len(costs) - 1, J, costs[0], run.info()["bytes"] / 2**20)
    return {"J": np.array(costs), **mats}


def main(out: Path, base_flow: Path | None = None, nonlinear: bool = False) -> dict:
    fs = _solver(out, base_flow, nonlinear)
    try:
        res = descend(fs, Controller.from_file(file=controller_file(), x0=None))
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "controller_gradient.npz", **res)
        return res
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    argv = [a for a in sys.argv[1:] if a != "--nonlinear"]
    main(Path(argv[0]) if argv else Path.cwd() / "data_output", Path(argv[1]) if len(argv) > 1 else None, nonlinear="--nonlinear" in sys.argv[1:])
