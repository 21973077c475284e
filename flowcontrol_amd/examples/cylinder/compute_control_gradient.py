"""Gradient of the linearised cylinder's sensor energy with respect to the actuation sequence, from one backward march on the device
(``flu.quadratic_cost_gradient``, ``fc_run_adjoint``), and a handful of steepest-descent steps with it.

The flow is the cylinder at Re = 100 linearised about its base flow (``is_eq_nonlinear=False``), started from the usual perturbation.
Over a horizon of ``n_steps`` steps the cost is ``J(u) = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)``; its gradient with respect to all
``n_steps x n_act`` controls costs one forward and one backward run, whatever their number (finite differences: one run each).  J is
quadratic in u, so the exact line search along ``-grad`` needs one more gradient: ``H g = grad(u + g) - grad(u)`` and
``alpha = g . g / g . H g``.

    python -m flowcontrol_amd.examples.cylinder.compute_control_gradient [--nonlinear | --gauss-newton] [out_dir [base_flow.npz]]

``--nonlinear`` runs the same descent on the nonlinear perturbation equations (``is_eq_nonlinear=True``): the forward run is taped on
the device (``AdjointRun(fs, tape=n_steps)``, 8 N bytes per step) and the backward march applies the transposed Jacobian of the
convective term at every taped state.  J is then no longer quadratic in u: the step from the gradient difference is a secant step, and
it is halved until the cost goes down.

``--gauss-newton`` (nonlinear equations too) replaces the secant steps by Gauss-Newton steps: the forward run at the present controls is
taped once, the gradient comes from one backward march on that tape, and the step solves ``(J^T Q J + R) d = -grad`` by a few
conjugate-gradient iterations whose products are ``flu.gauss_newton_product`` -- one tangent march (``fc_run_tangent``) and
one backward march each, on the SAME tape: no forward run per product.  The step is halved until the cost goes down.

``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the steady-state computation.  With that file the script ran
on an MI355X: the figures are in DESIGN §5.4.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC

logger = logging.getLogger(__name__)


def _solver(out: Path, base_flow: Path | None = None, nonlinear: bool = False):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.params_solver.is_eq_nonlinear = bool(nonlinear)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    if base_flow is None:
        fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
        fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    else:
        fs._assign_steady_state(*Function(fs.W, np.load(base_flow)["UP0"]).split())
    fs.initialize_time_stepping(ic=None)
    return fs


def descend(fs, n_steps: int = 400, n_iter: int = 5, r_weight: float = 1e-3) -> dict:
    """``n_iter`` steepest-descent steps with exact line search on the horizon of ``n_steps`` steps; returns the costs and the last
    control sequence.  A nonlinear solver is taped (see the module text); its step is halved until the cost goes down."""
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    fs._begin_stepping()
    dev = fs.th.device()
    Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
    u = np.zeros((n_steps, dev.n_act))
    costs = []
    with flu.AdjointRun(fs, tape=n_steps if nonlinear else None) as run:
        J, g = flu.quadratic_cost_gradient(fs, u, Q, R, adjoint=run)
        for it in range(n_iter):
            costs.append(J)
            gg = float(np.sum(g * g))
            logger.info("iteration %d: J = %.6e, |grad| = %.3e", it, J, np.sqrt(gg))
            if gg == 0.0:
                break
            _, g_shift = flu.quadratic_cost_gradient(fs, u + g, Q, R, adjoint=run)
            curv = float(np.sum(g * (g_shift - g)))  # g . H g
            if not curv > 0.0:
                break
            alpha = gg / curv
            J_new, g_new = flu.quadratic_cost_gradient(fs, u - alpha * g, Q, R, adjoint=run)
            for _ in range(8 if nonlinear else 0):
                if J_new <= J:
                    break
                alpha *= 0.5
                J_new, g_new = flu.quadratic_cost_gradient(fs, u - alpha * g, Q, R, adjoint=run)
            u = u - alpha * g
            J, g = J_new, g_new
        costs.append(J)
        logger.info("after %d steps: J = %.6e (from %.6e); adjoint setup %.1f MiB", len(costs) - 1, J, costs[0], run.info()["bytes"] / 2**20)
    return {"J": np.array(costs), "u": u}


def descend_gauss_newton(fs, n_steps: int = 400, n_iter: int = 3, r_weight: float = 1e-3, cg_iter: int = 8) -> dict:
    """``n_iter`` Gauss-Newton steps on the horizon of ``n_steps`` steps of a NONLINEAR solver, each from ``cg_iter`` CG iterations on
    ``(J^T Q J + R) d = -grad`` with the tape of one forward run; returns the costs and the last control sequence."""
    if not fs.params_solver.is_eq_nonlinear:
        raise ValueError("descend_gauss_newton: the linearised cost is quadratic -- descend() already takes exact steps")
    fs._begin_stepping()
    dev = fs.th.device()
    Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
    order = 1 if fs.order == 1 else 2
    slot = SLOT_BDF1 if order == 1 else SLOT_BDF2
    u = np.zeros((n_steps, dev.n_act))
    start = dev.get_state()
    cost = lambda y, uu: 0.5 * float(np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", uu, R, uu))  # noqa: E731
    costs = []
    with flu.AdjointRun(fs, tape=n_steps) as run:
        dev.tangent_reserve(1)
        try:
            for it in range(n_iter):
                y, _ = run.forward(u, first_order=order, compute_energy=False)  # the tape now holds the run at u
                J = cost(y, u)
                g = run.run(n_steps, w=y @ Q, first_order=order, state_gradients=False)[0] + u @ R
                costs.append(J)
                logger.info("iteration %d: J = %.6e, |grad| = %.3e", it, J, np.linalg.norm(g))
                d, r = np.zeros_like(u), -g
                p, rr = r.copy(), float(np.sum(r * r))
                for _ in range(cg_iter):
                    if rr == 0.0:
                        break
                    Gp = flu.gauss_newton_product(fs, u, Q, R, p, adjoint=run)  # (tape current: one tangent + one backward march)
                    alpha = rr / float(np.sum(p * Gp))
                    d, r = d + alpha * p, r - alpha * Gp
                    rr, rr0 = float(np.sum(r * r)), rr
                    p = r + (rr / rr0) * p
                dev.set_state(*start)
                step = 1.0
                for _ in range(8):
                    y_new, _ = dev.run(slot, n_steps, u + step * d, compute_energy=False)
                    dev.set_state(*start)
                    if cost(y_new, u + step * d) <= J:
                        break
                    step *= 0.5
                u = u + step * d
            y, _ = dev.run(slot, n_steps, u, compute_energy=False)
            dev.set_state(*start)
            costs.append(cost(y, u))
            logger.info("after %d Gauss-Newton steps: J = %.6e (from %.6e)", n_iter, costs[-1], costs[0])
        finally:
            dev.tangent_reserve(0)
    return {"J": np.array(costs), "u": u}


def main(out: Path, base_flow: Path | None = None, nonlinear: bool = False, gauss_newton: bool = False) -> dict:
    fs = _solver(out, base_flow, nonlinear or gauss_newton)
    try:
        res = descend_gauss_newton(fs) if gauss_newton else descend(fs)
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "control_gradient.npz", **res)
        return res
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    argv = [a for a in sys.argv[1:] if a not in ("--nonlinear", "--gauss-newton")]
    main(Path(argv[0]) if argv else Path.cwd() / "data_output", Path(argv[1]) if len(argv) > 1 else None, nonlinear="--nonlinear" in sys.argv[1:],
         gauss_newton="--gauss-newton" in sys.argv[1:])
