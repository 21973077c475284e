"""One control sequence for an ensemble of initial perturbations: steepest descent on the MEAN sensor energy of k runs of the cylinder,
with the gradients of all k runs from one batched backward march (``flu.batched_cost_gradient``, ``fc_run_adjoint_batch``).

k runs of the cylinder at Re = 100 start from k different perturbations (the usual vortex at k positions and amplitudes) and are driven
by ONE shared control sequence ``u [n_steps, n_act]``.  The cost is the ensemble mean ``J(u) = 1/k sum_s J_s(u)`` of
``J_s = 1/2 sum_m (y_{m,s}^T Q y_{m,s} + u_m^T R u_m)``; its gradient is the column mean of the k per-run gradients, which one batched
forward run and one batched backward march deliver together -- the factors are read once per step for all k columns, forwards and
backwards.  The mean is taken AFTER the march: a march on the mean trajectory would be the gradient of another cost.

    python -m flowcontrol_amd.examples.cylinder.compute_ensemble_gradient [--nonlinear] [--k 8] [out_dir [base_flow.npz]]

``--nonlinear`` runs the descent on the nonlinear perturbation equations: the batched forward run is taped on the device
(``AdjointRun(bfs, tape=n_steps)``, 8 N KB bytes per step with KB the padded batch width) and the march applies the transposed Jacobian
of the convective term at every taped state of every column.  The step is a secant step along ``-grad`` from one more gradient, halved
until the mean cost goes down.  ``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the steady-state computation.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.batch import BatchedFlowSolver
from flowcontrol_amd.examples.cylinder.compute_control_gradient import _solver
from flowcontrol_amd.flowsolverparameters import ParamIC

logger = logging.getLogger(__name__)


def ensemble(k: int) -> list[ParamIC]:
    """k perturbations of the wake: the vortex of the single-run examples moved downstream and off the axis, at decreasing amplitude."""
    return [ParamIC(xloc=1.5 + 1.5 * s / max(k - 1, 1), yloc=0.3 * np.sin(2.1 * s), radius=0.5, amplitude=1.0 - 0.5 * s / max(k, 1)) for s in range(k)]


def descend(fs, k: int = 8, n_steps: int = 200, n_iter: int = 5, r_weight: float = 1e-3) -> dict:
    """``n_iter`` descent steps on the mean cost over ``k`` initial perturbations with one shared control sequence; returns the mean
    costs, the per-run costs of the last iterate and the control sequence."""
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    bfs = BatchedFlowSolver(fs, k)
    bfs.initialize_time_stepping(ics=ensemble(k))
    dev = bfs.dev
    Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
    u = np.zeros((n_steps, dev.n_act))

    def mean_gradient(run, uu):
        J, g = flu.batched_cost_gradient(bfs, np.repeat(uu[:, None, :], k, axis=1), Q, R, adjoint=run)
        return float(J.mean()), g.mean(axis=1), J  # (the mean AFTER the march)

    costs = []
    try:
        with flu.AdjointRun(bfs, tape=n_steps if nonlinear else None) as run:
            J, g, Js = mean_gradient(run, u)
            for it in range(n_iter):
                costs.append(J)
                gg = float(np.sum(g * g))
                logger.info("iteration %d: mean J = %.6e (runs %.3e .. %.3e), |grad| = %.3e", it, J, Js.min(), Js.max(), np.sqrt(gg))
                if gg == 0.0:
                    break
                _, g_shift, _ = mean_gradient(run, u + g)
                curv = float(np.sum(g * (g_shift - g)))  # g . H g (exact for the linearised equations)
                if not curv > 0.0:
                    break
                alpha = gg / curv
                J_new, g_new, Js_new = mean_gradient(run, u - alpha * g)
                for _ in range(8):
                    if J_new <= J:
                        break
                    alpha *= 0.5
                    J_new, g_new, Js_new = mean_gradient(run, u - alpha * g)
                u = u - alpha * g
                J, g, Js = J_new, g_new, Js_new
            costs.append(J)
            info = dev.adjoint_batch_info(1)
            logger.info("after %d steps: mean J = %.6e (from %.6e); per slot %.1f MiB tiled transposed factors, %.1f MiB march buffers, %.1f MiB tape",
                        len(costs) - 1, J, costs[0], info["tile_bytes"] / 2**20, info["march_bytes"] / 2**20, info["tape_bytes"] / 2**20)
    finally:
        bfs.close()
    return {"J": np.array(costs), "J_runs": Js, "u": u}


def main(out: Path, base_flow: Path | None = None, nonlinear: bool = False, k: int = 8) -> dict:
    fs = _solver(out, base_flow, nonlinear)
    try:
        res = descend(fs, k=k)
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "ensemble_gradient.npz", **res)
        return res
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    argv, k, nonlinear = [], 8, False
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--nonlinear":
            nonlinear = True
        elif a == "--k":
            k = int(next(it))
        elif a.startswith("--k="):
            k = int(a[4:])
        else:
            argv.append(a)
    main(Path(argv[0]) if argv else Path.cwd() / "data_output", Path(argv[1]) if len(argv) > 1 else None, nonlinear=nonlinear, k=k)
