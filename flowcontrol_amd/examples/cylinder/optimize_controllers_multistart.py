"""Multi-start gradient descent on the shipped cylinder controller: k perturbed copies of ``Kopt_reduced13.mat`` descend TOGETHER, one
batched gradient per iteration (``flu.batched_closed_loop_gradient``, ``fc_run_adjoint_closed_loop_batch``).

The flow is the cylinder at Re = 100 about its base flow; run s of a ``BatchedFlowSolver`` starts from the usual perturbation and is
closed around candidate s.  Over a horizon of ``n_steps`` steps the cost of a candidate is
``J_s = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)``.  One iteration is ONE batched forward run and ONE batched backward march: the
factors are read once per step for all k candidates, where k single descents (optimize_controller_gradient.py) read them k times.
Every candidate takes its own step along ``-grad`` over its continuous-time ``(A, B, C, D)``: a step that moves its matrices by
``first_move`` of their norm at first, halved for that candidate whenever its cost did not go down (the candidate then stays where it
was), doubled (up to the first size) when it did.

    python -m flowcontrol_amd.examples.cylinder.optimize_controllers_multistart [--nonlinear] [out_dir [base_flow.npz]]

``--nonlinear`` runs the same descent on the nonlinear perturbation equations (``AdjointRun(bfs, tape=n_steps, loop=n_steps)``).
``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the steady-state computation.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.batch import BatchedFlowSolver
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cylinder.compute_control_gradient import _solver
from flowcontrol_amd.examples.data import controller_file

logger = logging.getLogger(__name__)

NAMES = ("A", "B", "C", "D")


def descend(fs, K: Controller, k: int = 8, n_steps: int = 200, n_iter: int = 5, r_weight: float = 1e-3, first_move: float = 1e-2, spread: float = 0.02,
            seed: int = 0) -> dict:
    """``n_iter`` joint descent steps of ``k`` copies of ``K`` whose matrices are perturbed by ``spread`` (relative, entry by entry;
    copy 0 is ``K`` itself); returns the costs ``J [n_iter + 1, k]`` and the best candidate's matrices."""
    rng = np.random.default_rng(seed)
    bfs = BatchedFlowSolver(fs, k)
    bfs.initialize_time_stepping()
    dev = bfs.dev
    Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
    mats = [{q: getattr(K, q) * (1.0 + (spread if s else 0.0) * rng.standard_normal(getattr(K, q).shape)) for q in NAMES} for s in range(k)]
    x0 = np.array(K.x, copy=True)
    make = lambda ms: [Controller(m["A"], m["B"], m["C"], m["D"], x0=x0) for m in ms]  # noqa: E731
    norm = lambda d: float(np.sqrt(sum(np.sum(d[q] ** 2) for q in NAMES)))  # noqa: E731
    nonlinear = bool(fs.params_solver.is_eq_nonlinear)
    try:
        with flu.AdjointRun(bfs, tape=n_steps if nonlinear else None, loop=n_steps) as run:
            J, g = flu.batched_closed_loop_gradient(bfs, make(mats), n_steps, Q, R, adjoint=run)
            costs = [J.copy()]
            move = np.full(k, first_move)
            for it in range(n_iter):
                logger.info("iteration %d: J = %s", it, np.array2string(J, precision=5))
                trial = []
                for s in range(k):
                    gn = norm(g[s])
                    alpha = move[s] * norm(mats[s]) / gn if gn > 0.0 else 0.0
                    trial.append({q: mats[s][q] - alpha * g[s][q] for q in NAMES})
                J_new, g_new = flu.batched_closed_loop_gradient(bfs, make(trial), n_steps, Q, R, adjoint=run)
                for s in range(k):
                    if np.isfinite(J_new[s]) and J_new[s] < J[s]:
                        mats[s], J[s], g[s] = trial[s], J_new[s], g_new[s]
                        move[s] = min(first_move, 2.0 * move[s])
                    else:
                        move[s] *= 0.5
                costs.append(J.copy())
            best = int(np.argmin(J))
            logger.info("after %d iterations: best candidate %d, J = %.6e (the shipped controller: %.6e)", n_iter, best, J[best], costs[0][0])
    finally:
        bfs.close()
    return {"J": np.array(costs), "best": best, **mats[best]}


def main(out: Path, base_flow: Path | None = None, nonlinear: bool = False) -> dict:
    fs = _solver(out, base_flow, nonlinear)
    try:
        res = descend(fs, Controller.from_file(file=controller_file(), x0=None))
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "controllers_multistart.npz", **res)
        return res
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    argv = [a for a in sys.argv[1:] if a != "--nonlinear"]
    main(Path(argv[0]) if argv else Path.cwd() / "data_output", Path(argv[1]) if len(argv) > 1 else None, nonlinear="--nonlinear" in sys.argv[1:])
