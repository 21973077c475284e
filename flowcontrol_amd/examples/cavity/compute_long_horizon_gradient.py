"""Gradient of a closed-loop cost of the open-cavity flow (Re = 7500, nonlinear equations) over a LONG horizon on an MI355X: base flow
as the other cavity scripts compute it, the first-order low-pass controller of ``run_cavity_example --closed-loop`` around it, then
``J = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` over the next ``num_steps`` steps and its gradient with respect to the controller's
matrices from ONE forward closed-loop run and ONE backward march on the device (``flu.closed_loop_gradient``).

The adjoint of the nonlinear stepper reads the forward trajectory.  Kept whole, that is 8 N bytes per step -- over the 10 000 steps of
``run_cavity_example`` more than the run's own working set by orders of magnitude.  ``checkpoint_every="auto"`` keeps a pair of time
levels every ceil(sqrt(2 n)) steps and one dense segment instead, and the march recomputes one segment at a time ("Checkpointed tape",
DESIGN §5.4): the same gradient bit for bit, for one more forward run.  The script prints the bytes held next to what the dense tape
would have needed.  Device extension: the reference's optimiser is derivative-free.

    python -m flowcontrol_amd.examples.cavity.compute_long_horizon_gradient [num_steps] [--every auto|C]
"""
import argparse
import logging
import time
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.adjoint import AdjointRun, checkpoint_spacing
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cavity.cavityflowsolver import DEFAULT_MESH, CavityFlowSolver
from flowcontrol_amd.flowsolverparameters import ParamIC


def main(num_steps: int = 10000, every: int | str = "auto", r_weight: float = 1e-3, path_out: Path | None = None):
    logging.basicConfig(level=logging.INFO)
    out = Path(path_out) if path_out else Path.cwd() / "data_output"
    fs = CavityFlowSolver.make_default(Re=7500, path_out=out, num_steps=num_steps, save_every=0, verbose=0, meshpath=DEFAULT_MESH)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.1)
    t0 = time.perf_counter()
    fs.compute_steady_state(method="picard", max_iter=10, tol=1e-7, u_ctrl=[0.0])
    fs.compute_steady_state(method="newton", max_iter=10, u_ctrl=[0.0], initial_guess=fs.fields.UP0)
    print(f"base flow on {fs.th.N} dofs: {time.perf_counter() - t0:.2f} s")
    fs.initialize_time_stepping(ic=None)
    K = Controller(A=[[-100.0]], B=[[1.0]], C=[[50.0]], D=[[0.0]])
    n = int(num_steps)
    c = checkpoint_spacing(every, n)
    try:
        with AdjointRun(fs, tape=n, loop=n, checkpoint_every=c) as run:
            dev = run.dev
            Q, R = np.eye(dev.n_sens), r_weight * np.eye(dev.n_act)
            t0 = time.perf_counter()
            J, g = flu.closed_loop_gradient(fs, K, n, Q, R, adjoint=run)
            wall = time.perf_counter() - t0
            info = run.info()
    finally:
        fs.th.release_device()
    tape = info["tape"]
    dense = 8 * fs.th.N * (n + 2)
    print(f"{n} closed-loop steps forward and back: {wall:.2f} s; J = {J:.6e}")
    print(f"state tape: checkpoints every {tape['every']} steps, {tape['bytes'] / 1e6:.1f} MB held ({tape['replayed']} forward steps recomputed); "
          f"the dense tape would hold {dense / 1e6:.1f} MB ({dense / tape['bytes']:.1f} x)")
    for name in ("A", "B", "C", "D"):
        print(f"  dJ/d{name} = {np.asarray(g[name]).ravel()}")
    return J, g, info


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("num_steps", nargs="?", type=int, default=10000)
    ap.add_argument("--every", default="auto")
    a = ap.parse_args()
    main(a.num_steps, a.every if a.every == "auto" else int(a.every))
