"""Transient growth of the open-cavity flow (Re = 7500) on an MI355X: base flow and linearised operator as the other cavity scripts
compute them, then the gain curve G(T) over a list of horizons (``flu.transient_growth``: every horizon warm-started from the previous
one), then the leading optimal perturbation of the last horizon and its response, written as checkpoint series with the package's
exporter (``flu.write_xdmf``).  Device extension: the reference has no transient-growth analysis.

    python -m flowcontrol_amd.examples.cavity.compute_transient_growth [--fine] [--horizons 100,200,400] [--modes 2] [--tol 1e-6] [--max-iter 50]
"""
import argparse
import logging
import time
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.examples.cavity.cavityflowsolver import DEFAULT_MESH, CavityFlowSolver
from flowcontrol_amd.fem.spaces import Function


def main(horizons=(100, 200, 400), n_modes: int = 2, fine: bool = False, path_out: Path | None = None, tol: float = 1e-6, max_iter: int = 50):
    logging.basicConfig(level=logging.INFO)
    out = Path(path_out) if path_out else Path.cwd() / "data_output"
    mesh = DEFAULT_MESH.with_name("cavity_fine.npz") if fine else DEFAULT_MESH
    fs = CavityFlowSolver.make_default(Re=7500, path_out=out, num_steps=max(horizons), save_every=0, verbose=0, meshpath=mesh)
    fs.params_solver.is_eq_nonlinear = False  # optimal perturbations are those of the linearised stepper
    t0 = time.perf_counter()
    fs.compute_steady_state(method="picard", max_iter=10, tol=1e-7, u_ctrl=[0.0])
    fs.compute_steady_state(method="newton", max_iter=10, u_ctrl=[0.0], initial_guess=fs.fields.UP0)
    print(f"base flow on {fs.th.N} dofs: {time.perf_counter() - t0:.2f} s")
    fs.initialize_time_stepping(ic=None)
    t0 = time.perf_counter()
    gains, results = flu.transient_growth(fs, horizons, n_modes=n_modes, tol=tol, max_iter=max_iter)
    dt = fs.params_time.dt
    print(f"G(T) over {len(horizons)} horizons: {time.perf_counter() - t0:.2f} s")
    for n, g, r in zip(horizons, gains, results):
        print(f"  T = {n * dt:8.3f} ({n} steps): gains {g}, {r.iterations} iterations, converged {r.converged}, residuals {r.residuals}")
    last = results[-1]
    flu.write_xdmf(out / "optimal_perturbation.xdmf", Function(fs.W, last.modes[0]), "optimal_perturbation", time_step=0.0)
    flu.write_xdmf(out / "optimal_response.xdmf", Function(fs.W, last.responses[0]), "optimal_response", time_step=horizons[-1] * dt)
    np.savetxt(out / "transient_growth.csv", np.c_[np.asarray(horizons) * dt, gains], delimiter=",", header="T," + ",".join(f"G{i}" for i in range(gains.shape[1])))
    return gains, results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fine", action="store_true")
    ap.add_argument("--horizons", default="100,200,400")
    ap.add_argument("--modes", type=int, default=2)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=50)
    a = ap.parse_args()
    main(tuple(int(n) for n in a.horizons.split(",")), a.modes, a.fine, tol=a.tol, max_iter=a.max_iter)
