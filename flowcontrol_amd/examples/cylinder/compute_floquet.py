"""Floquet multipliers of the vortex-shedding cylinder at Re = 100: linear stability of a TIME-PERIODIC nonlinear flow
(``flu.floquet_multipliers``, ``fc_run_tangent_batch``).

The nonlinear perturbation equations (``is_eq_nonlinear=True``) are run as a batch of k identical simulations until the wake sheds
periodically.  The period is taken from the zero crossings of the first sensor's signal (mean removed) over the last part of that run
and ROUNDED TO WHOLE STEPS -- an approximation: the flow does not return exactly after n steps, so the map whose eigenvalues are
printed is that of n steps along a nearly closed orbit.  One such period is taped on the device (8 N KB bytes per step) and a block
Arnoldi iteration on the pair map ``(dx_0, dx_{-1}) -> (dx_n, dx_{n-1})`` about the trajectory of column 0 gives the leading
multipliers, k tangent marches per apply.  The basis vectors live on the host.

A limit cycle has the time-shift mode: its multiplier is 1.  The distance of the closest computed multiplier from 1 is printed as a
sanity figure for the period, the horizon of the transient and the Arnoldi size together; it is not asserted.

    python -m flowcontrol_amd.examples.cylinder.compute_floquet [--transient N] [--k K] [--blocks B] [out_dir [base_flow.npz]]

``base_flow.npz`` (key ``UP0``, e.g. tests/golden/cylinder_O1.npz) skips the steady-state computation.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.batch import BatchedFlowSolver
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC

logger = logging.getLogger(__name__)


def nonlinear_cylinder(out: Path, base_flow: Path | None = None):
    """The nonlinear cylinder at Re = 100 with its base flow (computed, or read from ``base_flow``) and the usual perturbation."""
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.params_solver.is_eq_nonlinear = True
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    if base_flow is None:
        fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
        fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    else:
        fs._assign_steady_state(*Function(fs.W, np.load(base_flow)["UP0"]).split())
    fs.initialize_time_stepping(ic=None)
    return fs


def period_in_steps(signal: np.ndarray) -> tuple[int, float]:
    """``(n, exact)``: the mean spacing of the upward zero crossings of ``signal`` minus its mean, in steps (linear interpolation
    between samples), and that spacing rounded to whole steps."""
    s = np.asarray(signal, dtype=float) - np.mean(signal)
    up = np.flatnonzero((s[:-1] < 0.0) & (s[1:] >= 0.0))
    if up.size < 3:
        raise RuntimeError("period_in_steps: fewer than three upward zero crossings -- the run is too short or the flow does not oscillate")
    t = up + s[up] / (s[up] - s[up + 1])
    exact = float(np.mean(np.diff(t)))
    return int(round(exact)), exact


def main(out: Path, base_flow: Path | None = None, transient: int = 30000, k: int = 8, blocks: int = 6, n_modes: int = 6) -> dict:
    fs = nonlinear_cylinder(out, base_flow)
    try:
        bfs = BatchedFlowSolver(fs, k)
        bfs.initialize_time_stepping()
        na = fs.params_control.actuator_number
        zero = np.zeros((k, na))
        tail = min(transient, 4000)
        y0 = np.empty(tail)
        for it in range(transient):
            y = bfs.step(zero)
            if y is None or np.any(bfs.diverged):
                raise RuntimeError(f"the transient run stopped at step {it}")
            if it >= transient - tail:
                y0[it - (transient - tail)] = y[0, 0]
        n, exact = period_in_steps(y0)
        logger.info("shedding period: %.3f steps = %.4f time units, rounded to %d steps (an approximation: the orbit does not close exactly)",
                    exact, exact * fs.params_time.dt, n)
        # the period goes onto the tape through the device handle: from here on the BatchedFlowSolver's own clock and log stand still
        dev = bfs.dev
        dev.adjoint_tape_reserve_batch(n)
        try:
            flu.forward_batch_taped(bfs, np.zeros((n, k, max(na, 1))))
            tape_bytes = dev.adjoint_tape_info_batch()["bytes"]
            lam, _, res = flu.floquet_multipliers(bfs, n, n_modes, blocks=blocks, vectors=True)
        finally:
            dev.adjoint_tape_reserve_batch(0)
        for i, (mu, r) in enumerate(zip(lam, res)):
            logger.info("multiplier %d: %+.6f %+.6fi, |mu| = %.6f, residual %.2e", i, mu.real, mu.imag, abs(mu), r)
        shift = float(np.min(np.abs(lam - 1.0)))
        logger.info("distance of the closest multiplier from 1 (the time-shift mode): %.3e; tape held %.1f MiB", shift, tape_bytes / 2**20)
        out.mkdir(parents=True, exist_ok=True)
        res_d = {"period_steps": n, "period_exact": exact, "multipliers": lam, "residuals": res, "shift_distance": shift, "tape_bytes": tape_bytes}
        np.savez(out / "floquet.npz", **res_d)
        return res_d
    finally:
        fs.th.release_device()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    args, opts = [], {"--transient": 30000, "--k": 8, "--blocks": 6}
    it = iter(sys.argv[1:])
    for a in it:
        if a in opts:
            opts[a] = int(next(it))
        else:
            args.append(a)
    main(Path(args[0]) if args else Path.cwd() / "data_output", Path(args[1]) if len(args) > 1 else None, transient=opts["--transient"], k=opts["--k"],
         blocks=opts["--blocks"])
