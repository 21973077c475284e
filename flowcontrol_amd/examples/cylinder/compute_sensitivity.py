"""Structural sensitivity and resolvent gains of the linearised cylinder flow at Re = 100: the leading right mode u and left
(adjoint) mode u+ of A x = lambda E x, the wavemaker field |u+| |u| / |u+^H E u| (Giannetti & Luchini 2007) at the P2 nodes, and the
three largest resolvent gains over a short frequency grid.  Both modes come from ONE factorisation of A - target E on the device
(``flu.get_mat_vp(..., left=True)``: the left solve runs on the transposed factor values of the same elimination), every frequency
of the gain curve from one factorisation of i w E - A (``flu.resolvent_gains``).  Written to ``sensitivity.npz``.

    python -m flowcontrol_amd.examples.cylinder.compute_sensitivity [out_dir]
"""
import logging
import sys
import time
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.operatorgetter import OperatorGetter

logger = logging.getLogger(__name__)


def wavemaker(vecp: np.ndarray, vecl: np.ndarray, E, nn: int) -> np.ndarray:
    """|u+|(x) |u|(x) / |u+^H E u| at the nn velocity nodes (W layout: u_x [nn], u_y [nn], p)."""
    mag = lambda v: np.sqrt(np.abs(v[:nn]) ** 2 + np.abs(v[nn : 2 * nn]) ** 2)  # noqa: E731
    return mag(vecl) * mag(vecp) / abs(np.vdot(vecl, E @ vecp))


def main(out: Path, target: complex = 0.1 + 0.8j, ww=None, ngains: int = 3) -> dict:
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
    fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    A, E, _, _ = OperatorGetter(fs).get_all()
    ww = np.linspace(0.4, 1.2, 9) if ww is None else np.atleast_1d(np.asarray(ww, dtype=float))
    t0 = time.time()
    valp, vecp, vecl = flu.get_mat_vp(A, E, n=1, target=target, tol=1e-9, flowsolver=fs, left=True)
    logger.info("leading eigenvalue %s, right and left mode in %.2fs", np.array2string(valp, precision=6), time.time() - t0)
    nn = fs.th.nn
    field = wavemaker(vecp[:, 0], vecl[:, 0], E, nn)
    peak = int(np.argmax(field))
    logger.info("wavemaker: maximum %.4g at (%.3f, %.3f)", field[peak], *fs.th.node_coords[peak])
    t0 = time.time()
    gains = flu.resolvent_gains(A, E, ww, n=ngains, tol=1e-8, flowsolver=fs)  # (1e-10 is out of reach for a cluster of close gains)
    logger.info("resolvent gains on %d frequencies in %.2fs: largest %.4g at w = %.3f", ww.size, time.time() - t0, gains[0].max(),
                ww[int(np.argmax(gains[0]))])
    res = {"eigenvalue": valp[0], "right_mode": vecp[:, 0], "left_mode": vecl[:, 0], "wavemaker": field, "node_coords": fs.th.node_coords,
           "ww": ww, "gains": gains}
    out.mkdir(parents=True, exist_ok=True)
    np.savez(out / "sensitivity.npz", **res)
    return res


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path.cwd())
