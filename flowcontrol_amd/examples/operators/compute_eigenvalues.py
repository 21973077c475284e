"""Shift-invert eigenvalues of the linearised cylinder flow — the reference's ``src/examples/operators/compute_eigenvalues.py``
(SLEPc Krylov-Schur with MUMPS, ``utils/eig``): ``neig_at_target`` eigenpairs of A x = lambda E x near each target, gathered,
saved (``eig.npz``) and plotted when matplotlib imports.  Here every target is one factorisation of A - target E on the device and a
Krylov-Schur iteration whose basis stays there (``flowcontrol_amd.linalg.get_mat_vp``).  Expected at Re = 100 (the reference's
comment): one unstable pair, 0.132643 +- 0.770015j.

    python -m flowcontrol_amd.examples.operators.compute_eigenvalues [out_dir]
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


def main(out: Path, targets=(0.1 + 0.8j, 0.0, 1j, 2j), neig_at_target: int = 2) -> np.ndarray:
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
    fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    A, E, _, _ = OperatorGetter(fs).get_all()
    lam_all, vec_all = [], []
    for target in targets:
        t0 = time.time()
        valp, vecp = flu.get_mat_vp_slepc(A, E, n=neig_at_target, target=target, tol=1e-9, flowsolver=fs)
        logger.info("target %s: %s (%.2fs)", target, np.array2string(valp, precision=6), time.time() - t0)
        lam_all.append(valp)
        vec_all.append(vecp)
    lam = np.concatenate(lam_all)
    out.mkdir(parents=True, exist_ok=True)
    np.savez(out / "eig.npz", eigenvalues=lam, eigenvectors=np.concatenate(vec_all, axis=1), targets=np.asarray(targets))
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        fig, ax = plt.subplots()
        ax.scatter(lam.real, lam.imag, marker="+")
        ax.axvline(0.0, color="k", lw=0.5)
        ax.set_xlabel("Re(lambda)")
        ax.set_ylabel("Im(lambda)")
        fig.savefig(out / "eig.png")
        plt.close(fig)
    except ImportError:
        logger.info("matplotlib not available: no spectrum plot")
    return lam


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path.cwd())
