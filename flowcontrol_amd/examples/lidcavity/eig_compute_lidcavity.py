"""Eigenvalues of the lid-driven cavity near the Hopf bifurcation — the reference's ``src/examples/lidcavity/eig_compute_lidcavity.py``
(SLEPc Krylov-Schur with a MUMPS shift-invert): three eigenvalues of A x = lambda E x at each of the targets 0, 1j, 2j, 3j, from
the matrices ``eig_compute_operators_lidcavity`` wrote.  Here the four targets share ONE symbolic phase of the device's shifted
solver (one :class:`~flowcontrol_amd.linalg.ShiftedOperator`, refactorised per target); the flow is enclosed, so one pressure dof
is pinned inside the shifted factorisation (``pressure_pin="auto"``), which leaves the finite eigenvalues where they are, and the
device's GMRES stands by for a solve whose refinement stalls (``krylov=True``).

    python -m flowcontrol_amd.examples.lidcavity.eig_compute_lidcavity [out_dir]
"""

from __future__ import annotations

import logging
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

from flowcontrol_amd import linalg
from flowcontrol_amd.examples.lidcavity.compute_steady_state_increasing_Re import Re_final
from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver

logger = logging.getLogger(__name__)

TARGETS = (0j, 1j, 2j, 3j)
NEIG = 3


def compute(fs, A, E, targets=TARGETS, neig: int = NEIG, tol: float = 1e-12):
    """(LAMBDA [len(targets) * neig], V [N, len(targets) * neig], stats per target) on the device handle of ``fs``."""
    op = linalg.ShiftedOperator(fs, A, E, pressure_pin="auto", krylov=True)
    lam_all, vec_all, stats = [], [], []
    rescues = 0
    try:
        for target in targets:
            t0 = time.perf_counter()
            lam, vec = linalg.get_mat_vp(A, E, n=neig, target=target, tol=tol, operator=op)
            now = op.krylov_info()["rescues"]  # (Arnoldi steps included: the library counts them)
            stats.append({"target": complex(target), "seconds": time.perf_counter() - t0, "refactor_ms": op.info()["refactor_ms"],
                          "rescued": now > rescues})
            rescues = now
            if np.any(lam.real > 0):
                logger.warning("eigenvalue with positive real part at target %s: %s", target, lam[lam.real > 0])
            lam_all.append(lam)
            vec_all.append(vec)
    finally:
        op.release()
    return np.concatenate(lam_all), np.concatenate(vec_all, axis=1), stats


def plot_eig(LAMBDA, path: Path) -> None:
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logger.info("matplotlib not available: no spectrum plot")
        return
    fig, ax = plt.subplots()
    ax.plot(LAMBDA.real, LAMBDA.imag, "g.", LAMBDA.real, -LAMBDA.imag, "r.")
    ax.axhline(0.0, color="k", ls="--")
    ax.axvline(0.0, color="k", ls="--")
    ax.grid(True)
    ax.set_title("Eigenvalues")
    fig.savefig(path)
    plt.close(fig)


def main(path_out: Path | None = None, meshpath=None):
    out = Path(path_out) if path_out else Path(__file__).parent / "data_output"
    ops = out / "operators"
    A, E = sp.load_npz(ops / "A.npz").tocsr(), sp.load_npz(ops / "E.npz").tocsr()
    # the solver lends its device handle (the CSR pattern A and E live on); its own time stepping is not used
    fs = LidCavityFlowSolver.make_default(Re=Re_final, path_out=out, meshpath=meshpath)
    t0 = time.perf_counter()
    try:
        LAMBDA, V, stats = compute(fs, A, E)
    finally:
        fs.th.release_device()
    for s in stats:
        print(f"target {s['target']}: {s['seconds']:.2f} s (numeric factorisation {s['refactor_ms']:.1f} ms"
              f"{', GMRES rescue used' if s['rescued'] else ''})")
    for i, lam in enumerate(LAMBDA):
        print(f"eigenvalue {i + 1:2d}: {lam.real:+.8f} {lam.imag:+.8f}j")
    np.savez_compressed(ops / "eigenValues", LAMBDA)
    np.savez_compressed(ops / "eigenVectors", V)
    np.savetxt(ops / "eigenValues.txt", LAMBDA, delimiter=",")
    plot_eig(LAMBDA, ops / "eigenValues.png")
    print(f"{LAMBDA.size} eigenvalues in {time.perf_counter() - t0:.1f} s")
    return LAMBDA, V


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else None)
