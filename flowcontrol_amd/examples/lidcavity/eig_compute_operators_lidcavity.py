"""Operators A and E of the lid-driven cavity linearised about its base flow — the reference's
``src/examples/lidcavity/eig_compute_operators_lidcavity.py`` (Re = 8000, just above the supercritical Hopf bifurcation near
Re ≈ 7 700).  The base flow comes from the continuation in Re of ``compute_steady_state_increasing_Re`` (its files under
``<out>/steady`` are reused when they exist); the two matrices go to ``<out>/operators/A.npz`` and ``E.npz``, where
``eig_compute_lidcavity`` reads them.

    python -m flowcontrol_amd.examples.lidcavity.eig_compute_operators_lidcavity [out_dir]
"""

from __future__ import annotations

import logging
import sys
from pathlib import Path

import scipy.sparse as sp

from flowcontrol_amd import io
from flowcontrol_amd.examples.lidcavity.compute_steady_state_increasing_Re import RE_LIST, Re_final, continuation
from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.operatorgetter import OperatorGetter

logger = logging.getLogger(__name__)


def main(path_out: Path | None = None, Re: float = Re_final, meshpath=None) -> tuple[sp.csr_matrix, sp.csr_matrix]:
    out = Path(path_out) if path_out else Path(__file__).parent / "data_output"
    files = (out / "steady" / f"U0_Re={Re}.xdmf", out / "steady" / f"P0_Re={Re}.xdmf")
    if not all(f.exists() for f in files):
        logger.info("no base flow at Re = %s under %s: continuation in Re", Re, out / "steady")
        continuation([r for r in RE_LIST if r < Re] + [Re], path_out=out, meshpath=meshpath)
    fs = LidCavityFlowSolver.make_default(Re=Re, path_out=out, meshpath=meshpath)
    try:
        U00, P00 = Function(fs.V), Function(fs.P)
        io.read_xdmf(files[0], U00, "U0")
        io.read_xdmf(files[1], P00, "P0")
        # one Newton pass from the stored pair: the base flow of THIS solver, to its own tolerance
        fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0], initial_guess=fs.merge(U00, P00))
        opget = OperatorGetter(fs)
        A = sp.csr_matrix(opget.get_A(UP0=fs.fields.UP0, autodiff=True))
        E = sp.csr_matrix(opget.get_mass_matrix())
    finally:
        fs.th.release_device()
    (out / "operators").mkdir(parents=True, exist_ok=True)
    sp.save_npz(out / "operators" / "A.npz", A)
    sp.save_npz(out / "operators" / "E.npz", E)
    logger.info("A, E of order %d (%d / %d nonzeros) -> %s", A.shape[0], A.nnz, E.nnz, out / "operators")
    return A, E


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else None)
