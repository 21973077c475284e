"""POD and DMD of the cylinder flow at Re = 100 from state snapshots kept on the device (``FlowSolver.record_snapshots``).

1. Nonlinear run from the usual perturbation of the base flow until the limit cycle is reached, then ``n_snap`` snapshots every
   ``every`` steps: ``flu.pod`` of the centred snapshots in the energy inner product -- singular values, energy fractions, and the
   leading modes (which cross to the host only because this script writes them).
2. Linearised run (``is_eq_nonlinear=False``) past its transient, snapshots likewise: ``flu.dmd`` with two modes; the leading pair
   ``lam_bdf2`` is printed next to the leading eigenvalue of the operator pencil (``flu.get_mat_vp``).

The snapshots are gathered by a launch of the step itself; the runs are ``FlowSolver.run`` calls with no synchronisation in between.

    python -m flowcontrol_amd.examples.cylinder.compute_pod_dmd [out_dir]

This script has not been run on a GPU yet: the step counts below (transients, window lengths) are estimates from the growth rate
0.13 and the shedding period of about 8 time units, not tuned values; the DMD half is what tests/test_modal_gpu.py runs.
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.flowsolverparameters import ParamIC
from flowcontrol_amd.operatorgetter import OperatorGetter

logger = logging.getLogger(__name__)


def _solver(out: Path, linear: bool, UP0=None):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.params_solver.is_eq_nonlinear = not linear
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    if UP0 is None:
        fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
        fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    else:
        fs._assign_steady_state(*UP0.split())
    fs.initialize_time_stepping(ic=None)
    return fs


def pod_of_the_limit_cycle(out: Path, transient: int = 30000, n_snap: int = 128, every: int = 25, n_modes: int = 6, fs=None) -> dict:
    own = fs is None
    fs = fs or _solver(out, linear=False)
    try:
        bank = fs.record_snapshots(n_snap, every=every, first=transient)
        fs.run(transient + n_snap * every, np.zeros(2))
        res = flu.pod(bank, r=n_modes, center=True, weight="energy", modes=True)
        logger.info("POD of %d snapshots (every %d steps): sigma = %s", bank.count, every, np.array2string(res.sigma[:10], precision=4))
        logger.info("energy fractions: %s (pairs of equal energy are the travelling shedding modes)", np.array2string(res.energy[:10], precision=4))
        out.mkdir(parents=True, exist_ok=True)
        np.savez(out / "pod_modes.npz", sigma=res.sigma, energy=res.energy, modes=res.modes, mean=res.mean, V=res.V)
        bank.close()
        return {"sigma": res.sigma, "energy": res.energy, "UP0": fs.fields.UP0}
    finally:
        if own:
            fs.th.release_device()


def dmd_of_the_linear_flow(out: Path, transient: int = 6000, n_snap: int = 100, every: int = 20, UP0=None) -> dict:
    fs = _solver(out, linear=True, UP0=UP0)
    try:
        bank = fs.record_snapshots(n_snap, every=every, first=transient)
        fs.run(transient + n_snap * every, np.zeros(2))
        res = flu.dmd(bank, r=2, dt=fs.params_time.dt, weight="energy")
        bank.close()
        A, E, _, _ = OperatorGetter(fs).get_all()
        valp, _ = flu.get_mat_vp(A, E, n=2, target=0.13 + 0.77j, tol=1e-10, flowsolver=fs)
        lead = valp[0]  # (nearest the target first)
        lam2 = res.lam_bdf2[np.argmax(res.lam_bdf2.imag)]
        lam = res.lam[np.argmax(res.lam.imag)]
        logger.info("DMD (r = 2) of %d snapshots every %d steps: mu = %s", n_snap, every, res.mu)
        logger.info("leading pair: lam_bdf2 = %.7f%+.7fi, log(mu) / (every dt) = %.7f%+.7fi, get_mat_vp = %.7f%+.7fi (distance %.3e)",
                    lam2.real, lam2.imag, lam.real, lam.imag, lead.real, lead.imag, abs(lam2 - lead))
        return {"mu": res.mu, "lam_bdf2": lam2, "lam": lam, "get_mat_vp": lead}
    finally:
        fs.th.release_device()


def main(out: Path) -> dict:
    p = pod_of_the_limit_cycle(out)
    d = dmd_of_the_linear_flow(out, UP0=p.pop("UP0"))
    return {**p, **d}


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path.cwd() / "data_output")
