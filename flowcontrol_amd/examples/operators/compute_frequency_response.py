"""Frequency response H(jw) = C (jwE - A)^-1 B of the cylinder flow — the reference's
``src/examples/operators/compute_frequency_response.py``: base flow, ``OperatorGetter.get_all()``, 50 log-spaced frequencies in
[1e-2, 1e2], one file with the whole H and one per (output, input) pair (``save_Hw``; ``.npz`` here instead of ``.mat``), Bode
plots when matplotlib imports.  Every frequency is one factorisation of jwE - A on the device (``flowcontrol_amd.linalg``).

    python -m flowcontrol_amd.examples.operators.compute_frequency_response [out_dir]
"""
import logging
import sys
from pathlib import Path

import numpy as np

from flowcontrol_amd import utils as flu
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.operatorgetter import OperatorGetter

logger = logging.getLogger(__name__)


def save_Hw(H, ww, save_dir: Path, save_suffix: str = "", input_labels=None, output_labels=None) -> None:
    """The whole H [ny, nu, nw] and one file per (output, input) pair, as the reference's ``utils/io.py::save_Hw``."""
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    ny, nu, _ = H.shape
    input_labels = input_labels or [f"u{i}" for i in range(nu)]
    output_labels = output_labels or [f"y{i}" for i in range(ny)]
    np.savez(save_dir / f"Hw{save_suffix}.npz", H=H, ww=ww, input_labels=input_labels, output_labels=output_labels)
    for i in range(ny):
        for j in range(nu):
            np.savez(save_dir / f"Hw_{output_labels[i]}_{input_labels[j]}{save_suffix}.npz", H=H[i, j], ww=ww)


def plot_Hw(H, ww, save_dir: Path, input_labels=None, output_labels=None) -> None:
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logger.info("matplotlib not available: no Bode plots")
        return
    ny, nu, _ = H.shape
    input_labels = input_labels or [f"u{i}" for i in range(nu)]
    output_labels = output_labels or [f"y{i}" for i in range(ny)]
    for i in range(ny):
        for j in range(nu):
            fig, ax = plt.subplots(2, 1, sharex=True)
            ax[0].loglog(ww, np.abs(H[i, j]))
            ax[1].semilogx(ww, np.unwrap(np.angle(H[i, j])) * 180 / np.pi)
            ax[0].set_ylabel("|H|")
            ax[1].set_ylabel("phase [deg]")
            ax[1].set_xlabel("w")
            fig.savefig(Path(save_dir) / f"bode_{output_labels[i]}_{input_labels[j]}.png")
            plt.close(fig)


def main(out: Path) -> None:
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out / "cylinder" / "data_output")
    fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
    fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    A, E, B, C = OperatorGetter(fs).get_all()
    ww = np.logspace(-2, 2, 50)
    H, ww = flu.get_frequency_response_parallel(A, B, C, E, ww, verbose=True, n_jobs=2, flowsolver=fs)
    save_dir = out / "cylinder" / "frequency_response"
    labels = dict(input_labels=["up", "lo"], output_labels=["fb", "perf1", "perf2"])
    save_Hw(H, ww, save_dir=save_dir, **labels)
    plot_Hw(H, ww, save_dir=save_dir, **labels)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else Path.cwd())
