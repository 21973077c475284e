"""Closed-loop identification of the cylinder flow at Re = 100: the plant's frequency response measured in the time domain and laid
next to the analytic one.

The flow is unstable, so its input-output behaviour can only be measured with a stabilising controller in the loop: the shipped
``Kopt_reduced13.mat`` feeds the first probe back to both actuators and a small multisine is added at the plant input.  M = 8 phase
realisations run as the 8 columns of one batch with controllers, excitation and plant on the device
(``sysid.closed_loop_frequency_response``); the perturbation equations are the linearised ones (``is_eq_nonlinear=False``), so the
measured response is that of the operators ``OperatorGetter`` returns, H(jw) = C (jwE - A)^-1 B, up to the time discretisation.

    python -m flowcontrol_amd.examples.cylinder.identify_closed_loop [N] [P] [P_skip]
"""

import sys
import time
from pathlib import Path

import numpy as np

from flowcontrol_amd import linalg, sysid
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.flowsolverparameters import ParamIC
from flowcontrol_amd.operatorgetter import OperatorGetter

CONTROLLER = Path(__file__).resolve().parent / "data_input" / "Kopt_reduced13.mat"
M = 8
AMPLITUDE = 1e-3
W_BAND = (0.5, 10.0)  # rad per time unit: around the shedding frequency (about 1 rad) and a decade above


def main(N: int = 2000, P: int = 4, P_skip: int = 2, path_out: Path | None = None):
    out = Path(path_out) if path_out else Path.cwd() / "data_output"
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out, num_steps=N * P)
    fs.params_solver.is_eq_nonlinear = False
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.0)  # from rest: the response is the excitation's alone
    fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
    fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
    dt = fs.params_time.dt
    nyquist = np.pi / dt
    K = Controller.from_file(file=CONTROLLER, x0=None)
    t0 = time.perf_counter()
    res = sysid.closed_loop_frequency_response(fs, K, N=N, P=P, M=M, amplitude=AMPLITUDE, fmin=W_BAND[0] / nyquist, fmax=W_BAND[1] / nyquist,
                                               P_skip=P_skip)
    seconds = time.perf_counter() - t0
    print(f"{M} realisations x {N * P} closed-loop steps on the device: {seconds:.1f} s = {M * N * P / seconds:.0f} simulated steps/s")
    ww = res["ww"]
    A, E, B, C = OperatorGetter(fs).get_all()
    H, _ = linalg.get_frequency_response_sequential(A, B, C, E, ww, verbose=False, flowsolver=fs)
    H_dir = H.sum(axis=1).T  # both actuators together (the direction of the excitation): (n_w, n_sens)
    rel = np.abs(res["G"] - H_dir) / np.abs(H_dir)
    print("     w      |G| measured   |H| analytic   rel. deviation   spread / |G|   (first sensor)")
    for i in range(ww.size):
        print(f"{ww[i]:8.4f}   {abs(res['G'][i, 0]):12.5e}   {abs(H_dir[i, 0]):12.5e}   {rel[i, 0]:12.3e}   {res['G_std'][i, 0] / abs(res['G'][i, 0]):12.3e}")
    worst = np.unravel_index(np.argmax(rel), rel.shape)
    print(f"largest relative deviation over the band, all sensors: {rel.max():.3e} (w = {ww[worst[0]]:.4f}, sensor {worst[1] + 1}); "
          f"first sensor: {rel[:, 0].max():.3e}; w dt at the band's end: {ww[-1] * dt:.3f}")
    fs.th.release_device()
    return res, H_dir


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:4]]
    main(*args)
