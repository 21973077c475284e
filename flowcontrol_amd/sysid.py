"""Closed-loop identification: the plant's frequency response measured in the time domain, with a stabilising controller in the loop
and a multisine added at the plant input (the experiment the reference keeps ``signal.multisine`` / ``multisine_MP`` and
``save_Hw`` / ``plot_Hw`` for; an unstable flow such as the cylinder at Re = 100 cannot be measured in open loop).

The M phase realisations of the multisine are the M columns of one batch (``BatchedFlowSolver``): with ``on_device=True`` the
controllers, the excitation and the plant advance on the device (``fc_run_closed_loop_batch`` with ``fc_set_loop_signals``) and the
host sees the series once, at the end.  The estimate is the direct one, ``G = Y / U`` with ``U`` the input the plant actually saw
(controller output + excitation): exact for periodic data without noise, whatever the controller is.
"""

from __future__ import annotations

import numpy as np

from . import signal as _signal


def frf_from_series(y, u, w, N: int, P_skip: int = 1, bins=None) -> dict:
    """Frequency response from periodic series: ``y`` (M, n, n_out) outputs, ``u`` (M, n) the input the plant saw, ``w`` (M, n) the
    excitation that was added to the loop, all of period ``N`` over ``n = P N`` steps (a leading axis of one realisation may be left
    out).  The first ``P_skip`` periods are dropped, the rest is averaged over its whole periods and transformed (DFT over N points).

    ``bins``: the harmonics of ``1 / N`` to report; ``None`` — those that ``w`` excites in every realisation (DC and the Nyquist bin
    are never taken).  Returns ``{"bins", "G" (n_bins, n_out): mean over the realisations of Y_m / U_m, "G_std": their spread
    (sample standard deviation of the complex values; zeros for M = 1), "Y" (M, n_bins, n_out), "U" (M, n_bins)}``."""
    y, u, w = np.asarray(y, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if u.ndim == 1:
        y, u, w = y[None], u[None], w[None]
    if y.ndim == 2:
        y = y[:, :, None]
    M, n = u.shape
    N, P_skip = int(N), int(P_skip)
    if y.shape[:2] != (M, n) or w.shape != (M, n):
        raise ValueError(f"y {y.shape}, u {u.shape} and w {w.shape} do not describe the same realisations and steps")
    if N < 2 or n % N:
        raise ValueError(f"the series hold {n} steps: not a whole number of periods of {N}")
    P = n // N
    if not 0 <= P_skip < P:
        raise ValueError(f"P_skip = {P_skip} leaves none of the {P} periods")

    def spectrum(a):  # (M, n, ...) -> (M, N // 2 + 1, ...): one period, averaged over the kept ones
        kept = a[:, P_skip * N :].reshape(M, P - P_skip, N, *a.shape[2:])
        return np.fft.rfft(kept.mean(axis=1), axis=1) / N

    Yf, Uf = spectrum(y), spectrum(u)
    if bins is None:
        Wa = np.abs(spectrum(w))
        inner = np.arange(1, (N + 1) // 2)  # without DC, without the Nyquist bin of an even N
        bins = inner[np.all(Wa[:, inner] > 1e-6 * Wa.max(), axis=0)] if Wa.max() > 0.0 else inner[:0]
    bins = np.asarray(bins, dtype=np.int64).reshape(-1)
    if bins.size and (bins.min() < 1 or bins.max() >= (N + 1) // 2):
        raise ValueError("bins must lie strictly between DC and the Nyquist bin")
    Y, U = Yf[:, bins], Uf[:, bins]
    Gm = Y / U[:, :, None]
    G = Gm.mean(axis=0)
    G_std = np.sqrt((np.abs(Gm - G) ** 2).sum(axis=0) / (M - 1)) if M > 1 else np.zeros(G.shape)
    return {"bins": bins, "G": G, "G_std": G_std, "Y": Y, "U": U}


def closed_loop_frequency_response(fs, controller, *, N: int, P: int, M: int, amplitude: float, fmin: float, fmax: float, P_skip: int = 1,
                                   direction=None, feedback=None, skip_even: bool = False, seed: int = 0, on_device: bool = True) -> dict:
    """The frequency response of ``fs``'s plant from actuators (along ``direction``; default: ones) to sensors, measured with
    ``controller`` (an LTI ``Controller``) closing the loop in each of M simultaneous runs (``BatchedFlowSolver(fs, M)``, the solver's
    own initial condition in every column) and ``amplitude`` times a multisine of period ``N`` steps added at the plant input for
    ``P`` periods.  The M realisations come from :func:`flowcontrol_amd.signal.multisine` (``fmin``, ``fmax`` as fractions of the
    Nyquist frequency, ``skip_even``: odd harmonics only), drawn with ``np.random.seed(seed)``; the global random state is put back.

    ``feedback``: ``None`` (``yc = -y_meas[0]``) or ``(G, g0)``.  ``on_device=False`` steps the same experiment with the controllers on
    the host (one round trip per step).  Returns :func:`frf_from_series`'s dictionary — the first ``P_skip`` periods dropped, the
    excited harmonics only — with ``"ww"``, the frequencies of ``bins`` in rad per time unit."""
    from .batch import BatchedFlowSolver
    from .controller import Controller

    if not isinstance(controller, Controller):
        raise TypeError("closed_loop_frequency_response closes the loop with an LTI Controller")
    if callable(feedback):
        raise TypeError("give feedback as None or as a pair (G, g0)")
    N, P, M = int(N), int(P), int(M)
    dt = fs.params_time.dt
    n_act = fs.params_control.actuator_number
    d = np.ones(n_act) if direction is None else np.asarray(direction, dtype=np.float64).reshape(n_act)
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        ms = _signal.multisine_MP(M, P, unwrap=False, N=N, Fs=1.0 / dt, fmin=fmin, fmax=fmax, skip_even=skip_even)  # (M, N P)
    finally:
        np.random.set_state(state)
    w = amplitude * ms
    n = N * P
    w_u = np.ascontiguousarray(w.T[:, :, None] * d)  # (n, M, n_act)
    Ks = [Controller(controller.A, controller.B, controller.C, controller.D, x0=np.array(controller.x, dtype=np.float64)) for _ in range(M)]
    bfs = BatchedFlowSolver(fs, M)
    try:
        bfs.initialize_time_stepping(ics=None)
        if on_device:
            out = bfs.run_closed_loop(n, Ks, feedback, w_u=w_u)
            if out is None:
                raise RuntimeError("the residual monitor stopped the identification run")
            y, u, _ = out
        else:
            y, u = _host_loop(fs, bfs, Ks, feedback, w_u)
        if np.any(bfs.diverged):
            raise RuntimeError(f"identification runs {np.flatnonzero(bfs.diverged).tolist()} became non-finite: lower the amplitude")
    finally:
        bfs.close()
    u_d = u @ d / float(d @ d)  # (n, M): the applied input along the direction
    res = frf_from_series(y.transpose(1, 0, 2), u_d.T, w, N, P_skip)
    res["ww"] = 2.0 * np.pi * res["bins"] / (N * dt)
    return res


def _host_loop(fs, bfs, Ks, feedback, w_u):
    """The experiment with ``Controller.step`` on the host between two batched steps, in the device loop's order of operations."""
    n_sens = len(fs.params_control.sensor_list)
    n_act = fs.params_control.actuator_number
    if feedback is None:
        G, g0 = np.zeros((1, n_sens)), np.zeros(1)
        G[0, 0] = -1.0
    else:
        G, g0 = np.atleast_2d(np.asarray(feedback[0], dtype=np.float64)), np.atleast_1d(np.asarray(feedback[1], dtype=np.float64))
    dt = fs.params_time.dt
    ys, us = [], []
    for s in range(w_u.shape[0]):
        u = np.zeros((len(Ks), n_act))
        for i, K in enumerate(Ks):
            if bfs.diverged[i]:
                continue
            cmd = np.atleast_1d(np.asarray(K.step(y=G @ bfs.y_meas[i] + g0, dt=dt), dtype=np.float64)).ravel()
            u[i] = (cmd if cmd.size == n_act else cmd[0]) + w_u[s, i]
        y = bfs.step(u)
        if y is None:
            raise RuntimeError("the residual monitor stopped the identification run")
        ys.append(np.array(y, dtype=np.float64)), us.append(u)
    return np.stack(ys), np.stack(us)


__all__ = ["frf_from_series", "closed_loop_frequency_response"]
