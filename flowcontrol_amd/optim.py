"""Controller-optimisation helpers around the time-stepping path (the reference's ``src/utils/optim.py``), plus what that file
cannot have: the candidates of one optimiser iteration evaluated TOGETHER.

The reference evaluates a cost function point by point (``fun_array``: one closed-loop ``FlowSolver`` simulation per candidate
controller, ``optim.py:48-68``).  All candidates of an iteration share the flow solver's operators — only the controller differs
— so here up to 32 of them run as one ``BatchedFlowSolver`` (``closed_loop_costs``): the factors are read once per time step for
all candidates.  The scalar helpers keep the reference's names, arguments and file formats (``J_costfun.csv``,
``J_costfun_cummin.csv``, ``timeseries/timeseries_iter_XXXX[_DIVERGED].csv``).
"""

from __future__ import annotations

import logging
from collections.abc import Callable, Sequence
from pathlib import Path

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)


# ── scalar helpers (reference optim.py) ──────────────────────────────────────────────────────────────────────────────
def fun_array(x: np.ndarray, fun: Callable[..., float], **kwargs) -> np.ndarray:
    """``fun`` on every row of ``x`` (n_points, dim) → costs (n_points, 1), one evaluation after the other (optim.py:48-68)."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    return np.array([[float(fun(row, **kwargs))] for row in x])


def cummin(y: np.ndarray, return_index: bool = True):
    """Running minimum of a column vector (n, 1) and, optionally, the index where each running minimum was first reached
    (optim.py:112-137)."""
    y = np.asarray(y, dtype=float).reshape(-1, 1)
    best = np.minimum.accumulate(y, axis=0)
    if not return_index:
        return best
    # first position (up to step i) whose value equals the running minimum of step i; a NaN cost (a run that was stopped early)
    # propagates through the running minimum and matches nothing: index 0 then, as the reference's argmax over an all-False row gives
    hit = np.isclose(best, y.T) & np.tri(y.shape[0], dtype=bool)
    return best, hit.argmax(1)


def write_results(x_data, y_data, optim_path, verbose: bool = True) -> None:
    """All evaluations (``J_costfun.csv``) and the best-so-far sequence (``J_costfun_cummin.csv``), columns J, x0, x1, …
    (optim.py:140-174)."""
    optim_path = Path(optim_path)
    X = np.atleast_2d(np.asarray(x_data, dtype=float))
    J = np.asarray(y_data, dtype=float).reshape(-1, 1)
    cols = ["J"] + [f"x{i}" for i in range(X.shape[1])]
    if verbose:
        logger.info("Logging results to: %s", optim_path)
    pd.DataFrame(np.hstack([J, X]), columns=cols).to_csv(optim_path / "J_costfun.csv", index=False)
    best, idx = cummin(J)
    pd.DataFrame(np.hstack([best, X[idx]]), columns=cols).to_csv(optim_path / "J_costfun_cummin.csv", index=False)


def sobol_sample(ndim: int, npt: int, xlimits=None, skip: int = 1000, seed: int | None = None) -> np.ndarray:
    """``npt`` points of the (unscrambled) Sobol sequence in ``ndim`` dimensions after skipping ``skip`` points (+ a random offset
    when ``seed`` is given), scaled into ``xlimits`` (ndim, 2) or (2, ndim) (optim.py:177-224)."""
    from scipy.stats.qmc import Sobol

    engine = Sobol(d=ndim, scramble=False)
    n_skip = int(skip) + (int(np.random.default_rng(seed).integers(10000)) if seed is not None else 0)
    if n_skip > 0:
        engine.fast_forward(n_skip)
    pts = engine.random(npt)
    if xlimits is not None:
        lim = np.asarray(xlimits, dtype=float)
        if lim.shape == (2, ndim):  # rows = lower / upper bounds (also how the reference reads a square array)
            lim = lim.T
        if lim.shape != (ndim, 2):
            raise ValueError(f"xlimits has wrong shape {lim.shape}, expected ({ndim}, 2)")
        pts = lim[:, 0] + pts * (lim[:, 1] - lim[:, 0])
    return pts


def compute_signal_cost(signal, Tnorm: float, criterion: str, scaling: Callable | None = None) -> float:
    """Time-averaged (``"integral"``: Σ scaling(signal) · Tnorm) or final (``"terminal"``) cost of a time series; Tnorm =
    dt / (t − Tc) (optim.py:230-272)."""
    if criterion not in ("integral", "terminal"):
        raise ValueError(f"Unknown criterion {criterion!r}: expected 'integral' or 'terminal'.")
    f = scaling if scaling is not None else (lambda v: v)
    s = pd.Series(signal) if not isinstance(signal, pd.Series) else signal
    return float(np.sum(f(s)) * Tnorm) if criterion == "integral" else float(f(s.iloc[-1]))


def compute_control_cost(u_ctrl, Tnorm: float) -> float:
    """Time-normalised control effort Σ_t Σ_channels u² · Tnorm (optim.py:275-291)."""
    return float(np.nansum(np.asarray(u_ctrl, dtype=float) ** 2) * Tnorm)


def write_optim_csv(timeseries: pd.DataFrame, savedir, diverged: bool, iteration: int) -> None:
    """``<savedir>/timeseries/timeseries_iter_XXXX[_DIVERGED].csv`` (optim.py:294-318)."""
    d = Path(savedir) / "timeseries"
    d.mkdir(parents=True, exist_ok=True)
    timeseries.to_csv(d / f"timeseries_iter_{int(iteration):04d}{'_DIVERGED' if diverged else ''}.csv", index=False)


# ── the candidates of one iteration, together ────────────────────────────────────────────────────────────────────────
def closed_loop_costs(fs, controllers: Sequence, num_steps: int, u_penalty: float = 0.0, signal: str = "dE", criterion: str = "integral",
                      feedback: Callable | None = None, ics=None, Tc: float = 0.0, diverged_cost: float = np.inf, on_device: bool = False,
                      w_y=None, w_u=None, u_limits=None):
    """Cost J = xQx + u_penalty · uRu of every controller in ``controllers`` (≤ 32) for ``num_steps`` closed-loop steps of ``fs``'s case,
    all candidates advanced in lock step on one handle (``BatchedFlowSolver``).

    ``controllers[i].step(y=…, dt=…)`` is called once per time step with ``feedback(y_meas_i)`` (default: minus the first
    measurement, the reference's cylinder loop) and must return the actuator command(s) (a scalar is applied to every actuator).
    ``signal``: a column of the time series (``"dE"``: full-state energy, ``"y_meas_1"`` …).  Returns ``(J, timeseries)``:
    costs (k,) — ``diverged_cost`` for a run that became non-finite — and the k time-series DataFrames.

    ``on_device=True``: the controllers are advanced on the device between two steps (``BatchedFlowSolver.run_closed_loop``), so the
    host leaves the loop; every candidate must then be a ``Controller`` (LTI) and ``feedback`` ``None`` or a pair ``(G, g0)``
    (``yc = G @ y_meas + g0``) — a Python callable cannot run there and is refused.

    ``w_y`` (added to what the controllers see), ``w_u`` (added to what they command) and ``u_limits = (lo, hi)`` score the candidates
    against a reference or sensor noise, an input disturbance and limited actuators: ``u = min(max(cmd + w_u, lo), hi)``, the logged and
    penalised ``u`` being the clamped one.  One row set ``(num_steps, ·)`` is shared by all candidates, or ``(num_steps, k, ·)`` gives
    one per candidate; the limits are scalars, per actuator or ``(k, n_act)``.  Both settings of ``on_device`` take them."""
    from .batch import BatchedFlowSolver
    from .controller import loop_limits, loop_signal_rows_batch

    k = len(controllers)
    if on_device:
        from .controller import Controller

        if callable(feedback):
            raise TypeError("on_device=True: a Python callable cannot run on the device; give feedback as None or as a pair (G, g0)")
        for K in controllers:
            if not isinstance(K, Controller):
                raise TypeError(f"on_device=True: every candidate must be a Controller (LTI), got {type(K).__name__}")
    n_act = fs.params_control.actuator_number
    fb = feedback if (feedback is not None and not on_device) else (lambda y: -y[0])
    dt = fs.params_time.dt
    limits = loop_limits(u_limits, (k, n_act))
    if w_u is not None:
        w_u = loop_signal_rows_batch(w_u, num_steps, k, n_act, "w_u")
    if w_y is not None and not on_device:  # (on the device the bank knows the width of yc)
        w_y = np.asarray(w_y, dtype=np.float64)
        w_y = loop_signal_rows_batch(w_y, num_steps, k, 1 if w_y.ndim == 1 else w_y.shape[-1], "w_y")
    bfs = BatchedFlowSolver(fs, k)
    bfs.initialize_time_stepping(ics=ics)
    throw = fs.params_solver.throw_error
    fs.params_solver.throw_error = False  # a diverging candidate is a data point, not an error
    try:
        alive = True
        if on_device and bfs.run_closed_loop(num_steps, list(controllers), feedback, w_y=w_y, w_u=w_u, u_limits=limits) is None:  # a residual breach
            alive = False
        for s in range(0 if on_device else num_steps):
            u = np.zeros((k, n_act))
            for i, K in enumerate(controllers):
                if bfs.diverged[i]:
                    continue  # that run has ended (its measurements are NaN): no command
                yc = fb(bfs.y_meas[i])
                if w_y is not None:
                    yc = yc + (w_y[s, i] if np.ndim(yc) else w_y[s, i, 0])
                cmd = np.atleast_1d(np.asarray(K.step(y=yc, dt=dt), dtype=float)).ravel()
                u[i] = cmd if cmd.size == n_act else cmd[0]
                if w_u is not None:
                    u[i] = u[i] + w_u[s, i]
                if limits is not None:
                    u[i] = np.minimum(np.maximum(u[i], limits[0][i]), limits[1][i])
            if bfs.step(u) is None:  # a residual breach: the factors all candidates share are broken
                alive = False
                break
        series = [bfs.timeseries(i) for i in range(k)]
        if bfs.breached:  # the monitor's verdict on the LAST step arrives with the log: costs of a broken last step are not ranked
            alive = False
        J = np.empty(k)
        for i, ts in enumerate(series):
            if bool(bfs.diverged[i]):  # a diverging candidate ends there; the others run to the end
                J[i] = diverged_cost
                continue
            t_end = float(ts["time"].iloc[-1])
            Tnorm = dt / max(t_end - Tc, dt)
            ucols = [c for c in ts.columns if c.startswith("u_ctrl_")]
            J[i] = compute_signal_cost(ts[signal].dropna(), Tnorm, criterion) + u_penalty * compute_control_cost(ts[ucols], Tnorm)
        if not alive:  # stopped early: mark the finite runs as unevaluated rather than rank them
            J[~np.asarray(bfs.diverged, dtype=bool)] = np.nan
        return J, series
    finally:
        fs.params_solver.throw_error = throw
        bfs.close()


def fun_array_batched(x: np.ndarray, make_controller: Callable, fs, num_steps: int, batch: int = 32, on_device: bool = False, **kwargs) -> np.ndarray:
    """``fun_array`` for closed-loop costs: rows of ``x`` are controller parameters, ``make_controller(row)`` builds the controller;
    the points are evaluated ``batch`` at a time on one handle (``on_device``: as in :func:`closed_loop_costs`).  Returns costs (n_points, 1)."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    out = np.empty((x.shape[0], 1))
    for a in range(0, x.shape[0], batch):
        rows = x[a : a + batch]
        J, _ = closed_loop_costs(fs, [make_controller(r) for r in rows], num_steps, on_device=on_device, **kwargs)
        out[a : a + rows.shape[0], 0] = J
    return out


def energy_cost_weights(num_steps: int, dt: float, n_sens: int, n_act: int, criterion: str = "integral", u_penalty: float = 0.0, Tc: float = 0.0,
                        Tstart: float = 0.0):
    """The reference's cost ``J = compute_signal_cost(dE, Tnorm, criterion) + u_penalty * compute_control_cost(u, Tnorm)`` of a run of
    ``num_steps`` steps, written as the cost the adjoint marches differentiate, ``sum_m e_m dE_m + 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)``:
    returns ``(e (n,), Q, R, Tnorm, w0)``.  ``Tnorm = dt / max(t_end - Tc, dt)`` as in :func:`closed_loop_costs`;
    ``criterion="integral"``: ``e_m = Tnorm``, ``"terminal"``: ``e = (0, .., 0, 1)``; ``Q = 0``; ``R = 2 u_penalty Tnorm I``.  ``w0`` weights
    the energy of the initial row of the time series, which the integral sums too (a constant of the run: no gradient)."""
    if criterion not in ("integral", "terminal"):
        raise ValueError(f"Unknown criterion {criterion!r}: expected 'integral' or 'terminal'.")
    n = int(num_steps)
    t_end = Tstart + n * dt
    Tnorm = dt / max(t_end - Tc, dt)
    e = np.full(n, Tnorm) if criterion == "integral" else np.r_[np.zeros(n - 1), 1.0]
    w0 = Tnorm if criterion == "integral" else 0.0
    return e, np.zeros((n_sens, n_sens)), 2.0 * u_penalty * Tnorm * np.eye(n_act), Tnorm, w0


def closed_loop_cost_gradients(fs, controllers: Sequence, num_steps: int, Q=None, R=None, batch: int = 32, ics=None, signal: str | None = None,
                               criterion: str = "integral", u_penalty: float = 0.0, Tc: float = 0.0, checkpoint_every=None, **loop_kwargs):
    """``J_i = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` of every LTI ``Controller`` in ``controllers`` -- any number of candidates -- over
    ``num_steps`` closed-loop steps of ``fs``'s case, and the gradient of every cost with respect to its candidate's matrices:
    ``(J (n,), grads)``, ``grads[i]`` the dict of :func:`flowcontrol_amd.adjoint.closed_loop_gradient`.  The candidates run in chunks of
    at most ``batch`` (<= 32) on ONE ``BatchedFlowSolver`` with one reused ``AdjointRun``: one batched forward run and one batched
    backward march per chunk (``fc_run_adjoint_closed_loop_batch``); a last, shorter chunk is filled with repeats of its last candidate,
    whose results are dropped.  Every chunk starts from the same initial conditions ``ics`` (as in :func:`closed_loop_costs`: one per
    run of the batch, default the solver's own).  ``loop_kwargs``: ``feedback``, ``w_y``, ``w_u``, ``u_limits`` of
    ``BatchedFlowSolver.run_closed_loop``; a signal given per candidate is ``(num_steps, n, .)``, limits per candidate ``(n, n_act)``.

    ``signal="dE"`` differentiates the cost :func:`closed_loop_costs` ranks candidates by, the reference's
    ``J = Tnorm sum dE + u_penalty Tnorm sum |u|^2`` (``criterion``, ``u_penalty``, ``Tc`` as there; :func:`energy_cost_weights` maps them to
    the energy weights and ``R`` of the march; ``Q`` and ``R``, if given, are added on top).  ``J`` then equals what
    ``closed_loop_costs(..., on_device=True)`` returns for the same candidates, the share of the time series' initial row included -- for
    candidates whose runs stay finite.  Nothing is done here about a diverging candidate: :func:`closed_loop_costs` ends such a run and
    gives it ``diverged_cost``, whereas here its ``J`` and its gradients come back non-finite (check ``np.isfinite(J)``).  The forward runs
    are taped on a linearised solver too.  ``checkpoint_every`` (int or ``"auto"``): the batched state tape is a checkpointed one
    (``AdjointRun``): ``2 ceil(n / c) + c + 2`` batched states instead of ``n + 2``, the same gradients bit for bit."""
    from .adjoint import AdjointRun, batched_closed_loop_gradient
    from .batch import BatchedFlowSolver

    if signal not in (None, "dE"):
        raise ValueError(f"signal must be None (the quadratic cost of Q and R) or 'dE', got {signal!r}: other columns of the time series are sensor outputs -- weight them with Q")
    n_sens_, n_act_ = len(fs.params_control.sensor_list), fs.params_control.actuator_number
    energy, J0w = None, 0.0
    if signal == "dE":
        energy, Q0, R0, _, J0w = energy_cost_weights(num_steps, fs.params_time.dt, n_sens_, n_act_, criterion, u_penalty, Tc, fs.params_time.Tstart)
        Q = Q0 if Q is None else Q0 + np.asarray(Q, dtype=np.float64).reshape(n_sens_, n_sens_)
        R = R0 if R is None else R0 + np.asarray(R, dtype=np.float64).reshape(n_act_, n_act_)
    elif Q is None or R is None:
        raise TypeError("closed_loop_cost_gradients: give Q and R, or signal='dE'")

    controllers = list(controllers)
    total = len(controllers)
    if total == 0:
        return np.empty(0), []
    k = min(int(batch), total)
    if not 1 <= k <= 32:
        raise ValueError(f"batch must be in [1, 32], got {batch!r}")
    n_act = fs.params_control.actuator_number
    bfs = BatchedFlowSolver(fs, k)
    bfs.initialize_time_stepping(ics=ics)

    def chunk_of(v, idx, per_step):
        """the rows of a per-candidate array for the candidates ``idx`` (anything shared is passed on as it is)"""
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64)
        if per_step:
            return a[:, idx] if a.ndim == 3 else v
        return a[idx] if (a.ndim == 2 and a.shape == (total, n_act)) else v

    J, grads = np.empty(total), []
    try:
        taped = fs.params_solver.is_eq_nonlinear or energy is not None
        # (checkpoint_every: the batched state tape of a long horizon in bounded memory -- AdjointRun; same gradients bit for bit)
        with AdjointRun(bfs, tape=num_steps if taped else None, loop=num_steps, checkpoint_every=checkpoint_every if taped else None) as run:
            for a in range(0, total, k):
                idx = [min(a + j, total - 1) for j in range(k)]
                kw = {key: chunk_of(loop_kwargs[key], idx, True) for key in ("w_y", "w_u") if key in loop_kwargs}
                if loop_kwargs.get("u_limits") is not None:
                    kw["u_limits"] = tuple(chunk_of(v, idx, False) for v in loop_kwargs["u_limits"])
                if energy is not None:
                    kw["energy"] = energy
                Jc, gc = batched_closed_loop_gradient(bfs, [controllers[i] for i in idx], num_steps, Q, R, feedback=loop_kwargs.get("feedback"), adjoint=run,
                                                      **kw)
                if J0w:
                    Jc = Jc + J0w * bfs.initial_energy  # (the initial row of the time series: dE of the initial condition)
                m = min(k, total - a)
                J[a : a + m] = Jc[:m]
                grads.extend(gc[:m])
    finally:
        bfs.close()
    return J, grads


__all__ = ["fun_array", "cummin", "write_results", "sobol_sample", "compute_signal_cost", "compute_control_cost", "write_optim_csv",
           "closed_loop_costs", "fun_array_batched", "energy_cost_weights", "closed_loop_cost_gradients"]
