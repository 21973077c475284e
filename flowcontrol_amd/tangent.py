"""Tangent-linear march: Jacobian-vector products of a nonlinear run (``fc_run_tangent`` / ``fc_run_tangent_batch``,
csrc/fc_tangent.hip.h).

The adjoint marches (``adjoint.py``) apply ``Phi^T``, the transposed Jacobian of a taped nonlinear run; the functions here apply ``Phi``
itself: a perturbation of the controls and of the two initial time levels is stepped along the trajectory on the state tape, with the
exact derivative of the convective term at every taped state and on the direct factors of the forward steps.

* :func:`tangent_run` / :func:`batched_tangent_run`: a taped forward run followed by the march.
* :func:`gauss_newton_product`: ``J^T Q J v + R v`` for the cost of :func:`flowcontrol_amd.adjoint.quadratic_cost_gradient` -- one tangent
  march, then one adjoint march on the same tape.
* :func:`closed_loop_tangent` / :func:`batched_closed_loop_tangent` / :func:`closed_loop_gauss_newton_product`: the same for a closed
  loop -- the controller's tangent step (csrc/fc_tangent_loop.hip.h) ahead of every plant step, directions over the controller's
  matrices, the feedback map, the signals and the initial states; on a linearised solver too.
* ``energy=True`` on the four tangent runs adds ``dde``, the directional derivative ``x_m^T M dx_m`` of the energy every step logs
  (``fc_tangent_set_energy``, csrc/fc_tangent_energy.hip.h); ``energy=e`` on the two products adds the Gauss-Newton matrix of
  ``sum_m e_m dE_m``: the tangent march keeps its states on a tangent tape and the adjoint march is forced with ``e_m M dx_m``
  (``fc_tangent_tape_reserve``, ``fc_set_adjoint_energy_source``; DESIGN §5.6 "Energy").
* :func:`floquet_multipliers`: a block Arnoldi iteration on the pair map ``P: (dx_0, dx_{-1}) -> (dx_n, dx_{n-1})`` over one period of a
  time-periodic nonlinear run.  The driver (:func:`block_arnoldi`) is written against a backend ``apply(V) -> P V``;
  :class:`DeviceTangentBlocks` is the device's.

The three runs stand on the skeleton of ``adjoint.py``: ``_horizon`` saves the state (for the tangent runs it also reserves the tape),
puts the state back and frees the tape afterwards, in that order; ``_adjoint_setup`` owns the ``AdjointRun`` of
:func:`gauss_newton_product`; the batched forward steps are ``adjoint.forward_steps_batch``.
"""

from __future__ import annotations

from contextlib import contextmanager, nullcontext

import numpy as np

from ._lib import SLOT_BDF2
from .adjoint import (_BATCHED, _SINGLE, AdjointRun, _adjoint_setup, _device_of, _energy_needs_tape, _first_order, _horizon, _slot, _weights, energy_rows,
                      forward_steps_batch)


def _check_tangent(fs, who: str) -> None:
    """The conditions of a tangent march on a FlowSolver; ValueError naming the one that fails."""
    if not fs.params_solver.is_eq_nonlinear:
        raise ValueError(f"{who}: is_eq_nonlinear=False -- the forward run of the linearised stepper is its own tangent: step the perturbation")
    if getattr(fs.params_solver, "time_scheme", "bdf") == "cn":
        raise ValueError(f"{who}: time_scheme='cn' -- the tangent march is that of the BDF stepper")
    comm = getattr(fs, "comm", None)
    if comm is not None and getattr(comm, "world", 1) > 1:
        raise ValueError(f"{who}: multi-GPU run -- the state tape is kept on single-GPU handles")


class _reserved_tangent:
    """The march's buffers on the handle for the length of a call, freed on the way out if this call reserved them."""

    def __init__(self, dev):
        self.dev = dev
        self.own = False

    def __enter__(self):
        if not self.dev.tangent_info()["reserved"]:
            self.dev.tangent_reserve(1)
            self.own = True
        return self

    def __exit__(self, *exc):
        if self.own:
            self.dev.tangent_reserve(0)
        return False


class _tangent_energy:
    """``energy=True`` of a tangent run: the energy option on the reserved buffers for the length of the call
    (``DeviceSolver.tangent_set_energy``), put back on the way out if this call switched it on.  ``on`` false: no device call at all."""

    def __init__(self, dev, on: bool):
        self.dev, self.on, self.own = dev, bool(on), False

    def __enter__(self):
        if self.on and not self.dev.tangent_energy_info()["on"]:
            self.dev.tangent_set_energy(1)
            self.own = True
        return self

    def __exit__(self, *exc):
        if self.own:
            self.dev.tangent_set_energy(0)
        return False


@contextmanager
def _tangent_tape(dev, n):
    """The tangent tape of ``n`` steps on the handle for the length of a product (``DeviceSolver.tangent_tape_reserve``), freed on
    every way out.  ``n`` None: nothing is reserved and no device call is made."""
    if n is None:
        yield
        return
    dev.tangent_tape_reserve(n)
    try:
        yield
    finally:
        dev.tangent_tape_reserve(0)


def tangent_run(fs, u_seq, du_seq=None, dx0=None, dxm1=None, first_order: int | None = None, energy: bool = False):
    """The forward device run of ``len(u_seq)`` steps from the solver's present state, taped, and the tangent march over it
    (``fc_run_tangent``): ``(dy [n, n_sens], dx_n [N], dx_{n-1} [N])`` for the perturbations ``du_seq [n, n_act]`` of the controls and
    ``dx0``, ``dxm1`` [N] (W layout; pressure rows are never read) of the two time levels the run starts from (``None``: zero).  ``fs``:
    a nonlinear FlowSolver or a DeviceSolver.  The state the run started from is put back and the tape freed; the solver's log is not
    written to.  A handle that already holds a state tape (an :class:`AdjointRun`) loses it: use :func:`gauss_newton_product` or
    ``AdjointRun.forward`` with ``DeviceSolver.run_tangent`` to share one.

    ``energy=True``: the result also carries ``dde [n]``, the directional derivative ``d(dE_m) = x_m^T M_s dx_m`` of the perturbation
    kinetic energy every step logs (``fc_tangent_set_energy``; DESIGN §5.6 "Energy"), as a fourth entry.  ``energy=False`` makes exactly
    the device calls it made before the option existed."""
    dev, fso = _device_of(fs, taped=True)
    if fso is not None:
        _check_tangent(fso, "tangent_run")
    u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, max(dev.n_act, 1)))
    n, slot = u.shape[0], _slot(_first_order(fso, first_order))
    with _horizon(dev, _SINGLE, tape=n), _reserved_tangent(dev), _tangent_energy(dev, energy):
        dev.adjoint_tape_begin()
        dev.run(slot, n, u, compute_energy=False)
        out = dev.run_tangent(slot, n, du_seq, dx0, dxm1)
        return (*out, dev.tangent_energy()) if energy else out


def forward_batch_taped(bfs_or_dev, u_seq, first_order: int = 2):
    """``len(u_seq)`` batched forward steps with the controls ``u_seq [n, k, n_act]`` from the present batched state onto the batched
    state tape (``fc_adjoint_tape_reserve_batch``, reserved by the caller; taping begins here): ``y [n, k, n_sens]``.  What
    ``AdjointRun.forward_batch`` does, without the transposed factors an ``AdjointRun`` builds.  A BatchedFlowSolver's log, step count
    and clock are not advanced: the steps go to its device handle."""
    dev = _device_of(bfs_or_dev, taped=True)[0] if hasattr(bfs_or_dev, "fs") else bfs_or_dev
    k = dev.batch_k
    u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, k, max(dev.n_act, 1)))
    dev.adjoint_tape_begin_batch()
    return forward_steps_batch(dev, k, u, int(first_order))[0]


def batched_tangent_run(bfs, u_seq, du_seq=None, dx0=None, dxm1=None, ref_col: int | None = None, first_order: int | None = None,
                        energy: bool = False):
    """The k runs of a :class:`BatchedFlowSolver` over their NEXT ``len(u_seq)`` steps with the controls ``u_seq [n, k, n_act]``, taped,
    and k tangent marches in lock step (``fc_run_tangent_batch``): ``(dy [n, k, n_sens], dx_n [k, N], dx_{n-1} [k, N])`` for
    ``du_seq [n, k, n_act]``, ``dx0``, ``dxm1 [k, N]`` (``None``: zero).  ``ref_col=None``: column s perturbs run s; ``ref_col=c``: every
    column perturbs run c -- k directions about one trajectory.  The batched state is put back and the tape freed; the log is not
    written to.  The tape holds every run's states, 8 N KB bytes per step, also with ``ref_col``.  ``energy=True``: a fourth entry
    ``dde [n, k]``, column s the derivative of the energy of the run column s perturbs (:func:`tangent_run`)."""
    dev, fso = _device_of(bfs, taped=True)
    _check_tangent(fso, "batched_tangent_run")
    u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, bfs.k, max(dev.n_act, 1)))
    n, order = u.shape[0], _first_order(bfs, first_order)
    with _horizon(dev, _BATCHED, tape=n), _reserved_tangent(dev), _tangent_energy(dev, energy):
        dev.adjoint_tape_begin_batch()
        forward_steps_batch(dev, bfs.k, u, order)
        out = dev.run_tangent_batch(_slot(order), n, du_seq, dx0, dxm1, ref_col)
        return (*out, dev.tangent_energy()) if energy else out


def gauss_newton_product(fs, u_seq, Q, R, v_seq, adjoint: AdjointRun | None = None, energy=None):
    """``G v = J^T Q_s J v + R_s v`` for the cost ``1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` of
    :func:`flowcontrol_amd.adjoint.quadratic_cost_gradient` at the controls ``u_seq`` (``J = dy/du`` of the nonlinear run, ``Q_s``, ``R_s``
    the symmetric parts): (n, n_act).  One tangent march, ``dy = J v``, then one adjoint march with ``w = Q_s dy`` on the SAME tape.
    ``adjoint``: an ``AdjointRun(fs, tape >= n)`` to reuse (else one is set up and released).  If its tape already holds a run of
    ``len(u_seq)`` steps -- the forward run of a gradient evaluation at these controls -- the forward run is not repeated (the caller
    vouches that the tape is that of ``u_seq``); otherwise the run is taped from the solver's present state, which is put back.

    ``energy`` (a scalar or ``(n,)``, the weights ``e_m`` of :func:`flowcontrol_amd.adjoint.quadratic_cost_gradient`): the cost also
    holds ``sum_m e_m dE_m`` and the product also ``H_E v = sum_m e_m X_m^T M_s X_m v``, ``X_m = dx_m/du``, the Gauss-Newton matrix of
    that term (the second-derivative term ``sum e_m x_m^T M d2x_m`` of the nonlinear run is left out, as it is for ``Q``).  The
    tangent march then keeps its states on a tangent tape and the adjoint march forces step m with ``e_m M_s dx_m``
    (``energy_source=1``); the tape is freed on every way out.  ``H_E`` is positive semi-definite for ``e >= 0``; negative weights are
    accepted and ``H`` is then not semi-definite.  ``energy=None`` makes exactly the device calls of the call without it."""
    u = np.asarray(u_seq, dtype=np.float64)
    with _adjoint_setup(adjoint, fs, tape=u.shape[0]) as adj:
        dev, fso = adj.dev, adj.fs
        if fso is not None:
            _check_tangent(fso, "gauss_newton_product")
        if not adj.tape or adj.every:
            raise ValueError("gauss_newton_product: the AdjointRun needs a dense state tape (AdjointRun(fs, tape=n)); a tangent march over a checkpointed tape is not built")
        u = np.ascontiguousarray(u.reshape(-1, dev.n_act))
        n = u.shape[0]
        v = np.ascontiguousarray(np.asarray(v_seq, dtype=np.float64).reshape(n, dev.n_act))
        Qs, Rs = _weights(dev, Q, R)
        e = energy_rows(energy, n)
        held = {} if e is None else {"energy": e, "energy_source": 1}
        order = _first_order(fso)
        tape = dev.adjoint_tape_info()
        current = tape["begun"] and tape["count"] == n and not tape["overflowed"]
        # (a tape that holds the run: nothing runs forward and there is no state to put back; else the horizon's exit ends the tape)
        with nullcontext() if current else _horizon(dev, _SINGLE):
            if not current:
                adj.forward(u, first_order=order, compute_energy=False)
            with _tangent_tape(dev, None if e is None else n):
                with _reserved_tangent(dev):
                    dy, _, _ = dev.run_tangent(_slot(order), n, v)
                g, _, _ = adj.run(n, w=dy @ Qs, first_order=order, state_gradients=False, **held)
        return g + v @ Rs


# ── closed loops: Jacobian-vector products of the controller problem (fc_run_tangent_closed_loop; DESIGN §5.6 "Closed loop") ─────
#: keys of a closed-loop direction: those of ``closed_loop_gradient``'s ``grads``
LOOP_DIRECTION_KEYS = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "A", "B")


def _check_loop_tangent(fs, who: str) -> None:
    """The conditions of a closed-loop tangent on a FlowSolver (a linearised one is fine); ValueError naming the one that fails."""
    if getattr(fs.params_solver, "time_scheme", "bdf") == "cn":
        raise ValueError(f"{who}: time_scheme='cn' -- the tangent march is that of the BDF stepper")
    comm = getattr(fs, "comm", None)
    if comm is not None and getattr(comm, "world", 1) > 1:
        raise ValueError(f"{who}: multi-GPU run -- the tapes are kept on single-GPU handles")


def _loop_direction(direction, controller, size, packed, dt: float, na: int) -> dict:
    """One controller's ``direction`` (keys :data:`LOOP_DIRECTION_KEYS`, each in the shape of ``closed_loop_gradient``'s entry) as the
    device takes it: continuous ``A, B`` pushed through the zero-order hold (:meth:`Controller.discrete_tangent`) and added to
    ``Ad, Bd``, every matrix zero-padded from the controller's own ``size = (nstates, noutputs)`` to the bank's."""
    d = {k: v for k, v in dict(direction or {}).items() if v is not None}
    unknown = set(d) - set(LOOP_DIRECTION_KEYS)
    if unknown:
        raise KeyError(f"closed-loop direction: unknown keys {sorted(unknown)} (known: {LOOP_DIRECTION_KEYS})")
    nxc, p = size
    nx, nyc, nuc = packed["nx"], packed["nyc"], packed["nuc"]
    if controller.ninputs != nyc:  # (pack_controllers holds this; the continuous and the bank's shapes below are then the same)
        raise ValueError(f"closed-loop direction: the controller takes {controller.ninputs} inputs, the bank's feedback map gives {nyc}")
    if "A" in d or "B" in d:
        nin = controller.ninputs
        tA, tB = controller.discrete_tangent(dt, d.pop("A", np.zeros((nxc, nxc))), d.pop("B", np.zeros((nxc, nin))))
        d["Ad"] = tA + (np.asarray(d["Ad"], dtype=np.float64).reshape(nxc, nxc) if "Ad" in d else 0.0)
        d["Bd"] = tB + (np.asarray(d["Bd"], dtype=np.float64).reshape(nxc, nin) if "Bd" in d else 0.0)
    pads = {"Ad": ((nx, nx), (slice(nxc), slice(nxc))), "Bd": ((nx, nyc), (slice(nxc),)), "C": ((nuc, nx), (slice(p), slice(nxc))),
            "D": ((nuc, nyc), (slice(p),)), "S": ((na, nuc), (slice(None), slice(p))), "x0": ((nx,), (slice(nxc),))}
    out = {}
    for key, a in d.items():
        a = np.asarray(a, dtype=np.float64)
        if key in pads:
            shape, cut = pads[key]
            full = np.zeros(shape)
            full[cut] = a.reshape(full[cut].shape)
            a = full
        out[key] = a
    return out


def _forward_loop_taped(dev, mode, adj, n: int, y0, order: int, nonlinear: bool):
    """The taped closed-loop forward run both closed-loop tangents march over: through ``adj`` (an AdjointRun with ``loop >= n``) if
    given, else onto a loop tape reserved here -- it goes with the bank when the horizon ends -- and the horizon's state tape."""
    if adj is not None:
        return adj._forward_loop("forward_closed_loop", mode, n, y0, order, False)
    getattr(dev, mode.loop_reserve)(n)
    if nonlinear:
        getattr(dev, mode.tape_begin)()
    getattr(dev, mode.loop_begin)()
    return getattr(dev, mode.run_closed_loop)(_slot(order), n, y0, compute_energy=False)


def _loop_inputs(who: str, fso, adjoint, dt, y0, first_order, n_sens: int):
    """``(dt, y0, first order, nonlinear)`` of a closed-loop driver: a FlowSolver's own, or -- on a bare DeviceSolver, which knows
    neither -- the caller's, with the tapes of ``adjoint`` saying whether the states are taped."""
    if fso is None and (adjoint is None or dt is None or y0 is None):
        raise ValueError(f"{who}: on a DeviceSolver give adjoint= (an AdjointRun with loop >= n, and tape >= n on a nonlinear scheme), dt= and y0=")
    if fso is not None:
        _check_loop_tangent(fso, who)
    if adjoint is not None and adjoint.every:
        raise ValueError(f"{who}: a tangent march over a checkpointed tape is not built (AdjointRun without checkpoint_every)")
    nonlinear = bool(fso.params_solver.is_eq_nonlinear) if fso is not None else adjoint.tape > 0
    y0 = np.asarray(fso.y_meas if y0 is None else y0, dtype=np.float64).reshape(n_sens).copy()
    return (fso.params_time.dt if dt is None else float(dt)), y0, _first_order(fso, first_order), nonlinear


def closed_loop_tangent(fs, controller, n_steps: int, direction, feedback=None, w_y=None, w_u=None, u_limits=None, adjoint: AdjointRun | None = None,
                        dt: float | None = None, y0=None, first_order: int | None = None, energy: bool = False) -> dict:
    """The directional derivative of the closed loop of ``fs`` with the LTI ``controller`` over the NEXT ``n_steps`` steps (the loop of
    :func:`flowcontrol_amd.adjoint.closed_loop_gradient`: ``feedback``, ``w_y``, ``w_u``, ``u_limits`` as there) along ``direction``: a
    dict with any of the keys of that function's ``grads`` -- ``Ad, Bd, C, D, G, g0, S, x0, y0, w_y, w_u`` and the continuous-time
    ``A, B`` (:meth:`Controller.discrete_tangent`), each in the shape of the gradient's entry; absent: zero.  One taped closed-loop run
    and one tangent march on the device (``fc_run_tangent_closed_loop``): ``{"y", "u"`` of the run, ``"dy"`` (n, n_sens), ``"du"`` (n, n_act; exactly 0 where a limit holds
    the control), ``"xi"`` (nstates,), ``"dxn"``, ``"dxnm1"`` (N,)``}``.  Works on both kinds of solver.  The flow state and the
    controller state are put back and the solver's log is not written to.  ``adjoint``: an ``AdjointRun(fs, loop >= n[, tape >= n])``
    whose tapes to use (dense); else the tapes are reserved and freed here, and no transposed factors are built.  ``fs`` may be a bare
    DeviceSolver: then ``adjoint`` (set up on it), ``dt`` and ``y0`` (the measurement the first controller step reads) are needed,
    and ``first_order`` (the BDF order of the first step) defaults to 2.

    ``energy=True``: the result also carries ``"dde"`` (n,), the derivative of the energy every step logs (:func:`tangent_run`).  The
    march then reads the taped states on a linearised solver too: the run is taped there as well (with ``adjoint=``: it needs
    ``tape >= n``)."""
    from .controller import Controller, loop_limits, loop_signal_rows

    if not isinstance(controller, Controller):
        raise TypeError("closed_loop_tangent differentiates an LTI Controller")
    dev, fso = (adjoint.dev, adjoint.fs) if adjoint is not None else _device_of(fs, taped=True)
    dt, y0, order, nonlinear = _loop_inputs("closed_loop_tangent", fso, adjoint, dt, y0, first_order, dev.n_sens)
    n, na = int(n_steps), dev.n_act
    bank = ([controller], dt, feedback, loop_signal_rows(w_y, n, (controller.ninputs,), "w_y"), loop_signal_rows(w_u, n, (na,), "w_u"),
            loop_limits(u_limits, (1, na)))
    taped = nonlinear or bool(energy)  # (the energy reads x_m: the states are taped on a linearised solver too)
    with _horizon(dev, _SINGLE, bank=bank, tape=n if (taped and adjoint is None) else None) as packed, _reserved_tangent(dev), _tangent_energy(dev, energy):
        size = packed["sizes"][0]
        y, u, _ = _forward_loop_taped(dev, _SINGLE, adjoint, n, y0, order, taped)
        t = dev.run_tangent_closed_loop(_slot(order), n, _loop_direction(direction, controller, size, packed, dt, na))
        extra = {"dde": dev.tangent_energy()} if energy else {}
    return {"y": y, "u": u, "dy": t["dy"], "du": t["du"], "xi": t["xi"][:size[0]], "dxn": t["dxn"], "dxnm1": t["dxnm1"], **extra}


def batched_closed_loop_tangent(bfs, controllers, n_steps: int, directions, ref_col: int | None = None, feedback=None, w_y=None, w_u=None, u_limits=None,
                                adjoint: AdjointRun | None = None, energy: bool = False) -> dict:
    """The k closed loops of a :class:`BatchedFlowSolver` -- ``controllers[s]`` around run s -- over their NEXT ``n_steps`` steps, and
    k tangents in lock step (``fc_run_tangent_closed_loop_batch``): ``directions`` is a list of k dicts as :func:`closed_loop_tangent`
    takes one.  ``ref_col=None``: column s differentiates loop s; ``ref_col=c``: every column differentiates loop c along its own
    direction (k directions about one loop; ``directions[s]`` is then sized for ``controllers[c]``).  Returns ``y`` (n, k, n_sens),
    ``u`` (n, k, n_act) of the runs and ``dy``, ``du`` with the same shapes, ``xi`` (k, nx of the bank), ``dxn`` / ``dxnm1`` (k, N).
    The batched state and the controllers' states are put back; the log is not written to.  ``energy=True``: also ``dde`` (n, k), as
    :func:`closed_loop_tangent`'s."""
    from .controller import Controller, loop_limits, loop_signal_rows_batch

    controllers, directions = list(controllers), list(directions)
    k = bfs.k
    if len(controllers) != k or len(directions) != k:
        raise ValueError(f"expected {k} controllers and {k} directions, got {len(controllers)} and {len(directions)}")
    if not all(isinstance(K, Controller) for K in controllers):
        raise TypeError("batched_closed_loop_tangent differentiates LTI Controllers")
    dev, fso = (adjoint.dev, adjoint.fs) if adjoint is not None else _device_of(bfs, taped=True)
    _check_loop_tangent(fso, "batched_closed_loop_tangent")
    if bfs.order == "cn":
        raise ValueError("batched_closed_loop_tangent: time_scheme='cn' -- the tangent march is that of the BDF stepper")
    if adjoint is not None and (adjoint.batch is not bfs or adjoint.every):
        raise ValueError("batched_closed_loop_tangent: the AdjointRun must be set up on this BatchedFlowSolver with dense tapes")
    n, nonlinear = int(n_steps), bool(fso.params_solver.is_eq_nonlinear)
    dt, na = bfs.params_time.dt, dev.n_act
    bank = (controllers, dt, feedback, loop_signal_rows_batch(w_y, n, k, controllers[0].ninputs, "w_y"), loop_signal_rows_batch(w_u, n, k, na, "w_u"),
            loop_limits(u_limits, (k, na)))
    order = _first_order(bfs)
    taped = nonlinear or bool(energy)
    with _horizon(dev, _BATCHED, flush=bfs._flush, bank=bank, tape=n if (taped and adjoint is None) else None) as packed, _reserved_tangent(dev), \
            _tangent_energy(dev, energy):
        y0 = np.where(bfs.diverged[:, None], 0.0, np.asarray(bfs.y_meas, dtype=np.float64).reshape(k, dev.n_sens))
        y, u = _forward_loop_taped(dev, _BATCHED, adjoint, n, y0, order, taped)[:2]
        about = (lambda s: s) if ref_col is None else (lambda s: int(ref_col))
        cols = [_loop_direction(directions[s], controllers[about(s)], packed["sizes"][about(s)], packed, dt, na) for s in range(k)]
        stacked = {}
        for key in sorted(set().union(*cols)):
            shape = next(c[key].shape for c in cols if key in c)
            per = [c.get(key, np.zeros(shape)) for c in cols]
            stacked[key] = np.stack(per, axis=1 if key in ("w_y", "w_u") else 0)
        t = dev.run_tangent_closed_loop_batch(_slot(order), n, stacked, ref_col=ref_col)
        if energy:
            t = {**t, "dde": dev.tangent_energy()}
    return {"y": y, "u": u, **t}


def closed_loop_gauss_newton_product(fs, controller, n_steps: int, Q, R, direction, feedback=None, w_y=None, w_u=None, u_limits=None,
                                     adjoint: AdjointRun | None = None, dt: float | None = None, y0=None, first_order: int | None = None,
                                     energy=None) -> dict:
    """``H v = J^T diag(Q_s, R_s) J v`` for the cost ``1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` of
    :func:`flowcontrol_amd.adjoint.closed_loop_gradient` at ``controller``, with ``J = d(y, u)/d theta`` the Jacobian of the loop's
    measurements and clamped controls with respect to everything a ``direction`` may move, ``v = direction`` (as
    :func:`closed_loop_tangent` takes it) and ``Q_s, R_s`` the symmetric parts.  One taped closed-loop run, one tangent march
    (``dy, du = J v``), then one adjoint march with ``w = dy Q_s``, ``r = du R_s`` on the SAME tapes.  Returns a dict with the keys of
    ``closed_loop_gradient``'s ``grads`` (``A, B`` of the continuous-time controller included).

    This is the Gauss-Newton matrix of the loop WITH ITS CLAMP PATTERN HELD: where a limit holds a control value neither march lets a
    perturbation through, so ``H`` is that of the loop whose clamped controls are constants.  It is symmetric positive semi-definite;
    the curvature of the clamp itself (a control value entering or leaving a limit) is not in it.  A batched product is not built.
    ``adjoint``: an ``AdjointRun(fs, loop >= n[, tape >= n])`` with dense tapes to reuse.  ``fs`` may be a bare DeviceSolver, as for
    :func:`closed_loop_tangent` (``adjoint``, ``dt``, ``y0``).

    ``energy`` (a scalar or ``(n,)``): the weights ``e_m`` of a cost term ``sum_m e_m dE_m``
    (:func:`flowcontrol_amd.adjoint.closed_loop_gradient`); the product then also holds ``H_E v = sum_m e_m X_m^T M_s X_m v`` with
    ``X_m = dx_m/d theta``, as :func:`gauss_newton_product` forms it: the tangent march keeps its states on a tangent tape, the adjoint
    march forces step m with ``e_m M_s dx_m``, the tape is freed on every way out.  On a linearised solver the run is then taped (the
    marches read ``x_m`` and ``dx_m``); an ``adjoint`` passed in needs ``tape >= n``.  Negative weights are accepted: ``H`` is then not
    semi-definite.  Not built: a checkpointed tape, the second-derivative term of a nonlinear run.  ``energy=None`` is the call without
    the keyword, device call for device call."""
    from .adjoint import _controller_gradients, _tape_for
    from .controller import Controller, loop_limits, loop_signal_rows

    if not isinstance(controller, Controller):
        raise TypeError("closed_loop_gauss_newton_product differentiates an LTI Controller")
    n = int(n_steps)
    e = energy_rows(energy, n)
    held = {} if e is None else {"energy": e, "energy_source": 1}
    tape = _tape_for(fs, n, e, None)[0] if hasattr(fs, "params_solver") else None
    with _adjoint_setup(adjoint, fs, tape=tape, loop=n) as adj:
        dev = adj.dev
        _energy_needs_tape(adj, e, "closed_loop_gauss_newton_product", "fs, tape=n, loop=n")
        dt, y0, order, _ = _loop_inputs("closed_loop_gauss_newton_product", adj.fs, adjoint, dt, y0, first_order, dev.n_sens)
        na = dev.n_act
        Qs, Rs = _weights(dev, Q, R)
        bank = ([controller], dt, feedback, loop_signal_rows(w_y, n, (controller.ninputs,), "w_y"), loop_signal_rows(w_u, n, (na,), "w_u"),
                loop_limits(u_limits, (1, na)))
        with _horizon(dev, _SINGLE, bank=bank) as packed, _reserved_tangent(dev):
            size = packed["sizes"][0]
            adj.forward_closed_loop(n, y0, first_order=order)
            with _tangent_tape(dev, None if e is None else n):
                t = dev.run_tangent_closed_loop(_slot(order), n, _loop_direction(direction, controller, size, packed, dt, na))
                g = adj.run_closed_loop_adjoint(n, w=t["dy"] @ Qs, r=t["du"] @ Rs, first_order=order, state_gradients=False, **held)
        return _controller_gradients(g, controller, size, dt)


# ── block Arnoldi on a backend apply(V) -> P V ───────────────────────────────────────────────────────────────────────────────────
def block_arnoldi(apply, V0, blocks: int):
    """``blocks`` steps of the block Arnoldi iteration of the linear map behind ``apply(V [m, k]) -> P V [m, k]`` from the start block
    ``V0 [m, k]`` (Euclidean inner product): two passes of block Gram-Schmidt against all earlier blocks, then a QR of the remainder.
    Returns ``(Qb, H)``: the ``blocks + 1`` orthonormal blocks ``[m, k]`` and the block Hessenberg matrix ``((blocks + 1) k, blocks k)``
    with ``P [Q_0 .. Q_{b-1}] = [Q_0 .. Q_b] H``.  The basis lives on the host; only ``apply`` runs elsewhere."""
    V0 = np.asarray(V0, dtype=np.float64)
    m, k = V0.shape
    if blocks < 1:
        raise ValueError("block_arnoldi: blocks must be at least 1")
    q, r = np.linalg.qr(V0)
    if np.min(np.abs(np.diag(r))) <= 1e-13 * np.max(np.abs(np.diag(r))):
        raise ValueError("block_arnoldi: the start block is rank deficient")
    Qb = [q]
    H = np.zeros(((blocks + 1) * k, blocks * k))
    for j in range(blocks):
        W = np.array(apply(Qb[j]), dtype=np.float64).reshape(m, k)
        if not np.all(np.isfinite(W)):
            raise RuntimeError(f"block_arnoldi: non-finite block from apply in step {j}")
        for _ in range(2):
            for i in range(j + 1):
                h = Qb[i].T @ W
                W -= Qb[i] @ h
                H[i * k:(i + 1) * k, j * k:(j + 1) * k] += h
        q, r = np.linalg.qr(W)
        H[(j + 1) * k:(j + 2) * k, j * k:(j + 1) * k] = r
        Qb.append(q)
    return Qb, H


def _by_modulus(lam, rtol: float = 1e-9):
    """Indices of ``lam`` by modulus, descending.  Neighbours whose moduli agree within ``rtol`` of the group's largest (a conjugate
    pair) form a group, ordered by imaginary part, descending -- so that round-off does not decide the order inside a pair."""
    order = np.argsort(-np.abs(lam), kind="stable")
    out, group = [], []
    for i in order:
        if group and abs(lam[group[0]]) - abs(lam[i]) > rtol * abs(lam[group[0]]):
            out += sorted(group, key=lambda q: -lam[q].imag)
            group = []
        group.append(int(i))
    out += sorted(group, key=lambda q: -lam[q].imag)
    return np.array(out, dtype=int)


def ritz_pairs(Qb, H, n_modes: int, vectors: bool = False):
    """The ``n_modes`` Ritz values of largest modulus of a :func:`block_arnoldi` result (``numpy.linalg.eigvals`` of the square block
    Hessenberg matrix, sorted by modulus, descending) -- with ``vectors`` ``(values, V [m, n_modes], residuals)``: unit Ritz vectors and
    ``|P v - lambda v| / |lambda|``, formed from the Arnoldi relation (the last sub-diagonal block times the tail of the eigenvector)."""
    k = Qb[0].shape[1]
    b = len(Qb) - 1
    Hm = H[:b * k, :b * k]
    if not vectors:
        lam = np.linalg.eigvals(Hm)
        return lam[_by_modulus(lam)][:n_modes]
    lam, Y = np.linalg.eig(Hm)
    idx = _by_modulus(lam)[:n_modes]
    lam, Y = lam[idx], Y[:, idx]
    V = np.hstack(Qb[:b]) @ Y
    res = np.linalg.norm(H[b * k:, (b - 1) * k:] @ Y[(b - 1) * k:], axis=0) / np.maximum(np.abs(lam), np.finfo(float).tiny)
    return lam, V, res


class DeviceTangentBlocks:
    """The device backend of :func:`floquet_multipliers`: ``apply(V [2 N, k]) -> P V``, the pair map over the ``n_steps`` BDF2 steps on
    the batched state tape of ``bfs_or_dev``, about the trajectory of column ``ref_col`` (one ``fc_run_tangent_batch`` per apply, k
    columns wide).  Rows ``[:N]`` of a column are ``dx_0`` / ``dx_n``, rows ``[N:]`` ``dx_{-1}`` / ``dx_{n-1}`` (W layout)."""

    def __init__(self, bfs_or_dev, n_steps: int, ref_col: int = 0):
        self.dev = _device_of(bfs_or_dev, taped=True)[0] if hasattr(bfs_or_dev, "fs") else bfs_or_dev
        self.n, self.ref_col = int(n_steps), int(ref_col)
        self.k, self.size = self.dev.batch_k, 2 * self.dev.N
        self.applies = 0

    def apply(self, V):
        N = self.dev.N
        V = np.asarray(V, dtype=np.float64).reshape(2 * N, self.k)
        _, dxn, dxnm1 = self.dev.run_tangent_batch(SLOT_BDF2, self.n, None, np.ascontiguousarray(V[:N].T), np.ascontiguousarray(V[N:].T), self.ref_col)
        self.applies += 1
        return np.vstack([dxn.T, dxnm1.T])


def floquet_multipliers(bfs, period_steps: int, n_modes: int, blocks: int = 8, start=None, seed: int = 0, vectors: bool = False):
    """The ``n_modes`` leading Floquet multipliers of the time-periodic nonlinear run whose period of ``period_steps`` BDF2 steps sits
    on the batched state tape of ``bfs`` (column 0 is the trajectory; :func:`forward_batch_taped`, ``AdjointRun(bfs, tape=n).forward_batch`` or
    ``adjoint_tape_reserve_batch`` / ``_begin_batch`` and the steps): eigenvalues of the pair map
    ``P: (dx_0, dx_{-1}) -> (dx_n, dx_{n-1})``, approximated by ``blocks`` steps of :func:`block_arnoldi` with the batch's k columns
    per apply and the Euclidean inner product on the pair.  ``bfs`` may also be any backend with ``apply(V [m, k]) -> P V``, ``k`` and
    ``size`` (the tests run the driver on a numpy model).  ``start [size, k]``: the start block (default: random, ``seed``).

    Returns the Ritz values sorted by modulus (descending) -- with ``vectors`` ``(values, V [size, n_modes], residuals)``, the
    residuals ``|P v - lambda v| / |lambda|``.  The basis of ``(blocks + 1) k`` pair vectors lives on the HOST; only the k-column
    applies run on the device (a device-resident basis is not part of this driver).  The tangent buffers are reserved for the call if
    they are not yet."""
    backend = bfs if hasattr(bfs, "apply") else DeviceTangentBlocks(bfs, period_steps, ref_col=0)
    k, m = int(backend.k), int(backend.size)
    if n_modes < 1 or n_modes > blocks * k:
        raise ValueError(f"floquet_multipliers: n_modes must be in [1, blocks * k = {blocks * k}]")
    V0 = np.random.default_rng(seed).standard_normal((m, k)) if start is None else np.asarray(start, dtype=np.float64).reshape(m, k)
    dev = getattr(backend, "dev", None)
    if dev is not None:
        with _reserved_tangent(dev):
            Qb, H = block_arnoldi(backend.apply, V0, blocks)
    else:
        Qb, H = block_arnoldi(backend.apply, V0, blocks)
    return ritz_pairs(Qb, H, n_modes, vectors)


__all__ = ["tangent_run", "batched_tangent_run", "forward_batch_taped", "gauss_newton_product", "closed_loop_tangent", "batched_closed_loop_tangent",
           "closed_loop_gauss_newton_product", "block_arnoldi", "ritz_pairs", "DeviceTangentBlocks", "floquet_multipliers"]
