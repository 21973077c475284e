"""Adjoint time stepping: gradients of a run's cost (``fc_run_adjoint``, csrc/fc_adjoint.hip.h).

The linearised stepper (``is_eq_nonlinear=False``) is the constant linear recurrence

    A_s x_{m+1} = Z M (cm_n x_m + cm_nn x_{m-1}) + B~ u_{m+1},        y_m = C x_m

and for a cost ``J = sum_m w_m . y_m + z . x_n`` its exact discrete adjoint is the same recurrence run backwards on the transposed
factors: no forward trajectory is stored, a backward step costs a forward one.  :class:`AdjointRun` holds the transposed factors of
both order slots on the device; :func:`run_gradient` is one backward march; :func:`quadratic_cost_gradient` runs forward and backward
for ``J = 1/2 sum (y^T Q y + u^T R u)``.

The nonlinear stepper (``is_eq_nonlinear=True``) adds the explicit convective term ``cc_n N(x_m) + cc_nn N(x_{m-1})`` to the right-hand
side, and its adjoint the transposed Jacobian ``J(x_m)^T`` at every backward step (csrc/fc_adjoint_nl.hip.h): the march needs the
forward trajectory.  It is opt-in -- ``AdjointRun(fs, tape=capacity)`` reserves a state tape of ``capacity`` steps on the device
(8 N bytes per step), :meth:`AdjointRun.forward` runs the forward steps onto it and :meth:`AdjointRun.run` marches back over exactly
that run.  :meth:`FlowSolver.cost_gradient` does all of it for both kinds of solver.

A closed loop (``fc_run_closed_loop``) puts an LTI controller between the sensors and the actuators.  ``AdjointRun(fs, loop=capacity)``
reserves a loop tape (``fc_adjoint_loop_reserve``: the controller state before its update, the measurement read and the unclamped
control of every step), :meth:`AdjointRun.forward_closed_loop` runs the loop onto it and :meth:`AdjointRun.run_closed_loop_adjoint`
marches back with the controller's adjoint inside the march (csrc/fc_adjoint_loop.hip.h): one forward and one backward run give the
gradient of the cost with respect to every matrix of the controller, the feedback map, the loop signals and the initial states.
:func:`closed_loop_gradient` does all of it for ``J = 1/2 sum (y^T Q y + u^T R u)``.

k closed loops of a :class:`BatchedFlowSolver` -- one controller per run -- are differentiated together: ``AdjointRun(bfs, loop=n)``
reserves the batched loop tape once a bank of k controllers is on the device (``fc_adjoint_loop_reserve_batch``),
:meth:`AdjointRun.forward_closed_loop_batch` runs the k loops onto it and :meth:`AdjointRun.run_closed_loop_adjoint_batch` is ONE
backward march for all of them (csrc/fc_adjoint_loop_batch.hip.h: the transposed factors are read once per step for all columns).
:func:`batched_closed_loop_gradient` returns the k costs and the k sets of gradients.

``energy=`` on the four gradient functions and on the ``AdjointRun.run*`` marches adds ``sum_m e_m dE_m`` to the cost, ``dE_m = 1/2 x_m^T
M x_m`` being the perturbation kinetic energy every step logs (csrc/fc_adjoint_energy.hip.h): backward step m then carries the forcing
``e_m M x_m``, read from the state tape -- so with ``energy`` a linearised solver is taped too (8 N bytes per step, 8 N KB batched).

The gradient functions here and the tangent runs of ``tangent.py`` share one skeleton.  ``_Mode`` names what differs between a single
and a batched handle (the ``DeviceSolver`` methods of the tapes, the state and the marches; the subscripts of the cost) and has two
instances.  ``_adjoint_setup`` yields the :class:`AdjointRun` to work with and closes it on the way out iff this call made it;
``_horizon`` saves the state, loads ``x0`` and a controller bank, and on the way out -- whatever way that is -- puts the state back,
then takes the bank off, then frees a tape it reserved.  A driver keeps what is its own: which forward run and which march it calls
and what it derives from the result.
"""

from __future__ import annotations

import math
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

from ._lib import SLOT_BDF1, SLOT_BDF2

_SLOTS = (SLOT_BDF1, SLOT_BDF2)

#: What differs between the single and the batched handle: names of ``DeviceSolver`` methods, and the einsum subscripts of the cost.
_Mode = namedtuple("_Mode", "tape_reserve tape_reserve_sparse tape_begin tape_info loop_reserve loop_begin loop_info get_state set_state "
                            "run_closed_loop march march_loop cost energy")
_SINGLE = _Mode("adjoint_tape_reserve", "adjoint_tape_reserve_sparse", "adjoint_tape_begin", "adjoint_tape_info", "adjoint_loop_reserve",
                "adjoint_loop_begin", "adjoint_loop_info", "get_state", "set_state", "run_closed_loop", "run_adjoint", "run_adjoint_closed_loop",
                "mi,ij,mj->", "m,m->")
_BATCHED = _Mode("adjoint_tape_reserve_batch", "adjoint_tape_reserve_sparse_batch", "adjoint_tape_begin_batch", "adjoint_tape_info_batch",
                 "adjoint_loop_reserve_batch", "adjoint_loop_begin_batch", "adjoint_loop_info_batch", "get_state_batch", "set_state_batch",
                 "run_closed_loop_batch", "run_adjoint_batch", "run_adjoint_closed_loop_batch", "mki,ij,mkj->k", "mk,mk->k")


def _slot(order: int) -> int:
    return SLOT_BDF1 if order == 1 else SLOT_BDF2


def energy_rows(energy, n: int, k: int | None = None):
    """The weights ``e_m`` of the energy term as rows: a scalar, ``(n,)`` or -- batched, ``k`` given -- ``(n, k)`` -> ``(n,)`` / ``(n, k)``;
    ``None`` stays ``None``."""
    if energy is None:
        return None
    e = np.asarray(energy, dtype=np.float64)
    if e.ndim == 0:
        e = np.full(n, float(e))
    if e.ndim == 1 and e.shape[0] != n or e.ndim > (1 if k is None else 2):
        raise ValueError(f"energy must be a scalar, ({n},)" + ("" if k is None else f" or ({n}, {k})") + f", got {e.shape}")
    if k is not None:
        e = np.repeat(e[:, None], k, axis=1) if e.ndim == 1 else e
        if e.shape != (n, k):
            raise ValueError(f"energy must be a scalar, ({n},) or ({n}, {k}), got {e.shape}")
    return np.ascontiguousarray(e)


class _held_energy:
    """The weights on the handle for the length of a march; cleared on the way out, whatever way that is.  ``source=1``: they multiply
    the tangent tape's ``dx_m`` (``DeviceSolver.set_adjoint_energy_source``); the source goes back to 0 ahead of the rows."""

    def __init__(self, dev, rows, source: int = 0):
        self.dev, self.rows, self.source = dev, rows, int(source) if rows is not None else 0

    def __enter__(self):
        if self.rows is not None:
            self.dev.set_adjoint_energy(self.rows)
        if self.source:
            try:
                self.dev.set_adjoint_energy_source(self.source)
            except Exception:
                self.dev.set_adjoint_energy(None)  # (no march follows and no __exit__: the rows do not stay behind)
                raise

    def __exit__(self, exc_type, exc, tb):
        if self.rows is None:
            return False
        try:
            try:
                if self.source:
                    self.dev.set_adjoint_energy_source(0)
            finally:
                self.dev.set_adjoint_energy(None)  # (clearing the rows also puts the source back on the device)
        except Exception:
            if exc_type is None:
                raise  # (the march went through: a clearing that fails is the error to report)
            # the march raised and that error goes on; the clearing's own is second to it
        return False


def _is_batched(obj) -> bool:
    from .batch import BatchedFlowSolver

    return isinstance(obj, BatchedFlowSolver)


def _device_of(fs_or_dev, taped: bool = False):
    """(device handle, FlowSolver or None): a FlowSolver is made ready to step first.  A BatchedFlowSolver gives its handle (with the
    batch set) and the FlowSolver whose operators it shares."""
    if _is_batched(fs_or_dev):
        bfs = fs_or_dev
        _check_flowsolver(bfs.fs, taped)
        if not bfs._ready:
            bfs._prepare()
        bfs._flush()
        return bfs.dev, bfs.fs
    if hasattr(fs_or_dev, "th") and hasattr(fs_or_dev, "params_solver"):
        fs = fs_or_dev
        _check_flowsolver(fs, taped)
        fs._begin_stepping()
        fs._flush_log()  # (energy / residual of an overlapped last step are collected before anything else uses the handle)
        return fs.th.device(), fs
    return fs_or_dev, None


def _check_flowsolver(fs, taped: bool = False) -> None:
    """The conditions of :meth:`FlowSolver.adjoint_run`; ValueError naming the one that fails.  ``taped``: the caller keeps a state
    tape, which is what a nonlinear solver needs."""
    if fs.params_solver.is_eq_nonlinear and not taped:
        raise ValueError("adjoint_run: is_eq_nonlinear=True -- the adjoint of the nonlinear stepper reads the forward trajectory from a state "
                         "tape: AdjointRun(fs, tape=n_steps), its forward() and run(), or FlowSolver.cost_gradient")
    if getattr(fs.params_solver, "time_scheme", "bdf") == "cn":
        raise ValueError("adjoint_run: time_scheme='cn' -- the backward march is the adjoint of the BDF stepper (order 2)")
    comm = getattr(fs, "comm", None)
    if comm is not None and getattr(comm, "world", 1) > 1:
        raise ValueError("adjoint_run: multi-GPU run -- the transposed factors are built on single-GPU handles")
    if getattr(fs, "factor_bits", 64) != 64:
        raise ValueError(f"adjoint_run: factor_bits={fs.factor_bits} -- compressed factors are a preconditioner; the adjoint needs the direct fp64 factors")


def checkpoint_spacing(checkpoint_every, n_steps: int) -> int:
    """The spacing ``c`` of a checkpointed tape of ``n_steps`` steps: 0 for ``None`` (the dense tape), ``ceil(sqrt(2 n))`` for
    ``"auto"`` (the minimiser of the ``2 ceil(n / c) + c`` columns held, up to rounding), else the positive int given."""
    if checkpoint_every is None:
        return 0
    if not n_steps:
        raise ValueError("checkpoint_every needs a state tape (tape=n_steps)")
    if isinstance(checkpoint_every, str):
        if checkpoint_every != "auto":
            raise ValueError(f"checkpoint_every must be a positive int or 'auto', got {checkpoint_every!r}")
        return math.isqrt(2 * int(n_steps) - 1) + 1
    c = int(checkpoint_every)
    if c <= 0 or c != checkpoint_every:
        raise ValueError(f"checkpoint_every must be a positive int or 'auto', got {checkpoint_every!r}")
    return c


def _adjoint_for(adjoint, checkpoint_every, make):
    """The AdjointRun a gradient function works with: ``adjoint`` if given (``checkpoint_every`` must then be what it was set up with,
    or None), else ``make()``."""
    if adjoint is None:
        return make()
    if checkpoint_every is not None and checkpoint_spacing(checkpoint_every, adjoint.tape) != adjoint.every:
        raise ValueError(f"checkpoint_every={checkpoint_every!r}, but the AdjointRun passed in was set up with "
                         f"checkpoint_every={adjoint.every or None!r}")
    return adjoint


@contextmanager
def _adjoint_setup(adjoint, target, tape=None, loop=None, checkpoint_every=None):
    """Ownership: the AdjointRun a driver works with (:func:`_adjoint_for`; a new one is ``AdjointRun(target, tape, loop,
    checkpoint_every)``), closed on the way out -- whatever way that is -- if and only if this call made it."""
    adj = _adjoint_for(adjoint, checkpoint_every, lambda: AdjointRun(target, tape=tape, loop=loop, checkpoint_every=checkpoint_every))
    try:
        yield adj
    finally:
        if adjoint is None:
            adj.close()


@contextmanager
def _horizon(dev, mode, flush=None, x0=None, start=None, bank=None, tape=None):
    """One horizon on ``dev``, after which the handle is where it was.  On entry: ``flush()`` (a BatchedFlowSolver's ``_flush``), the
    start state read with the mode's getter (``start``: the state to put back instead, nothing is read), a state tape of ``tape``
    steps reserved, the controller bank ``(controllers, dt, feedback, w_y, w_u, limits)`` put on the device -- yielded as packed --
    ``x0`` loaded, the loop signals and the limits set.  On exit, whatever way out: the start state goes back, then the bank comes off
    (also when putting the state back raised), then the tape is freed."""
    controllers, dt, feedback, w_y, w_u, limits = bank if bank is not None else (None,) * 6
    if flush is not None:
        flush()
    setter, reserve = getattr(dev, mode.set_state), getattr(dev, mode.tape_reserve)
    start = getattr(dev, mode.get_state)() if start is None else start
    if tape is not None:
        reserve(tape)
    packed = None if bank is None else dev.set_controllers(controllers, dt, feedback)  # (reads every controller.x; the host objects are not advanced)
    try:
        if x0 is not None:
            setter(*x0)
        if w_y is not None or w_u is not None:
            dev.set_loop_signals(w_y, w_u)
        if limits is not None:
            dev.set_control_limits(*limits)
        yield packed
    finally:
        try:
            setter(*start)
        finally:
            if bank is not None:
                dev.set_controllers(None, dt)
            if tape is not None:
                reserve(0)


def _weights(dev, Q, R):
    """``(Qs, Rs)``: the symmetric parts of ``Q`` (n_sens, n_sens) and ``R`` (n_act, n_act) -- what the cost and its gradient see."""
    Q = np.asarray(Q, dtype=np.float64).reshape(dev.n_sens, dev.n_sens)
    R = np.asarray(R, dtype=np.float64).reshape(dev.n_act, dev.n_act)
    return 0.5 * (Q + Q.T), 0.5 * (R + R.T)


def _cost(mode, y, u, Qs, Rs, e=None, dE=None):
    """``1/2 sum_m (y_m^T Qs y_m + u_m^T Rs u_m) [+ sum_m e_m dE_m]``: a 0-d array, batched ``(k,)``."""
    J = 0.5 * (np.einsum(mode.cost, y, Qs, y) + np.einsum(mode.cost, u, Rs, u))
    return J if e is None else J + np.einsum(mode.energy, e, dE)


def _tape_for(fs, n: int, energy, checkpoint_every):
    """``(tape, checkpoint_every)`` of the setup a driver makes: a run is taped where the march reads the trajectory -- a nonlinear
    solver, an energy term -- and only then is there a tape to checkpoint."""
    return (n, checkpoint_every) if (fs.params_solver.is_eq_nonlinear or energy is not None) else (None, None)


def _energy_needs_tape(adj, energy, who: str, setup: str) -> None:
    if energy is not None and not adj.tape:
        raise ValueError(f"{who}: energy= reads the forward trajectory -- the AdjointRun needs a state tape (AdjointRun({setup}))")


def _first_order(solver, first_order=None) -> int:
    """BDF order of a run's first step: ``first_order`` if given, else 1 where ``solver`` (a FlowSolver, a BatchedFlowSolver or None)
    is at order 1, else 2 -- also for a batch whose order is ``"cn"``."""
    if first_order is not None:
        return int(first_order)
    return 1 if getattr(solver, "order", 2) == 1 else 2


def forward_steps_batch(dev, k: int, u, first_order: int = 2, compute_energy: bool = False):
    """THE batched forward step loop: ``u.shape[0]`` steps of the k runs on ``dev`` with the controls ``u [n, k, n_act]``, the first on
    the slot of ``first_order``: ``(y [n, k, n_sens], dE [n, k])``.  Taping is begun by the caller."""
    y, dE = np.empty((u.shape[0], k, dev.n_sens)), np.empty((u.shape[0], k))
    for m in range(u.shape[0]):
        y[m], dE[m], _ = dev.step_batch(_slot(first_order) if m == 0 else SLOT_BDF2, u[m], compute_energy=bool(compute_energy))
    return y, dE


class AdjointRun:
    """The adjoint setup of one device handle: transposed factor values of the BDF1 and BDF2 slots (``fc_set_adjoint_factors``) and,
    from the first march on, its buffers.  ``tape=capacity`` also reserves a state tape of that many steps (``fc_adjoint_tape_reserve``),
    which a nonlinear solver needs: :meth:`forward` runs the forward steps onto it, :meth:`run` marches back over them.  ``close()``
    frees all of it (also called when the handle is released through ``th.release_device()``); the handle then steps as if the setup
    had never existed.

    ``checkpoint_every=c`` (an int, or ``"auto"`` = ceil(sqrt(2 tape)), which minimises the columns held) makes the state tape a
    CHECKPOINTED one (``fc_adjoint_tape_reserve_sparse``): ``2 ceil(tape / c) + c + 2`` columns instead of ``tape + 2``, for horizons
    whose dense tape does not fit.  The marches recompute one segment of c steps at a time and return the dense tape's gradients bit
    for bit, at the cost of one more forward run.  On a BatchedFlowSolver it is the batched tape that is checkpointed
    (``fc_adjoint_tape_reserve_sparse_batch``).  ``None`` (the default) is the dense tape."""

    def __init__(self, fs_or_dev, slots=_SLOTS, tape: int | None = None, loop: int | None = None, checkpoint_every: int | str | None = None):
        self.tape = int(tape) if tape else 0
        if self.tape < 0:
            raise ValueError(f"tape must be a number of steps, got {tape!r}")
        self.every = checkpoint_spacing(checkpoint_every, self.tape)
        self.loop = int(loop) if loop else 0  # steps of the closed-loop tape, reserved once a controller bank is on the device
        if self.loop < 0:
            raise ValueError(f"loop must be a number of steps, got {loop!r}")
        self.batch = fs_or_dev if _is_batched(fs_or_dev) else None  # the BatchedFlowSolver whose k runs the marches differentiate
        self.mode = _SINGLE if self.batch is None else _BATCHED  # (the tapes this setup reserves and frees are that mode's)
        self.dev, self.fs = _device_of(fs_or_dev, taped=self.tape > 0)
        dev = self.dev
        if getattr(dev, "world", 1) > 1 or getattr(dev, "part", None) is not None:
            raise ValueError("adjoint_run: partitioned handle -- the transposed factors are built on single-GPU handles")
        if self.fs is not None:
            from .flowsolver import _DeviceNDSolver

            plug = [o for o, sv in self.fs.solvers.items() if not isinstance(sv, _DeviceNDSolver)]
            if plug:
                raise ValueError(f"adjoint_run: the steps of order {plug} run a plug-in solver (_make_solver override), not the device's direct factors")
        self.slots = tuple(int(s) for s in slots)
        self._closed = False
        self._hook = None
        built = []
        try:
            for s in self.slots:
                dev.set_adjoint_factors(s, 1)
                built.append(s)
                if self.batch is not None:
                    dev.set_adjoint_batch(s, 1)
            if self.tape:
                self._reserve_tape(self.tape)
        except Exception:
            for s in built:
                if self.batch is not None:
                    dev.set_adjoint_batch(s, -1)
                dev.set_adjoint_factors(s, -1)
            raise
        hooks = getattr(dev.th, "_release_hooks", None)
        if hooks is None:
            hooks = dev.th._release_hooks = []
        self._hook = self.close
        hooks.append(self._hook)

    def info(self) -> dict:
        """Per slot what ``fc_adjoint_info`` reports, and the device bytes held in all.  ``tape``: ``fc_adjoint_tape_info`` -- of a
        checkpointed tape also ``every`` and ``replayed`` (forward steps the last march recomputed); ``tape_mode`` says which it is.
        On a BatchedFlowSolver ``tape`` is the BATCHED tape's info (``fc_adjoint_tape_info_batch``, with ``KB``) -- the tape such a
        setup reserves; it used to report the single tape's, which a batched setup never holds."""
        per = {s: self.dev.adjoint_info(s) for s in _SLOTS}
        total = sum(v["slot_bytes"] for v in per.values()) + per[SLOT_BDF1]["shared_bytes"]
        tape = self._call(self.mode.tape_info)
        return {"slots": per, "bytes": total, "export_ms": sum(v["export_ms"] for v in per.values()), "tape": tape,
                "tape_mode": "checkpointed" if "every" in tape else ("dense" if tape["capacity"] else None),
                "loop": self.dev.adjoint_loop_info(), "loop_batch": self.dev.adjoint_loop_info_batch()}

    def _call(self, name: str, *args, **kwargs):
        return getattr(self.dev, name)(*args, **kwargs)

    def _reserve_tape(self, capacity: int) -> None:
        """The state tape of this setup's mode and kind, dense or checkpointed; 0 frees it."""
        if self.every:
            self._call(self.mode.tape_reserve_sparse, capacity, self.every if capacity else 0)
        else:
            self._call(self.mode.tape_reserve, capacity)

    def _k(self, who: str, mode):
        """The width of a march or a forward run of ``mode``: None for the single one, else the batch's k (which must be there)."""
        if mode is _SINGLE:
            return None
        if self.batch is None:
            raise ValueError(f"AdjointRun.{who}: set up on a BatchedFlowSolver")
        return self.batch.k

    def _forward_open(self, who: str, mode, u_seq, first_order: int, compute_energy: bool):
        """The open-loop forward run behind :meth:`forward` and :meth:`forward_batch`: ``(y, dE)``, taped if there is a tape."""
        dev, k = self.dev, self._k(who, mode)
        u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(*((-1,) if k is None else (-1, k)), max(dev.n_act, 1)))
        if self.tape:
            if u.shape[0] > self.tape:
                raise ValueError(f"AdjointRun.{who}: {u.shape[0]} steps on a tape of {self.tape}")
            self._call(mode.tape_begin)
        if k is None:
            return dev.run(_slot(first_order), u.shape[0], u, compute_energy=compute_energy)
        return forward_steps_batch(dev, k, u, first_order, compute_energy)

    def _forward_loop(self, who: str, mode, n_steps: int, y0, first_order: int, compute_energy: bool):
        """The closed-loop forward run behind :meth:`forward_closed_loop` and :meth:`forward_closed_loop_batch`: what the device's
        run returns.  The loop tape is reserved here if the bank on the device has none of this capacity."""
        k = self._k(who, mode)
        if not self.loop:
            raise ValueError(f"AdjointRun.{who}: no loop tape -- AdjointRun({'fs_or_dev' if k is None else 'bfs'}, loop=capacity)")
        n = int(n_steps)
        if n > self.loop or (self.tape and n > self.tape):
            raise ValueError(f"AdjointRun.{who}: {n} steps on a tape of {min(self.loop, self.tape or self.loop)}")
        if self._call(mode.loop_info)["capacity"] != self.loop:  # (a new or freed bank: the reserve follows the bank)
            self._call(mode.loop_reserve, self.loop)
        if self.tape:
            self._call(mode.tape_begin)
        self._call(mode.loop_begin)
        return self._call(mode.run_closed_loop, _slot(first_order), n, y0, compute_energy=compute_energy)

    def _march(self, who: str, mode, march: str, n_steps: int, first_order: int, energy, *args, source: int = 0):
        """The backward march behind the four ``run*`` methods -- ``march``: the mode's open-loop or closed-loop one; ``args``: its
        weights, terminal and ``state_gradients`` -- with the energy weights on the handle for its length.  ``source=1`` (single
        marches): the weights multiply the tangent tape's states."""
        k = self._k(who, mode)
        if first_order not in (1, 2):
            raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
        with _held_energy(self.dev, energy_rows(energy, int(n_steps), k), source):
            return self._call(march, _slot(first_order), n_steps, *args)

    def forward(self, u_seq, first_order: int | None = None, compute_energy: bool = True):
        """The forward device run of ``len(u_seq)`` steps from the present state, taped (``fc_adjoint_tape_begin``, then
        :meth:`DeviceSolver.run`): ``(y [n, n_sens], dE [n])``.  ``first_order``: BDF order of the first step (default: a FlowSolver's
        current order, else 2).  :meth:`run` with the same ``n`` and ``first_order`` then marches back over it."""
        if not self.tape:
            raise ValueError("AdjointRun.forward: no state tape -- AdjointRun(fs_or_dev, tape=capacity)")
        return self._forward_open("forward", _SINGLE, u_seq, _first_order(self.fs, first_order), compute_energy)

    def run(self, n_steps: int, w=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None, energy_source: int = 0):
        """One backward march (:meth:`DeviceSolver.run_adjoint`): ``(g [n, n_act], dx0 [N], dxm1 [N])``.  ``first_order``: the BDF
        order (1 or 2) of the FIRST step of the forward run the cost belongs to.  ``energy`` (scalar or ``(n,)``): the cost also holds
        ``sum_m energy[m - 1] dE_m``; the march then reads the state tape of the run (:meth:`forward`) on either kind of solver.
        ``energy_source=1``: the forcing of backward step m is ``energy[m - 1] M dx_m`` with ``dx_m`` from the tangent tape
        (``DeviceSolver.tangent_tape_reserve`` and a tangent march of the same run first): the backward half of
        :func:`flowcontrol_amd.tangent.gauss_newton_product` with ``energy=``."""
        return self._march("run", _SINGLE, _SINGLE.march, n_steps, first_order, energy, w, terminal, state_gradients, source=energy_source)

    def forward_batch(self, u_seq, first_order: int = 2, compute_energy: bool = False):
        """``len(u_seq)`` batched forward steps of the k runs from the present batched state with the controls ``u_seq [n, k, n_act]``,
        taped if this setup has a tape (``fc_adjoint_tape_begin_batch``): ``y [n, k, n_sens]`` -- with ``compute_energy``
        ``(y, dE [n, k])``.  The BatchedFlowSolver's log and counters are not written to."""
        y, dE = self._forward_open("forward_batch", _BATCHED, u_seq, first_order, compute_energy)
        return (y, dE) if compute_energy else y

    def run_batch(self, n_steps: int, w=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None):
        """One batched backward march (:meth:`DeviceSolver.run_adjoint_batch`): ``(g [n, k, n_act], dx0 [k, N], dxm1 [k, N])``.
        ``energy`` (scalar, ``(n,)`` or ``(n, k)``): as :meth:`run`, per column."""
        return self._march("run_batch", _BATCHED, _BATCHED.march, n_steps, first_order, energy, w, terminal, state_gradients)

    def forward_closed_loop(self, n_steps: int, y0, first_order: int | None = None, compute_energy: bool = False):
        """The closed-loop device run of ``n_steps`` steps from the present state with the bank on the device
        (:meth:`DeviceSolver.set_controllers` first), onto the loop tape -- and, if this setup has one, the state tape:
        ``(y [n, n_sens], u [n, n_act], dE [n])``.  ``y0``: the measurement the first controller step reads."""
        return self._forward_loop("forward_closed_loop", _SINGLE, n_steps, y0, _first_order(self.fs, first_order), compute_energy)

    def run_closed_loop_adjoint(self, n_steps: int, w=None, r=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None,
                                energy_source: int = 0) -> dict:
        """One backward march over the taped closed-loop run (:meth:`DeviceSolver.run_adjoint_closed_loop`): the dict of gradients.
        ``energy``, ``energy_source``: as :meth:`run`."""
        return self._march("run_closed_loop_adjoint", _SINGLE, _SINGLE.march_loop, n_steps, first_order, energy, w, r, terminal, state_gradients,
                           source=energy_source)

    def forward_closed_loop_batch(self, n_steps: int, y0, first_order: int = 2, compute_energy: bool = False):
        """The closed-loop run of ``n_steps`` batched steps from the present batched state with the bank of k controllers on the device
        (:meth:`DeviceSolver.set_controllers` first), onto the batched loop tape -- and, if this setup has one, the batched state tape:
        ``(y [n, k, n_sens], u [n, k, n_act], dE [n, k], first_bad_step [k])``.  ``y0`` (k, n_sens): the measurements the first
        controller step reads.  The BatchedFlowSolver's log and counters are not written to."""
        return self._forward_loop("forward_closed_loop_batch", _BATCHED, n_steps, y0, first_order, compute_energy)[:4]

    def run_closed_loop_adjoint_batch(self, n_steps: int, w=None, r=None, terminal=None, first_order: int = 2, state_gradients: bool = True,
                                      energy=None) -> dict:
        """One backward march over the taped run of k closed loops (:meth:`DeviceSolver.run_adjoint_closed_loop_batch`): the dict of
        gradients, every array with a leading k.  ``energy``: as :meth:`run_batch`."""
        return self._march("run_closed_loop_adjoint_batch", _BATCHED, _BATCHED.march_loop, n_steps, first_order, energy, w, r, terminal, state_gradients)

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        hooks = getattr(self.dev.th, "_release_hooks", None)
        if hooks is not None and self._hook in hooks:
            hooks.remove(self._hook)
        if getattr(self.dev, "_h", None):
            if self.tape:
                self._reserve_tape(0)
            if self.loop:
                self._call(self.mode.loop_reserve, 0)
            for s in self.slots:
                if self.batch is not None:
                    self.dev.set_adjoint_batch(s, -1)
                self.dev.set_adjoint_factors(s, -1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run_gradient(fs_or_dev, n_steps: int, w=None, terminal=None, first_order: int | None = None):
    """Gradient of ``J = sum_m w[m - 1] . y_m + terminal . x_n`` over a forward run of ``n_steps`` steps: ``(g, dx0, dxm1)`` with
    ``g[m - 1] = dJ/du_m`` (n_steps, n_act) and the gradients with respect to the two initial time levels (W layout, N each).
    ``first_order``: BDF order of the run's first step (default: a FlowSolver's current order, else 2).  ``fs_or_dev`` may be an
    :class:`AdjointRun` (kept), a FlowSolver or a DeviceSolver (set up and released around the call)."""
    if isinstance(fs_or_dev, AdjointRun):
        return fs_or_dev.run(n_steps, w, terminal, _first_order(fs_or_dev.fs, first_order))
    with AdjointRun(fs_or_dev) as adj:
        return adj.run(n_steps, w, terminal, _first_order(adj.fs, first_order))


def quadratic_cost_gradient(fs, u_seq, Q, R, x0=None, adjoint: AdjointRun | None = None, energy=None, checkpoint_every: int | str | None = None):
    """``J = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` of the forward device run of ``len(u_seq)`` steps from the solver's present state
    (or from ``x0 = (u_n, u_nn[, p_n])``), and its gradient with respect to the control sequence: ``(J, grad [n, n_act])`` with
    ``grad = g + u R^T`` from one backward march weighted by ``w_m = Q y_m``.  The state the run started from is put back, so repeated
    calls evaluate the same horizon (a line search, a finite-difference check); the solver's log is not written to.
    ``adjoint``: an :class:`AdjointRun` to reuse (else one is set up and released).  A nonlinear solver needs one with a state tape of
    at least ``len(u_seq)`` steps (``AdjointRun(fs, tape=n)``): the forward run then goes through :meth:`AdjointRun.forward`.
    ``energy`` (scalar or ``(n,)``): J also holds ``sum_m energy[m - 1] dE_m`` with the forward run's own ``dE`` series; the run is then
    taped on a linearised solver too (a reused ``adjoint`` needs the tape).  ``checkpoint_every`` (int or ``"auto"``): the run is taped
    on a checkpointed tape of that spacing (:class:`AdjointRun`) -- same gradient, bit for bit, in a fraction of the memory, for one more
    forward run; a reused ``adjoint`` must have been set up with it."""
    n_tape = np.asarray(u_seq).shape[0] if (energy is not None or checkpoint_every is not None) else None
    with _adjoint_setup(adjoint, fs, tape=n_tape, checkpoint_every=checkpoint_every) as adj:
        _energy_needs_tape(adj, energy, "quadratic_cost_gradient", "fs, tape=n")
        dev = adj.dev
        u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, dev.n_act))
        n = u.shape[0]
        Qs, Rs = _weights(dev, Q, R)
        order, e = _first_order(adj.fs), energy_rows(energy, n)
        # (a run from x0 started from x0: that is the state put back, and nothing is read from the device)
        with _horizon(dev, _SINGLE, x0=x0, start=None if x0 is None else tuple(x0)):
            if adj.tape:
                y, dE = adj.forward(u, first_order=order, compute_energy=e is not None)
            else:
                y, dE = dev.run(_slot(order), n, u, compute_energy=False)
            g, _, _ = adj.run(n, w=y @ Qs, first_order=order, state_gradients=False, energy=e)
        return float(_cost(_SINGLE, y, u, Qs, Rs, e, dE)), g + u @ Rs


def batched_cost_gradient(bfs, u_seq, Q, R, x0=None, adjoint: AdjointRun | None = None, state_gradient: bool = False, energy=None,
                          checkpoint_every: int | str | None = None):
    """``J_s = 1/2 sum_m (y_{m,s}^T Q y_{m,s} + u_{m,s}^T R u_{m,s})`` of the k runs of a :class:`BatchedFlowSolver` over their NEXT
    ``len(u_seq)`` steps with the controls ``u_seq [n, k, n_act]`` (from their present states, or from ``x0 = (u_n, u_nn[, p_n])`` with
    arrays ``(k, .)``), and the gradients: ``(J [k], grad [n, k, n_act])`` -- with ``state_gradient`` also ``dJ/dx0 [k, N]`` (W layout)
    -- from one batched forward run and ONE batched backward march (``fc_run_adjoint_batch``: the transposed factors are read once per
    step for all k columns).  Works for both kinds of solver: with ``is_eq_nonlinear=True`` the forward run is taped on the device
    (8 N KB bytes per step).  The batched state is put back, so repeated calls evaluate the same horizon; the log is not written to.
    ``adjoint``: an ``AdjointRun(bfs[, tape=n])`` to reuse (else one is set up and released).  ``energy`` (scalar, ``(n,)`` or
    ``(n, k)``): ``J_s`` also holds ``sum_m energy[m - 1, s] dE_{m,s}`` with the forward run's own ``dE``; the run is then taped on a
    linearised solver too.  ``checkpoint_every`` (int or ``"auto"``): where a tape is kept it is a checkpointed one
    (:class:`AdjointRun`); a reused ``adjoint`` must have been set up with it."""
    u = np.asarray(u_seq, dtype=np.float64)
    n = u.shape[0]
    tape, every = _tape_for(bfs.fs, n, energy, checkpoint_every)
    with _adjoint_setup(adjoint, bfs, tape=tape, checkpoint_every=every) as adj:
        if adj.batch is not bfs:
            raise ValueError("batched_cost_gradient: the AdjointRun must be set up on this BatchedFlowSolver")
        _energy_needs_tape(adj, energy, "batched_cost_gradient", "bfs, tape=n")
        dev, k = adj.dev, bfs.k
        u = np.ascontiguousarray(u.reshape(n, k, dev.n_act))
        Qs, Rs = _weights(dev, Q, R)
        order, e = _first_order(bfs), energy_rows(energy, n, k)
        with _horizon(dev, _BATCHED, flush=bfs._flush, x0=x0):
            y, dE = adj._forward_open("forward_batch", _BATCHED, u, order, e is not None)
            g, dx0, _ = adj.run_batch(n, w=y @ Qs, first_order=order, state_gradients=state_gradient, energy=e)
        J, grad = _cost(_BATCHED, y, u, Qs, Rs, e, dE), g + u @ Rs
        return (J, grad, dx0) if state_gradient else (J, grad)


def _controller_gradients(g, controller, size, dt: float, s: int | None = None) -> dict:
    """The gradients of one controller out of a closed-loop march's dict ``g`` -- of run ``s`` of a batched one -- cut from the
    zero-padded bank to the controller's own ``size = (nstates, noutputs)``, with ``A, B`` of its continuous-time form."""
    nxc, p = size
    at = (lambda q: g[q]) if s is None else (lambda q: g[q][s])
    rows = (lambda q: g[q]) if s is None else (lambda q: g[q][:, s])
    d = {"Ad": at("Ad")[:nxc, :nxc], "Bd": at("Bd")[:nxc], "C": at("C")[:p, :nxc], "D": at("D")[:p], "G": at("G"), "g0": at("g0"), "S": at("S")[:, :p],
         "x0": at("x0")[:nxc], "y0": at("y0"), "w_y": rows("w_y"), "w_u": rows("w_u")}
    d["A"], d["B"] = controller.discrete_gradient(dt, d["Ad"], d["Bd"])
    return d


def closed_loop_gradient(fs, controller, n_steps: int, Q, R, feedback=None, w_y=None, w_u=None, u_limits=None, adjoint: AdjointRun | None = None,
                         energy=None, checkpoint_every: int | str | None = None):
    """``J = 1/2 sum_m (y_m^T Q y_m + u_m^T R u_m)`` of the closed loop of ``fs`` with the LTI ``controller`` over the NEXT ``n_steps``
    steps (the loop of :meth:`FlowSolver.run_closed_loop`: ``feedback``, ``w_y``, ``w_u``, ``u_limits`` as there; ``u`` is the clamped
    control), and its gradient: ``(J, grads)`` from one forward closed-loop run and one backward march on the device.  ``grads`` holds
    ``Ad, Bd, C, D`` (the discrete controller stepped at the solver's ``dt``), ``G, g0`` (feedback map), ``S`` (fan-out to the
    actuators), ``x0`` (the controller's initial state), ``y0`` (the first measurement), ``w_y`` (n, nyc), ``w_u`` (n, n_act), and
    ``A, B`` of the continuous-time controller (:meth:`Controller.discrete_gradient`; ``C`` and ``D`` are the same in both forms).
    Where a limit clamps a control value the gradient does not pass through it.  The flow state and the controller state are put
    back, so repeated calls evaluate the same horizon; the solver's log is not written to.  ``adjoint``: an :class:`AdjointRun` with
    ``loop >= n_steps`` (and, for a nonlinear solver, ``tape >= n_steps``) to reuse; else one is set up and released.  ``energy``
    (scalar or ``(n,)``): J also holds ``sum_m energy[m - 1] dE_m`` with the closed loop's own ``dE`` series; the run is then taped on
    a linearised solver too (a reused ``adjoint`` needs ``tape >= n_steps``).  ``checkpoint_every`` (int or ``"auto"``): the state tape
    is a checkpointed one of that spacing (:class:`AdjointRun`): the horizon is bounded by the loop tape's few rows per step, not by
    8 N bytes per step; the replayed segments read the taped controls, no controller runs again."""
    from .controller import Controller, loop_limits, loop_signal_rows

    if not isinstance(controller, Controller):
        raise TypeError("closed_loop_gradient differentiates an LTI Controller")
    n = int(n_steps)
    tape, every = _tape_for(fs, n, energy, checkpoint_every)
    with _adjoint_setup(adjoint, fs, tape=tape, loop=n, checkpoint_every=every) as adj:
        dev = adj.dev
        if adj.fs is None:
            raise ValueError("closed_loop_gradient: the AdjointRun must be set up on the FlowSolver")
        _energy_needs_tape(adj, energy, "closed_loop_gradient", "fs, tape=n, loop=n")
        e = energy_rows(energy, n)
        dt, na = fs.params_time.dt, dev.n_act
        Qs, Rs = _weights(dev, Q, R)
        bank = ([controller], dt, feedback, loop_signal_rows(w_y, n, (controller.ninputs,), "w_y"), loop_signal_rows(w_u, n, (na,), "w_u"),
                loop_limits(u_limits, (1, na)))
        order = _first_order(adj.fs)
        with _horizon(dev, _SINGLE, bank=bank) as packed:
            y0 = np.asarray(fs.y_meas, dtype=np.float64).reshape(dev.n_sens).copy()
            y, u, dE = adj.forward_closed_loop(n, y0, first_order=order, compute_energy=e is not None)
            g = adj.run_closed_loop_adjoint(n, w=y @ Qs, r=u @ Rs, first_order=order, state_gradients=False, energy=e)
        return float(_cost(_SINGLE, y, u, Qs, Rs, e, dE)), _controller_gradients(g, controller, packed["sizes"][0], dt)


def batched_closed_loop_gradient(bfs, controllers, n_steps: int, Q, R, feedback=None, w_y=None, w_u=None, u_limits=None, adjoint: AdjointRun | None = None,
                                 energy=None, checkpoint_every: int | str | None = None):
    """``J_s = 1/2 sum_m (y_{m,s}^T Q y_{m,s} + u_{m,s}^T R u_{m,s})`` of the k closed loops of a :class:`BatchedFlowSolver` --
    ``controllers[s]`` (LTI ``Controller``) around run s -- over their NEXT ``n_steps`` steps (the loop of
    :meth:`BatchedFlowSolver.run_closed_loop`: ``feedback``, ``w_y``, ``w_u``, ``u_limits`` as there), and the gradients of every loop:
    ``(J [k], grads)`` from one batched forward run and ONE batched backward march (``fc_run_adjoint_closed_loop_batch``).  ``grads`` is
    a list of k dicts with the keys of :func:`closed_loop_gradient`, each cut to its controller's own size (controllers of different
    orders share the zero-padded bank).  The batched state and the controllers' states are put back, so repeated calls evaluate the
    same horizon; the log is not written to.  ``adjoint``: an ``AdjointRun(bfs, loop=n[, tape=n])`` to reuse (``tape`` for a nonlinear
    solver); else one is set up and released.  ``energy`` (scalar, ``(n,)`` or ``(n, k)``): ``J_s`` also holds
    ``sum_m energy[m - 1, s] dE_{m,s}`` with the loops' own ``dE`` series; the run is then taped on a linearised solver too.
    ``checkpoint_every`` (int or ``"auto"``): where a state tape is kept it is a checkpointed one (:class:`AdjointRun`) -- the tapes of
    wide batches over long horizons in bounded memory; a reused ``adjoint`` must have been set up with it."""
    from .controller import Controller, loop_limits, loop_signal_rows_batch

    controllers = list(controllers)
    if len(controllers) != bfs.k:
        raise ValueError(f"expected {bfs.k} controllers, got {len(controllers)}")
    if not all(isinstance(K, Controller) for K in controllers):
        raise TypeError("batched_closed_loop_gradient differentiates LTI Controllers")
    if bfs.order == "cn":
        raise ValueError("batched_closed_loop_gradient: time_scheme='cn' -- the backward march is the adjoint of the BDF stepper")
    n = int(n_steps)
    tape, every = _tape_for(bfs.fs, n, energy, checkpoint_every)
    with _adjoint_setup(adjoint, bfs, tape=tape, loop=n, checkpoint_every=every) as adj:
        if adj.batch is not bfs:
            raise ValueError("batched_closed_loop_gradient: the AdjointRun must be set up on this BatchedFlowSolver")
        _energy_needs_tape(adj, energy, "batched_closed_loop_gradient", "bfs, tape=n, loop=n")
        dev, k = adj.dev, bfs.k
        e = energy_rows(energy, n, k)
        dt, na = bfs.params_time.dt, dev.n_act
        Qs, Rs = _weights(dev, Q, R)
        bank = (controllers, dt, feedback, loop_signal_rows_batch(w_y, n, k, controllers[0].ninputs, "w_y"), loop_signal_rows_batch(w_u, n, k, na, "w_u"),
                loop_limits(u_limits, (k, na)))
        order = _first_order(bfs)
        with _horizon(dev, _BATCHED, flush=bfs._flush, bank=bank) as packed:
            y0 = np.where(bfs.diverged[:, None], 0.0, np.asarray(bfs.y_meas, dtype=np.float64).reshape(k, dev.n_sens))
            y, u, dE, _ = adj.forward_closed_loop_batch(n, y0, first_order=order, compute_energy=e is not None)
            g = adj.run_closed_loop_adjoint_batch(n, w=y @ Qs, r=u @ Rs, first_order=order, state_gradients=False, energy=e)
        return _cost(_BATCHED, y, u, Qs, Rs, e, dE), [_controller_gradients(g, K, packed["sizes"][s], dt, s) for s, K in enumerate(controllers)]


__all__ = ["AdjointRun", "run_gradient", "quadratic_cost_gradient", "batched_cost_gradient", "closed_loop_gradient", "batched_closed_loop_gradient"]
