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
"""

from __future__ import annotations

import math

import numpy as np

from ._lib import SLOT_BDF1, SLOT_BDF2

_SLOTS = (SLOT_BDF1, SLOT_BDF2)


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
    """The weights on the handle for the length of a march; cleared on the way out, whatever way that is."""

    def __init__(self, dev, rows):
        self.dev, self.rows = dev, rows

    def __enter__(self):
        if self.rows is not None:
            self.dev.set_adjoint_energy(self.rows)

    def __exit__(self, exc_type, exc, tb):
        if self.rows is None:
            return False
        try:
            self.dev.set_adjoint_energy(None)
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
                if self.batch is not None and self.every:
                    dev.adjoint_tape_reserve_sparse_batch(self.tape, self.every)
                elif self.batch is not None:
                    dev.adjoint_tape_reserve_batch(self.tape)
                elif self.every:
                    dev.adjoint_tape_reserve_sparse(self.tape, self.every)
                else:
                    dev.adjoint_tape_reserve(self.tape)
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
        tape = self.dev.adjoint_tape_info_batch() if self.batch is not None else self.dev.adjoint_tape_info()
        return {"slots": per, "bytes": total, "export_ms": sum(v["export_ms"] for v in per.values()), "tape": tape,
                "tape_mode": "checkpointed" if "every" in tape else ("dense" if tape["capacity"] else None),
                "loop": self.dev.adjoint_loop_info(), "loop_batch": self.dev.adjoint_loop_info_batch()}

    def forward(self, u_seq, first_order: int | None = None, compute_energy: bool = True):
        """The forward device run of ``len(u_seq)`` steps from the present state, taped (``fc_adjoint_tape_begin``, then
        :meth:`DeviceSolver.run`): ``(y [n, n_sens], dE [n])``.  ``first_order``: BDF order of the first step (default: a FlowSolver's
        current order, else 2).  :meth:`run` with the same ``n`` and ``first_order`` then marches back over it."""
        if not self.tape:
            raise ValueError("AdjointRun.forward: no state tape -- AdjointRun(fs_or_dev, tape=capacity)")
        u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, max(self.dev.n_act, 1)))
        if u.shape[0] > self.tape:
            raise ValueError(f"AdjointRun.forward: {u.shape[0]} steps on a tape of {self.tape}")
        order = _first_order(self.fs, first_order)
        self.dev.adjoint_tape_begin()
        return self.dev.run(SLOT_BDF1 if order == 1 else SLOT_BDF2, u.shape[0], u, compute_energy=compute_energy)

    def run(self, n_steps: int, w=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None):
        """One backward march (:meth:`DeviceSolver.run_adjoint`): ``(g [n, n_act], dx0 [N], dxm1 [N])``.  ``first_order``: the BDF
        order (1 or 2) of the FIRST step of the forward run the cost belongs to.  ``energy`` (scalar or ``(n,)``): the cost also holds
        ``sum_m energy[m - 1] dE_m``; the march then reads the state tape of the run (:meth:`forward`) on either kind of solver."""
        if first_order not in (1, 2):
            raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
        with _held_energy(self.dev, energy_rows(energy, int(n_steps))):
            return self.dev.run_adjoint(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n_steps, w, terminal, state_gradients)

    def forward_batch(self, u_seq, first_order: int = 2, compute_energy: bool = False):
        """``len(u_seq)`` batched forward steps of the k runs from the present batched state with the controls ``u_seq [n, k, n_act]``,
        taped if this setup has a tape (``fc_adjoint_tape_begin_batch``): ``y [n, k, n_sens]`` -- with ``compute_energy``
        ``(y, dE [n, k])``.  The BatchedFlowSolver's log and counters are not written to."""
        if self.batch is None:
            raise ValueError("AdjointRun.forward_batch: set up on a BatchedFlowSolver")
        dev, k = self.dev, self.batch.k
        u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, k, max(dev.n_act, 1)))
        if self.tape:
            if u.shape[0] > self.tape:
                raise ValueError(f"AdjointRun.forward_batch: {u.shape[0]} steps on a tape of {self.tape}")
            dev.adjoint_tape_begin_batch()
        y, dE = np.empty((u.shape[0], k, dev.n_sens)), np.empty((u.shape[0], k))
        for m in range(u.shape[0]):
            y[m], dE[m], _ = dev.step_batch(SLOT_BDF1 if (m == 0 and first_order == 1) else SLOT_BDF2, u[m], compute_energy=bool(compute_energy))
        return (y, dE) if compute_energy else y

    def run_batch(self, n_steps: int, w=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None):
        """One batched backward march (:meth:`DeviceSolver.run_adjoint_batch`): ``(g [n, k, n_act], dx0 [k, N], dxm1 [k, N])``.
        ``energy`` (scalar, ``(n,)`` or ``(n, k)``): as :meth:`run`, per column."""
        if self.batch is None:
            raise ValueError("AdjointRun.run_batch: set up on a BatchedFlowSolver")
        if first_order not in (1, 2):
            raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
        with _held_energy(self.dev, energy_rows(energy, int(n_steps), self.batch.k)):
            return self.dev.run_adjoint_batch(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n_steps, w, terminal, state_gradients)

    def forward_closed_loop(self, n_steps: int, y0, first_order: int | None = None, compute_energy: bool = False):
        """The closed-loop device run of ``n_steps`` steps from the present state with the bank on the device
        (:meth:`DeviceSolver.set_controllers` first), onto the loop tape -- and, if this setup has one, the state tape:
        ``(y [n, n_sens], u [n, n_act], dE [n])``.  ``y0``: the measurement the first controller step reads."""
        if not self.loop:
            raise ValueError("AdjointRun.forward_closed_loop: no loop tape -- AdjointRun(fs_or_dev, loop=capacity)")
        n = int(n_steps)
        if n > self.loop or (self.tape and n > self.tape):
            raise ValueError(f"AdjointRun.forward_closed_loop: {n} steps on a tape of {min(self.loop, self.tape or self.loop)}")
        if self.dev.adjoint_loop_info()["capacity"] != self.loop:  # (a new or freed bank: the reserve follows the bank)
            self.dev.adjoint_loop_reserve(self.loop)
        order = _first_order(self.fs, first_order)
        if self.tape:
            self.dev.adjoint_tape_begin()
        self.dev.adjoint_loop_begin()
        return self.dev.run_closed_loop(SLOT_BDF1 if order == 1 else SLOT_BDF2, n, y0, compute_energy=compute_energy)

    def run_closed_loop_adjoint(self, n_steps: int, w=None, r=None, terminal=None, first_order: int = 2, state_gradients: bool = True, energy=None) -> dict:
        """One backward march over the taped closed-loop run (:meth:`DeviceSolver.run_adjoint_closed_loop`): the dict of gradients.
        ``energy``: as :meth:`run`."""
        if first_order not in (1, 2):
            raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
        with _held_energy(self.dev, energy_rows(energy, int(n_steps))):
            return self.dev.run_adjoint_closed_loop(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n_steps, w, r, terminal, state_gradients)

    def forward_closed_loop_batch(self, n_steps: int, y0, first_order: int = 2, compute_energy: bool = False):
        """The closed-loop run of ``n_steps`` batched steps from the present batched state with the bank of k controllers on the device
        (:meth:`DeviceSolver.set_controllers` first), onto the batched loop tape -- and, if this setup has one, the batched state tape:
        ``(y [n, k, n_sens], u [n, k, n_act], dE [n, k], first_bad_step [k])``.  ``y0`` (k, n_sens): the measurements the first
        controller step reads.  The BatchedFlowSolver's log and counters are not written to."""
        if self.batch is None:
            raise ValueError("AdjointRun.forward_closed_loop_batch: set up on a BatchedFlowSolver")
        if not self.loop:
            raise ValueError("AdjointRun.forward_closed_loop_batch: no loop tape -- AdjointRun(bfs, loop=capacity)")
        n = int(n_steps)
        if n > self.loop or (self.tape and n > self.tape):
            raise ValueError(f"AdjointRun.forward_closed_loop_batch: {n} steps on a tape of {min(self.loop, self.tape or self.loop)}")
        dev = self.dev
        if dev.adjoint_loop_info_batch()["capacity"] != self.loop:  # (a new or freed bank: the reserve follows the bank)
            dev.adjoint_loop_reserve_batch(self.loop)
        if self.tape:
            dev.adjoint_tape_begin_batch()
        dev.adjoint_loop_begin_batch()
        y, u, dE, bad, _ = dev.run_closed_loop_batch(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n, y0, compute_energy=compute_energy)
        return y, u, dE, bad

    def run_closed_loop_adjoint_batch(self, n_steps: int, w=None, r=None, terminal=None, first_order: int = 2, state_gradients: bool = True,
                                      energy=None) -> dict:
        """One backward march over the taped run of k closed loops (:meth:`DeviceSolver.run_adjoint_closed_loop_batch`): the dict of
        gradients, every array with a leading k.  ``energy``: as :meth:`run_batch`."""
        if self.batch is None:
            raise ValueError("AdjointRun.run_closed_loop_adjoint_batch: set up on a BatchedFlowSolver")
        if first_order not in (1, 2):
            raise ValueError(f"first_order must be 1 or 2, got {first_order!r}")
        with _held_energy(self.dev, energy_rows(energy, int(n_steps), self.batch.k)):
            return self.dev.run_adjoint_closed_loop_batch(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n_steps, w, r, terminal, state_gradients)

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        hooks = getattr(self.dev.th, "_release_hooks", None)
        if hooks is not None and self._hook in hooks:
            hooks.remove(self._hook)
        if getattr(self.dev, "_h", None):
            if self.tape:
                if self.batch is not None and self.every:
                    self.dev.adjoint_tape_reserve_sparse_batch(0, 0)
                elif self.batch is not None:
                    self.dev.adjoint_tape_reserve_batch(0)
                elif self.every:
                    self.dev.adjoint_tape_reserve_sparse(0, 0)
                else:
                    self.dev.adjoint_tape_reserve(0)
            if self.loop:
                if self.batch is not None:
                    self.dev.adjoint_loop_reserve_batch(0)
                else:
                    self.dev.adjoint_loop_reserve(0)
            for s in self.slots:
                if self.batch is not None:
                    self.dev.set_adjoint_batch(s, -1)
                self.dev.set_adjoint_factors(s, -1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _first_order(fs, first_order):
    if first_order is not None:
        return int(first_order)
    return 1 if (fs is not None and fs.order == 1) else 2


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
    own = adjoint is None
    n_tape = np.asarray(u_seq).shape[0] if (energy is not None or checkpoint_every is not None) else None
    adj = _adjoint_for(adjoint, checkpoint_every, lambda: AdjointRun(fs, tape=n_tape, checkpoint_every=checkpoint_every))
    try:
        if energy is not None and not adj.tape:
            raise ValueError("quadratic_cost_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape (AdjointRun(fs, tape=n))")
        dev, fso = adj.dev, adj.fs
        u = np.ascontiguousarray(np.asarray(u_seq, dtype=np.float64).reshape(-1, dev.n_act))
        n = u.shape[0]
        Q = np.asarray(Q, dtype=np.float64).reshape(dev.n_sens, dev.n_sens)
        R = np.asarray(R, dtype=np.float64).reshape(dev.n_act, dev.n_act)
        start = dev.get_state() if x0 is None else tuple(x0)
        if x0 is not None:
            dev.set_state(*start)
        order = _first_order(fso, None)
        e = energy_rows(energy, n)
        if adj.tape:
            y, dE = adj.forward(u, first_order=order, compute_energy=e is not None)
        else:
            y, dE = dev.run(SLOT_BDF1 if order == 1 else SLOT_BDF2, n, u, compute_energy=False)
        g, _, _ = adj.run(n, w=y @ (0.5 * (Q + Q.T)), first_order=order, state_gradients=False, energy=e)
        dev.set_state(*start)
        J = 0.5 * (np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", u, R, u))
        if e is not None:
            J = J + float(e @ dE)
        return float(J), g + u @ (0.5 * (R + R.T))
    finally:
        if own:
            adj.close()


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
    own = adjoint is None
    taped = bfs.fs.params_solver.is_eq_nonlinear or energy is not None
    adj = _adjoint_for(adjoint, checkpoint_every if taped else None,
                       lambda: AdjointRun(bfs, tape=n if taped else None, checkpoint_every=checkpoint_every if taped else None))
    try:
        if adj.batch is not bfs:
            raise ValueError("batched_cost_gradient: the AdjointRun must be set up on this BatchedFlowSolver")
        if energy is not None and not adj.tape:
            raise ValueError("batched_cost_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape (AdjointRun(bfs, tape=n))")
        dev, k = adj.dev, bfs.k
        u = np.ascontiguousarray(u.reshape(n, k, dev.n_act))
        Qs = np.asarray(Q, dtype=np.float64).reshape(dev.n_sens, dev.n_sens)
        Rs = np.asarray(R, dtype=np.float64).reshape(dev.n_act, dev.n_act)
        Qs, Rs = 0.5 * (Qs + Qs.T), 0.5 * (Rs + Rs.T)
        bfs._flush()
        start = dev.get_state_batch()
        order = 1 if getattr(bfs, "order", 2) == 1 else 2
        e = energy_rows(energy, n, k)
        try:
            if x0 is not None:
                dev.set_state_batch(*x0)
            if e is not None:
                y, dE = adj.forward_batch(u, first_order=order, compute_energy=True)
            else:
                y = adj.forward_batch(u, first_order=order)
            g, dx0, _ = adj.run_batch(n, w=y @ Qs, first_order=order, state_gradients=state_gradient, energy=e)
        finally:
            dev.set_state_batch(*start)
        J = 0.5 * (np.einsum("mki,ij,mkj->k", y, Qs, y) + np.einsum("mki,ij,mkj->k", u, Rs, u))
        if e is not None:
            J = J + np.einsum("mk,mk->k", e, dE)
        grad = g + u @ Rs
        return (J, grad, dx0) if state_gradient else (J, grad)
    finally:
        if own:
            adj.close()


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
    own = adjoint is None
    taped = fs.params_solver.is_eq_nonlinear or energy is not None
    adj = _adjoint_for(adjoint, checkpoint_every if taped else None,
                       lambda: AdjointRun(fs, tape=n if taped else None, loop=n, checkpoint_every=checkpoint_every if taped else None))
    try:
        dev, fso = adj.dev, adj.fs
        if fso is None:
            raise ValueError("closed_loop_gradient: the AdjointRun must be set up on the FlowSolver")
        if energy is not None and not adj.tape:
            raise ValueError("closed_loop_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape (AdjointRun(fs, tape=n, loop=n))")
        e = energy_rows(energy, n)
        dt = fs.params_time.dt
        ns, na = dev.n_sens, dev.n_act
        Qs = np.asarray(Q, dtype=np.float64).reshape(ns, ns)
        Rs = np.asarray(R, dtype=np.float64).reshape(na, na)
        Qs, Rs = 0.5 * (Qs + Qs.T), 0.5 * (Rs + Rs.T)
        wy = loop_signal_rows(w_y, n, (controller.ninputs,), "w_y")
        wu = loop_signal_rows(w_u, n, (na,), "w_u")
        limits = loop_limits(u_limits, (1, na))
        order = _first_order(fso, None)
        start = dev.get_state()
        y0 = np.asarray(fs.y_meas, dtype=np.float64).reshape(ns).copy()
        bank = dev.set_controllers([controller], dt, feedback)  # (reads controller.x; the host object is not advanced)
        try:
            if wy is not None or wu is not None:
                dev.set_loop_signals(wy, wu)
            if limits is not None:
                dev.set_control_limits(*limits)
            y, u, dE = adj.forward_closed_loop(n, y0, first_order=order, compute_energy=e is not None)
            g = adj.run_closed_loop_adjoint(n, w=y @ Qs, r=u @ Rs, first_order=order, state_gradients=False, energy=e)
        finally:
            try:
                dev.set_state(*start)
            finally:
                dev.set_controllers(None, dt)
        J = 0.5 * (np.einsum("mi,ij,mj->", y, Qs, y) + np.einsum("mi,ij,mj->", u, Rs, u))
        if e is not None:
            J = J + float(e @ dE)
        nxc, p = bank["sizes"][0]
        grads = {"Ad": g["Ad"][:nxc, :nxc], "Bd": g["Bd"][:nxc], "C": g["C"][:p, :nxc], "D": g["D"][:p], "G": g["G"], "g0": g["g0"], "S": g["S"][:, :p],
                 "x0": g["x0"][:nxc], "y0": g["y0"], "w_y": g["w_y"], "w_u": g["w_u"]}
        grads["A"], grads["B"] = controller.discrete_gradient(dt, grads["Ad"], grads["Bd"])
        return float(J), grads
    finally:
        if own:
            adj.close()


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
    own = adjoint is None
    taped = bfs.fs.params_solver.is_eq_nonlinear or energy is not None
    adj = _adjoint_for(adjoint, checkpoint_every if taped else None,
                       lambda: AdjointRun(bfs, tape=n if taped else None, loop=n, checkpoint_every=checkpoint_every if taped else None))
    try:
        if adj.batch is not bfs:
            raise ValueError("batched_closed_loop_gradient: the AdjointRun must be set up on this BatchedFlowSolver")
        if energy is not None and not adj.tape:
            raise ValueError("batched_closed_loop_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape "
                             "(AdjointRun(bfs, tape=n, loop=n))")
        e = energy_rows(energy, n, bfs.k)
        dev, k = adj.dev, bfs.k
        dt = bfs.params_time.dt
        ns, na = dev.n_sens, dev.n_act
        Qs = np.asarray(Q, dtype=np.float64).reshape(ns, ns)
        Rs = np.asarray(R, dtype=np.float64).reshape(na, na)
        Qs, Rs = 0.5 * (Qs + Qs.T), 0.5 * (Rs + Rs.T)
        wy = loop_signal_rows_batch(w_y, n, k, controllers[0].ninputs, "w_y")
        wu = loop_signal_rows_batch(w_u, n, k, na, "w_u")
        limits = loop_limits(u_limits, (k, na))
        bfs._flush()
        order = 1 if bfs.order == 1 else 2
        start = dev.get_state_batch()
        y0 = np.where(bfs.diverged[:, None], 0.0, np.asarray(bfs.y_meas, dtype=np.float64).reshape(k, ns))
        bank = dev.set_controllers(controllers, dt, feedback)  # (reads every controller.x; the host objects are not advanced)
        try:
            if wy is not None or wu is not None:
                dev.set_loop_signals(wy, wu)
            if limits is not None:
                dev.set_control_limits(*limits)
            y, u, dE, _ = adj.forward_closed_loop_batch(n, y0, first_order=order, compute_energy=e is not None)
            g = adj.run_closed_loop_adjoint_batch(n, w=y @ Qs, r=u @ Rs, first_order=order, state_gradients=False, energy=e)
        finally:
            try:
                dev.set_state_batch(*start)
            finally:
                dev.set_controllers(None, dt)
        J = 0.5 * (np.einsum("mki,ij,mkj->k", y, Qs, y) + np.einsum("mki,ij,mkj->k", u, Rs, u))
        if e is not None:
            J = J + np.einsum("mk,mk->k", e, dE)
        grads = []
        for s, K in enumerate(controllers):
            nxc, p = bank["sizes"][s]
            d = {"Ad": g["Ad"][s, :nxc, :nxc], "Bd": g["Bd"][s, :nxc], "C": g["C"][s, :p, :nxc], "D": g["D"][s, :p], "G": g["G"][s], "g0": g["g0"][s],
                 "S": g["S"][s][:, :p], "x0": g["x0"][s, :nxc], "y0": g["y0"][s], "w_y": g["w_y"][:, s], "w_u": g["w_u"][:, s]}
            d["A"], d["B"] = K.discrete_gradient(dt, d["Ad"], d["Bd"])
            grads.append(d)
        return J, grads
    finally:
        if own:
            adj.close()


__all__ = ["AdjointRun", "run_gradient", "quadratic_cost_gradient", "batched_cost_gradient", "closed_loop_gradient", "batched_closed_loop_gradient"]
