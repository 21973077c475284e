"""Host stand-ins for the gradient drivers (``flowcontrol_amd/adjoint.py``, ``flowcontrol_amd/tangent.py``): a device that records
every call made on it, and the two solver objects the drivers accept.  No GPU, no library.

:class:`RecordingDevice` answers the public ``DeviceSolver`` methods the drivers use.  Each call is appended to ``calls`` as
``(name, args, kwargs)`` with arrays frozen by value (:func:`frozen`), and returns arrays of the shapes the real method returns,
filled with fixed, strictly positive dyadic entries (:func:`filled`): no cost sum built from them cancels and every product is
reproducible bit for bit.  The little state it keeps is what the drivers read back: the fill of the state tape, the capacity of the
loop tape, whether the tangent buffers are reserved, the controller bank.  ``fail = {name: i}`` makes the i-th call of ``name``
raise :class:`Marker` after it has been recorded.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np


class Marker(Exception):
    """What a call named in ``RecordingDevice.fail`` raises."""


def frozen(v):
    """``v`` as a literal that compares by value: arrays become ``("f8", shape, [flat values])``; tuples, lists and dicts are walked;
    anything that is neither data nor a container is named by its type."""
    if isinstance(v, np.ndarray):
        return ("f8" if v.dtype == np.float64 else str(v.dtype), tuple(v.shape), v.ravel().tolist())
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if isinstance(v, (tuple, list)):
        return tuple(frozen(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, frozen(x)) for k, x in sorted(v.items()))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return f"<{type(v).__name__}>"


def filled(name: str, *shape):
    """A float64 array of ``shape`` with entries in [1, 2), multiples of 1/16, fixed by ``name`` and the position."""
    salt = sum(name.encode())
    size = int(np.prod(shape, dtype=np.int64))
    return (1.0 + ((np.arange(size) * 7 + salt) % 16) / 16.0).reshape(shape)


class RecordingDevice:
    _RECORD_ONLY = ("set_adjoint_factors", "set_adjoint_batch", "set_adjoint_energy", "adjoint_loop_begin", "adjoint_loop_begin_batch",
                    "set_loop_signals", "set_control_limits")

    def __init__(self, N: int = 6, n_sens: int = 2, n_act: int = 1, batch_k: int = 0):
        self.N, self.n_sens, self.n_act, self.batch_k = N, n_sens, n_act, batch_k
        self.nn, self.nv = N // 3, N - 2 * (N // 3)
        self.world, self.part = 1, None
        self.th = SimpleNamespace()
        self._h = 1
        self.calls: list = []
        self.fail: dict = {}
        self._seen: dict = {}
        self._ctrl_bank = None
        self._tape = {False: self._no_tape(), True: self._no_tape()}  # (batched?) -> the state tape's fill
        self._loop = {False: 0, True: 0}
        self._tangent = False

    @staticmethod
    def _no_tape():
        return {"capacity": 0, "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0}

    def _rec(self, name, *args, **kwargs):
        self.calls.append((name, frozen(args), frozen(kwargs)))
        self._seen[name] = self._seen.get(name, 0) + 1
        if self.fail.get(name) == self._seen[name]:
            raise Marker(name)

    def __getattr__(self, name):
        if name in RecordingDevice._RECORD_ONLY:
            return lambda *a, **kw: self._rec(name, *a, **kw)
        raise AttributeError(name)

    # ── state ──
    def get_state(self):
        self._rec("get_state")
        return filled("u_n", 2 * self.nn), filled("u_nn", 2 * self.nn), filled("p_n", self.nv)

    def get_state_batch(self):
        self._rec("get_state_batch")
        k = self.batch_k
        return filled("u_n", k, 2 * self.nn), filled("u_nn", k, 2 * self.nn), filled("p_n", k, self.nv)

    def set_state(self, *state):
        self._tape[False]["begun"] = False
        self._rec("set_state", *state)

    def set_state_batch(self, *state):
        self._tape[True]["begun"] = False
        self._rec("set_state_batch", *state)

    # ── tapes ──
    def _reserve(self, batched, name, capacity, *every):
        self._tape[batched] = dict(self._no_tape(), capacity=int(capacity), **({"every": every[0], "replayed": 0} if every and every[0] else {}))
        self._rec(name, capacity, *every)

    def adjoint_tape_reserve(self, capacity):
        self._reserve(False, "adjoint_tape_reserve", capacity)

    def adjoint_tape_reserve_sparse(self, capacity, every):
        self._reserve(False, "adjoint_tape_reserve_sparse", capacity, every)

    def adjoint_tape_reserve_batch(self, capacity):
        self._reserve(True, "adjoint_tape_reserve_batch", capacity)

    def adjoint_tape_reserve_sparse_batch(self, capacity, every):
        self._reserve(True, "adjoint_tape_reserve_sparse_batch", capacity, every)

    def adjoint_tape_begin(self):
        self._tape[False].update(begun=True, count=0)
        self._rec("adjoint_tape_begin")

    def adjoint_tape_begin_batch(self):
        self._tape[True].update(begun=True, count=0)
        self._rec("adjoint_tape_begin_batch")

    def adjoint_tape_info(self):
        self._rec("adjoint_tape_info")
        return dict(self._tape[False])

    def adjoint_tape_info_batch(self):
        self._rec("adjoint_tape_info_batch")
        return dict(self._tape[True], KB=self.batch_k)

    def adjoint_loop_reserve(self, capacity):
        self._loop[False] = int(capacity)
        self._rec("adjoint_loop_reserve", capacity)

    def adjoint_loop_reserve_batch(self, capacity):
        self._loop[True] = int(capacity)
        self._rec("adjoint_loop_reserve_batch", capacity)

    def _loop_info(self, batched):
        return {"capacity": self._loop[batched], "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0,
                "bad": 0 if batched else False, "row": 0}

    def adjoint_loop_info(self):
        self._rec("adjoint_loop_info")
        return self._loop_info(False)

    def adjoint_loop_info_batch(self):
        self._rec("adjoint_loop_info_batch")
        return self._loop_info(True)

    def adjoint_info(self, slot):
        self._rec("adjoint_info", slot)
        return {"available": True, "slot_bytes": 64, "shared_bytes": 32, "export_ms": 0.5}

    def tangent_reserve(self, on=1):
        self._tangent = bool(on)
        self._rec("tangent_reserve", on)

    def tangent_info(self):
        self._rec("tangent_info")
        return {"reserved": self._tangent, "KB": self.batch_k, "bytes": 0, "steps": 0, "route": 0, "marches": 0, "run_ms": 0.0}

    # ── the controller bank (a new or freed bank drops the loop tapes, as on the device) ──
    def set_controllers(self, controllers, dt, feedback=None):
        from flowcontrol_amd.controller import pack_controllers

        self._loop = {False: 0, True: 0}
        self._rec("set_controllers", None if controllers is None else len(controllers), dt, feedback)
        self._ctrl_bank = pack_controllers(controllers, dt, self.n_sens, self.n_act, feedback) if controllers else None
        return self._ctrl_bank

    # ── forward runs ──
    def _taped(self, batched, n):
        if self._tape[batched]["begun"]:
            self._tape[batched]["count"] += n

    def run(self, slot, n, u, compute_energy=True):
        self._rec("run", slot, n, u, compute_energy=compute_energy)
        self._taped(False, n)
        return filled("y", n, self.n_sens), filled("dE", n)

    def step_batch(self, slot, u, compute_energy=True, u_force=None):
        self._rec("step_batch", slot, u, compute_energy=compute_energy)
        self._taped(True, 1)
        k, m = self.batch_k, self._seen["step_batch"]
        return filled(f"y{m}", k, self.n_sens), filled(f"dE{m}", k), None

    def run_closed_loop(self, slot, n, y0, compute_energy=True):
        self._rec("run_closed_loop", slot, n, y0, compute_energy=compute_energy)
        self._taped(False, n)
        return filled("y", n, self.n_sens), filled("u", n, self.n_act), filled("dE", n)

    def run_closed_loop_batch(self, slot, n, y0, compute_energy=True):
        self._rec("run_closed_loop_batch", slot, n, y0, compute_energy=compute_energy)
        self._taped(True, n)
        k = self.batch_k
        return filled("y", n, k, self.n_sens), filled("u", n, k, self.n_act), filled("dE", n, k), np.full(k, -1, dtype=np.int32), np.zeros((k, 4))

    # ── marches ──
    def _pair(self, on, *shape):
        return (filled("dx0", *shape), filled("dxm1", *shape)) if on else (None, None)

    def run_adjoint(self, slot, n, w=None, terminal=None, state_gradients=True):
        self._rec("run_adjoint", slot, n, w, terminal, state_gradients)
        return (filled("g", int(n), self.n_act), *self._pair(state_gradients, self.N))

    def run_adjoint_batch(self, slot, n, w=None, terminal=None, state_gradients=True):
        self._rec("run_adjoint_batch", slot, n, w, terminal, state_gradients)
        return (filled("g", int(n), self.batch_k, self.n_act), *self._pair(state_gradients, self.batch_k, self.N))

    def _loop_gradients(self, n, lead, state_gradients):
        b, ns, na = self._ctrl_bank, self.n_sens, self.n_act
        nx, nyc, nuc = b["nx"], b["nyc"], b["nuc"]
        shapes = {"Ad": (nx, nx), "Bd": (nx, nyc), "C": (nuc, nx), "D": (nuc, nyc), "G": (nyc, ns), "g0": (nyc,), "S": (na, nuc), "x0": (nx,), "y0": (ns,)}
        out = {q: filled(q, *lead, *s) for q, s in shapes.items()}
        out.update({q: filled(q, n, *lead, w) for q, w in (("w_y", nyc), ("w_u", na), ("ubar", na))})
        out["dx0"], out["dxm1"] = self._pair(state_gradients, *lead, self.N)
        return out

    def run_adjoint_closed_loop(self, slot, n, w=None, r=None, terminal=None, state_gradients=True):
        self._rec("run_adjoint_closed_loop", slot, n, w, r, terminal, state_gradients)
        return self._loop_gradients(int(n), (), state_gradients)

    def run_adjoint_closed_loop_batch(self, slot, n, w=None, r=None, terminal=None, state_gradients=True):
        self._rec("run_adjoint_closed_loop_batch", slot, n, w, r, terminal, state_gradients)
        return self._loop_gradients(int(n), (self.batch_k,), state_gradients)

    def run_tangent(self, slot, n, du=None, dx0=None, dxm1=None):
        self._rec("run_tangent", slot, n, du, dx0, dxm1)
        return filled("dy", int(n), self.n_sens), filled("dxn", self.N), filled("dxnm1", self.N)

    def run_tangent_batch(self, slot, n, du=None, dx0=None, dxm1=None, ref_col=None):
        self._rec("run_tangent_batch", slot, n, du, dx0, dxm1, ref_col)
        k = self.batch_k
        return filled("dy", int(n), k, self.n_sens), filled("dxn", k, self.N), filled("dxnm1", k, self.N)


def fake_flowsolver(dev: RecordingDevice, nonlinear: bool = False, order: int = 2, dt: float = 0.125):
    """What the drivers read of a FlowSolver, on ``dev``; ``_begin_stepping`` and ``_flush_log`` are recorded in ``dev.calls``."""
    dev.th.device = lambda: dev
    return SimpleNamespace(th=dev.th, params_solver=SimpleNamespace(is_eq_nonlinear=nonlinear, time_scheme="bdf"), params_time=SimpleNamespace(dt=dt),
                           solvers={}, order=order, y_meas=filled("y_meas", dev.n_sens),
                           _begin_stepping=lambda: dev._rec("fs._begin_stepping"), _flush_log=lambda: dev._rec("fs._flush_log"))


def fake_batched(dev: RecordingDevice, nonlinear: bool = False, order=2, dt: float = 0.125):
    """A BatchedFlowSolver that never ran its ``__init__``: the attributes the drivers read, and a recorded ``_flush``."""
    from flowcontrol_amd.batch import BatchedFlowSolver

    bfs = object.__new__(BatchedFlowSolver)
    bfs.k, bfs.dev, bfs._ready, bfs.order = dev.batch_k, dev, True, order
    bfs.fs = fake_flowsolver(dev, nonlinear, 2 if order == "cn" else order, dt)
    bfs.diverged = np.zeros(dev.batch_k, dtype=bool)
    bfs.y_meas = filled("y_meas", dev.batch_k, dev.n_sens)
    bfs.params_time = bfs.fs.params_time
    bfs._flush = lambda: dev._rec("bfs._flush")
    return bfs
