"""The gradient drivers of ``flowcontrol_amd/adjoint.py`` and ``flowcontrol_amd/tangent.py`` on a recording device (CPU only).

The seven drivers -- ``quadratic_cost_gradient``, ``batched_cost_gradient``, ``closed_loop_gradient``, ``batched_closed_loop_gradient``,
``tangent_run``, ``batched_tangent_run``, ``gauss_newton_product`` -- launch nothing themselves: what they own is the ORDER of the device
calls (save the state, load ``x0``, bank on, tapes begun, forward, march, state back, bank off, release).  ``tests/support/recording_device.py``
records that order with every array argument; ``EXPECTED``, at the bottom of this file, holds the traces and the returned values of the
code as it stood BEFORE the drivers were folded onto one skeleton, so the comparison is against that code, not against the code under
test.

All inputs are small dyadic rationals (multiples of 1/16, weights multiples of 1/8): every product and sum the drivers form on the host
is exact in float64, so the recorded numbers do not depend on the order of a summation or on the BLAS at hand.  The one exception,
``A`` / ``B`` of the closed-loop gradients, goes through a matrix exponential; it is checked against ``Controller.discrete_gradient`` of
the pinned ``Ad`` / ``Bd`` instead of against a literal.

Two behaviours differ from the recorded code on purpose and have test functions of their own:
``test_quadratic_cost_gradient_puts_the_state_back_when_a_run_raises`` and ``test_quadratic_cost_uses_the_symmetric_part``.
"""

from __future__ import annotations

import numpy as np
import pytest

from flowcontrol_amd import adjoint as adj_mod
from flowcontrol_amd import tangent as tan_mod
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from flowcontrol_amd.adjoint import AdjointRun
from flowcontrol_amd.controller import Controller
from tests.support.recording_device import Marker, RecordingDevice, fake_batched, fake_flowsolver, filled, frozen

N, NS, NA, NSTEPS, K, EVERY, DT = 6, 2, 1, 3, 3, 2, 0.125
Q = np.array([[2.0, 0.5], [0.25, 3.0]])  # (not symmetric: the symmetric part is what the weights use)
R = np.array([[0.75]])
BATCHED = ("bcg", "bclg", "btan")
LOOPED = ("clg", "bclg")
TANGENT = ("tan", "btan")
FORWARD = {"qcg": "run", "bcg": "step_batch", "clg": "run_closed_loop", "bclg": "run_closed_loop_batch", "tan": "run", "btan": "step_batch", "gnp": "run"}
MARCH = {"qcg": "run_adjoint", "bcg": "run_adjoint_batch", "clg": "run_adjoint_closed_loop", "bclg": "run_adjoint_closed_loop_batch",
         "tan": "run_tangent", "btan": "run_tangent_batch", "gnp": "run_adjoint"}


def controllers(k):
    two = lambda s: Controller([[-1.0, 0.5], [0.0, -2.0 - s]], [[1.0], [0.5]], [[1.0, 0.25]], [[0.125]], x0=np.array([0.25, 0.5]))  # noqa: E731
    one = Controller([[-1.5]], [[1.0]], [[0.5]], [[0.25]])  # (a smaller one: the bank is zero-padded, the gradients are cut back)
    return [two(0.0), one, two(0.5)][:k]


def make(kind, nonlinear=False, order=2):
    """(device, solver) for a driver: the batched drivers get a BatchedFlowSolver of K runs."""
    dev = RecordingDevice(N, NS, NA, K if kind in BATCHED else 0)
    return dev, (fake_batched if kind in BATCHED else fake_flowsolver)(dev, nonlinear, order, DT)


def call(kind, solver, adjoint=None, **kw):
    """One call of the driver ``kind`` with this file's inputs; ``kw`` goes to the driver."""
    lead = (NSTEPS, K) if kind in BATCHED else (NSTEPS,)
    u = filled("u_seq", *lead, NA)
    if kind == "qcg":
        return adj_mod.quadratic_cost_gradient(solver, u, Q, R, adjoint=adjoint, **kw)
    if kind == "bcg":
        return adj_mod.batched_cost_gradient(solver, u, Q, R, adjoint=adjoint, **kw)
    if kind == "clg":
        return adj_mod.closed_loop_gradient(solver, kw.pop("controller", controllers(1)[0]), NSTEPS, Q, R, adjoint=adjoint, **kw)
    if kind == "bclg":
        return adj_mod.batched_closed_loop_gradient(solver, kw.pop("controllers", controllers(K)), NSTEPS, Q, R, adjoint=adjoint, **kw)
    if kind == "tan":
        return tan_mod.tangent_run(solver, u, filled("du", *lead, NA), filled("dx0", N), filled("dxm1", N), **kw)
    if kind == "btan":
        return tan_mod.batched_tangent_run(solver, u, filled("du", *lead, NA), filled("dx0", K, N), filled("dxm1", K, N), **kw)
    assert kind == "gnp"
    return tan_mod.gauss_newton_product(solver, u, Q, R, filled("v", NSTEPS, NA), adjoint=adjoint)


def x0_of(kind):
    lead = (K,) if kind in BATCHED else ()
    return filled("x0a", *lead, 4), filled("x0b", *lead, 4), filled("x0c", *lead, 2)


def _cases():
    """name -> (kind, solver options, AdjointRun options of a reused setup or None, driver options, prime the tape first)."""
    c = {}
    for who in ("own", "reused"):
        r = who == "reused"
        for kind in ("qcg", "bcg", "clg", "bclg"):
            loop = {"loop": NSTEPS} if kind in LOOPED else {}
            tape = dict(loop, tape=NSTEPS)
            c[f"{kind}-{who}-plain"] = (kind, {}, loop if r else None, {}, False)
            c[f"{kind}-{who}-order1"] = (kind, {"order": 1}, loop if r else None, {}, False)
            c[f"{kind}-{who}-energy"] = (kind, {}, tape if r else None, {"energy": 0.5}, False)
            c[f"{kind}-{who}-nonlinear-ckpt"] = (kind, {"nonlinear": True}, dict(tape, checkpoint_every=EVERY) if r else None, {"checkpoint_every": EVERY}, False)
            if kind != "qcg" or r:  # (quadratic_cost_gradient tapes only on request: its own setup on a nonlinear solver is a refusal)
                c[f"{kind}-{who}-nonlinear"] = (kind, {"nonlinear": True}, tape if r else None, {}, False)
            if kind in ("qcg", "bcg"):
                c[f"{kind}-{who}-x0"] = (kind, {}, loop if r else None, {"x0": x0_of(kind)}, False)
                c[f"{kind}-{who}-energy-ckpt"] = (kind, {}, dict(tape, checkpoint_every=EVERY) if r else None, {"energy": 0.5, "checkpoint_every": EVERY}, False)
            else:
                lead = (NSTEPS, K) if kind == "bclg" else (NSTEPS,)
                sig = {"feedback": (np.array([[-1.0, 0.5]]), np.array([0.25])), "w_y": filled("w_y", *lead, 1), "w_u": filled("w_u", *lead, NA), "u_limits": (-2.0, 2.0)}
                c[f"{kind}-{who}-signals"] = (kind, {}, loop if r else None, sig, False)
        c[f"bcg-{who}-state-gradient"] = ("bcg", {}, {} if r else None, {"state_gradient": True}, False)
        c[f"bcg-{who}-cn"] = ("bcg", {"order": "cn"}, {} if r else None, {}, False)  # (a "cn" batch still starts on the BDF2 slot)
        c[f"gnp-{who}-taped-here"] = ("gnp", {"nonlinear": True}, {"tape": NSTEPS} if r else None, {}, False)
        c[f"gnp-{who}-order1"] = ("gnp", {"nonlinear": True, "order": 1}, {"tape": NSTEPS} if r else None, {}, False)
    c["gnp-reused-tape-holds-the-run"] = ("gnp", {"nonlinear": True}, {"tape": NSTEPS}, {}, True)
    c["gnp-reused-longer-tape"] = ("gnp", {"nonlinear": True}, {"tape": NSTEPS + 2}, {}, False)
    for kind in TANGENT:
        c[f"{kind}-plain"] = (kind, {"nonlinear": True}, None, {}, False)
        c[f"{kind}-order1"] = (kind, {"nonlinear": True, "order": 1}, None, {}, False)
        c[f"{kind}-first-order-given"] = (kind, {"nonlinear": True}, None, {"first_order": 1}, False)
    c["btan-ref-col"] = ("btan", {"nonlinear": True}, None, {"ref_col": 1}, False)
    c["btan-cn"] = ("btan", {"nonlinear": True, "order": "cn"}, None, {}, False)
    return c


CASES = _cases()


def run_case(name):
    """(trace, frozen result, the reused AdjointRun or None) of one case."""
    kind, opts, reuse, kw, prime = CASES[name]
    dev, solver = make(kind, **opts)
    adjoint = None if reuse is None else AdjointRun(solver, **reuse)
    if prime:
        adjoint.forward(filled("u_seq", NSTEPS, NA), compute_energy=False)
    del dev.calls[:]
    out = call(kind, solver, adjoint, **dict(kw))
    return list(dev.calls), frozen(out), adjoint


def without_AB(result):
    """The frozen result of a closed-loop driver with ``A`` and ``B`` taken out of every gradient dict (checked on their own)."""
    J, grads = result
    cut = lambda d: tuple(kv for kv in d if kv[0] not in ("A", "B"))  # noqa: E731
    return (J, cut(grads)) if grads and isinstance(grads[0][0], str) else (J, tuple(cut(d) for d in grads))


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_trace_and_values(name):
    kind = CASES[name][0]
    trace, result, adjoint = run_case(name)
    want_trace, want = EXPECTED[name]
    assert trace == want_trace
    if adjoint is not None:
        assert not adjoint._closed  # (a setup passed in is the caller's to release)
    if kind in LOOPED:
        result, want = without_AB(result), without_AB(want)
    if kind == "qcg":  # (J: the symmetric part of Q regroups a sum of 15 positive products -- far inside 1e-13 of it)
        assert result[0] == pytest.approx(want[0], rel=1e-13, abs=0.0)
        result, want = result[1:], want[1:]
    assert result == want


@pytest.mark.parametrize("kind", LOOPED)
def test_continuous_gradients_come_from_the_cut_discrete_ones(kind):
    """``A``, ``B``: ``Controller.discrete_gradient`` at the solver's dt of each controller's own cut of ``Ad``, ``Bd``."""
    dev, solver = make(kind)
    Ks = controllers(K if kind == "bclg" else 1)
    _, grads = call(kind, solver, **({"controllers": Ks} if kind == "bclg" else {"controller": Ks[0]}))
    for ctrl, g in zip(Ks, grads if kind == "bclg" else [grads]):
        assert g["Ad"].shape == (ctrl.nstates, ctrl.nstates) and g["Bd"].shape == (ctrl.nstates, 1)
        A, B = ctrl.discrete_gradient(DT, g["Ad"], g["Bd"])
        assert np.array_equal(g["A"], A) and np.array_equal(g["B"], B)


# ── AdjointRun: what the constructor and close() put on the handle, in which order ──────────────────────────────────────────────────
SETUPS = {f"{'batched' if b else 'single'}-{tape}{'-loop' if loop else ''}": (b, tape, loop)
          for b in (False, True) for tape in ("no-tape", "dense", "checkpointed") for loop in (False, True)}


def run_setup(name):
    b, tape, loop = SETUPS[name]
    dev, solver = make("bcg" if b else "qcg", nonlinear=tape != "no-tape")
    kw = {} if tape == "no-tape" else {"tape": NSTEPS, **({"checkpoint_every": EVERY} if tape == "checkpointed" else {})}
    run = AdjointRun(solver, loop=NSTEPS if loop else None, **kw)
    built = len(dev.calls)
    assert dev.th._release_hooks == [run.close]
    info = run.info()
    del dev.calls[built:]
    run.close()
    run.close()  # (a second close does nothing)
    assert dev.th._release_hooks == []
    return list(dev.calls[:built]), list(dev.calls[built:]), frozen(info)


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_adjoint_run_setup_and_close(name):
    assert run_setup(name) == EXPECTED["setup-" + name]


def test_adjoint_run_takes_back_what_it_built_when_the_reserve_fails():
    dev, bfs = make("bcg", nonlinear=True)
    dev.fail = {"adjoint_tape_reserve_sparse_batch": 1}
    with pytest.raises(Marker):
        AdjointRun(bfs, tape=NSTEPS, checkpoint_every=EVERY)
    tail = [(c[0], c[1]) for c in dev.calls[-4:]]
    assert tail == [(f, (s, -1)) for s in (SLOT_BDF1, SLOT_BDF2) for f in ("set_adjoint_batch", "set_adjoint_factors")]
    assert not hasattr(dev.th, "_release_hooks")


def test_forward_batch_taped():
    """``tangent.forward_batch_taped`` on a BatchedFlowSolver and on a bare device: the same step loop, taping begun first."""
    for bare in (False, True):
        dev, bfs = make("btan", nonlinear=True)
        y = tan_mod.forward_batch_taped(dev if bare else bfs, filled("u_seq", NSTEPS, K, NA), first_order=1)
        assert (list(dev.calls), frozen(y)) == EXPECTED["forward-batch-taped-" + ("device" if bare else "solver")]


# ── failure paths ───────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _names(calls):
    return [c[0] for c in calls]


def check_exit_path(kind, dev, adjoint, failed, start, tangent_was_reserved=False):
    """After a driver raised out of the call named ``failed``: the state ``start`` went back, then the bank came off, then the tapes
    this call reserved were freed, and an owned AdjointRun was closed last -- a reused one not at all."""
    calls, names = dev.calls, _names(dev.calls)
    setter = "set_state_batch" if kind in BATCHED else "set_state"
    at = len(names) - 1 - names[::-1].index(failed)  # the failing call (the last of that name)
    if failed != setter:
        back = [i for i in range(at + 1, len(calls)) if calls[i][:2] == (setter, start)]
        assert len(back) == 1, f"the start state is put back once after {failed} raised"
        at = back[0]
    if kind in LOOPED:
        assert calls[at + 1] == ("set_controllers", (None, DT, None), ()), "the bank comes off right after the state went back"
        at += 1
    if kind in TANGENT:
        rest = [c[:2] for c in calls[at + 1:]]
        free = ("adjoint_tape_reserve_batch" if kind in BATCHED else "adjoint_tape_reserve", (0,))
        assert rest == [free], "the tape this call reserved is freed after the state went back"
        assert (("tangent_reserve", (0,)) in [c[:2] for c in calls]) == (not tangent_was_reserved)
        return
    released = [i for i, c in enumerate(calls) if c[0] == "set_adjoint_factors" and c[1][1] == -1]
    if adjoint is None:  # this call's own setup: closed last, after the state and the bank
        assert released and released[0] > at and calls[-1][:2] == ("set_adjoint_factors", (SLOT_BDF2, -1))
        assert set(names[at + 1:]) <= {"adjoint_tape_reserve", "adjoint_tape_reserve_batch", "adjoint_tape_reserve_sparse", "adjoint_tape_reserve_sparse_batch",
                                       "adjoint_loop_reserve", "adjoint_loop_reserve_batch", "set_adjoint_batch", "set_adjoint_factors"}
    else:
        assert not released and not adjoint._closed
        assert len(calls) == at + 1


def fail_in(kind, failed, reused, tangent_was_reserved=False, **kw):
    nonlinear = kind in TANGENT or kind == "gnp"
    dev, solver = make(kind, nonlinear=nonlinear)
    adjoint = None
    if reused and kind not in TANGENT:
        adjoint = AdjointRun(solver, tape=NSTEPS if nonlinear else None, loop=NSTEPS if kind in LOOPED else None)
    if tangent_was_reserved:
        dev.tangent_reserve(1)
    del dev.calls[:]
    dev.fail = {failed: dev._seen.get(failed, 0) + (2 if (failed.startswith("set_state") and "x0" in kw) else 1)}
    with pytest.raises(Marker, match=f"^{failed}$"):
        call(kind, solver, adjoint, **kw)
    dev.fail = {}
    trace = list(dev.calls)
    start = kw["x0"] if (kind == "qcg" and "x0" in kw) else (dev.get_state_batch if kind in BATCHED else dev.get_state)()
    dev.calls[:] = trace  # (quadratic_cost_gradient with x0 runs from x0 and leaves the solver there: that is its start state)
    check_exit_path(kind, dev, adjoint, failed, frozen(tuple(start)), tangent_was_reserved)


SIX = ("bcg", "clg", "bclg", "tan", "btan", "gnp")


@pytest.mark.parametrize("kind, stage, reused", [(kind, stage, reused) for kind in SIX for stage in ("forward", "march", "setter")
                                                 for reused in ((False,) if kind in TANGENT else (False, True))])  # (the tangent runs take no AdjointRun)
def test_exit_path_when_a_device_call_raises(kind, stage, reused):
    setter = "set_state_batch" if kind in BATCHED else "set_state"
    fail_in(kind, {"forward": FORWARD[kind], "march": MARCH[kind], "setter": setter}[stage], reused)


@pytest.mark.parametrize("kind", TANGENT + ("gnp",))
@pytest.mark.parametrize("was_reserved", (False, True), ids=("reserves", "reserved-before"))
def test_tangent_buffers_are_freed_by_the_call_that_reserved_them(kind, was_reserved):
    dev, solver = make(kind, nonlinear=True)
    if was_reserved:
        dev.tangent_reserve(1)
    del dev.calls[:]
    dev.fail = {"run_tangent_batch" if kind == "btan" else "run_tangent": 1}
    with pytest.raises(Marker):
        call(kind, solver)
    assert (("tangent_reserve", (0,), ()) in dev.calls) == (not was_reserved)
    assert dev._tangent == was_reserved


@pytest.mark.parametrize("reused", (False, True), ids=("own", "reused"))
def test_quadratic_cost_gradient_exit_path_when_the_state_setter_raises(reused):
    fail_in("qcg", "set_state", reused)
    fail_in("qcg", "set_state", reused, x0=x0_of("qcg"))


@pytest.mark.parametrize("reused", (False, True), ids=("own", "reused"))
@pytest.mark.parametrize("stage", ("forward", "march"))
def test_quadratic_cost_gradient_puts_the_state_back_when_a_run_raises(stage, reused):
    """Deliberate change 1: the code recorded in ``EXPECTED`` left the solver on the state the failed run reached."""
    fail_in("qcg", {"forward": FORWARD, "march": MARCH}[stage]["qcg"], reused)
    fail_in("qcg", {"forward": FORWARD, "march": MARCH}[stage]["qcg"], reused, x0=x0_of("qcg"))


def test_quadratic_cost_uses_the_symmetric_part():
    """Deliberate change 2: ``J`` is formed with the symmetric parts of ``Q`` and ``R``, the ones the weights use (the recorded code
    used ``Q`` as given: the same number but for the grouping of the sum -- exactly the same with this file's dyadic inputs)."""
    dev, fs = make("qcg")
    J, _ = call("qcg", fs)
    y, u = filled("y", NSTEPS, NS), filled("u_seq", NSTEPS, NA)
    Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    assert J == 0.5 * (np.einsum("mi,ij,mj->", y, Qs, y) + np.einsum("mi,ij,mj->", u, Rs, u))
    assert J == pytest.approx(EXPECTED["qcg-own-plain"][1][0], rel=1e-13, abs=0.0)


# ── refusals: raised before the device is touched, with these words ─────────────────────────────────────────────────────────────
def test_first_order_must_be_1_or_2():
    dev, fs = make("qcg")
    dev_b, bfs = make("bcg")
    run, run_b = AdjointRun(fs, tape=NSTEPS, loop=NSTEPS), AdjointRun(bfs, tape=NSTEPS, loop=NSTEPS)
    before = len(dev.calls), len(dev_b.calls)
    for march in (run.run, run.run_closed_loop_adjoint, run_b.run_batch, run_b.run_closed_loop_adjoint_batch):
        with pytest.raises(ValueError, match=r"^first_order must be 1 or 2, got 3$"):
            march(NSTEPS, first_order=3)
    assert (len(dev.calls), len(dev_b.calls)) == before


def test_forward_needs_its_tape():
    dev, fs = make("qcg")
    dev_b, bfs = make("bcg")
    run, run_b = AdjointRun(fs), AdjointRun(bfs)
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward: no state tape -- AdjointRun\(fs_or_dev, tape=capacity\)$"):
        run.forward(filled("u", NSTEPS, NA))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop: no loop tape -- AdjointRun\(fs_or_dev, loop=capacity\)$"):
        run.forward_closed_loop(NSTEPS, filled("y0", NS))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop_batch: no loop tape -- AdjointRun\(bfs, loop=capacity\)$"):
        run_b.forward_closed_loop_batch(NSTEPS, filled("y0", K, NS))


def test_more_steps_than_the_tape_holds():
    dev, fs = make("qcg")
    dev_b, bfs = make("bcg")
    run, run_b = AdjointRun(fs, tape=2, loop=NSTEPS), AdjointRun(bfs, tape=2, loop=NSTEPS)
    short, short_b = AdjointRun(fs, loop=1), AdjointRun(bfs, loop=1)
    before = len(dev.calls), len(dev_b.calls)
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward: 3 steps on a tape of 2$"):
        run.forward(filled("u", NSTEPS, NA))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_batch: 3 steps on a tape of 2$"):
        run_b.forward_batch(filled("u", NSTEPS, K, NA))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop: 3 steps on a tape of 2$"):
        run.forward_closed_loop(NSTEPS, filled("y0", NS))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop_batch: 3 steps on a tape of 2$"):
        run_b.forward_closed_loop_batch(NSTEPS, filled("y0", K, NS))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop: 3 steps on a tape of 1$"):
        short.forward_closed_loop(NSTEPS, filled("y0", NS))
    with pytest.raises(ValueError, match=r"^AdjointRun\.forward_closed_loop_batch: 3 steps on a tape of 1$"):
        short_b.forward_closed_loop_batch(NSTEPS, filled("y0", K, NS))
    assert (len(dev.calls), len(dev_b.calls)) == before


def test_batched_methods_need_a_batched_solver():
    dev, fs = make("qcg")
    run = AdjointRun(fs, tape=NSTEPS, loop=NSTEPS)
    before = len(dev.calls)
    for name, args in (("forward_batch", (filled("u", NSTEPS, K, NA),)), ("run_batch", (NSTEPS,)), ("forward_closed_loop_batch", (NSTEPS, filled("y0", K, NS))),
                       ("run_closed_loop_adjoint_batch", (NSTEPS,))):
        with pytest.raises(ValueError, match=rf"^AdjointRun\.{name}: set up on a BatchedFlowSolver$"):
            getattr(run, name)(*args)
    assert len(dev.calls) == before
    dev_b, bfs = make("bcg")
    dev_c, other = make("bcg")
    with pytest.raises(ValueError, match=r"^batched_cost_gradient: the AdjointRun must be set up on this BatchedFlowSolver$"):
        call("bcg", bfs, AdjointRun(other))
    with pytest.raises(ValueError, match=r"^batched_closed_loop_gradient: the AdjointRun must be set up on this BatchedFlowSolver$"):
        call("bclg", bfs, AdjointRun(other, loop=NSTEPS))
    with pytest.raises(ValueError, match=r"^closed_loop_gradient: the AdjointRun must be set up on the FlowSolver$"):
        call("clg", fs, AdjointRun(dev, loop=NSTEPS))


@pytest.mark.parametrize("kind, words", (
    ("qcg", r"quadratic_cost_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape \(AdjointRun\(fs, tape=n\)\)"),
    ("bcg", r"batched_cost_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape \(AdjointRun\(bfs, tape=n\)\)"),
    ("clg", r"closed_loop_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape \(AdjointRun\(fs, tape=n, loop=n\)\)"),
    ("bclg", r"batched_closed_loop_gradient: energy= reads the forward trajectory -- the AdjointRun needs a state tape \(AdjointRun\(bfs, tape=n, loop=n\)\)")))
def test_energy_needs_a_tape(kind, words):
    dev, solver = make(kind)
    run = AdjointRun(solver, loop=NSTEPS if kind in LOOPED else None)
    before = len(dev.calls)
    with pytest.raises(ValueError, match=f"^{words}$"):
        call(kind, solver, run, energy=0.5)
    assert len(dev.calls) == before and not run._closed


@pytest.mark.parametrize("kind", ("qcg", "bcg", "clg", "bclg"))
def test_checkpoint_every_must_be_the_reused_setups(kind):
    dev, solver = make(kind, nonlinear=True)
    run = AdjointRun(solver, tape=NSTEPS, loop=NSTEPS if kind in LOOPED else None, checkpoint_every=EVERY)
    dense = AdjointRun(solver, tape=NSTEPS, loop=NSTEPS if kind in LOOPED else None)
    before = len(dev.calls)
    with pytest.raises(ValueError, match=r"^checkpoint_every=3, but the AdjointRun passed in was set up with checkpoint_every=2$"):
        call(kind, solver, run, checkpoint_every=3)
    with pytest.raises(ValueError, match=r"^checkpoint_every=2, but the AdjointRun passed in was set up with checkpoint_every=None$"):
        call(kind, solver, dense, checkpoint_every=EVERY)
    assert len(dev.calls) == before
    with pytest.raises(ValueError, match=r"^checkpoint_every needs a state tape \(tape=n_steps\)$"):
        AdjointRun(solver, checkpoint_every=EVERY)
    with pytest.raises(ValueError, match=r"^checkpoint_every must be a positive int or 'auto', got 0$"):
        AdjointRun(solver, tape=NSTEPS, checkpoint_every=0)


def test_gauss_newton_product_needs_a_dense_tape():
    words = (r"^gauss_newton_product: the AdjointRun needs a dense state tape \(AdjointRun\(fs, tape=n\)\); a tangent march over a checkpointed tape "
             r"is not built$")
    dev, fs = make("gnp", nonlinear=True)
    for run in (AdjointRun(fs, tape=NSTEPS, checkpoint_every=EVERY), AdjointRun(dev)):
        before = len(dev.calls)
        with pytest.raises(ValueError, match=words):
            call("gnp", fs, run)
        assert len(dev.calls) == before and not run._closed
    dev, fs = make("gnp", nonlinear=False)
    with pytest.raises(ValueError, match=r"^gauss_newton_product: is_eq_nonlinear=False -- the forward run of the linearised stepper is its own tangent"):
        call("gnp", fs)
    assert dev.calls[-1][:2] == ("set_adjoint_factors", (SLOT_BDF2, -1))  # (the setup this call made is released)


def test_nonlinear_solver_needs_a_tape():
    dev, fs = make("qcg", nonlinear=True)
    with pytest.raises(ValueError, match=r"^adjoint_run: is_eq_nonlinear=True -- the adjoint of the nonlinear stepper reads the forward trajectory"):
        call("qcg", fs)
    assert dev.calls == []


def test_cn_is_refused():
    dev, fs = make("qcg")
    fs.params_solver.time_scheme = "cn"
    with pytest.raises(ValueError, match=r"^adjoint_run: time_scheme='cn' -- the backward march is the adjoint of the BDF stepper \(order 2\)$"):
        call("qcg", fs)
    for kind, who in (("tan", "tangent_run"), ("btan", "batched_tangent_run")):
        dev, solver = make(kind, nonlinear=True)
        (solver.fs if kind == "btan" else solver).params_solver.time_scheme = "cn"
        with pytest.raises(ValueError, match=r"^adjoint_run: time_scheme='cn'"):  # (the shared conditions of the handle come first)
            call(kind, solver)
    with pytest.raises(ValueError, match=r"^tangent_run: time_scheme='cn' -- the tangent march is that of the BDF stepper$"):
        tan_mod._check_tangent(solver.fs, "tangent_run")
    dev, bfs = make("bclg", order="cn")
    with pytest.raises(ValueError, match=r"^batched_closed_loop_gradient: time_scheme='cn' -- the backward march is the adjoint of the BDF stepper$"):
        call("bclg", bfs)
    assert dev.calls == []


def test_tangent_runs_refuse_a_linearised_solver():
    for kind, who in (("tan", "tangent_run"), ("btan", "batched_tangent_run")):
        dev, solver = make(kind, nonlinear=False)
        with pytest.raises(ValueError, match=rf"^{who}: is_eq_nonlinear=False -- the forward run of the linearised stepper is its own tangent: step the perturbation$"):
            call(kind, solver)
        assert not [c for c in dev.calls if not c[0].startswith(("fs.", "bfs."))]


def test_controllers_are_counted_and_typed():
    dev, bfs = make("bclg")
    with pytest.raises(ValueError, match=r"^expected 3 controllers, got 2$"):
        call("bclg", bfs, controllers=controllers(2))
    with pytest.raises(TypeError, match=r"^batched_closed_loop_gradient differentiates LTI Controllers$"):
        call("bclg", bfs, controllers=controllers(2) + [object()])
    dev1, fs = make("clg")
    with pytest.raises(TypeError, match=r"^closed_loop_gradient differentiates an LTI Controller$"):
        call("clg", fs, controller=object())
    assert dev.calls == [] and dev1.calls == []


def test_energy_rows_shapes():
    with pytest.raises(ValueError, match=r"^energy must be a scalar, \(3,\), got \(2,\)$"):
        adj_mod.energy_rows(np.ones(2), NSTEPS)
    with pytest.raises(ValueError, match=r"^energy must be a scalar, \(3,\) or \(3, 3\), got \(3, 2\)$"):
        adj_mod.energy_rows(np.ones((3, 2)), NSTEPS, K)


# ── the recorded traces and values (see the module docstring: taken from the code before the drivers shared a skeleton) ────────
# fmt: off
EXPECTED = {'bcg-own-cn': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                 ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                 ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                 ('run_adjoint_batch',
                  (1, 3,
                   ('f8', (3, 3, 2),
                    [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875, 3.6484375,
                     3.796875, 3.7265625, 6.375]),
                   None, False),
                  ()),
                 ('set_state_batch',
                  (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                   ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                   ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                  ()),
                 ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                 ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-energy': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                     ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                     ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', True),)),
                     ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', True),)),
                     ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                     ('run_adjoint_batch',
                      (1, 3,
                       ('f8', (3, 3, 2),
                        [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                         3.6484375, 3.796875, 3.7265625, 6.375]),
                       None, False),
                      ()),
                     ('set_adjoint_energy', (None,), ()),
                     ('set_state_batch',
                      (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                       ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                       ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                      ()),
                     ('adjoint_tape_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                     ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (('f8', (3,), [21.4091796875, 22.98681640625, 29.5068359375]),
                     ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-energy-ckpt': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                          ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_sparse_batch', (3, 2), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                          ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                          ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', True),)),
                          ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', True),)),
                          ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                          ('run_adjoint_batch',
                           (1, 3,
                            ('f8', (3, 3, 2),
                             [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                              3.6484375, 3.796875, 3.7265625, 6.375]),
                            None, False),
                           ()),
                          ('set_adjoint_energy', (None,), ()),
                          ('set_state_batch',
                           (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                            ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                            ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                           ()),
                          ('adjoint_tape_reserve_sparse_batch', (0, 0), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                          ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                         (('f8', (3,), [21.4091796875, 22.98681640625, 29.5068359375]),
                          ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-nonlinear': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                        ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                        ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                        ('run_adjoint_batch',
                         (1, 3,
                          ('f8', (3, 3, 2),
                           [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                            3.6484375, 3.796875, 3.7265625, 6.375]),
                          None, False),
                         ()),
                        ('set_state_batch',
                         (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                          ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                          ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                         ()),
                        ('adjoint_tape_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                        ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                       (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                        ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-nonlinear-ckpt': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                             ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_sparse_batch', (3, 2), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                             ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                             ('run_adjoint_batch',
                              (1, 3,
                               ('f8', (3, 3, 2),
                                [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                                 3.6484375, 3.796875, 3.7265625, 6.375]),
                               None, False),
                              ()),
                             ('set_state_batch',
                              (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                               ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                               ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                              ()),
                             ('adjoint_tape_reserve_sparse_batch', (0, 0), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                             ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                            (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                             ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-order1': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                     ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                     ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                     ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                     ('run_adjoint_batch',
                      (0, 3,
                       ('f8', (3, 3, 2),
                        [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                         3.6484375, 3.796875, 3.7265625, 6.375]),
                       None, False),
                      ()),
                     ('set_state_batch',
                      (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                       ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                       ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                      ()),
                     ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                     ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-plain': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                    ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                    ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                    ('run_adjoint_batch',
                     (1, 3,
                      ('f8', (3, 3, 2),
                       [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                        3.6484375, 3.796875, 3.7265625, 6.375]),
                      None, False),
                     ()),
                    ('set_state_batch',
                     (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                      ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                      ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                     ()),
                    ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                   (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                    ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-own-state-gradient': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                             ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                             ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                             ('run_adjoint_batch',
                              (1, 3,
                               ('f8', (3, 3, 2),
                                [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                                 3.6484375, 3.796875, 3.7265625, 6.375]),
                               None, True),
                              ()),
                             ('set_state_batch',
                              (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                               ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                               ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                              ()),
                             ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()),
                             ('set_adjoint_factors', (1, -1), ())],
                            (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                             ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]),
                             ('f8', (3, 6),
                              [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]))),
 'bcg-own-x0': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                 ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                 ('set_state_batch',
                  (('f8', (3, 4), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375]),
                   ('f8', (3, 4), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375]),
                   ('f8', (3, 2), [1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875])),
                  ()),
                 ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                 ('run_adjoint_batch',
                  (1, 3,
                   ('f8', (3, 3, 2),
                    [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875, 3.6484375,
                     3.796875, 3.7265625, 6.375]),
                   None, False),
                  ()),
                 ('set_state_batch',
                  (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                   ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                   ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                  ()),
                 ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                 ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-cn': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                    ('run_adjoint_batch',
                     (1, 3,
                      ('f8', (3, 3, 2),
                       [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                        3.6484375, 3.796875, 3.7265625, 6.375]),
                      None, False),
                     ()),
                    ('set_state_batch',
                     (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                      ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                      ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                     ())],
                   (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                    ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-energy': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_begin_batch', (), ()),
                        ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', True),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', True),)),
                        ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                        ('run_adjoint_batch',
                         (1, 3,
                          ('f8', (3, 3, 2),
                           [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                            3.6484375, 3.796875, 3.7265625, 6.375]),
                          None, False),
                         ()),
                        ('set_adjoint_energy', (None,), ()),
                        ('set_state_batch',
                         (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                          ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                          ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                         ())],
                       (('f8', (3,), [21.4091796875, 22.98681640625, 29.5068359375]),
                        ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-energy-ckpt': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_begin_batch', (), ()),
                             ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', True),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', True),)),
                             ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                             ('run_adjoint_batch',
                              (1, 3,
                               ('f8', (3, 3, 2),
                                [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                                 3.6484375, 3.796875, 3.7265625, 6.375]),
                               None, False),
                              ()),
                             ('set_adjoint_energy', (None,), ()),
                             ('set_state_batch',
                              (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                               ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                               ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                              ())],
                            (('f8', (3,), [21.4091796875, 22.98681640625, 29.5068359375]),
                             ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-nonlinear': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_begin_batch', (), ()),
                           ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                           ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                           ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                           ('run_adjoint_batch',
                            (1, 3,
                             ('f8', (3, 3, 2),
                              [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                               3.6484375, 3.796875, 3.7265625, 6.375]),
                             None, False),
                            ()),
                           ('set_state_batch',
                            (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                             ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                             ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                            ())],
                          (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                           ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-nonlinear-ckpt': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_begin_batch', (), ()),
                                ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                                ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                                ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                                ('run_adjoint_batch',
                                 (1, 3,
                                  ('f8', (3, 3, 2),
                                   [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125,
                                    4.21875, 3.6484375, 3.796875, 3.7265625, 6.375]),
                                  None, False),
                                 ()),
                                ('set_state_batch',
                                 (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                                  ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                                  ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                                 ())],
                               (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                                ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-order1': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                        ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                        ('run_adjoint_batch',
                         (0, 3,
                          ('f8', (3, 3, 2),
                           [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                            3.6484375, 3.796875, 3.7265625, 6.375]),
                          None, False),
                         ()),
                        ('set_state_batch',
                         (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                          ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                          ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                         ())],
                       (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                        ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-plain': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                       ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                       ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                       ('run_adjoint_batch',
                        (1, 3,
                         ('f8', (3, 3, 2),
                          [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                           3.6484375, 3.796875, 3.7265625, 6.375]),
                         None, False),
                        ()),
                       ('set_state_batch',
                        (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                         ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                         ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                        ())],
                      (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                       ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bcg-reused-state-gradient': ([('bfs._flush', (), ()), ('get_state_batch', (), ()),
                                ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                                ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                                ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                                ('run_adjoint_batch',
                                 (1, 3,
                                  ('f8', (3, 3, 2),
                                   [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125,
                                    4.21875, 3.6484375, 3.796875, 3.7265625, 6.375]),
                                  None, True),
                                 ()),
                                ('set_state_batch',
                                 (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                                  ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                                  ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                                 ())],
                               (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                                ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]),
                                ('f8', (3, 6),
                                 [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]))),
 'bcg-reused-x0': ([('bfs._flush', (), ()), ('get_state_batch', (), ()),
                    ('set_state_batch',
                     (('f8', (3, 4), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375]),
                      ('f8', (3, 4), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375]),
                      ('f8', (3, 2), [1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875])),
                     ()),
                    ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                    ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                    ('run_adjoint_batch',
                     (1, 3,
                      ('f8', (3, 3, 2),
                       [3.6484375, 3.796875, 3.7265625, 6.375, 3.4296875, 5.953125, 3.796875, 4.0078125, 3.5, 3.5859375, 3.578125, 6.1640625, 3.9453125, 4.21875,
                        3.6484375, 3.796875, 3.7265625, 6.375]),
                      None, False),
                     ()),
                    ('set_state_batch',
                     (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                      ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                      ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                     ())],
                   (('f8', (3,), [18.8779296875, 21.29931640625, 27.1630859375]),
                    ('f8', (3, 3, 1), [2.796875, 2.8125, 2.578125, 2.59375, 2.359375, 2.375, 2.140625, 2.90625, 2.921875]))),
 'bclg-own-energy': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                      ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                      ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()), ('adjoint_loop_reserve_batch', (3,), ()),
                      ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                      ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', True),)),
                      ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                      ('run_adjoint_closed_loop_batch',
                       (1, 3,
                        ('f8', (3, 3, 2),
                         [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                          3.796875, 4.0078125, 3.5, 3.5859375]),
                        ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                       ()),
                      ('set_adjoint_energy', (None,), ()),
                      ('set_state_batch',
                       (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                        ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                        ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                       ()),
                      ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve_batch', (0,), ()), ('adjoint_loop_reserve_batch', (0,), ()),
                      ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()),
                      ('set_adjoint_factors', (1, -1), ())],
                     (('f8', (3,), [22.45703125, 23.15966796875, 24.0234375]),
                      ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                        ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                        ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                        ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                        ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                        ('y0', ('f8', (2,), [1.5625, 1.0]))),
                       (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                        ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                        ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                        ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                       (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                        ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                        ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                        ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                        ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                        ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-own-nonlinear': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                         ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                         ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()), ('adjoint_loop_reserve_batch', (3,), ()),
                         ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                         ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                         ('run_adjoint_closed_loop_batch',
                          (1, 3,
                           ('f8', (3, 3, 2),
                            [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                             3.796875, 4.0078125, 3.5, 3.5859375]),
                           ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                          ()),
                         ('set_state_batch',
                          (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                           ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                           ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                          ()),
                         ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve_batch', (0,), ()), ('adjoint_loop_reserve_batch', (0,), ()),
                         ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()),
                         ('set_adjoint_factors', (1, -1), ())],
                        (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                         ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                           ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                           ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                           ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                           ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                           ('y0', ('f8', (2,), [1.5625, 1.0]))),
                          (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                           ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                           ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                           ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                          (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                           ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                           ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                           ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                           ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                           ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-own-nonlinear-ckpt': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                              ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_sparse_batch', (3, 2), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                              ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()), ('adjoint_loop_reserve_batch', (3,), ()),
                              ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                              ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                              ('run_adjoint_closed_loop_batch',
                               (1, 3,
                                ('f8', (3, 3, 2),
                                 [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375,
                                  4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]),
                                ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                               ()),
                              ('set_state_batch',
                               (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                                ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                                ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                               ()),
                              ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve_sparse_batch', (0, 0), ()), ('adjoint_loop_reserve_batch', (0,), ()),
                              ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()),
                              ('set_adjoint_factors', (1, -1), ())],
                             (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                              ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                                ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                                ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                                ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                                ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                                ('y0', ('f8', (2,), [1.5625, 1.0]))),
                               (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                                ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                                ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                                ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                               (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                                ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                                ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                                ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                                ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                                ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-own-order1': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                      ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()),
                      ('adjoint_loop_info_batch', (), ()), ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                      ('run_closed_loop_batch', (0, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                      ('run_adjoint_closed_loop_batch',
                       (0, 3,
                        ('f8', (3, 3, 2),
                         [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                          3.796875, 4.0078125, 3.5, 3.5859375]),
                        ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                       ()),
                      ('set_state_batch',
                       (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                        ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                        ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                       ()),
                      ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()),
                      ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                     (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                      ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                        ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                        ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                        ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                        ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                        ('y0', ('f8', (2,), [1.5625, 1.0]))),
                       (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                        ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                        ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                        ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                       (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                        ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                        ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                        ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                        ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                        ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-own-plain': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()),
                     ('adjoint_loop_info_batch', (), ()), ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                     ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                     ('run_adjoint_closed_loop_batch',
                      (1, 3,
                       ('f8', (3, 3, 2),
                        [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                         3.796875, 4.0078125, 3.5, 3.5859375]),
                       ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                      ()),
                     ('set_state_batch',
                      (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                       ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                       ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                      ()),
                     ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()),
                     ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                     ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                       ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                       ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                       ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                       ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                       ('y0', ('f8', (2,), [1.5625, 1.0]))),
                      (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                       ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                       ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                       ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                      (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                       ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                       ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                       ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                       ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                       ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-own-signals': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                       ('set_adjoint_batch', (1, 1), ()), ('bfs._flush', (), ()), ('get_state_batch', (), ()),
                       ('set_controllers', (3, 0.125, (('f8', (1, 2), [-1.0, 0.5]), ('f8', (1,), [0.25]))), ()),
                       ('set_loop_signals',
                        (('f8', (3, 3, 1), [1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375]),
                         ('f8', (3, 3, 1), [1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875])),
                        ()),
                       ('set_control_limits', (('f8', (3, 1), [-2.0, -2.0, -2.0]), ('f8', (3, 1), [2.0, 2.0, 2.0])), ()), ('adjoint_loop_info_batch', (), ()),
                       ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                       ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                       ('run_adjoint_closed_loop_batch',
                        (1, 3,
                         ('f8', (3, 3, 2),
                          [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                           3.796875, 4.0078125, 3.5, 3.5859375]),
                         ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                        ()),
                       ('set_state_batch',
                        (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                         ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                         ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                        ()),
                       ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()),
                       ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                      (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                       ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                         ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                         ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                         ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                         ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                         ('y0', ('f8', (2,), [1.5625, 1.0]))),
                        (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                         ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                         ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                         ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                        (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                         ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                         ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                         ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                         ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                         ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-energy': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()),
                         ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                         ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', True),)),
                         ('set_adjoint_energy', (('f8', (3, 3), [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),), ()),
                         ('run_adjoint_closed_loop_batch',
                          (1, 3,
                           ('f8', (3, 3, 2),
                            [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                             3.796875, 4.0078125, 3.5, 3.5859375]),
                           ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                          ()),
                         ('set_adjoint_energy', (None,), ()),
                         ('set_state_batch',
                          (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                           ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                           ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                          ()),
                         ('set_controllers', (None, 0.125, None), ())],
                        (('f8', (3,), [22.45703125, 23.15966796875, 24.0234375]),
                         ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                           ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                           ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                           ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                           ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                           ('y0', ('f8', (2,), [1.5625, 1.0]))),
                          (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                           ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                           ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                           ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                          (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                           ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                           ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                           ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                           ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                           ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-nonlinear': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()),
                            ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                            ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                            ('run_adjoint_closed_loop_batch',
                             (1, 3,
                              ('f8', (3, 3, 2),
                               [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                                3.796875, 4.0078125, 3.5, 3.5859375]),
                              ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                             ()),
                            ('set_state_batch',
                             (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                              ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                              ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                             ()),
                            ('set_controllers', (None, 0.125, None), ())],
                           (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                            ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                              ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                              ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                              ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                              ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                              ('y0', ('f8', (2,), [1.5625, 1.0]))),
                             (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                              ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                              ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                              ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                             (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                              ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                              ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                              ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                              ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                              ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-nonlinear-ckpt': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()),
                                 ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_tape_begin_batch', (), ()), ('adjoint_loop_begin_batch', (), ()),
                                 ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                                 ('run_adjoint_closed_loop_batch',
                                  (1, 3,
                                   ('f8', (3, 3, 2),
                                    [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375,
                                     4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]),
                                   ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                                  ()),
                                 ('set_state_batch',
                                  (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                                   ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                                   ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                                  ()),
                                 ('set_controllers', (None, 0.125, None), ())],
                                (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                                 ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                                   ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                                   ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                                   ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                                   ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                                   ('y0', ('f8', (2,), [1.5625, 1.0]))),
                                  (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                                   ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])),
                                   ('G', ('f8', (1, 2), [1.3125, 1.75])), ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])),
                                   ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])), ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])),
                                   ('y0', ('f8', (2,), [1.4375, 1.875]))),
                                  (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                                   ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                                   ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                                   ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                                   ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])),
                                   ('x0', ('f8', (2,), [1.25, 1.6875])), ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-order1': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()),
                         ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                         ('run_closed_loop_batch', (0, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                         ('run_adjoint_closed_loop_batch',
                          (0, 3,
                           ('f8', (3, 3, 2),
                            [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                             3.796875, 4.0078125, 3.5, 3.5859375]),
                           ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                          ()),
                         ('set_state_batch',
                          (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                           ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                           ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                          ()),
                         ('set_controllers', (None, 0.125, None), ())],
                        (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                         ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                           ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                           ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                           ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                           ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                           ('y0', ('f8', (2,), [1.5625, 1.0]))),
                          (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                           ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                           ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                           ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                          (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                           ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                           ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                           ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                           ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                           ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-plain': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, None), ()), ('adjoint_loop_info_batch', (), ()),
                        ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                        ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                        ('run_adjoint_closed_loop_batch',
                         (1, 3,
                          ('f8', (3, 3, 2),
                           [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                            3.796875, 4.0078125, 3.5, 3.5859375]),
                          ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                         ()),
                        ('set_state_batch',
                         (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                          ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                          ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                         ()),
                        ('set_controllers', (None, 0.125, None), ())],
                       (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                        ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                          ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                          ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                          ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                          ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                          ('y0', ('f8', (2,), [1.5625, 1.0]))),
                         (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                          ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                          ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                          ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                         (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                          ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                          ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                          ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                          ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                          ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'bclg-reused-signals': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('set_controllers', (3, 0.125, (('f8', (1, 2), [-1.0, 0.5]), ('f8', (1,), [0.25]))), ()),
                          ('set_loop_signals',
                           (('f8', (3, 3, 1), [1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375]),
                            ('f8', (3, 3, 1), [1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875])),
                           ()),
                          ('set_control_limits', (('f8', (3, 1), [-2.0, -2.0, -2.0]), ('f8', (3, 1), [2.0, 2.0, 2.0])), ()), ('adjoint_loop_info_batch', (), ()),
                          ('adjoint_loop_reserve_batch', (3,), ()), ('adjoint_loop_begin_batch', (), ()),
                          ('run_closed_loop_batch', (1, 3, ('f8', (3, 2), [1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625])), (('compute_energy', False),)),
                          ('run_adjoint_closed_loop_batch',
                           (1, 3,
                            ('f8', (3, 3, 2),
                             [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875, 2.984375, 5.3203125, 2.6875, 4.8984375, 4.390625, 4.8515625, 4.09375, 4.4296875,
                              3.796875, 4.0078125, 3.5, 3.5859375]),
                            ('f8', (3, 3, 1), [0.984375, 1.3125, 0.890625, 1.21875, 0.796875, 1.125, 1.453125, 1.03125, 1.359375]), None, False),
                           ()),
                          ('set_state_batch',
                           (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                            ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                            ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                           ()),
                          ('set_controllers', (None, 0.125, None), ())],
                         (('f8', (3,), [20.14453125, 21.19091796875, 21.8984375]),
                          ((('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                            ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                            ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                            ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                            ('w_u', ('f8', (3, 1), [1.6875, 1.0, 1.3125])), ('w_y', ('f8', (3, 1), [1.9375, 1.25, 1.5625])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                            ('y0', ('f8', (2,), [1.5625, 1.0]))),
                           (('A', ('f8', (1, 1), [0.11873205318098698])), ('Ad', ('f8', (1, 1), [1.0625])), ('B', ('f8', (1, 1), [0.14247573484966639])),
                            ('Bd', ('f8', (1, 1), [1.25])), ('C', ('f8', (1, 1), [1.0625])), ('D', ('f8', (1, 1), [1.6875])), ('G', ('f8', (1, 2), [1.3125, 1.75])),
                            ('S', ('f8', (1, 1), [1.625])), ('g0', ('f8', (1,), [1.875])), ('w_u', ('f8', (3, 1), [1.125, 1.4375, 1.75])),
                            ('w_y', ('f8', (3, 1), [1.375, 1.6875, 1.0])), ('x0', ('f8', (1,), [1.375])), ('y0', ('f8', (2,), [1.4375, 1.875]))),
                           (('A', ('f8', (2, 2), [0.2121621185885142, 0.1295404005710677, 0.18996268207515316, 0.11173527693572208])),
                            ('Ad', ('f8', (2, 2), [1.8125, 1.25, 1.6875, 1.125])), ('B', ('f8', (2, 1), [0.13219098459233017, 0.17154623778112188])),
                            ('Bd', ('f8', (2, 1), [1.125, 1.5625])), ('C', ('f8', (1, 2), [1.9375, 1.375])), ('D', ('f8', (1, 1), [1.125])),
                            ('G', ('f8', (1, 2), [1.1875, 1.625])), ('S', ('f8', (1, 1), [1.0625])), ('g0', ('f8', (1,), [1.3125])),
                            ('w_u', ('f8', (3, 1), [1.5625, 1.875, 1.1875])), ('w_y', ('f8', (3, 1), [1.8125, 1.125, 1.4375])), ('x0', ('f8', (2,), [1.25, 1.6875])),
                            ('y0', ('f8', (2,), [1.3125, 1.75])))))),
 'btan-cn': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
              ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
              ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
              ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
              ('run_tangent_batch',
               (1, 3, ('f8', (3, 3, 1), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                ('f8', (3, 6), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]),
                ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]), None),
               ()),
              ('tangent_reserve', (0,), ()),
              ('set_state_batch',
               (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
               ()),
              ('adjoint_tape_reserve_batch', (0,), ())],
             (('f8', (3, 3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25]),
              ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
              ('f8', (3, 6), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]))),
 'btan-first-order-given': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('tangent_info', (), ()),
                             ('tangent_reserve', (1,), ()), ('adjoint_tape_begin_batch', (), ()),
                             ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                             ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                             ('run_tangent_batch',
                              (0, 3, ('f8', (3, 3, 1), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                               ('f8', (3, 6),
                                [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]),
                               ('f8', (3, 6),
                                [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                               None),
                              ()),
                             ('tangent_reserve', (0,), ()),
                             ('set_state_batch',
                              (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                               ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                               ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                              ()),
                             ('adjoint_tape_reserve_batch', (0,), ())],
                            (('f8', (3, 3, 2),
                              [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25]),
                             ('f8', (3, 6),
                              [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                             ('f8', (3, 6),
                              [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]))),
 'btan-order1': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                  ('adjoint_tape_begin_batch', (), ()), ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                  ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                  ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                  ('run_tangent_batch',
                   (0, 3, ('f8', (3, 3, 1), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                    ('f8', (3, 6), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]),
                    ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                    None),
                   ()),
                  ('tangent_reserve', (0,), ()),
                  ('set_state_batch',
                   (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                    ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                    ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                   ()),
                  ('adjoint_tape_reserve_batch', (0,), ())],
                 (('f8', (3, 3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25]),
                  ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                  ('f8', (3, 6), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]))),
 'btan-plain': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                 ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                 ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                 ('run_tangent_batch',
                  (1, 3, ('f8', (3, 3, 1), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                   ('f8', (3, 6), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]),
                   ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                   None),
                  ()),
                 ('tangent_reserve', (0,), ()),
                 ('set_state_batch',
                  (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                   ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                   ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                  ()),
                 ('adjoint_tape_reserve_batch', (0,), ())],
                (('f8', (3, 3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25]),
                 ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                 ('f8', (3, 6), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]))),
 'btan-ref-col': ([('bfs._flush', (), ()), ('get_state_batch', (), ()), ('adjoint_tape_reserve_batch', (3,), ()), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                   ('adjoint_tape_begin_batch', (), ()), ('step_batch', (1, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                   ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                   ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),)),
                   ('run_tangent_batch',
                    (1, 3, ('f8', (3, 3, 1), [1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                     ('f8', (3, 6), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875]),
                     ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                     1),
                    ()),
                   ('tangent_reserve', (0,), ()),
                   ('set_state_batch',
                    (('f8', (3, 4), [1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                     ('f8', (3, 4), [1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                     ('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0])),
                    ()),
                   ('adjoint_tape_reserve_batch', (0,), ())],
                  (('f8', (3, 3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25]),
                   ('f8', (3, 6), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625]),
                   ('f8', (3, 6), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.3125, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]))),
 'clg-own-energy': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('adjoint_tape_reserve', (3,), ()), ('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()),
                     ('adjoint_loop_reserve', (3,), ()), ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                     ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', True),)),
                     ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                     ('run_adjoint_closed_loop',
                      (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False), ()),
                     ('set_adjoint_energy', (None,), ()),
                     ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                     ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve', (0,), ()), ('adjoint_loop_reserve', (0,), ()),
                     ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (24.37890625,
                     (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                      ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                      ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                      ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                      ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                      ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-own-nonlinear': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                        ('adjoint_tape_reserve', (3,), ()), ('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()),
                        ('adjoint_loop_reserve', (3,), ()), ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                        ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                        ('run_adjoint_closed_loop',
                         (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                         ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                        ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve', (0,), ()), ('adjoint_loop_reserve', (0,), ()),
                        ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                       (22.37890625,
                        (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                         ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                         ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                         ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                         ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                         ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-own-nonlinear-ckpt': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                             ('adjoint_tape_reserve_sparse', (3, 2), ()), ('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()),
                             ('adjoint_loop_reserve', (3,), ()), ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                             ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                             ('run_adjoint_closed_loop',
                              (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None,
                               False),
                              ()),
                             ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                             ('set_controllers', (None, 0.125, None), ()), ('adjoint_tape_reserve_sparse', (0, 0), ()), ('adjoint_loop_reserve', (0,), ()),
                             ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                            (22.37890625,
                             (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                              ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                              ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                              ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                              ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                              ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-own-order1': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                     ('adjoint_loop_begin', (), ()), ('run_closed_loop', (0, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                     ('run_adjoint_closed_loop',
                      (0, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False), ()),
                     ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                     ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()),
                     ('set_adjoint_factors', (1, -1), ())],
                    (22.37890625,
                     (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                      ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                      ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                      ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                      ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                      ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-own-plain': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                    ('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                    ('adjoint_loop_begin', (), ()), ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                    ('run_adjoint_closed_loop',
                     (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False), ()),
                    ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                    ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()),
                    ('set_adjoint_factors', (1, -1), ())],
                   (22.37890625,
                    (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                     ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                     ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                     ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                     ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                     ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-own-signals': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                      ('get_state', (), ()), ('set_controllers', (1, 0.125, (('f8', (1, 2), [-1.0, 0.5]), ('f8', (1,), [0.25]))), ()),
                      ('set_loop_signals', (('f8', (3, 1), [1.9375, 1.375, 1.8125]), ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ()),
                      ('set_control_limits', (('f8', (1, 1), [-2.0]), ('f8', (1, 1), [2.0])), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                      ('adjoint_loop_begin', (), ()), ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                      ('run_adjoint_closed_loop',
                       (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False), ()),
                      ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                      ('set_controllers', (None, 0.125, None), ()), ('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()),
                      ('set_adjoint_factors', (1, -1), ())],
                     (22.37890625,
                      (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                       ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                       ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                       ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                       ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                       ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-energy': ([('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                        ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                        ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', True),)),
                        ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                        ('run_adjoint_closed_loop',
                         (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                         ()),
                        ('set_adjoint_energy', (None,), ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                        ('set_controllers', (None, 0.125, None), ())],
                       (24.37890625,
                        (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                         ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                         ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                         ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                         ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                         ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-nonlinear': ([('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                           ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                           ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                           ('run_adjoint_closed_loop',
                            (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                            ()),
                           ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                           ('set_controllers', (None, 0.125, None), ())],
                          (22.37890625,
                           (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                            ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                            ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                            ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                            ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                            ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-nonlinear-ckpt': ([('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                                ('adjoint_tape_begin', (), ()), ('adjoint_loop_begin', (), ()),
                                ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                                ('run_adjoint_closed_loop',
                                 (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None,
                                  False),
                                 ()),
                                ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                                ('set_controllers', (None, 0.125, None), ())],
                               (22.37890625,
                                (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                                 ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                                 ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                                 ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                                 ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                                 ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-order1': ([('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                        ('adjoint_loop_begin', (), ()), ('run_closed_loop', (0, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                        ('run_adjoint_closed_loop',
                         (0, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                         ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                        ('set_controllers', (None, 0.125, None), ())],
                       (22.37890625,
                        (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                         ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                         ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                         ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                         ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                         ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-plain': ([('get_state', (), ()), ('set_controllers', (1, 0.125, None), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                       ('adjoint_loop_begin', (), ()), ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                       ('run_adjoint_closed_loop',
                        (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                        ()),
                       ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                       ('set_controllers', (None, 0.125, None), ())],
                      (22.37890625,
                       (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                        ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                        ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                        ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                        ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                        ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'clg-reused-signals': ([('get_state', (), ()), ('set_controllers', (1, 0.125, (('f8', (1, 2), [-1.0, 0.5]), ('f8', (1,), [0.25]))), ()),
                         ('set_loop_signals', (('f8', (3, 1), [1.9375, 1.375, 1.8125]), ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ()),
                         ('set_control_limits', (('f8', (1, 1), [-2.0]), ('f8', (1, 1), [2.0])), ()), ('adjoint_loop_info', (), ()), ('adjoint_loop_reserve', (3,), ()),
                         ('adjoint_loop_begin', (), ()), ('run_closed_loop', (1, 3, ('f8', (2,), [1.875, 1.3125])), (('compute_energy', False),)),
                         ('run_adjoint_closed_loop',
                          (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), ('f8', (3, 1), [0.984375, 1.3125, 0.890625]), None, False),
                          ()),
                         ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                         ('set_controllers', (None, 0.125, None), ())],
                        (22.37890625,
                         (('A', ('f8', (2, 2), [0.16056007266755803, 0.18621435780196952, 0.14559317684826528, 0.16984617716465858])),
                          ('Ad', ('f8', (2, 2), [1.3125, 1.75, 1.1875, 1.625])), ('B', ('f8', (2, 1), [0.16156675894618133, 0.20520793899542542])),
                          ('Bd', ('f8', (2, 1), [1.375, 1.8125])), ('C', ('f8', (1, 2), [1.1875, 1.625])), ('D', ('f8', (1, 1), [1.25])),
                          ('G', ('f8', (1, 2), [1.4375, 1.875])), ('S', ('f8', (1, 1), [1.1875])), ('g0', ('f8', (1,), [1.4375])),
                          ('w_u', ('f8', (3, 1), [1.6875, 1.125, 1.5625])), ('w_y', ('f8', (3, 1), [1.9375, 1.375, 1.8125])), ('x0', ('f8', (2,), [1.5, 1.9375])),
                          ('y0', ('f8', (2,), [1.5625, 1.0]))))),
 'forward-batch-taped-device': ([('adjoint_tape_begin_batch', (), ()), ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                                 ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                                 ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),))],
                                ('f8', (3, 3, 2),
                                 [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375])),
 'forward-batch-taped-solver': ([('bfs._flush', (), ()), ('adjoint_tape_begin_batch', (), ()),
                                 ('step_batch', (0, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                                 ('step_batch', (1, ('f8', (3, 1), [1.125, 1.5625, 1.0])), (('compute_energy', False),)),
                                 ('step_batch', (1, ('f8', (3, 1), [1.4375, 1.875, 1.3125])), (('compute_energy', False),))],
                                ('f8', (3, 3, 2),
                                 [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125, 1.6875, 1.125, 1.5625, 1.0, 1.4375, 1.875, 1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375])),
 'gnp-own-order1': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('adjoint_tape_reserve', (3,), ()), ('adjoint_tape_info', (), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                     ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                     ('run_tangent', (0, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                     ('run_adjoint', (0, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ()),
                     ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                     ('adjoint_tape_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'gnp-own-taped-here': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                         ('adjoint_tape_reserve', (3,), ()), ('adjoint_tape_info', (), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                         ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                         ('run_tangent', (1, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                         ('run_adjoint', (1, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ()),
                         ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                         ('adjoint_tape_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                        ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'gnp-reused-longer-tape': ([('adjoint_tape_info', (), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                             ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)), ('tangent_info', (), ()),
                             ('tangent_reserve', (1,), ()), ('run_tangent', (1, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                             ('run_adjoint', (1, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ()),
                             ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                            ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'gnp-reused-order1': ([('adjoint_tape_info', (), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                        ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                        ('run_tangent', (0, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                        ('run_adjoint', (0, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                       ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'gnp-reused-tape-holds-the-run': ([('adjoint_tape_info', (), ()), ('tangent_info', (), ()), ('tangent_reserve', (1,), ()),
                                    ('run_tangent', (1, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                                    ('run_adjoint', (1, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ())],
                                   ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'gnp-reused-taped-here': ([('adjoint_tape_info', (), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                            ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)), ('tangent_info', (), ()),
                            ('tangent_reserve', (1,), ()), ('run_tangent', (1, 3, ('f8', (3, 1), [1.375, 1.8125, 1.25]), None, None), ()), ('tangent_reserve', (0,), ()),
                            ('run_adjoint', (1, 3, ('f8', (3, 2), [4.09375, 4.4296875, 3.796875, 4.0078125, 3.5, 3.5859375]), None, False), ()),
                            ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                           ('f8', (3, 1), [2.46875, 3.234375, 2.25])),
 'qcg-own-energy': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('adjoint_tape_reserve', (3,), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                     ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)), ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                     ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                     ('set_adjoint_energy', (None,), ()),
                     ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                     ('adjoint_tape_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (24.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-own-energy-ckpt': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                          ('adjoint_tape_reserve_sparse', (3, 2), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                          ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                          ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                          ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                          ('set_adjoint_energy', (None,), ()),
                          ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                          ('adjoint_tape_reserve_sparse', (0, 0), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                         (24.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-own-nonlinear-ckpt': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                             ('adjoint_tape_reserve_sparse', (3, 2), ()), ('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                             ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                             ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                             ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                             ('adjoint_tape_reserve_sparse', (0, 0), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                            (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-own-order1': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                     ('get_state', (), ()), ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                     ('run_adjoint', (0, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                     ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                     ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                    (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-own-plain': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                    ('get_state', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                    ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                    ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                    ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                   (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-own-x0': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                 ('set_state', (('f8', (4,), [1.5625, 1.0, 1.4375, 1.875]), ('f8', (4,), [1.625, 1.0625, 1.5, 1.9375]), ('f8', (2,), [1.6875, 1.125])), ()),
                 ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                 ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                 ('set_state', (('f8', (4,), [1.5625, 1.0, 1.4375, 1.875]), ('f8', (4,), [1.625, 1.0625, 1.5, 1.9375]), ('f8', (2,), [1.6875, 1.125])), ()),
                 ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-energy': ([('get_state', (), ()), ('adjoint_tape_begin', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                        ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                        ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                        ('set_adjoint_energy', (None,), ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                       (24.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-energy-ckpt': ([('get_state', (), ()), ('adjoint_tape_begin', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', True),)),
                             ('set_adjoint_energy', (('f8', (3,), [0.5, 0.5, 0.5]),), ()),
                             ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                             ('set_adjoint_energy', (None,), ()),
                             ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                            (24.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-nonlinear': ([('get_state', (), ()), ('adjoint_tape_begin', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                           ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                           ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                          (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-nonlinear-ckpt': ([('get_state', (), ()), ('adjoint_tape_begin', (), ()),
                                ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                                ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                                ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])),
                                 ())],
                               (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-order1': ([('get_state', (), ()), ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                        ('run_adjoint', (0, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                        ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                       (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-plain': ([('get_state', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                       ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                       ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ())],
                      (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'qcg-reused-x0': ([('set_state', (('f8', (4,), [1.5625, 1.0, 1.4375, 1.875]), ('f8', (4,), [1.625, 1.0625, 1.5, 1.9375]), ('f8', (2,), [1.6875, 1.125])), ()),
                    ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                    ('run_adjoint', (1, 3, ('f8', (3, 2), [3.5, 3.5859375, 3.578125, 6.1640625, 3.28125, 5.7421875]), None, False), ()),
                    ('set_state', (('f8', (4,), [1.5625, 1.0, 1.4375, 1.875]), ('f8', (4,), [1.625, 1.0625, 1.5, 1.9375]), ('f8', (2,), [1.6875, 1.125])), ())],
                   (22.94140625, ('f8', (3, 1), [2.796875, 2.8125, 2.578125]))),
 'setup-batched-checkpointed': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                                 ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_sparse_batch', (3, 2), ())],
                                [('adjoint_tape_reserve_sparse_batch', (0, 0), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                                 ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                                (('bytes', 160), ('export_ms', 1.0),
                                 ('loop',
                                  (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                 ('loop_batch',
                                  (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                 ('slots',
                                  ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                   (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                 ('tape',
                                  (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('every', 2), ('lost', 0), ('overflowed', False),
                                   ('replayed', 0))),
                                 ('tape_mode', 'checkpointed'))),
 'setup-batched-checkpointed-loop': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                                      ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_sparse_batch', (3, 2), ())],
                                     [('adjoint_tape_reserve_sparse_batch', (0, 0), ()), ('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()),
                                      ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                                     (('bytes', 160), ('export_ms', 1.0),
                                      ('loop',
                                       (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                      ('loop_batch',
                                       (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                      ('slots',
                                       ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                        (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                      ('tape',
                                       (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('every', 2), ('lost', 0), ('overflowed', False),
                                        ('replayed', 0))),
                                      ('tape_mode', 'checkpointed'))),
 'setup-batched-dense': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                          ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ())],
                         [('adjoint_tape_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                          ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                         (('bytes', 160), ('export_ms', 1.0),
                          ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                          ('loop_batch', (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                          ('slots',
                           ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                            (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                          ('tape', (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('lost', 0), ('overflowed', False))),
                          ('tape_mode', 'dense'))),
 'setup-batched-dense-loop': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                               ('set_adjoint_batch', (1, 1), ()), ('adjoint_tape_reserve_batch', (3,), ())],
                              [('adjoint_tape_reserve_batch', (0,), ()), ('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()),
                               ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                              (('bytes', 160), ('export_ms', 1.0),
                               ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                               ('loop_batch',
                                (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                               ('slots',
                                ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                 (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                               ('tape', (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('lost', 0), ('overflowed', False))),
                               ('tape_mode', 'dense'))),
 'setup-batched-no-tape': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                            ('set_adjoint_batch', (1, 1), ())],
                           [('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_batch', (1, -1), ()),
                            ('set_adjoint_factors', (1, -1), ())],
                           (('bytes', 160), ('export_ms', 1.0),
                            ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                            ('loop_batch', (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                            ('slots',
                             ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                              (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                            ('tape', (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False))),
                            ('tape_mode', None))),
 'setup-batched-no-tape-loop': ([('bfs._flush', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_batch', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                                 ('set_adjoint_batch', (1, 1), ())],
                                [('adjoint_loop_reserve_batch', (0,), ()), ('set_adjoint_batch', (0, -1), ()), ('set_adjoint_factors', (0, -1), ()),
                                 ('set_adjoint_batch', (1, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                                (('bytes', 160), ('export_ms', 1.0),
                                 ('loop',
                                  (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                 ('loop_batch',
                                  (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                 ('slots',
                                  ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                   (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                 ('tape', (('KB', 3), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False))),
                                 ('tape_mode', None))),
 'setup-single-checkpointed': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                                ('adjoint_tape_reserve_sparse', (3, 2), ())],
                               [('adjoint_tape_reserve_sparse', (0, 0), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                               (('bytes', 160), ('export_ms', 1.0),
                                ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                ('loop_batch',
                                 (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                ('slots',
                                 ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                  (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                ('tape',
                                 (('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('every', 2), ('lost', 0), ('overflowed', False), ('replayed', 0))),
                                ('tape_mode', 'checkpointed'))),
 'setup-single-checkpointed-loop': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                                     ('adjoint_tape_reserve_sparse', (3, 2), ())],
                                    [('adjoint_tape_reserve_sparse', (0, 0), ()), ('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()),
                                     ('set_adjoint_factors', (1, -1), ())],
                                    (('bytes', 160), ('export_ms', 1.0),
                                     ('loop',
                                      (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                     ('loop_batch',
                                      (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                     ('slots',
                                      ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                       (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                     ('tape',
                                      (('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('every', 2), ('lost', 0), ('overflowed', False), ('replayed', 0))),
                                     ('tape_mode', 'checkpointed'))),
 'setup-single-dense': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                         ('adjoint_tape_reserve', (3,), ())],
                        [('adjoint_tape_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                        (('bytes', 160), ('export_ms', 1.0),
                         ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                         ('loop_batch', (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                         ('slots',
                          ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                           (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                         ('tape', (('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('lost', 0), ('overflowed', False))), ('tape_mode', 'dense'))),
 'setup-single-dense-loop': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ()),
                              ('adjoint_tape_reserve', (3,), ())],
                             [('adjoint_tape_reserve', (0,), ()), ('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()),
                              ('set_adjoint_factors', (1, -1), ())],
                             (('bytes', 160), ('export_ms', 1.0),
                              ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                              ('loop_batch', (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                              ('slots',
                               ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                              ('tape', (('begun', False), ('bytes', 0), ('capacity', 3), ('count', 0), ('lost', 0), ('overflowed', False))), ('tape_mode', 'dense'))),
 'setup-single-no-tape': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ())],
                          [('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                          (('bytes', 160), ('export_ms', 1.0),
                           ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                           ('loop_batch', (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                           ('slots',
                            ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                             (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                           ('tape', (('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False))), ('tape_mode', None))),
 'setup-single-no-tape-loop': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('set_adjoint_factors', (0, 1), ()), ('set_adjoint_factors', (1, 1), ())],
                               [('adjoint_loop_reserve', (0,), ()), ('set_adjoint_factors', (0, -1), ()), ('set_adjoint_factors', (1, -1), ())],
                               (('bytes', 160), ('export_ms', 1.0),
                                ('loop', (('bad', False), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                ('loop_batch',
                                 (('bad', 0), ('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False), ('row', 0))),
                                ('slots',
                                 ((0, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))),
                                  (1, (('available', True), ('export_ms', 0.5), ('shared_bytes', 32), ('slot_bytes', 64))))),
                                ('tape', (('begun', False), ('bytes', 0), ('capacity', 0), ('count', 0), ('lost', 0), ('overflowed', False))), ('tape_mode', None))),
 'tan-first-order-given': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('get_state', (), ()), ('adjoint_tape_reserve', (3,), ()),
                            ('tangent_info', (), ()), ('tangent_reserve', (1,), ()), ('adjoint_tape_begin', (), ()),
                            ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                            ('run_tangent',
                             (0, 3, ('f8', (3, 1), [1.5625, 1.0, 1.4375]), ('f8', (6,), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                              ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125])),
                             ()),
                            ('tangent_reserve', (0,), ()),
                            ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                            ('adjoint_tape_reserve', (0,), ())],
                           (('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0]), ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                            ('f8', (6,), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875]))),
 'tan-order1': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('get_state', (), ()), ('adjoint_tape_reserve', (3,), ()), ('tangent_info', (), ()),
                 ('tangent_reserve', (1,), ()), ('adjoint_tape_begin', (), ()), ('run', (0, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                 ('run_tangent',
                  (0, 3, ('f8', (3, 1), [1.5625, 1.0, 1.4375]), ('f8', (6,), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                   ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125])),
                  ()),
                 ('tangent_reserve', (0,), ()),
                 ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                 ('adjoint_tape_reserve', (0,), ())],
                (('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0]), ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                 ('f8', (6,), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875]))),
 'tan-plain': ([('fs._begin_stepping', (), ()), ('fs._flush_log', (), ()), ('get_state', (), ()), ('adjoint_tape_reserve', (3,), ()), ('tangent_info', (), ()),
                ('tangent_reserve', (1,), ()), ('adjoint_tape_begin', (), ()), ('run', (1, 3, ('f8', (3, 1), [1.8125, 1.25, 1.6875])), (('compute_energy', False),)),
                ('run_tangent',
                 (1, 3, ('f8', (3, 1), [1.5625, 1.0, 1.4375]), ('f8', (6,), [1.75, 1.1875, 1.625, 1.0625, 1.5, 1.9375]),
                  ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125])),
                 ()),
                ('tangent_reserve', (0,), ()),
                ('set_state', (('f8', (4,), [1.125, 1.5625, 1.0, 1.4375]), ('f8', (4,), [1.0, 1.4375, 1.875, 1.3125]), ('f8', (2,), [1.8125, 1.25])), ()),
                ('adjoint_tape_reserve', (0,), ())],
               (('f8', (3, 2), [1.8125, 1.25, 1.6875, 1.125, 1.5625, 1.0]), ('f8', (6,), [1.625, 1.0625, 1.5, 1.9375, 1.375, 1.8125]),
                ('f8', (6,), [1.5, 1.9375, 1.375, 1.8125, 1.25, 1.6875])))}
# fmt: on
