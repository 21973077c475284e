"""Loop signals and actuator limits of the device closed loops (``fc_set_loop_signals``, ``fc_set_control_limits``,
``fc_get_loop_cursor``): the extended ``fc_ctrl_step`` against its numpy model, the runs against the host loop with the same signals,
the cursor across the cuts of a run, and what must not have moved.  All on the shipped O1 cylinder with the golden base flow."""
import tempfile

import numpy as np
import pytest

from flowcontrol_amd import _lib, optim, sysid
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from flowcontrol_amd.batch import BatchedFlowSolver
from flowcontrol_amd.controller import Controller, bank_step
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.examples.data import controller_file
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC

pytestmark = pytest.mark.gpu

DT = 0.005
EPS = 2.0**-53
SMALL = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.02)
GAINS = [0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
ICS = [ParamIC(xloc=2.0 + 0.1 * i, yloc=0.05 * i, radius=0.5, amplitude=0.02 + 0.002 * i) for i in range(8)]


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def _solver(golden_dir, n=50, ic=SMALL, **kw):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=n, **kw)
    fs.params_ic = ic
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


def _shipped(gain=1.0):
    K0 = Controller.from_file(file=controller_file(), x0=None)
    return Controller(A=K0.A, B=K0.B, C=gain * K0.C, D=gain * K0.D)


@pytest.fixture(scope="module")
def prepared(golden_dir):
    """One prepared cylinder solver (operators, factors and state on the device)."""
    fs = _solver(golden_dir)
    fs.initialize_time_stepping(ic=None)
    fs._begin_stepping()
    yield fs
    fs.th.release_device()


def _signals(n, k=None, n_act=2, seed=0):
    """Sinusoidal w_u on both actuators (different phases, per column when k is given) and a constant w_y."""
    s = np.arange(n)[:, None]
    if k is None:
        return np.full((n, 1), 1e-3), 5e-3 * np.sin(2 * np.pi * s / 20.0 + np.array([0.3, 1.7])[None, :n_act])
    col = np.arange(k)[None, :, None]
    w_u = 5e-3 * np.sin(2 * np.pi * s[:, :, None] / (15.0 + col) + np.array([0.3, 1.7])[None, None, :n_act] + 0.4 * col + seed)
    w_y = 1e-3 * np.cos(0.2 * s[:, :, None] + col)
    return w_y, w_u


# ── 1. the kernel ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _random_bank(rng, k, nx, nyc, nuc, n_sens, n_act):
    """A bank at the kernel's largest nyc / nuc, which ``pack_controllers`` (one output, or one per actuator) does not build."""
    Ad = rng.standard_normal((k, nx, nx)) * (0.5 / np.sqrt(max(nx, 1)))
    return {"k": k, "nx": nx, "nyc": nyc, "nuc": nuc, "Ad": Ad, "Bd": rng.standard_normal((k, nx, nyc)), "C": rng.standard_normal((k, nuc, nx)),
            "D": rng.standard_normal((k, nuc, nyc)), "x0": rng.standard_normal((k, nx)), "G": rng.standard_normal((k, nyc, n_sens)),
            "g0": rng.standard_normal((k, nyc)), "S": rng.standard_normal((k, n_act, nuc)), "sizes": [(nx, nuc)] * k}


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("nx", [0, 13, 65, 200])
def test_kernel_with_signals_and_limits_matches_bank_step(prepared, k, nx):
    """``fc_ctrl_apply`` with signals and limits set, 50 steps of random measurements, against ``bank_step`` (float64 numpy), the state
    reset to numpy's before every step.  nx = 65 puts one row on a lane's second trip; nyc = 8 and nuc = 32 are the kernel's largest.

    The bound is the one of ``test_closed_loop_gpu.py``'s kernel test with one more addition in the yc and u stages: a sum of n
    products errs by at most n eps sum |a_j| |v_j| in any order (fused or not), every output is a chain of such sums, each stage within
    (nx + nyc + 3) eps times its sum of absolute terms -- products, constant and signal -- carried through the absolute values of the
    later stages.  The clamp is 1-Lipschitz and keeps the bound; an entry that numpy finds beyond its limit by more than the bound must
    equal the limit bit for bit.  Limits: the median of |v| per simulation and actuator, so about half of the entries clamp; the second
    actuator has no lower limit (-inf).  Two calls on the same input and row are bit-identical, and every call moves the cursor by one."""
    dev = prepared.th.device()
    n_sens, n_act = dev.n_sens, dev.n_act
    nyc, nuc = 8, 32
    rng = np.random.default_rng(1000 * k + nx)
    dev.set_batch(k if k > 1 else 0)
    bank = _random_bank(rng, k, nx, nyc, nuc, n_sens, n_act)
    p = _lib.ptr
    _lib.check(dev.lib.fc_set_controllers(dev._h, k, nx, nyc, nuc, p(bank["Ad"]), p(bank["Bd"]), p(bank["C"]), p(bank["D"]), p(bank["x0"]),
                                          p(bank["G"]), p(bank["g0"]), p(bank["S"])))
    dev._ctrl_bank = bank
    n = 50
    ys, w_y, w_u = rng.standard_normal((n, k, n_sens)), rng.standard_normal((n, k, nyc)), 3.0 * rng.standard_normal((n, k, n_act))
    # numpy first: the whole sequence, without limits for their choice, then with them
    xs, vs = [bank["x0"].copy()], []
    for s in range(n):
        v, xn = bank_step(bank, xs[-1], ys[s], w_y=w_y[s], w_u=w_u[s])
        vs.append(v), xs.append(xn)
    hi = np.median(np.abs(np.stack(vs)), axis=0)
    lo = -hi.copy()
    lo[:, 1] = -np.inf
    # the rows in the order of the calls: every tenth step is applied twice
    calls = [s for s in range(n) for _ in range(2 if s % 10 == 0 else 1)]
    dev.set_loop_signals(w_y[calls], w_u[calls])
    dev.set_control_limits(lo, hi)
    assert dev.loop_cursor() == 0
    c = (nx + nyc + 3) * EPS
    worst, made, clamped = 0.0, 0, 0
    for s in range(n):
        x = xs[s]
        u_ref, x_ref = bank_step(bank, x, ys[s], w_y=w_y[s], w_u=w_u[s], u_lo=lo, u_hi=hi)
        assert np.array_equal(x_ref, xs[s + 1])  # (the clamp does not reach the state)
        dev.controller_state(x)
        u = dev.ctrl_apply(ys[s])
        x_dev = dev.controller_state()
        made += 1
        assert dev.loop_cursor() == made
        if s % 10 == 0:  # the same input and the same row again: the same bits
            dev.controller_state(x)
            assert np.array_equal(dev.ctrl_apply(ys[s]), u) and np.array_equal(dev.controller_state(), x_dev)
            made += 1
            assert dev.loop_cursor() == made
        for i in range(k):
            aG, aC, aD, aAd, aBd, aS = (np.abs(bank[m][i]) for m in ("G", "C", "D", "Ad", "Bd", "S"))
            yc_abs = aG @ np.abs(ys[s, i]) + np.abs(bank["g0"][i]) + np.abs(w_y[s, i])
            e_yc = c * yc_abs
            uc_abs = aC @ np.abs(x[i]) + aD @ yc_abs
            e_uc = c * uc_abs + aD @ e_yc
            e_u = c * (aS @ uc_abs + np.abs(w_u[s, i])) + aS @ e_uc
            e_x = c * (aAd @ np.abs(x[i]) + aBd @ yc_abs) + aBd @ e_yc
            assert np.all(np.abs(u[i] - u_ref[i]) <= e_u), (s, i, np.abs(u[i] - u_ref[i]).max(), e_u.max())
            assert np.all(np.abs(x_dev[i] - x_ref[i]) <= e_x), (s, i)
            below, above = vs[s][i] < lo[i] - e_u, vs[s][i] > hi[i] + e_u
            assert np.array_equal(u[i][below], lo[i][below]) and np.array_equal(u[i][above], hi[i][above]), (s, i)
            clamped += int(below.sum() + above.sum())
            worst = max(worst, float(np.max(np.abs(u[i] - u_ref[i]) / np.maximum(e_u, 1e-300))))
    print(f"k={k} nx={nx}: largest |err| / bound = {worst:.3f}; {clamped} of {n * k * n_act} entries clamped")
    assert 0.2 * n * k * n_act <= clamped <= 0.8 * n * k * n_act
    # the rows are used up: one more call is refused, and nothing moves
    assert dev.lib.fc_ctrl_apply(dev._h, k, np.zeros((k, n_sens)), np.zeros((k, n_act))) == _lib.FC_ERR_INVALID
    assert dev.loop_cursor() == len(calls)
    dev.set_controllers(None, DT)
    assert dev.loop_cursor() == 0
    dev.set_batch(0)


# ── 2. unset equals today ────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_zero_signals_free_limits_and_freed_signals_change_nothing(prepared):
    """30 steps three times: with all-zero w_y, w_u and (-inf, +inf) limits; with nothing set; with signals and limits set and freed
    again (``fc_set_loop_signals(n_rows = 0)``, ``fc_set_control_limits(NULL, NULL)``) before the run.  The last two launch the same
    kernels with the same null pointers: the same bits.  Zero signals and infinite limits are equal as numbers (v + 0.0 and a clamp at
    +-inf change no value)."""
    fs = prepared
    dev = fs.th.device()
    n = 30

    def run(**kw):
        fs.params_ic = SMALL
        fs.initialize_time_stepping(ic=None)
        K = _shipped()
        y, u, dE = fs.run_closed_loop(n, K, **kw)
        return y, u, dE, K.x.copy()

    plain = run()
    zero = run(w_y=np.zeros((n, 1)), w_u=np.zeros((n, 2)), u_limits=(-np.inf, np.inf))
    set_controllers = dev.set_controllers

    def set_then_free(controllers, dt, feedback=None):
        bank = set_controllers(controllers, dt, feedback)
        if controllers:
            dev.set_loop_signals(np.ones((n, 1, 1)), np.ones((n, 1, 2)))
            dev.set_control_limits(-1e-3, 1e-3)
            _lib.check(dev.lib.fc_set_loop_signals(dev._h, 1, 0, None, None))
            dev.set_control_limits(None, None)
        return bank

    dev.set_controllers = set_then_free
    try:
        freed = run()
    finally:
        del dev.set_controllers
    for a, b, c in zip(plain, zero, freed):
        assert np.array_equal(a, c, equal_nan=True)
        assert np.all((a == b) | (np.isnan(a) & np.isnan(b)))
    assert np.abs(plain[1]).max() > 0.0


# ── 3. device loop against host loop ─────────────────────────────────────────────────────────────────────────────────────────────
def test_device_loop_with_signals_and_binding_limits_matches_the_host_loop(prepared, golden_dir):
    """40 steps, the shipped controller, sinusoidal w_u on both actuators, a constant w_y, and limits at half the peak |u| of the
    unconstrained host loop: ``FlowSolver.run_closed_loop`` against ``_closed_loop_on_host`` on a second solver, y, u, dE and the
    final controller state within 1e-8 of each series' maximum (the project's closed-loop tolerance).  The clamp is honest: on the
    HOST loop's rows at least 5 steps have a clamped actuator and at least 5 have none."""
    n = 40
    w_y, w_u = _signals(n)
    host = _solver(golden_dir)

    def host_loop(limits):
        host.initialize_time_stepping(ic=None)
        host._begin_stepping()
        K = _shipped()
        y, u, dE = host._closed_loop_on_host(n, K, None, w_y=w_y, w_u=w_u, u_limits=limits)
        return y, u, dE, K.x.copy()

    peak = float(np.abs(host_loop(None)[1]).max())
    L = 0.5 * peak
    hy, hu, hdE, hx = host_loop((-L, L))
    host.th.release_device()
    at_limit = np.any(np.abs(hu) == L, axis=1)
    print(f"peak |u| without limits {peak:.4e}; {int(at_limit.sum())} of {n} host steps clamp")
    assert at_limit.sum() >= 5 and (~at_limit).sum() >= 5
    assert np.abs(hu).max() == L
    fs = prepared
    fs.params_ic = SMALL
    fs.initialize_time_stepping(ic=None)
    K = _shipped()
    y, u, dE = fs.run_closed_loop(n, K, w_y=w_y, w_u=w_u, u_limits=(-L, L))
    ts = fs.timeseries
    assert np.array_equal(ts[[c for c in ts.columns if c.startswith("u_ctrl_")]].to_numpy()[1:], u)  # the log holds the clamped u
    for name, a, b in (("y", y, hy), ("u", u, hu), ("dE", dE, hdE), ("x", K.x, hx)):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        dev_ = float(np.nanmax(np.abs(a - b)))
        print(f"{name}: largest deviation device - host {dev_:.3e}, series maximum {float(np.nanmax(np.abs(b))):.3e}")
        assert dev_ <= 1e-8 * float(np.nanmax(np.abs(b))), name
    assert np.abs(u).max() == L


# ── 4. the cursor ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_cursor_carries_the_rows_across_the_cuts_of_single_and_batched_runs(prepared, golden_dir):
    """A 50-step single run cut at ``save_every = 7`` (eight cuts) equals the run in one piece bit for bit; a batch of 8 with other rows
    in every column is bit-identical for chunk 1, 7 and 64, and its column i matches the single run with column i's rows at the
    tolerances of the batch test without signals (1e-12 for y and dE, 1e-11 for u and the controller state)."""
    n = 50
    w_y8, w_u8 = _signals(n, k=8)
    limits = (-4e-3, 4e-3)
    cut = _solver(golden_dir, n=n, ic=ICS[3], save_every=7)
    cut.initialize_time_stepping(ic=None)
    Kc = _shipped(GAINS[3])
    pieces = cut.run_closed_loop(n, Kc, w_y=w_y8[:, 3], w_u=w_u8[:, 3], u_limits=limits)
    cut.th.release_device()

    fs = prepared
    singles = []
    for i, a in enumerate(GAINS):
        fs.params_ic = ICS[i]
        fs.initialize_time_stepping(ic=None)
        K = _shipped(a)
        singles.append((*fs.run_closed_loop(n, K, w_y=w_y8[:, i], w_u=w_u8[:, i], u_limits=limits), K.x.copy()))
    for a, b in zip(pieces, singles[3][:3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(Kc.x, singles[3][3])

    def batch(chunk):
        bfs = BatchedFlowSolver(fs, 8)
        bfs.initialize_time_stepping(ics=ICS)
        Ks = [_shipped(a) for a in GAINS]
        out = bfs.run_closed_loop(n, Ks, chunk=chunk, w_y=w_y8, w_u=w_u8, u_limits=limits)
        assert not bfs.diverged.any()
        bfs.close()
        return (*out, np.stack([K.x for K in Ks]))

    b64 = batch(64)
    for chunk in (1, 7):
        for a, b in zip(batch(chunk), b64):
            assert np.array_equal(a, b, equal_nan=True), chunk
    y, u, dE, x = b64
    clamped = np.abs(u) == 4e-3
    print(f"batch: {int(clamped.sum())} of {u.size} controls at their limit")
    assert clamped.any() and not clamped.all()
    for i in range(8):
        y1, u1, dE1, x1 = singles[i]
        assert _rel(y[:, i], y1) < 1e-12 and _rel(dE[:, i], dE1) < 1e-12, f"run {i}"
        assert _rel(u[:, i], u1) < 1e-11 and _rel(x[i], x1) < 1e-11, f"run {i}"


# ── 5. an ended run stays ended ──────────────────────────────────────────────────────────────────────────────────────────────────
def test_an_ended_run_gets_no_excitation_and_leaves_the_others_alone(prepared):
    fs = prepared
    dev = fs.th.device()
    n = 5
    _, w_u = _signals(n, k=8)
    assert np.all(w_u[:, 2] != 0.0)

    def run(spoil):
        bfs = BatchedFlowSolver(fs, 8)
        bfs.initialize_time_stepping(ics=ICS)
        if spoil is not None:  # a non-finite entry in ONE run's state (as tests/test_closed_loop_gpu.py makes a run end)
            u_n, u_nn, p_n = dev.get_state_batch()
            u_n[spoil, 17] = np.inf
            dev.set_state_batch(u_n, u_nn, p_n)
        dev.set_controllers([_shipped(a) for a in GAINS], DT)
        dev.set_loop_signals(None, w_u)
        # one step more than there are rows: refused before anything is enqueued
        y0 = np.ascontiguousarray(bfs.y_meas)
        code = dev.lib.fc_run_closed_loop_batch(dev._h, SLOT_BDF1, 8, n + 1, y0, None, None, None, 1, None, None)
        assert code == _lib.FC_ERR_INVALID and dev.loop_cursor() == 0
        out = dev.run_closed_loop_batch(SLOT_BDF1, n, bfs.y_meas)
        assert dev.loop_cursor() == n
        dev.set_controllers(None, DT)
        bfs.close()
        return out

    yc, uc, dEc, badc, _ = run(None)
    assert np.all(badc == -1)
    y, u, dE, bad, info = run(2)
    assert bad.tolist() == [-1, -1, 0, -1, -1, -1, -1, -1] and info[2, 3] != 0
    assert np.all(u[1:, 2] == 0.0)  # from the step after the non-finite one on: no command, whatever w_u says
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal(y[:, keep], yc[:, keep]) and np.array_equal(u[:, keep], uc[:, keep]) and np.array_equal(dE[:, keep], dEc[:, keep])


# ── 6. refusals ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_refusals(prepared, golden_dir, monkeypatch):
    fs = prepared
    dev = fs.th.device()
    dev.set_batch(0)
    lib, h, p = dev.lib, dev._h, _lib.ptr
    n = 20
    _, w_u = _signals(n)
    one, two = np.ones((1, 2)), np.ones((2, 2))
    # no bank
    assert lib.fc_set_loop_signals(h, 1, n, None, p(np.ascontiguousarray(w_u))) != _lib.FC_OK
    assert lib.fc_set_control_limits(h, 1, p(-one), p(one)) != _lib.FC_OK

    def run(try_too_long):
        fs.params_ic = SMALL
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev.set_controllers([_shipped()], DT)
        dev.set_loop_signals(None, w_u)
        y0 = np.ascontiguousarray(np.asarray(fs.y_meas, dtype=np.float64))
        if try_too_long:
            # wrong k
            assert lib.fc_set_loop_signals(h, 2, n, None, p(np.zeros((n, 2, 2)))) == _lib.FC_ERR_INVALID
            assert lib.fc_set_control_limits(h, 2, p(-two), p(two)) == _lib.FC_ERR_INVALID
            # limits that are none
            assert lib.fc_set_control_limits(h, 1, p(one), p(-one)) == _lib.FC_ERR_INVALID
            assert lib.fc_set_control_limits(h, 1, p(np.array([[np.nan, 0.0]])), p(one)) == _lib.FC_ERR_INVALID
            assert lib.fc_set_control_limits(h, 1, p(-one), p(np.array([[1.0, np.nan]]))) == _lib.FC_ERR_INVALID
            assert lib.fc_set_control_limits(h, 1, p(-one), None) == _lib.FC_ERR_INVALID
            with pytest.raises(FcError):
                dev.set_control_limits(1.0, -1.0)
            # a run one step longer than the rows
            assert lib.fc_run_closed_loop(h, SLOT_BDF1, n + 1, y0, None, None, None, 1) == _lib.FC_ERR_INVALID
            assert dev.loop_cursor() == 0
        y, u, dE = dev.run_closed_loop(SLOT_BDF1, n, y0)
        assert dev.loop_cursor() == n
        if try_too_long:  # the rows are used up
            assert lib.fc_run_closed_loop(h, SLOT_BDF2, 1, y0, None, None, None, 1) == _lib.FC_ERR_INVALID
        x = dev.controller_state()
        dev.set_controllers(None, DT)
        return y, u, dE, x

    fresh = run(False)
    for a, b in zip(run(True), fresh):  # nothing was enqueued by the refused calls
        assert np.array_equal(a, b)
    # the public face refuses what the device would refuse
    with pytest.raises(ValueError):
        fs.run_closed_loop(3, _shipped(), u_limits=(1.0, -1.0))
    with pytest.raises(ValueError):
        fs.run_closed_loop(3, _shipped(), w_u=np.zeros((4, 2)))
    K = _shipped()
    L = 1e-3

    def first_u(f):  # what the host loop must command in its first step
        cmd = _shipped().step(y=-np.asarray(f.y_meas, dtype=np.float64)[:1] + 1e-3, dt=DT)
        return np.minimum(np.maximum(np.full(2, cmd[0]) + w_u[0], -L), L)

    # a Crank-Nicolson slot: refused with signals set, the public face runs the host loop with them
    cn = _solver(golden_dir, n=4)
    cn.params_solver.time_scheme = "cn"
    cn.initialize_time_stepping(ic=None)
    cn.step(u_ctrl=[0.0, 0.0])
    dcn = cn.th.device()
    dcn.set_controllers([K], DT)
    dcn.set_loop_signals(None, w_u)
    dcn.set_control_limits(-L, L)
    with pytest.raises(FcError, match="Crank-Nicolson"):
        dcn.run_closed_loop(SLOT_BDF1, 2, np.zeros(3))
    dcn.set_controllers(None, DT)
    expect = first_u(cn)
    out = cn.run_closed_loop(2, _shipped(), w_y=np.full((2, 1), 1e-3), w_u=w_u[:2], u_limits=(-L, L))
    assert out is not None and out[0].shape == (2, 3) and np.array_equal(out[1][0], expect) and np.abs(out[1]).max() <= L
    cn.th.release_device()
    # a partitioned handle
    monkeypatch.setenv("FC_FORCE_COMM", "1")
    part = _solver(golden_dir, n=4)
    part.initialize_time_stepping(ic=None)
    dp = part.th.device()
    dp.join(0, 1, lambda b: b)
    part._joined = True
    part.step([0.0, 0.0])
    assert dp.part is not None
    dp.set_controllers([K], DT)
    dp.set_loop_signals(None, w_u)
    with pytest.raises(FcError, match="partitioned"):
        dp.run_closed_loop(SLOT_BDF2, 2, np.zeros(3))
    dp.set_controllers(None, DT)
    expect = first_u(part)
    out = part.run_closed_loop(2, _shipped(), w_y=np.full((2, 1), 1e-3), w_u=w_u[:2], u_limits=(-L, L))
    assert out is not None and np.array_equal(out[1][0], expect) and np.abs(out[1]).max() <= L
    part.th.release_device()


# ── 7. nothing else moved ────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_plain_steps_after_setting_and_freeing_signals_are_those_of_a_fresh_solver(golden_dir):
    def ten_steps(fs):
        out = []
        for n in range(10):
            out.append(fs.step(u_ctrl=[0.05 * np.sin(0.3 * n), -0.02]).copy())
        ts = fs.timeseries
        return np.stack(out), ts["dE"].to_numpy().copy(), fs.fields.u_n.vector().get_local().copy()

    fresh = _solver(golden_dir, n=10)
    fresh.initialize_time_stepping(ic=None)
    ref = ten_steps(fresh)
    fresh.th.release_device()

    fs = _solver(golden_dir, n=10)
    fs.initialize_time_stepping(ic=None)
    fs._begin_stepping()
    dev = fs.th.device()
    dev.set_controllers([_shipped()], DT)
    dev.set_loop_signals(np.ones((4, 1, 1)), np.ones((4, 1, 2)))
    dev.set_control_limits(-0.5, 0.5)
    assert np.abs(dev.ctrl_apply(np.ones((1, 3)))).max() <= 0.5 and dev.loop_cursor() == 1
    dev.set_loop_signals(None, None)
    dev.set_control_limits(None, None)
    dev.set_controllers(None, DT)
    got = ten_steps(fs)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b, equal_nan=True)
    fs.th.release_device()


# ── 8. costs ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_costs_under_a_disturbance_and_limits_on_the_device_are_those_of_the_host_loop(golden_dir):
    fs = _solver(golden_dir, n=20)
    gains = [0.0, 0.5, 1.0, 2.0]
    n, pen = 20, 0.3
    w_y, w_u = _signals(n)
    kw = dict(u_penalty=pen, w_y=w_y, w_u=w_u, u_limits=(-4e-3, 4e-3))
    J_host, s_host = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, **kw)
    J_dev, s_dev = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, on_device=True, **kw)
    print("costs host", J_host, "device", J_dev)
    assert np.all(np.isfinite(J_host)) and np.all(np.abs(J_dev - J_host) <= 1e-7 * np.abs(J_host))
    ucols = [c for c in s_dev[0].columns if c.startswith("u_ctrl_")]
    u0 = s_dev[0][ucols].to_numpy()[1:]  # gain 0: the clamped excitation alone
    assert np.array_equal(u0, np.clip(w_u, -4e-3, 4e-3))
    J_plain, _ = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, u_penalty=pen, on_device=True)
    assert np.all(J_plain != J_dev)
    # one row set per candidate: the same rows four times are the shared rows
    per = dict(kw, w_y=np.repeat(w_y[:, None], 4, axis=1), w_u=np.repeat(w_u[:, None], 4, axis=1))
    again = optim.fun_array_batched(np.array(gains)[:, None], lambda r: _shipped(r[0]), fs, n, batch=4, on_device=True, **per)
    assert np.array_equal(again[:, 0], J_dev)
    fs.th.release_device()


# ── 9. identification, small ─────────────────────────────────────────────────────────────────────────────────────────────────────
def test_closed_loop_frequency_response_on_the_device_is_the_host_loops(golden_dir):
    """M = 4 realisations, N = 16, P = 3 from rest (no initial perturbation: the response is the excitation's alone): the device run
    against the same experiment stepped with the controllers on the host.  The plumbing, not the physics."""
    fs = _solver(golden_dir, n=48, ic=ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.0))
    kw = dict(N=16, P=3, M=4, amplitude=1e-2, fmin=0.1, fmax=0.6, P_skip=1, seed=3)
    state = np.random.get_state()[1].copy()
    dev = sysid.closed_loop_frequency_response(fs, _shipped(), on_device=True, **kw)
    host = sysid.closed_loop_frequency_response(fs, _shipped(), on_device=False, **kw)
    assert np.array_equal(np.random.get_state()[1], state)  # the caller's random stream is left alone
    assert np.array_equal(dev["bins"], [1, 2, 3, 4]) and np.array_equal(host["bins"], dev["bins"])
    assert np.allclose(dev["ww"], 2 * np.pi * dev["bins"] / (16 * DT), rtol=1e-15)
    assert dev["G"].shape == (4, 3) and dev["G_std"].shape == (4, 3) and dev["Y"].shape == (4, 4, 3) and dev["U"].shape == (4, 4)
    err = np.abs(dev["G"] - host["G"]) / np.abs(host["G"])
    print(f"largest relative deviation of G, device - host: {err.max():.3e}; |G| from {np.abs(host['G']).min():.3e} to {np.abs(host['G']).max():.3e}")
    assert np.all(np.isfinite(host["G"])) and err.max() <= 1e-8
    fs.th.release_device()
