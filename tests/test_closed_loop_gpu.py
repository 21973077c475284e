"""Closed loops on the device: the controller bank kernel (``fc_ctrl_step``), ``fc_run_closed_loop`` / ``fc_run_closed_loop_batch``
and their Python faces (``FlowSolver.run_closed_loop``, ``BatchedFlowSolver.run_closed_loop``, ``optim.closed_loop_costs(on_device=True)``)
against the host loop they replace: ``Controller.step`` between two ``step`` calls (reference ``controller.py:136-159``,
``examples/cylinder/run_cylinder_example.py``)."""
import tempfile

import numpy as np
import pytest

from flowcontrol_amd import _lib, optim
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from flowcontrol_amd.batch import BatchedFlowSolver
from flowcontrol_amd.controller import Controller, bank_step
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.examples.data import controller_file
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC

pytestmark = pytest.mark.gpu

# reference tests/integration/test_cylinder.py:66-74 (the constants tests/test_flowsolver_gpu.py::test_cylinder_regression holds)
_U0_MAX_REF = np.float64(1.1921615450014942)
_U0_MEAN_REF = np.float64(0.336746427968607)
_U_MAX_REF = np.float64(1.325070045534714)
_U_MEAN_REF = np.float64(0.3376859329866094)
_LAST_TIME_REF = np.float64(0.1)
_LAST_Y_MEAS_1_REF = np.float64(0.011615482723602308)
_LAST_Y_MEAS_2_REF = np.float64(0.003860524805395703)
_LAST_Y_MEAS_3_REF = np.float64(0.0038461597025207803)
_LAST_DE_REF = np.float64(0.09462807324653322)

DT = 0.005
EPS = 2.0**-53


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def _ycols(ts):
    return [c for c in ts.columns if c.startswith("y_meas_")]


def _ucols(ts):
    return [c for c in ts.columns if c.startswith("u_ctrl_")]


def _solver(golden_dir, n=50, ic=None, **kw):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=n, **kw)
    fs.params_ic = ic if ic is not None else ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
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


def _random_controller(rng, nx, nyc, nuc):
    if nx == 0:
        K = Controller(np.zeros((0, 0)), np.zeros((0, 1)), np.zeros((1, 0)), [[0.0]])  # (the constructor shapes static gains 1 x 1)
        K.B, K.C, K.D = np.zeros((0, nyc)), np.zeros((nuc, 0)), rng.standard_normal((nuc, nyc))
        K.ninputs, K.noutputs = nyc, nuc
        return K
    A = rng.standard_normal((nx, nx)) / np.sqrt(nx)
    A -= (np.max(np.linalg.eigvals(A).real) + 5.0) * np.eye(nx)
    return Controller(A, rng.standard_normal((nx, nyc)), rng.standard_normal((nuc, nx)), rng.standard_normal((nuc, nyc)))


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("nx", [0, 13, 64, 200])
def test_kernel_matches_numpy_within_the_rounding_bound(prepared, k, nx):
    """``fc_ctrl_apply`` over 50 steps of random measurements against numpy (float64).  The bound is derived: a sum of n products
    formed in any order errs by at most n eps sum |a_ij| |v_j| (eps = 2^-53, to first order); every output here is a chain of such
    products (yc = G y + g0, then uc = C x + D yc or x = Ad x + Bd yc, then u = S uc), so the error of each stage is bounded by
    (nx + nyc + 2) eps times the stage's sum of absolute products, carried through the absolute values of the later stages.  The
    state is reset to numpy's before every step, so the bound stays the one-step bound.  Two calls with the same input are
    bit-identical."""
    dev = prepared.th.device()
    n_sens, n_act = dev.n_sens, dev.n_act
    rng = np.random.default_rng(100 * k + nx)
    nyc, nuc = 2, n_act
    dev.set_batch(k if k > 1 else 0)
    Ks = [_random_controller(rng, nx, nyc, nuc) for _ in range(k)]
    for K in Ks:
        K.x = rng.standard_normal(nx)
    G, g0 = rng.standard_normal((k, nyc, n_sens)), rng.standard_normal((k, nyc))
    bank = dev.set_controllers(Ks, DT, feedback=(G, g0))
    assert bank["nx"] == nx
    x = bank["x0"].copy()
    assert np.array_equal(dev.controller_state(), x)
    c = (nx + nyc + 2) * EPS
    worst = 0.0
    for step in range(50):
        y = rng.standard_normal((k, n_sens))
        u_ref, x_ref = bank_step(bank, x, y)
        dev.controller_state(x)
        u = dev.ctrl_apply(y)
        x_dev = dev.controller_state()
        if step % 10 == 0:  # the same input again: the same bits
            dev.controller_state(x)
            assert np.array_equal(dev.ctrl_apply(y), u) and np.array_equal(dev.controller_state(), x_dev)
        for i in range(k):
            aG, aC, aD, aAd, aBd, aS = (np.abs(bank[m][i]) for m in ("G", "C", "D", "Ad", "Bd", "S"))
            yc_abs = aG @ np.abs(y[i]) + np.abs(bank["g0"][i])
            e_yc = c * yc_abs
            uc_abs = aC @ np.abs(x[i]) + aD @ yc_abs
            e_uc = c * uc_abs + aD @ e_yc
            e_u = c * (aS @ uc_abs) + aS @ e_uc
            e_x = c * (aAd @ np.abs(x[i]) + aBd @ yc_abs) + aBd @ e_yc
            assert np.all(np.abs(u[i] - u_ref[i]) <= e_u), (step, i, np.abs(u[i] - u_ref[i]).max(), e_u.max())
            assert np.all(np.abs(x_dev[i] - x_ref[i]) <= e_x), (step, i)
            worst = max(worst, float(np.max(np.abs(u[i] - u_ref[i]) / np.maximum(e_u, 1e-300))))
        x = x_ref
    print(f"k={k} nx={nx}: largest |err| / bound = {worst:.3f}")
    dev.set_controllers(None, DT)
    dev.set_batch(0)


def test_single_closed_loop_reproduces_the_reference_constants_and_the_host_loop(tmp_path_factory, golden_dir):
    """The cylinder case of ``test_cylinder_regression`` (same mesh, controller file, start time, step count) through
    ``FlowSolver.run_closed_loop``: the reference-held constants at that test's tolerances, and y, u, dE within 1e-8 of the same build's
    ``step`` + ``Controller.step`` loop."""
    import flowcontrol_amd.utils as flu

    def case(tag, on_device):
        path_out = tmp_path_factory.mktemp(tag)
        fs = CylinderFlowSolver.make_default(Re=100, path_out=path_out, num_steps=10, save_every=5)
        fs.compute_steady_state(method="picard", max_iter=3, tol=1e-7, u_ctrl=[0.0, 0.0])
        fs.compute_steady_state(method="newton", max_iter=25, u_ctrl=[0.0, 0.0], initial_guess=fs.fields.UP0)
        assert np.isclose(flu.apply_fun(fs.fields.U0, np.max), _U0_MAX_REF, rtol=1e-6)
        assert np.isclose(flu.apply_fun(fs.fields.U0, np.mean), _U0_MEAN_REF, rtol=1e-6)
        Kss = Controller.from_file(file=controller_file(), x0=None)

        def loop(f):
            if on_device:
                out = f.run_closed_loop(f.params_time.num_steps, Kss)
                assert out is not None
                return
            for _ in range(f.params_time.num_steps):
                u = Kss.step(y=-f.y_meas[0], dt=f.params_time.dt)
                f.step(u_ctrl=[u[0], u[0]])

        fs.initialize_time_stepping(ic=None)
        loop(fs)
        fs.write_timeseries()
        first = fs.timeseries.copy()
        x_mid = Kss.x.copy()
        fs.th.release_device()
        fr = CylinderFlowSolver.make_default(Re=100, path_out=path_out, num_steps=10, save_every=5, Tstart=0.05)
        fr.load_steady_state()
        fr.initialize_time_stepping(Tstart=fr.params_time.Tstart)
        loop(fr)
        fr.write_timeseries()
        second = fr.timeseries.copy()
        u_max, u_mean = flu.apply_fun(fr.fields.Usave, np.max), flu.apply_fun(fr.fields.Usave, np.mean)
        fr.th.release_device()
        return first, second, u_max, u_mean, x_mid, Kss.x.copy(), (fs.iter, fs.t, fr.iter, fr.t)

    first, second, u_max, u_mean, x_mid, x_end, where = case("cl_device", True)
    g = np.load(golden_dir / "cylinder_O1.npz")
    assert _rel(first[["y_meas_1", "y_meas_2", "y_meas_3"]].to_numpy(), g["cl_y"][:11]) < 1e-8
    assert _rel(first["dE"].to_numpy(), g["cl_dE"][:11]) < 1e-8
    last = second.iloc[-1]
    assert np.isclose(u_max, _U_MAX_REF, rtol=1e-4), f"u_max: {u_max} != {_U_MAX_REF}"
    assert np.isclose(u_mean, _U_MEAN_REF, rtol=1e-6), f"u_mean: {u_mean} != {_U_MEAN_REF}"
    assert np.isclose(last["time"], _LAST_TIME_REF, rtol=1e-6), f"time: {last['time']}"
    assert np.isclose(last["y_meas_1"], _LAST_Y_MEAS_1_REF, rtol=1e-4), f"y_meas_1: {last['y_meas_1']}"
    assert np.isclose(last["y_meas_2"], _LAST_Y_MEAS_2_REF, rtol=1e-4), f"y_meas_2: {last['y_meas_2']}"
    assert np.isclose(last["y_meas_3"], _LAST_Y_MEAS_3_REF, rtol=1e-4), f"y_meas_3: {last['y_meas_3']}"
    assert np.isclose(last["dE"], _LAST_DE_REF, rtol=1e-4), f"dE: {last['dE']}"
    assert _rel(second[["y_meas_1", "y_meas_2", "y_meas_3"]].to_numpy(), g["cl_y"][10:21]) < 1e-8
    # the same build's host loop
    h_first, h_second, _, _, hx_mid, hx_end, h_where = case("cl_host", False)
    assert where == h_where
    worst = 0.0
    for a, b in ((first, h_first), (second, h_second)):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
        assert np.array_equal(a["time"].to_numpy(), b["time"].to_numpy())
        for cols in (_ycols(a), _ucols(a), ["dE"]):
            x, y = a[cols].to_numpy()[1:], b[cols].to_numpy()[1:]
            assert np.array_equal(np.isnan(x), np.isnan(y))
            dev_ = float(np.nanmax(np.abs(x - y)))
            worst = max(worst, dev_ / float(np.nanmax(np.abs(y))))
            assert dev_ <= 1e-8 * float(np.nanmax(np.abs(y))), (cols, dev_)
    print(f"largest deviation device loop - host loop, relative to the series' maximum: {worst:.3e}")
    assert np.abs(x_mid - hx_mid).max() <= 1e-8 * np.abs(hx_mid).max()
    assert np.abs(x_end - hx_end).max() <= 1e-8 * np.abs(hx_end).max()


GAINS = [0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
# (small perturbations: with unit amplitude in the near wake the loops of gain >= 1 command |u| > 4 within ten steps and the
#  semi-implicit scheme blows up before step 50 -- on the host loop as on the device one -- which is not what these tests are about)
ICS = [ParamIC(xloc=2.0 + 0.1 * i, yloc=0.05 * i, radius=0.5, amplitude=0.02 + 0.002 * i) for i in range(8)]


def _batch_run(fs, chunk, n=50, spoil=None):
    bfs = BatchedFlowSolver(fs, 8)
    bfs.initialize_time_stepping(ics=ICS)
    if spoil is not None:  # a non-finite entry in ONE run's state (as tests/test_batch_gpu.py makes a run diverge)
        u_n, u_nn, p_n = bfs.dev.get_state_batch()
        u_n[spoil, 17] = np.inf
        bfs.dev.set_state_batch(u_n, u_nn, p_n)
    Ks = [_shipped(a) for a in GAINS]
    throw = fs.params_solver.throw_error
    fs.params_solver.throw_error = False
    try:
        out = bfs.run_closed_loop(n, Ks, chunk=chunk)
    finally:
        fs.params_solver.throw_error = throw
    series = [bfs.timeseries(i) for i in range(8)]
    diverged = bfs.diverged.copy()
    bfs.close()
    return out, series, np.stack([K.x for K in Ks]), diverged


def test_batch_of_eight_controllers_equals_the_single_runs_for_every_chunk(prepared):
    fs = prepared
    (y64, u64, dE64), series, x64, diverged = _batch_run(fs, 64)
    assert not diverged.any() and y64.shape == (50, 8, 3) and u64.shape == (50, 8, 2)
    for chunk in (1, 7):
        (y, u, dE), s2, x, _ = _batch_run(fs, chunk)
        assert np.array_equal(y, y64) and np.array_equal(u, u64) and np.array_equal(dE, dE64, equal_nan=True) and np.array_equal(x, x64)
        for a, b in zip(series, s2):
            cols = [c for c in a.columns if "runtime" not in c]
            assert np.array_equal(a[cols].to_numpy(), b[cols].to_numpy(), equal_nan=True)
    for i, a in enumerate(GAINS):
        fs.params_ic = ICS[i]
        fs.initialize_time_stepping(ic=None)
        K = _shipped(a)
        y1, u1, dE1 = fs.run_closed_loop(50, K)
        ts = series[i]
        assert _rel(ts[_ycols(ts)].to_numpy()[1:], y1) < 1e-12, f"run {i}"
        assert _rel(ts["dE"].to_numpy()[1:], dE1) < 1e-12
        assert _rel(ts[_ucols(ts)].to_numpy()[1:], u1) < 1e-11
        assert _rel(x64[i], K.x) < 1e-11
        assert np.array_equal(ts[_ycols(ts)].to_numpy()[1:], y64[:, i]) and np.array_equal(ts[_ucols(ts)].to_numpy()[1:], u64[:, i])


@pytest.mark.parametrize("chunk", [64, 7])
def test_a_run_that_ends_early_leaves_the_others_alone(prepared, chunk):
    fs = prepared
    (yc, uc, dEc), clean, _, _ = _batch_run(fs, chunk)
    dev = fs.th.device()
    # the C entry point names the step
    bfs = BatchedFlowSolver(fs, 8)
    bfs.initialize_time_stepping(ics=ICS)
    u_n, u_nn, p_n = dev.get_state_batch()
    u_n[2, 17] = np.inf
    dev.set_state_batch(u_n, u_nn, p_n)
    dev.set_controllers([_shipped(a) for a in GAINS], DT)
    y, u, dE, bad, info = dev.run_closed_loop_batch(SLOT_BDF1, 5, bfs.y_meas)
    assert bad.tolist() == [-1, -1, 0, -1, -1, -1, -1, -1] and info[2, 3] != 0
    assert np.all(u[1:, 2] == 0.0)  # from the step after the non-finite one on: no command
    assert np.array_equal(np.delete(y, 2, axis=1), np.delete(yc[:5], 2, axis=1))
    dev.set_controllers(None, DT)
    bfs.close()
    # the public face: that run's series ends there, the others equal a batch without it
    (y, u, dE), series, _, diverged = _batch_run(fs, chunk, spoil=2)
    assert diverged.tolist() == [False, False, True, False, False, False, False, False]
    assert np.all(np.isnan(y[:, 2])) and np.all(np.isnan(dE[:, 2]))
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal(y[:, keep], yc[:, keep]) and np.array_equal(u[:, keep], uc[:, keep]) and np.array_equal(dE[:, keep], dEc[:, keep])
    ts = series[2]
    assert np.all(np.isnan(ts[_ycols(ts)].to_numpy()[1:]))


def test_nothing_else_moved(golden_dir):
    """10 plain ``step`` calls after ``set_controllers``, a closed-loop run on a second solver and ``fc_set_controllers(k = 0)`` are
    bit-identical to 10 steps of a fresh solver."""
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

    other = _solver(golden_dir, n=10)
    other.initialize_time_stepping(ic=None)
    fs = _solver(golden_dir, n=10)
    fs.initialize_time_stepping(ic=None)
    fs._begin_stepping()
    dev = fs.th.device()
    dev.set_controllers([_shipped()], DT)
    dev.ctrl_apply(np.ones((1, 3)))
    assert other.run_closed_loop(7, _shipped()) is not None
    dev.set_controllers(None, DT)
    got = ten_steps(fs)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b, equal_nan=True)
    other.th.release_device()
    fs.th.release_device()


def test_costs_on_the_device_are_the_costs_of_the_host_loop(golden_dir):
    fs = _solver(golden_dir, n=20)
    gains = [0.0, 0.5, 1.0, 2.0]
    n, pen = 20, 0.3
    J_host, s_host = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, u_penalty=pen)
    J_dev, s_dev = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, u_penalty=pen, on_device=True)
    print("costs host", J_host, "device", J_dev)
    assert np.all(np.isfinite(J_host)) and np.all(np.abs(J_dev - J_host) <= 1e-7 * np.abs(J_host))
    for a, b in zip(s_host, s_dev):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
    G = np.zeros((1, 3))
    G[0, 0] = -1.0
    J_g, _ = optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, u_penalty=pen, feedback=(G, np.zeros(1)), on_device=True)
    assert np.array_equal(J_g, J_dev)
    again = optim.fun_array_batched(np.array(gains)[:, None], lambda r: _shipped(r[0]), fs, n, batch=3, u_penalty=pen, on_device=True)
    assert np.all(np.abs(again[:, 0] - J_host) <= 1e-7 * np.abs(J_host))
    with pytest.raises(TypeError, match="callable"):
        optim.closed_loop_costs(fs, [_shipped(a) for a in gains], n, feedback=lambda y: -y[0], on_device=True)
    with pytest.raises(TypeError, match="Controller"):
        optim.closed_loop_costs(fs, [lambda y, dt: 0.0] * 4, n, on_device=True)
    fs.th.release_device()


def test_refusals(prepared, golden_dir, monkeypatch):
    fs = prepared
    dev = fs.th.device()
    K = _shipped()
    dev.set_batch(0)
    y0 = np.zeros(3)
    with pytest.raises(FcError):  # no bank
        _lib.check(dev.lib.fc_ctrl_apply(dev._h, 1, np.zeros((1, 3)), np.zeros((1, 2))))
    with pytest.raises(FcError):
        _lib.check(dev.lib.fc_run_closed_loop(dev._h, SLOT_BDF2, 3, y0, None, None, None, 1))
    with pytest.raises(FcError):  # k larger than the batch
        dev.set_controllers([K, K], DT)
    dev.set_batch(4)
    with pytest.raises(FcError):
        dev.set_controllers([K] * 5, DT)
    dev.set_controllers([K] * 3, DT)
    with pytest.raises(FcError):  # the bank's k is not the batch's
        dev.run_closed_loop_batch(SLOT_BDF2, 2, np.zeros((4, 3)))
    with pytest.raises(FcError):  # ... nor 1
        dev.run_closed_loop(SLOT_BDF2, 2, y0)
    dev.set_batch(0)
    # sizes that do not match
    z = np.zeros(64)
    for nx, nyc, nuc in ((257, 1, 1), (4, 9, 1), (4, 0, 1), (4, 1, 33), (-1, 1, 1)):
        big = np.zeros(max(nx, 1) * max(nx, 1) + 4096)
        code = dev.lib.fc_set_controllers(dev._h, 1, nx, nyc, nuc, _lib.ptr(big), _lib.ptr(big), _lib.ptr(big), _lib.ptr(big), None, _lib.ptr(big),
                                          None, _lib.ptr(big))
        assert code == _lib.FC_ERR_INVALID, (nx, nyc, nuc)
    assert dev.lib.fc_set_controllers(dev._h, 1, 4, 1, 1, None, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), None, _lib.ptr(z), None, _lib.ptr(z)) == _lib.FC_ERR_INVALID
    with pytest.raises(ValueError):  # a controller with two inputs behind the one-row reference feedback
        dev.set_controllers([Controller(-np.eye(2), np.ones((2, 2)), np.ones((1, 2)), np.zeros((1, 2)))], DT)
    with pytest.raises(ValueError):
        dev.set_controllers([K], DT, feedback=(np.zeros((1, 5)), np.zeros(1)))
    dev.set_controllers([K], DT)
    with pytest.raises(FcError):
        dev.run_closed_loop(SLOT_BDF2, 0, y0)
    with pytest.raises(FcError):
        dev.run_closed_loop(7, 2, y0)
    dev.set_controllers(None, DT)
    with pytest.raises(TypeError):
        fs.run_closed_loop(3, K, feedback=lambda y: -y[0])
    with pytest.raises(TypeError):
        fs.run_closed_loop(3, lambda y: 0.0)
    # a Crank-Nicolson slot
    cn = _solver(golden_dir, n=4)
    cn.params_solver.time_scheme = "cn"
    cn.initialize_time_stepping(ic=None)
    cn.step(u_ctrl=[0.0, 0.0])
    dcn = cn.th.device()
    dcn.set_controllers([K], DT)
    with pytest.raises(FcError, match="Crank-Nicolson"):
        dcn.run_closed_loop(SLOT_BDF1, 2, y0)
    dcn.set_controllers(None, DT)
    host = cn.run_closed_loop(2, _shipped())  # the public face takes the host loop there
    assert host is not None and host[0].shape == (2, 3)
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
    with pytest.raises(FcError, match="partitioned"):
        dp.run_closed_loop(SLOT_BDF2, 2, y0)
    dp.set_controllers(None, DT)
    part.th.release_device()
