"""The energy term of the adjoint marches' cost on the host (tests/support/adjoint_energy_cases.py): the three host models with
``sum e_m dE_m`` in the cost against central differences of their own cost, the np.longdouble model of the new right-hand side and its
fp64 distance per mesh, and the cost mapping of ``optim.closed_loop_cost_gradients(signal="dE")``.  No GPU."""
import numpy as np
import pandas as pd
import pytest

from tests.support import adjoint_energy_cases as ec
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_march_cases as mc

L = np.longdouble
KINDS = {False: "lin", True: "nl"}


@pytest.fixture(scope="module")
def plants():
    out = {}
    for nl in (False, True):
        model, x0, xm1 = lc.host_plant(nl)
        out[nl] = (ec.with_energy(model), x0, xm1)
    return out


def _directional(J, h):
    return (J(h) - J(-h)) / (2.0 * h)


def _rel_fd(fd, gd):
    """|fd - g . d| / |fd|; a group the run does not depend on (the controller's Ad at n = 1: lambda_1 = 0) must give 0 = 0."""
    if fd == 0.0:
        assert gd == 0.0, gd
        return 0.0
    return abs(fd - gd) / abs(fd)


CASES = [(nonlinear, first_order, n) for n in (1, 2, 5) for first_order in (1, 2) for nonlinear in (False, True)]


def _measure(plants, nonlinear, first_order, n):
    """The largest model-vs-central-differences distance of one case, {(kind, "open" | "loop"): distance}; asserts on the way that the
    energy term shows in the gradients."""
    model, x0, xm1 = plants[nonlinear]
    kind = KINDS[nonlinear]
    e = ec.weights(n)
    assert len(set(e.tolist())) == n and (n < 2 or e[1] == 0.0) and np.count_nonzero(e) >= n - 1
    rng = np.random.default_rng(100 * n + first_order)
    nn2 = int(np.count_nonzero(model.M.diagonal()))
    ns, na = model.C.shape[0], model.n_act
    # open loop ------------------------------------------------------------------------------------------------------------------
    u = 0.3 * rng.standard_normal((n, na))
    w, z = rng.standard_normal((n, ns)), rng.standard_normal(model.N)
    X, _ = model.forward(first_order, u, x0, xm1)
    g, dx0, dxm1, _ = model.adjoint_energy(first_order, X, w, z, e)
    g_plain = model.adjoint(first_order, n, w, z)[0] if not nonlinear else model.adjoint(first_order, X, w, z)[0]
    assert lm.rel(g, g_plain) > 100 * ec.FD_TOL, "the energy term does not show in the gradient: the test would pass without it"
    worst = 0.0
    h = ec.FD_STEP_OPEN
    for grp, grad in (("u", g), ("x0", dx0), ("xm1", dxm1)):
        if grp == "xm1" and first_order == 1:
            assert not np.any(grad)
            continue
        d = rng.standard_normal(grad.shape)
        if grp != "u":
            d[nn2:] = 0.0
        J = {"u": lambda s: model.cost(first_order, u + s * d, x0, xm1, w, z, e), "x0": lambda s: model.cost(first_order, u, x0 + s * d, xm1, w, z, e),
             "xm1": lambda s: model.cost(first_order, u, x0, xm1 + s * d, w, z, e)}[grp]
        fd = _directional(J, h)
        err = _rel_fd(fd, float(np.sum(grad * d)))
        print(f"{kind} open, first order {first_order}, n = {n}, {grp}: {err:.2e}")
        worst = max(worst, err)
    worst_open = worst
    # closed loop ----------------------------------------------------------------------------------------------------------------
    loop0, w, r, z = lc.make_case(model, x0, xm1, first_order, n, limits=False, seed=40 + n)
    loop = ec.EnergyLoop.of(loop0, e)
    f = loop.forward()
    g = loop.adjoint(f, w, r, z)
    worst = 0.0
    for grp in lm.GROUPS:
        if grp == "dxm1" and first_order == 1:
            continue
        d = lc.fd_direction(grp, g[grp].shape, nn2=nn2)
        fd = loop.fd_directional(grp, d, ec.FD_STEP_LOOP, w, r, z)
        err = _rel_fd(fd, float(np.sum(g[grp] * d)))
        print(f"{kind} loop, first order {first_order}, n = {n}, {grp}: {err:.2e}")
        worst = max(worst, err)
    plain = lm.Loop.adjoint(loop0, loop0.forward(), w, r, z)
    assert lm.rel(g["C"], plain["C"]) > 100 * ec.FD_TOL
    return {(kind, "open"): worst_open, (kind, "loop"): worst}


@pytest.fixture(scope="module")
def measured(plants):
    """case -> what _measure gives for it, computed when first asked for and once: the tests that read it need no order among them."""
    cache = {}

    def of(case):
        if case not in cache:
            cache[case] = _measure(plants, *case)
        return cache[case]

    return of


@pytest.mark.parametrize("nonlinear", [False, True])
@pytest.mark.parametrize("first_order", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_model_gradient_matches_central_differences(measured, nonlinear, first_order, n):
    """Open loop: dJ/du, dJ/dx0, dJ/dx_{-1}; closed loop: every group of adjoint_loop_model.GROUPS (the controller's matrices, the feedback
    map, the signals, the initial states) -- the model's gradient along one random direction per group against central differences of the
    model's OWN cost at the steps of the GPU tests, with sensor weights w, control weights r, a terminal vector and the weights of
    ``weights(n)`` (distinct, one zero row).  For the linearised plant J is quadratic along a direction of (u, x0, x_{-1}), so central
    differences are exact up to rounding: the bound is the rounding's, HOST_FD_DISTANCE, not a truncation estimate."""
    for key, worst in measured((nonlinear, first_order, n)).items():
        assert worst <= ec.HOST_FD_DISTANCE[key], (key, worst)


def test_fd_constants_are_tight(measured):
    """Each HOST_FD_DISTANCE bounds what the twelve cases measure (taken from the module's fixture: this test stands alone, under any
    selection or order) and exceeds it by less than a factor of two; the GPU bound is the sibling tests' 1e-6 wherever that is larger
    than ten times the constant -- everywhere but in the nonlinear closed loop."""
    largest = {}
    for case in CASES:
        for key, worst in measured(case).items():
            largest[key] = max(largest.get(key, 0.0), worst)
    assert len(largest) == 4
    for key, val in largest.items():
        print(key, f"measured {val:.2e}, constant {ec.HOST_FD_DISTANCE[key]:.2e}")
        assert val <= ec.HOST_FD_DISTANCE[key] < 2 * val, (key, val)
    assert ec.FD_TOL_SIBLING == 1e-6 == lc.FD_TOL and ec.FD_STEP_LOOP == lc.FD_EPS
    assert [ec.fd_tol(*k) for k in (("lin", "open"), ("lin", "loop"), ("nl", "open"), ("nl", "loop"))] == [1e-6, 1e-6, 1e-6, 10 * 4.6e-7]


def _model(mesh):
    full, _, _ = mc.host_operators(mesh)
    return ec.EnergyMarchModel(mesh, 2, "dirichlet", "five", full)


def test_host_constants():
    """fp64 against np.longdouble of EnergyMarchModel.rhs per mesh, linearised and nonlinear: HOST_ADJ_EN_RHS_ERROR bounds every
    measurement and exceeds the largest by less than a factor of two.  The longdouble model itself: equal to M (Z (..)) + e M x formed
    from the parent's pieces (linearity) to longdouble rounding; and the two mistakes miss by orders of magnitude."""
    worst = [0.0, 0.0]
    for i, mesh in enumerate(ec.EN_MESHES):
        m = _model(mesh)
        z1, z2, x, w, e = ec.step_inputs(m, 11 + i)
        assert np.any(x[m.dofs]) and np.any(z1[m.dofs])
        nn2 = 2 * m.nn
        for nl in (False, True):
            c = mc.step_coeffs(1, 3, nl)
            xt = x if nl else None
            ref = m.rhs(z1, z2, c, w, None, xt, e=e, x_state=x)
            f64 = m.rhs(z1, z2, c, w, None, xt, T=np.float64, e=e, x_state=x)
            e2, ei = mc.rel2(f64[:nn2], ref[:nn2]), mc.relmax(f64[:nn2], ref[:nn2])
            print(f"{mesh} {'nonlinear' if nl else 'linearised'}: {e2:.2e} / {ei:.2e}")
            worst = [max(worst[0], e2), max(worst[1], ei)]
            # linearity: the parent's right-hand side plus e times the unmasked mass product of x
            free0 = m.free
            try:
                m.free = np.ones_like(free0)
                mass_x = mc.MarchModel.elem_part(m, x, np.zeros(m.N), (1.0, 0.0, 0.0, 0.0))
            finally:
                m.free = free0
            pieces = mc.MarchModel.rhs(m, z1, z2, c, w, None, xt) + L(e) * mass_x
            assert mc.rel2(ref, pieces) <= 64 * float(np.finfo(L).eps)
            for wrong in ("x_masked", "no_energy"):
                miss = mc.rel2(m.rhs(z1, z2, c, w, None, xt, wrong=wrong, e=e, x_state=x)[:nn2], ref[:nn2])
                assert miss >= 1e-6, (wrong, miss)
            # without a weight the subclass is the parent
            assert np.array_equal(m.rhs(z1, z2, c, w, None, xt), mc.MarchModel.rhs(m, z1, z2, c, w, None, xt))
    for got, const in zip(worst, ec.HOST_ADJ_EN_RHS_ERROR):
        assert got <= const < 2 * got, (got, const)


def test_routes_with_energy():
    """The six new codes stand behind the six old ones, grids unchanged; the names are DeviceSolver's."""
    from flowcontrol_amd.device import DeviceSolver

    assert len(DeviceSolver.ADJ_ELEM) == 7 and len(DeviceSolver.ADJ_ELEM_ENERGY) == 6
    for old, new in ec.ENERGY_OF.items():
        assert new == old + 6
    r = mc.predicted_route("9x9", 2, 5, {}, False, True, False)
    re = ec.route_with_energy(r)
    assert re[0] == ec.ELEM_EN and np.array_equal(re[1:], r[1:])


@pytest.mark.parametrize("criterion", ["integral", "terminal"])
def test_cost_mapping_reproduces_the_reference_cost(criterion):
    """(e, Q, R) of optim.energy_cost_weights on a synthetic time series -- an initial row without controls, then n rows:
    sum e_m dE_m + w0 dE_0 + 1/2 sum u^T R u  equals  compute_signal_cost(dE) + u_penalty compute_control_cost(u), as closed_loop_costs forms it."""
    from flowcontrol_amd import optim

    n, dt, na, ns, Tc, pen = 7, 0.005, 2, 3, 0.01, 0.35
    rng = np.random.default_rng(1)
    dE, u = rng.random(n + 1) + 0.1, rng.standard_normal((n, na))
    ts = pd.DataFrame({"time": dt * np.arange(n + 1), "dE": dE, "u_ctrl_1": np.r_[np.nan, u[:, 0]], "u_ctrl_2": np.r_[np.nan, u[:, 1]]})
    Tnorm_ref = dt / max(float(ts["time"].iloc[-1]) - Tc, dt)
    J_ref = optim.compute_signal_cost(ts["dE"].dropna(), Tnorm_ref, criterion) + pen * optim.compute_control_cost(ts[["u_ctrl_1", "u_ctrl_2"]], Tnorm_ref)
    e, Q, R, Tnorm, w0 = optim.energy_cost_weights(n, dt, ns, na, criterion, pen, Tc)
    assert Tnorm == Tnorm_ref and Q.shape == (ns, ns) and not Q.any() and np.array_equal(R, 2 * pen * Tnorm * np.eye(na))
    assert np.array_equal(e, np.full(n, Tnorm) if criterion == "integral" else np.r_[np.zeros(n - 1), 1.0])
    J = float(e @ dE[1:]) + w0 * dE[0] + 0.5 * float(np.einsum("mi,ij,mj->", u, R, u))
    assert abs(J - J_ref) <= 1e-14 * abs(J_ref)
    with pytest.raises(ValueError):
        optim.energy_cost_weights(n, dt, ns, na, "mean")


def test_energy_rows_of_the_python_layer():
    """adjoint.energy_rows: scalar, (n,), (n, k); wrong shapes refused; None stays None."""
    from flowcontrol_amd.adjoint import energy_rows

    assert energy_rows(None, 4) is None and energy_rows(None, 4, 3) is None
    assert np.array_equal(energy_rows(2.0, 3), [2.0, 2.0, 2.0]) and energy_rows(2.0, 3, 2).shape == (3, 2)
    assert np.array_equal(energy_rows([1.0, 0.0, 3.0], 3, 2), [[1, 1], [0, 0], [3, 3]])
    assert np.array_equal(energy_rows(np.arange(6.0).reshape(3, 2), 3, 2), np.arange(6.0).reshape(3, 2))
    for bad, k in (([1.0, 2.0], None), (np.ones((3, 2)), None), (np.ones((3, 3)), 2), (np.ones((2, 2)), 2)):
        with pytest.raises(ValueError):
            energy_rows(bad, 3, k)


def test_example_command_line_refuses_a_bad_cost_before_it_builds_a_solver():
    """``--cost`` without a value or with an unknown one ends in the argument parser (exit status 2, the choices named): no solver is
    built, no device is opened."""
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    for args, said in ((["--cost"], "expected one argument"), (["--cost", "bogus"], "invalid choice")):
        out = subprocess.run([sys.executable, "-m", "flowcontrol_amd.examples.cylinder.optimize_controller_gradient", *args], cwd=root, capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 2 and said in out.stderr and "Traceback" not in out.stderr, (out.returncode, out.stderr[-500:])


def test_clearing_the_weights_keeps_the_first_error():
    """adjoint._held_energy: the rows are set on the way in and cleared on the way out; if the march raised and the clearing raises too,
    the march's error is the one that comes out; a clearing that fails after a march that went through is reported; without rows the
    handle is not touched."""
    from flowcontrol_amd.adjoint import _held_energy

    class Dev:
        def __init__(self, fail_clear):
            self.calls, self.fail_clear = [], fail_clear

        def set_adjoint_energy(self, rows):
            self.calls.append(None if rows is None else "rows")
            if rows is None and self.fail_clear:
                raise RuntimeError("clearing refused")

    dev = Dev(False)
    with _held_energy(dev, np.ones(3)):
        assert dev.calls == ["rows"]
    assert dev.calls == ["rows", None]
    dev = Dev(True)
    with pytest.raises(ValueError, match="the march"):
        with _held_energy(dev, np.ones(3)):
            raise ValueError("the march failed")
    assert dev.calls == ["rows", None]
    with pytest.raises(RuntimeError, match="clearing refused"):
        with _held_energy(Dev(True), np.ones(3)):
            pass
    dev = Dev(True)
    with _held_energy(dev, None):
        pass
    assert dev.calls == []
