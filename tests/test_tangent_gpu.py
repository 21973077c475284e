"""The tangent-linear march on the MI355X (``fc_tangent_reserve``, ``fc_run_tangent``, ``fc_tangent_info``; csrc/fc_tangent.hip.h,
csrc/fc_tangent_run.hpp, flowcontrol_amd/tangent.py) against the scipy model of tests/support/tangent_model.py, against central
differences of the device's own forward run, and against the device's adjoint march through the dot-product identity.

Small problem: the nonlinear 7 x 5 square (N = 378, 70 cells, two Dirichlet actuators, one point sensor, one refinement sweep per
solve); the public functions run on the cylinder's O1 mesh."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd import utils as flu
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from tests.support import adjoint_nl_child as nl_case
from tests.support import adjoint_nl_model as nm
from tests.support import tangent_child as case
from tests.support.tangent_model import TangentModel

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY


@pytest.fixture(scope="module")
def square():
    sq = nl_case.NlSquare()
    yield sq
    sq.close()


@pytest.fixture()
def tan(square):
    """A tape of 6 steps and the tangent buffers for one test; both are released afterwards."""
    square.dev.adjoint_tape_reserve(6)
    square.dev.tangent_reserve(1)
    yield square
    square.dev.tangent_reserve(0)
    square.dev.adjoint_tape_reserve(0)
    for s in SLOTS:
        square.dev.set_adjoint_factors(s, -1)
    square.dev.set_time_scheme(square.dt, True)
    square.restart()


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


@pytest.mark.parametrize("first_order,n", case.CASES)
def test_single_march_against_the_model(tan, first_order, n):
    """1. dy, dx_n, dx_{n-1} within 1e-8 relative of the model with each of du, dx0, dxm1 given and NULL in turn; two marches
    bit-identical; against central differences of the device forward run (eps = 1e-4) within 1e-6; fc_tangent_info reports the
    eight-lane kernel.  70 cells: its last workgroup is partial.  (Measured defects: DESIGN section 5.6.)"""
    assert tan.th.mesh.cells.shape[0] == 70 and tan.dev.N == 378
    case.compare_tangent(tan, first_order, n, route=1)


def test_thread_per_cell_kernel():
    """2. The same comparison in a fresh child process with FC_ELEM_REG_MIN=1: the march runs fc_tan_elem_nl_reg (route 2)."""
    env = dict(os.environ, FC_ELEM_REG_MIN="1", PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "tangent_child.py"), "reg"], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    for ln in out.stdout.splitlines():
        if ln.startswith("tangent run"):
            print(ln)
    assert out.returncode == 0, f"child: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK reg" in out.stdout


@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_dot_product_identity_with_the_device_adjoint(tan, first_order, n):
    """3. <w, Phi v> = <Phi^T w, v> between the device tangent and the device adjoint on the SAME tape: the defect relative to the sum
    of the absolute terms is at most 1e-8.  (Figures: DESIGN section 5.6.)"""
    dev = tan.dev
    nn2 = 2 * tan.th.nn
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    slot = SLOT_BDF1 if first_order == 1 else SLOT_BDF2
    rng = np.random.default_rng(13)
    u, du = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    w, z = rng.standard_normal((n, dev.n_sens)), rng.standard_normal(dev.N)
    case.taped_run(tan, first_order, n, u)
    dy, dxn, _ = dev.run_tangent(slot, n, du, d0, dm1)
    g, gx0, gxm1 = dev.run_adjoint(slot, n, w, z)
    terms = [np.sum(w * dy), z @ dxn, -np.sum(g * du), -(gx0[:nn2] @ d0[:nn2]), -(gxm1[:nn2] @ dm1[:nn2])]
    defect = abs(sum(terms)) / sum(abs(t) for t in terms)
    print(f"device tangent x device adjoint, first order {first_order}, n = {n}: identity defect {defect:.3e}")
    assert defect <= 1e-8


def test_the_march_leaves_the_forward_state_alone(tan):
    """4. Adjoint gradients, the tape's columns, get_solution, the step counter and a further forward step are the same bits before
    and after a tangent march; a handle that never reserved launches what it launched."""
    dev = tan.dev
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    rng = np.random.default_rng(17)
    n = 4
    u, du = rng.standard_normal((n + 1, dev.n_act)), rng.standard_normal((n, dev.n_act))
    w, z = rng.standard_normal((n, dev.n_sens)), rng.standard_normal(dev.N)

    def observe(march):
        case.taped_run(tan, 1, n, u[:n])
        count = dev.step_counts()
        if march:
            dev.run_tangent(SLOT_BDF1, n, du, z, z)
        assert dev.step_counts() == count
        grads = dev.run_adjoint(SLOT_BDF1, n, w, z)
        tape, sol = dev.adjoint_tape_states(), dev.get_solution()
        y, _, _ = dev.step(SLOT_BDF2, u[n], compute_energy=False)
        return dict(zip(("g", "dx0", "dxm1", "tape", "solution", "y of a further step", "its solution"), [*grads, tape, sol, y, dev.get_solution()]))

    before, after = observe(False), observe(True)
    for name in before:
        assert np.array_equal(before[name], after[name]), f"{name} differs after a tangent march"
    # never reserved: same launches, same bits
    launches = [dev.sweep_launches(s).copy() for s in SLOTS]
    dev.tangent_reserve(0)
    dev.adjoint_tape_reserve(0)
    assert dev.tangent_info()["bytes"] == 0 and not dev.tangent_info()["reserved"]
    tan.restart()
    y_plain, _ = dev.run(SLOT_BDF1, n, u[:n], compute_energy=False)
    end_plain = dev.get_solution()
    dev.adjoint_tape_reserve(6)
    dev.tangent_reserve(1)
    assert dev.tangent_info()["bytes"] > 0
    _, y_taped = case.taped_run(tan, 1, n, u[:n])
    dev.run_tangent(SLOT_BDF1, n, du)
    assert np.array_equal(y_plain, y_taped) and np.array_equal(end_plain, dev.get_solution())
    assert all(np.array_equal(a, dev.sweep_launches(s)) for a, s in zip(launches, SLOTS))


def test_refusals(tan):
    """5. Every refusal returns its code with the reason in fc_last_error and enqueues nothing (the march counter stays)."""
    dev = tan.dev
    rng = np.random.default_rng(19)
    u = rng.standard_normal((8, dev.n_act))
    marches = dev.tangent_info()["marches"]
    # tape: not begun, another count, another first slot, overflowed, ended
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="not begun")
    case.taped_run(tan, 1, 4, u[:4])
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="holds 4 steps")
    refused(INV, dev.run_tangent, SLOT_BDF2, 4, match="first taped step")
    refused(INV, dev.run_tangent, SLOT_BDF1, 0, match="n_steps")
    dev.run_tangent(SLOT_BDF1, 4)
    dev.run(SLOT_BDF2, 4, u[4:])
    refused(INV, dev.run_tangent, SLOT_BDF1, 8, match="overflowed")
    tan.restart()
    refused(INV, dev.run_tangent, SLOT_BDF1, 4, match="not begun")
    # a step in flight
    case.taped_run(tan, 1, 2, u[:2])
    dev.step_begin(SLOT_BDF2, u[2])
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="in flight")
    dev.step_end()
    dev.run_tangent(SLOT_BDF1, 3)
    # an explicit right-hand-side operator (Crank-Nicolson) on a slot of the run
    dev.set_rhs_operator(SLOT_BDF2, (0.5 * tan.model.M)[:, : 2 * dev.nn])
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="Crank-Nicolson")
    dev.set_rhs_operator(SLOT_BDF2, None)
    dev.run_tangent(SLOT_BDF1, 3)
    # a linearised scheme, a Krylov method
    dev.set_time_scheme(tan.dt, False)
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="its own tangent")
    dev.set_time_scheme(tan.dt, True)
    dev.set_solver_options(refine=30, method="gmres")
    try:
        refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="Krylov")
    finally:
        dev.set_solver_options(refine=1, check_residual=1)
    # a checkpointed tape, no tape
    dev.adjoint_tape_reserve_sparse(6, 2)
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="checkpointed")
    dev.adjoint_tape_reserve_sparse(0, 0)
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="no tape is reserved")
    # no reserve; a reserve of another mode
    dev.tangent_reserve(0)
    refused(NOT_READY, dev.run_tangent, SLOT_BDF1, 3, match="fc_tangent_reserve")
    refused(INV, dev.tangent_reserve, 2)
    dev.tangent_reserve(1)
    dev.set_batch(4)
    try:
        assert not dev.tangent_info()["reserved"]  # (dropped with the mode it was laid out for)
        dev.tangent_reserve(1)
        assert dev.tangent_info()["KB"] == 4
        refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="fc_run_tangent_batch")
    finally:
        dev.set_batch(0)
    assert not dev.tangent_info()["reserved"] and dev.tangent_info()["marches"] == marches + 3


def test_partitioned_handles_are_refused():
    """5b. A handle with an exchange (a thread-rank partition through fc_set_host_exchange, in a child process) is refused by the
    reserve and by both marches with FC_ERR_INVALID and the reason."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "tangent_child.py"), "partitioned"], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, f"child: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK partitioned" in out.stdout


@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_body_force_actuators(tan, first_order, n):
    """5c. With body-force profiles on the two actuators (fc_set_force: B~ du then also holds the load vectors F du the gather adds) the
    tangent agrees with central differences of the device forward run within 1e-6 and with the device adjoint through the dot-product
    identity within 1e-8; the force term is shown to act."""
    from tests.support import step_cases as sc

    dev = tan.dev
    nn2 = 2 * tan.th.nn
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    slot = SLOT_BDF1 if first_order == 1 else SLOT_BDF2
    rng = np.random.default_rng(71)
    u, du = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    w, z = rng.standard_normal((n, dev.n_sens)), rng.standard_normal(dev.N)
    case.taped_run(tan, first_order, n, u)
    plain = dev.run_tangent(slot, n, du)[1]
    dev.set_force(sc.force_profiles(tan.th, 0))
    try:
        case.taped_run(tan, first_order, n, u)
        assert case.nm.rel(dev.run_tangent(slot, n, du)[1], plain) > 1e-6, "the body force does not act on the tangent"
        dy, dxn, _ = dev.run_tangent(slot, n, du, d0, dm1)
        g, gx0, gxm1 = dev.run_adjoint(slot, n, w, z)
        terms = [np.sum(w * dy), z @ dxn, -np.sum(g * du), -(gx0[:nn2] @ d0[:nn2]), -(gxm1[:nn2] @ dm1[:nn2])]
        defect = abs(sum(terms)) / sum(abs(t) for t in terms)

        def run(sign):
            dev.set_state(tan.u_n + sign * case.EPS * d0[:nn2], tan.u_nn + sign * case.EPS * dm1[:nn2], tan.p)
            yy, _ = dev.run(slot, n, u + sign * case.EPS * du, compute_energy=False)
            return yy, dev.get_solution()

        (yp, xp), (ym, xm) = run(1.0), run(-1.0)
        fd_y, fd_x = case.nm.rel(dy, (yp - ym) / (2 * case.EPS)), case.nm.rel(dxn, (xp - xm) / (2 * case.EPS))
        print(f"tangent run with body forces, first order {first_order}, n = {n}: identity defect {defect:.3e}, device central difference "
              f"y {fd_y:.3e}, x_n {fd_x:.3e}")
        assert defect <= 1e-8 and fd_y <= case.TOL_FD and fd_x <= case.TOL_FD
    finally:
        dev.set_force(None)


def test_gauss_newton_product_against_the_model(tan):
    """6. flu.gauss_newton_product on the square against the model's J^T Q J v + R v within 1e-8; v^T (G v) >= 0; G symmetric to 1e-10
    in two random directions; with a current tape the forward run is not repeated."""
    dev, model = tan.dev, tan.model
    tm = TangentModel(model)
    rng = np.random.default_rng(29)
    n = 5
    u = rng.standard_normal((n, dev.n_act))
    v, v2 = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    Q, R = np.array([[2.5]]), np.array([[0.3, 0.1], [0.0, 0.2]])
    Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    dev.adjoint_tape_reserve(0)
    with flu.AdjointRun(dev, tape=6) as adj:
        tan.restart()
        Gv = flu.gauss_newton_product(dev, u, Q, R, v, adjoint=adj)
        assert not dev.adjoint_tape_info()["begun"]  # (the run was taped by this call: the state is back, the tape ended)
        assert np.array_equal(dev.get_solution(), tan.x0)
        adj.forward(u, first_order=2, compute_energy=False)
        steps = dev.step_counts()[0]
        Gv_again = flu.gauss_newton_product(dev, u, Q, R, v, adjoint=adj)
        Gv2 = flu.gauss_newton_product(dev, u, Q, R, v2, adjoint=adj)
        assert dev.step_counts()[0] == steps, "the forward run was repeated on a current tape"
        assert np.array_equal(Gv, Gv_again)
    X, _ = model.forward(2, u, tan.x0, tan.xm1)
    dym = tm.tangent(2, X, v)[1]
    Gm = model.adjoint(2, X, dym @ Qs)[0] + v @ Rs
    err, sym = nm.rel(Gv, Gm), abs(np.sum(v2 * Gv) - np.sum(v * Gv2)) / abs(np.sum(v2 * Gv))
    print(f"gauss_newton_product on the square: against the model {err:.3e}, v.Gv = {np.sum(v * Gv):.6e}, symmetry defect {sym:.3e}")
    assert err <= 1e-8 and np.sum(v * Gv) >= 0.0 and sym <= 1e-10
    tan.restart()


# ── the public functions on the nonlinear cylinder, O1 ───────────────────────────────────────────────────────────────────────────
def test_public_functions_on_the_cylinder(golden_dir):
    """7. flu.tangent_run on the nonlinear cylinder (O1, 20 steps) against central differences of the forward device run in two random
    directions at eps = 1e-4: 1e-6 relative; and the dot-product identity <Q y, J v> = <J^T Q y, v> with the march of
    FlowSolver.cost_gradient within 1e-8 of the sum of the absolute terms.  The state is left where it was, tape and buffers released."""
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.params_solver.is_eq_nonlinear = True
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        n, nn2 = 20, 2 * fs.th.nn
        rng = np.random.default_rng(31)
        u = 0.5 * rng.standard_normal((n, dev.n_act))
        Q, R = np.diag(1.0 + np.arange(dev.n_sens)), 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2

        def run(uu, a=0.0, b=0.0):
            dev.set_state(state0[0] + a, state0[1] + b, *state0[2:])
            y, _ = dev.run(slot, n, uu, compute_energy=False)
            x = dev.get_solution()
            dev.set_state(*state0)
            return y, x

        eps, worst = 1e-4, 0.0
        for k in range(2):
            du, d0, dm1 = rng.standard_normal(u.shape), np.zeros(dev.N), np.zeros(dev.N)
            d0[:nn2], dm1[:nn2] = rng.standard_normal(nn2), rng.standard_normal(nn2)
            dy, dxn, _ = flu.tangent_run(fs, u, du, d0, dm1)
            assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state()))
            assert dev.adjoint_tape_info()["bytes"] == 0 and dev.tangent_info()["bytes"] == 0
            (yp, xp), (ym, xm) = run(u + eps * du, eps * d0[:nn2], eps * dm1[:nn2]), run(u - eps * du, -eps * d0[:nn2], -eps * dm1[:nn2])
            ey, ex = nm.rel(dy, (yp - ym) / (2 * eps)), nm.rel(dxn, (xp - xm) / (2 * eps))
            worst = max(worst, ey, ex)
            print(f"O1 nonlinear, 20 steps, direction {k}: tangent_run against central differences: y {ey:.3e}, x_n {ex:.3e}")
        assert worst <= 1e-6
        v = rng.standard_normal(u.shape)
        dy, _, _ = flu.tangent_run(fs, u, v)
        y, _ = run(u)
        _, grad = fs.cost_gradient(u, Q, R)
        lhs, rhs = float(np.sum((y @ Q) * dy)), float(np.sum((grad - u @ R) * v))
        defect = abs(lhs - rhs) / (abs(lhs) + abs(rhs))
        print(f"O1 nonlinear, 20 steps: <Q y, J v> = {lhs:.12e}, <J^T Q y, v> = {rhs:.12e}, identity defect {defect:.3e}")
        assert defect <= 1e-8
    finally:
        fs.th.release_device()
