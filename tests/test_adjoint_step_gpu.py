"""Adjoint time stepping on the MI355X (``fc_set_adjoint_factors``, ``fc_solve_transposed``, ``fc_run_adjoint``, ``fc_step_adjoint``;
csrc/fc_adjoint.hip.h, flowcontrol_amd/adjoint.py) against the scipy model of tests/support/adjoint_step_model.py.

Small problem: the linearised stepping problem of tests/test_modal_gpu.py::square (``Mesh.unit_square(8, 8)``, N = 659, two Dirichlet
actuators, one point sensor) with both order slots set up; the FlowSolver level runs on the cylinder's O1 mesh."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib, adjoint, modal
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC
from tests.support import adjoint_layout, ndsolver
from tests.support import adjoint_step_child as case

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SLOTS = (SLOT_BDF1, SLOT_BDF2)


@pytest.fixture(scope="module")
def square():
    sq = case.Square()
    yield sq
    sq.close()


@pytest.fixture()
def adj(square):
    """Transposed factors of both slots for one test; released afterwards."""
    for s in SLOTS:
        square.dev.set_adjoint_factors(s, 1)
    yield square
    for s in SLOTS:
        square.dev.set_adjoint_factors(s, -1)


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def test_transposed_export_bit_for_bit(adj):
    """1. The adjoint value array equals transpose_values of the direct array bit for bit, both slots; the plan has partial export
    tiles (ni not a multiple of 32) and several tiles per panel (nb > 32)."""
    dev = adj.dev
    fac = ndsolver.factorize_blocks(None, ndsolver.tree_of(dev), numeric=False)
    shapes = adjoint_layout.node_shapes(fac.nodes, "block")
    assert any(ni % 32 for ni, _, _ in shapes) and any(nb > 32 for _, nb, _ in shapes) and any(ni > 32 for ni, _, _ in shapes)
    for s in SLOTS:
        direct = dev.factor_values(s)
        want = adjoint_layout.transpose_values(direct, fac.nodes, "block")
        got = dev.adjoint_factor_values(s)
        assert not np.array_equal(want, direct)
        assert np.array_equal(got, want), f"slot {s}: {np.count_nonzero(got != want)} of {want.size} values differ"
        info = dev.adjoint_info(s)
        assert info["available"] and not info["stale"] and info["exports"] == 1 and info["slot_bytes"] >= 8 * direct.size


def test_transposed_solve(adj):
    """2. solve_transposed against splu(A).solve(b, trans="T") at 1e-10 relative; fc_solve of the same b is more than
    1e-3 away from it (the operator has convection); fc_solve before and after is bit-identical."""
    dev = adj.dev
    b = np.cos(0.61 * np.arange(dev.N) + 0.3)
    for order, s in ((1, SLOT_BDF1), (2, SLOT_BDF2)):
        x_before, _ = dev.solve(s, b)
        xt, info = dev.solve_transposed(s, b)
        x_after, info_d = dev.solve(s, b)
        ref = spla.splu(adj.A[order].tocsc()).solve(b, trans="T")
        e_t, e_d = case.rel(xt, ref), case.rel(x_after, ref)
        print(f"slot {s}: transposed solve error {e_t:.3e} (residual reported {info[1]:.3e}), direct solve distance {e_d:.3e}")
        assert e_t <= 1e-10
        assert e_d > 1e-3
        assert info[0] == info_d[0] and info[1] <= 1e-10
        assert np.array_equal(x_before, x_after)
        assert np.array_equal(dev.solve_transposed(s, b)[0], xt)


def test_adjoint_run_against_the_model(adj):
    """3. n = 12 from a BDF1 first step, random w, a terminal vector, non-zero controls on both actuators: g, dx0, dxm1 within 1e-8
    relative of the model, the dot-product identity of the device forward run with the device adjoint run at 1e-8, two identical
    adjoint runs bit-identical.  (Measured defects: DESIGN section 5.4.)"""
    case.compare_run(adj, 1, 12)


def test_second_startup_case(adj):
    """4. BDF2 from (x0, x_{-1}), n = 3: the shortest run in which cm_n and cm_nn both act on both state gradients."""
    out = case.compare_run(adj, 2, 3)
    assert out["dxm1"] > 0.0


@pytest.mark.parametrize("first_order,n", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_shortest_runs(adj, first_order, n):
    """The edges of the backward schedule: n = 1 (no later step weighs x_1, the BDF2 slot is touched only if the first step ran on it,
    dx0 has one term) and n = 2 (the first run in which mu_2 enters dx0), from either first slot; the figures and the bound of test 3."""
    out = case.compare_run(adj, first_order, n)
    assert (out["dxm1"] > 0.0) == (first_order == 2)


def test_single_steps_are_the_run(adj):
    """fc_adjoint_reset / fc_step_adjoint / fc_adjoint_mass_product, driven from the host with the run's coefficients, give the run's
    numbers bit for bit."""
    dev, dt = adj.dev, adj.dt
    n = 4
    rng = np.random.default_rng(11)
    w, z = rng.standard_normal((n, dev.n_sens)), rng.standard_normal(dev.N)
    g, dx0, dxm1 = dev.run_adjoint(SLOT_BDF1, n, w, z)
    dev.adjoint_reset(z)
    gs = np.zeros_like(g)
    for m in range(n, 0, -1):
        cn = 2.0 / dt if m + 1 <= n else 0.0
        cnn = -0.5 / dt if m + 2 <= n else 0.0
        gs[m - 1] = dev.step_adjoint(SLOT_BDF1 if m == 1 else SLOT_BDF2, cn, cnn, w[m - 1])
    assert np.array_equal(gs, g)
    assert np.array_equal(dev.adjoint_mass_product(1.0 / dt, -0.5 / dt), dx0)
    assert np.array_equal(dev.adjoint_mass_product(0.0, 0.0), dxm1)


def test_nothing_else_moved(square):
    """5. A forward series (y, dE), the state, the step count seen by a snapshot bank and the bank's columns are bit-identical before and
    after an adjoint setup, run and release; the bytes adjoint_info reports return to zero."""
    dev = square.dev
    u = np.random.default_rng(4).standard_normal((9, dev.n_act))

    def series():
        square.restart()
        bank = modal.SnapshotBank(dev, 4, every=2, first=1)
        try:
            y, dE = dev.run(SLOT_BDF1, 9, u)
            return y, dE, [np.array(a, copy=True) for a in dev.get_state()], bank.get(), bank.info()["steps"]
        finally:
            bank.close()

    before = series()
    assert all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    assert dev.adjoint_info(SLOT_BDF2)["bytes"] > 0
    square.restart()
    bank = modal.SnapshotBank(dev, 4, every=2, first=1)
    try:
        dev.run(SLOT_BDF1, 5, u[:5])
        mid = [np.array(a, copy=True) for a in dev.get_state()]
        steps_mid, cols_mid = bank.info()["steps"], bank.get()
        dev.run_adjoint(SLOT_BDF1, 6, np.ones((6, dev.n_sens)), np.ones(dev.N))
        assert dev.adjoint_info(SLOT_BDF2)["shared_bytes"] > 0
        assert all(np.array_equal(a, b) for a, b in zip(mid, dev.get_state()))
        assert bank.info()["steps"] == steps_mid and np.array_equal(bank.get(), cols_mid)
        y_rest, dE_rest = dev.run(SLOT_BDF2, 4, u[5:])  # the run goes on where it stood
    finally:
        bank.close()
    with_adj = series()
    for s in SLOTS:
        dev.set_adjoint_factors(s, -1)
    assert all(dev.adjoint_info(s)["bytes"] == 0 and not dev.adjoint_info(s)["available"] for s in SLOTS)
    after = series()
    for other in (with_adj, after):
        assert np.array_equal(before[0], other[0]) and np.array_equal(before[1], other[1])
        assert all(np.array_equal(a, b) for a, b in zip(before[2], other[2]))
        assert np.array_equal(before[3], other[3]) and before[4] == other[4]
    assert np.array_equal(y_rest, before[0][5:]) and np.array_equal(dE_rest, before[1][5:])


def test_staleness_and_refusals(square):
    """6. A refactorisation of the slot gives the right answer on the NEW operator; fc_update_operator and fc_apply_bc leave the
    transposed values stale (FC_ERR_NOT_READY); every refusal that can be built on the square is refused with its reason."""
    dev, dt = square.dev, square.dt
    b = np.sin(0.37 * np.arange(dev.N) + 0.2)
    INV, NOT = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
    refused(NOT, dev.solve_transposed, SLOT_BDF2, b, match="fc_set_adjoint_factors")  # nothing built
    refused(NOT, dev.run_adjoint, SLOT_BDF2, 2, None, b)
    refused(INV, dev.set_adjoint_factors, SLOT_BDF2, 2)
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    try:
        # switched off, and on again without a rebuild
        dev.set_adjoint_factors(SLOT_BDF2, 0)
        refused(NOT, dev.solve_transposed, SLOT_BDF2, b, match="switched off")
        dev.set_adjoint_factors(SLOT_BDF2, 1)
        assert dev.adjoint_info(SLOT_BDF2)["exports"] == 1
        # a Krylov method selected; a nonlinear time scheme (the step only, not the transposed solve)
        dev.set_solver_options(refine=20, method="gmres")
        refused(INV, dev.solve_transposed, SLOT_BDF2, b, match="Krylov")
        refused(INV, dev.run_adjoint, SLOT_BDF2, 2, None, b, match="Krylov")
        dev.set_solver_options(refine=1, method="refine")
        dev.set_time_scheme(dt, True)
        refused(INV, dev.run_adjoint, SLOT_BDF2, 2, None, b, match="nonlinear")
        refused(INV, dev.step_adjoint, SLOT_BDF2, 1.0, 0.0, match="nonlinear")
        dev.solve_transposed(SLOT_BDF2, b)
        dev.set_time_scheme(dt, False)
        # an explicit right-hand-side operator (Crank-Nicolson)
        dev.set_rhs_operator(SLOT_BDF2, (0.5 * square.M)[:, : 2 * dev.nn])
        refused(INV, dev.run_adjoint, SLOT_BDF2, 2, None, b, match="Crank-Nicolson")
        dev.set_rhs_operator(SLOT_BDF2, None)
        # a new operator in the slot: lagged factors are stale, a refactorisation follows the new operator
        dev.assemble_matrix(SLOT_BDF2, mass=1.5 / dt, nu=3.0 / square.Re, adv=square.U0, lin=square.U0)
        dev.apply_bc(SLOT_BDF2)
        refused(NOT, dev.solve_transposed, SLOT_BDF2, b)
        dev.update_operator(SLOT_BDF2)
        assert dev.adjoint_info(SLOT_BDF2)["stale"]
        refused(NOT, dev.solve_transposed, SLOT_BDF2, b, match="stale")
        refused(NOT, dev.run_adjoint, SLOT_BDF2, 2, None, b, match="stale")
        dev.refactor(SLOT_BDF2)
        assert not dev.adjoint_info(SLOT_BDF2)["stale"] and dev.adjoint_info(SLOT_BDF2)["exports"] == 2
        A_new = dev.matrix(SLOT_BDF2)
        xt, _ = dev.solve_transposed(SLOT_BDF2, b)
        assert case.rel(xt, spla.splu(A_new.tocsc()).solve(b, trans="T")) <= 1e-10
        assert case.rel(xt, spla.splu(square.A[2].tocsc()).solve(b, trans="T")) > 1e-6
        # the other slot was not touched
        assert not dev.adjoint_info(SLOT_BDF1)["stale"]
    finally:
        dev.set_rhs_operator(SLOT_BDF2, None)
        dev.set_time_scheme(dt, False)
        dev.set_solver_options(refine=1, method="refine")
        dev.assemble_matrix(SLOT_BDF2, mass=1.5 / dt, nu=1.0 / square.Re, adv=square.U0, lin=square.U0)
        dev.apply_bc(SLOT_BDF2)
        dev.refactor(SLOT_BDF2)
        for s in SLOTS:
            dev.set_adjoint_factors(s, -1)
    assert np.array_equal(dev.matrix(SLOT_BDF2).data, square.A[2].data)


def test_refusals_of_other_factor_kinds():
    """6 (continued). Compressed, truncated and factor-free slots on handles of their own."""
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    th = TaylorHood(Mesh.unit_square(8, 8))
    dofs, prof = case.bc_setup(th)
    U0 = case.smooth_velocity(th)
    INV = _lib.FC_ERR_INVALID
    for kind in ("compressed", "truncated", "factor_free"):
        dev = DeviceSolver(th)
        try:
            dev.set_bc(dofs, prof)
            dev.set_time_scheme(0.005, False)
            if kind == "compressed":
                dev.set_factor_precision(32)
            dev.assemble_matrix(SLOT_BDF2, mass=300.0, nu=0.01, adv=U0, lin=U0)
            dev.apply_bc(SLOT_BDF2)
            if kind == "factor_free":
                dev.setup_krylov(SLOT_BDF2)
                refused(INV, dev.set_adjoint_factors, SLOT_BDF2, 1, match="no factors")
            elif kind == "truncated":
                dev.setup_solver(SLOT_BDF2, truncate=1)
                dev.set_solver_options(refine=1, method="refine")
                refused(INV, dev.set_adjoint_factors, SLOT_BDF2, 1, match="truncated")
            else:
                dev.setup_solver(SLOT_BDF2)
                dev.set_solver_options(refine=1, method="refine")
                refused(INV, dev.set_adjoint_factors, SLOT_BDF2, 1, match="compressed")
            assert dev.adjoint_info(SLOT_BDF2)["bytes"] == 0
        finally:
            dev.close()


def _child(mode, extra_env):
    env = {k: v for k, v in os.environ.items() if k != "FC_UP_FORM"}
    env.update(extra_env, PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "adjoint_step_child.py"), mode], env=env, capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    for ln in out.stdout.splitlines():
        if ln.startswith("adjoint run"):
            print(ln)
    assert out.returncode == 0, f"child {mode}: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert f"CHILD OK {mode}" in out.stdout


def test_partitioned_handle_is_refused():
    """6 (continued). A thread-rank (host exchange) handle takes no transposed factors; in a child process."""
    _child("partitioned", {})


def test_column_form_up_sweep():
    """7. Test 3's comparison in a fresh child process with FC_UP_FORM=column: the column-form up-sweep reads the transposed array."""
    _child("run", {"FC_UP_FORM": "column"})


# ── FlowSolver level: the linearised cylinder on O1 ─────────────────────────────────────────────────────────────────────────────
def _solver(golden_dir, linear=True):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.params_solver.is_eq_nonlinear = not linear
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


def test_flowsolver_gradient_against_central_differences(golden_dir):
    """8. quadratic_cost_gradient on the linearised cylinder (O1, 20 steps) against central differences of the forward device run in
    three random directions.  J is quadratic in u: the central difference has no truncation error at any step, so the step is of the
    size of u itself; agreement 1e-8 relative.  FlowSolver.adjoint_run returns the same march; the state is left where it was."""
    fs = _solver(golden_dir)
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        n = 20
        rng = np.random.default_rng(20)
        u = 0.5 * rng.standard_normal((n, dev.n_act))
        Q = np.diag(1.0 + np.arange(dev.n_sens))
        R = 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        with adjoint.AdjointRun(fs) as run:
            J, grad = adjoint.quadratic_cost_gradient(fs, u, Q, R, adjoint=run)
            assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state()))
            worst = 0.0
            for k in range(3):
                d = 0.5 * rng.standard_normal(u.shape)
                Jp, _ = adjoint.quadratic_cost_gradient(fs, u + d, Q, R, adjoint=run)
                Jm, _ = adjoint.quadratic_cost_gradient(fs, u - d, Q, R, adjoint=run)
                fd, ad = 0.5 * (Jp - Jm), float(np.sum(grad * d))
                err = abs(fd - ad) / abs(fd)
                worst = max(worst, err)
                print(f"O1 linearised, 20 steps: J = {J:.6e}, direction {k}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.3e}")
            assert worst <= 1e-8
            info = run.info()
            print(f"adjoint setup on O1: {info['bytes'] / 2**20:.1f} MiB, export {info['export_ms']:.2f} ms")
            # FlowSolver.adjoint_run is the same march with its own setup
            y, _ = dev.run(SLOT_BDF1, n, u, compute_energy=False)
            dev.set_state(*state0)
            g_run, _, _ = run.run(n, w=y @ Q, first_order=1, state_gradients=False)
        g_fs, dx0, dxm1 = fs.adjoint_run(n, w=y @ Q)
        assert np.array_equal(g_fs, g_run) and dx0.shape == (dev.N,) and not dxm1.any()
        assert all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
    finally:
        fs.th.release_device()


def test_nonlinear_flowsolver_is_refused(golden_dir):
    """8 (continued). is_eq_nonlinear=True: ValueError naming the condition, before anything touches the device."""
    fs = _solver(golden_dir, linear=False)
    with pytest.raises(ValueError, match="is_eq_nonlinear"):
        fs.adjoint_run(5)
    with pytest.raises(ValueError, match="is_eq_nonlinear"):
        adjoint.quadratic_cost_gradient(fs, np.zeros((5, 2)), np.eye(1), np.eye(2))
