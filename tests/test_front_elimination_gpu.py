"""Front elimination (csrc/fc_front.hip.h) with forced row exchanges on every kernel route.

On the assembled operators the diagonal of every pivot block passes the 8x threshold, so the exchange path of
fc_fe_gj_block -- inside fc_fe_pivot<32 / 64>, inside the look-ahead of fc_fe_update<32 / 64> and inside the sub-steps of
fc_fe_pivot_huge -- and the un-permute of the inverse's columns never run.  Here the device factorises the matrices of
tests/support/front_cases.py (exactly zero diagonals, the dominant entry elsewhere in the same 32-aligned pivot block;
condition 150 ... 200, checked with the exchange census in tests/test_front_cases_host.py) on its own sparsity pattern, through the
32-, 64- and 128-column kernels, against the numpy multifrontal of tests/support/nd_numeric.py, which inverts the pivot blocks
with LAPACK.  fc_get_refactor_steps tells which kernels ran: a route that was not taken fails the test."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import front_cases as fcs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=fcs.CASES, ids=[c[0] for c in fcs.CASES])
def case(request):
    """One handle per mesh and tree shape: a real operator for the structure, then the host references of both seeds."""
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from tests.support import nd_numeric, ndsolver

    name, nx, ny, bits, depth, merge = request.param
    th, dofs, tree = fcs.host_case(nx, ny, bits)
    dev = DeviceSolver(th)
    try:
        x = th.node_coords
        U0 = np.r_[1.0 + 0.3 * np.sin(x[:, 0]) * np.cos(0.7 * x[:, 1]), 0.2 * np.cos(0.5 * x[:, 0] + 0.1) * np.sin(x[:, 1])]
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.005, True)
        dev.assemble_matrix(SLOT_BDF2, mass=300.0, nu=0.01, adv=U0, lin=U0)
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2, depth=depth, merge=merge)
        assert tuple(dev.tree_info()["bits"]) == tuple(bits)
        dtree = ndsolver.tree_of(dev)  # (asserts the permutation)
        assert np.array_equal(dtree.perm, tree.perm) and fcs.level_fronts(dtree) == fcs.level_fronts(tree)
        rowptr, colidx = fcs.taylor_hood_pattern(th)
        assert np.array_equal(dev.rowptr, rowptr) and np.array_equal(dev.colidx, colidx)  # the pattern the host test judged the matrices on
        original = dev.matrix(SLOT_BDF2).data.copy()
        refs = {}
        for seed in fcs.SEEDS:
            vals = fcs.pivot_stress_matrix(dev.rowptr, dev.colidx, tree, dofs, seed)
            A = sp.csr_matrix((vals, dev.colidx.copy(), dev.rowptr.copy()), shape=(dev.N, dev.N))
            refs[seed] = (vals, A, nd_numeric.factorize_blocks(A, tree).vals)
        yield dev, tree, refs, original
    finally:
        dev.close()


@pytest.mark.parametrize("seed", fcs.SEEDS)
@pytest.mark.parametrize("route", list(fcs.ROUTES))
def test_forced_exchanges_on_every_route(case, route, seed, monkeypatch):
    from flowcontrol_amd.device import SLOT_BDF2

    dev, tree, refs, original = case
    vals, A, ref = refs[seed]
    want = fcs.predicted_step_widths(tree, route)
    try:
        for knob, value in fcs.ROUTES[route].items():  # read per factorisation: one handle serves all routes
            monkeypatch.setenv(knob, value)
        dev.set_matrix_values(SLOT_BDF2, vals)
        dev.refactor(SLOT_BDF2)
        assert not dev.factors_inexact[SLOT_BDF2]  # the acceptance solve took the factors as exact
        took = dev.refactor_step_widths()
        assert np.array_equal(took, want), f"route not taken: {route} expects block steps {want.tolist()} per level, the device took {took.tolist()}"
        got = dev.factor_values(SLOT_BDF2)
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"[{route}, seed {seed}] widths {took.tolist()} factor error {err:.2e} (max |value| {np.abs(ref).max():.3g})")
        assert err <= 1e-10
        b = np.random.default_rng(100 + seed).standard_normal(dev.N)
        x, info = dev.solve(SLOT_BDF2, b)
        res = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
        print(f"[{route}, seed {seed}] residual {res:.2e}, monitor {info[1]:.2e}")
        assert res < 1e-11
        assert np.isfinite(info[1])
        dev.refactor(SLOT_BDF2)  # fixed order of operations, ties to the smallest row: the same bits
        assert np.array_equal(dev.factor_values(SLOT_BDF2), got)
    finally:
        monkeypatch.undo()
        dev.set_matrix_values(SLOT_BDF2, original)
        dev.refactor(SLOT_BDF2)
    assert np.array_equal(dev.refactor_step_widths(), fcs.predicted_step_widths(tree, "default"))


def test_step_width_getter_error_paths():
    """fc_get_refactor_steps: status codes for a null handle, a short buffer and a handle that has not factorised yet."""
    from flowcontrol_amd._lib import FC_ERR_INVALID
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    FC_ERR_NOT_READY = -5
    th = TaylorHood(Mesh.unit_square(4, 4))
    dev = DeviceSolver(th, 0)
    try:
        lib, h = dev.lib, dev._h
        buf = np.full(8, -7, dtype=np.int32)
        assert lib.fc_get_refactor_steps(None, 8, buf) == FC_ERR_INVALID
        assert lib.fc_get_refactor_steps(h, 8, buf) == FC_ERR_NOT_READY
        assert b"fc_refactor" in lib.fc_last_error()
        dofs = fcs.dirichlet_dofs(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.01, True)
        dev.assemble_matrix(SLOT_BDF2, mass=150.0, nu=0.01)
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2)
        levels = len(dev.tree_info()["bits"]) + 1
        assert lib.fc_get_refactor_steps(h, levels - 1, buf) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error
        assert lib.fc_get_refactor_steps(h, levels, buf) == 0
        assert np.all(buf[:levels] == 32) and np.all(buf[levels:] == -7)
        assert dev.refactor_step_widths().tolist() == [32] * levels
    finally:
        dev.close()
