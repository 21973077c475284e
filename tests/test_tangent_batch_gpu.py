"""The batched tangent-linear march on the MI355X (``fc_run_tangent_batch``; csrc/fc_tangent.hip.h, csrc/fc_tangent_run.hpp) against the
single march column by column, against the scipy model of tests/support/tangent_model.py about a shared reference trajectory, and the
Floquet driver of flowcontrol_amd/tangent.py through the device backend against the numpy backend.

The nonlinear 7 x 5 square (N = 378, 70 cells); k = 1, 5, 17 give the widths KB = 4, 8, 32, each with padding columns."""
import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd import utils as flu
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcDiverged, FcError
from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_nl_child as nl_case
from tests.support.tangent_model import ModelTangentBlocks, TangentModel

pytestmark = pytest.mark.gpu

TOL = 1e-8
KMAX = 17
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY


def slot_of(first_order):
    return SLOT_BDF1 if first_order == 1 else SLOT_BDF2


def column_inputs(sq, n):
    """Per column, the same for every k: start states, controls and the three perturbations (all different per column)."""
    un, unn, pp = bc.column_states(sq.u_n, sq.u_nn, sq.p, KMAX)
    rng = np.random.default_rng(53)
    na, N = sq.dev.n_act, sq.dev.N
    return {"un": un, "unn": unn, "pp": pp, "u": rng.standard_normal((n, KMAX, na)), "du": rng.standard_normal((n, KMAX, na)),
            "d0": rng.standard_normal((KMAX, N)), "dm1": rng.standard_normal((KMAX, N))}


def with_twin(a, k, axis):
    """The first k columns, the last one a copy of column 0 (k > 1): equal columns must come out bit-equal."""
    a = np.array(np.take(a, range(k), axis=axis))
    if k > 1:
        idx = [slice(None)] * a.ndim
        src = list(idx)
        idx[axis], src[axis] = k - 1, 0
        a[tuple(idx)] = a[tuple(src)]
    return np.ascontiguousarray(a)


@pytest.fixture(scope="module")
def square():
    sq = nl_case.NlSquare(refine=0)
    yield sq
    sq.close()


@pytest.fixture(scope="module")
def singles(square):
    """The single march of every column's run, once per case: {(first order, n): (dy [n, K, ns], dxn [K, N], dxnm1 [K, N])}."""
    dev = square.dev
    dev.adjoint_tape_reserve(6)
    dev.tangent_reserve(1)
    out = {}
    for first_order, n in nl_case.CASES:
        c = column_inputs(square, n)
        rows = []
        for s in range(KMAX):
            dev.set_state(c["un"][s], c["unn"][s], c["pp"][s])
            dev.adjoint_tape_begin()
            dev.run(slot_of(first_order), n, c["u"][:, s], compute_energy=False)
            rows.append(dev.run_tangent(slot_of(first_order), n, c["du"][:, s], c["d0"][s], c["dm1"][s]))
        out[(first_order, n)] = (np.stack([r[0] for r in rows], axis=1), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))
    dev.tangent_reserve(0)
    dev.adjoint_tape_reserve(0)
    square.restart()
    return out


def batch_on(sq, k, tape=6):
    dev = sq.dev
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(k)
    dev.adjoint_tape_reserve_batch(tape)
    dev.tangent_reserve(1)


def batch_off(sq):
    dev = sq.dev
    dev.tangent_reserve(0)
    dev.adjoint_tape_reserve_batch(0)
    dev.set_batch(0)
    dev.set_solver_options(refine=0, check_residual=1)
    sq.restart()


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


@pytest.mark.parametrize("k", [1, 5, 9, 17])
@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_batched_march(square, singles, first_order, n, k):
    """1. ref_col = -1: every column within 1e-8 of the single march of its run, equal columns bit-equal, two marches bit-identical.
    ref_col = 2 (0 for k = 1): every column within 1e-8 of the model's tangent about that trajectory.  A NaN planted in one column's
    dx0 marks that column alone; the others are the clean march's bits.  (Measured defects: DESIGN section 5.6.)"""
    dev, tm = square.dev, TangentModel(square.model)
    slot = slot_of(first_order)
    c = column_inputs(square, n)
    un, unn, pp = (with_twin(c[a], k, 0) for a in ("un", "unn", "pp"))
    u, du = with_twin(c["u"], k, 1), with_twin(c["du"], k, 1)
    d0, dm1 = with_twin(c["d0"], k, 0), with_twin(c["dm1"], k, 0)
    ref = singles[(first_order, n)]
    batch_on(square, k)
    try:
        assert dev.tangent_info()["KB"] == {1: 4, 5: 8, 9: 16, 17: 32}[k]
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, first_order, u, tape=True)
        X = dev.adjoint_tape_states_batch()  # [n + 2, k, N]
        dy, dxn, dxnm1 = dev.run_tangent_batch(slot, n, du, d0, dm1)
        again = dev.run_tangent_batch(slot, n, du, d0, dm1)
        assert all(np.array_equal(a, b) for a, b in zip((dy, dxn, dxnm1), again)), "two identical batched marches differ"
        assert dev.tangent_info()["route"] == 3 and dev.tangent_info()["steps"] == n
        own = k - 1 if k > 1 else 1  # (columns with a run of their own)
        nn2 = 2 * square.th.nn
        out = {"dy": bc.rel_columns(dy[:, :own], ref[0][:, :own], 1), "dxn": bc.rel_columns(dxn[:own], ref[1][:own], 0),
               "dxnm1": bc.rel_columns(dxnm1[:own, :nn2], ref[2][:own, :nn2], 0)}
        if k > 1:
            assert np.array_equal(dy[:, k - 1], dy[:, 0]) and np.array_equal(dxn[k - 1], dxn[0]) and np.array_equal(dxnm1[k - 1], dxnm1[0])
        # every column about ONE trajectory
        rc = 2 if k > 2 else 0
        sy, sxn, sxnm1 = dev.run_tangent_batch(slot, n, du, d0, dm1, rc)
        assert dev.tangent_info()["route"] == 4
        worst = 0.0
        for s in range(k):
            D, dym = tm.tangent(first_order, X[:, rc], du[:, s], d0[s], dm1[s])
            worst = max(worst, bc.rel(sy[:, s], dym), bc.rel(sxn[s], D[-1]), bc.rel(sxnm1[s, :nn2], D[-2][:nn2]))
        out["shared"] = worst
        # a NaN in one column
        bad = min(1, k - 1)
        d0_bad = d0.copy()
        d0_bad[bad, 7] = np.nan
        with pytest.raises(FcDiverged):
            dev.run_tangent_batch(slot, n, du, d0_bad, dm1)
        flags = dev.tangent_batch_flags
        assert flags[bad] == 1 and flags.sum() == 1, flags
        by, bxn, bxnm1 = dev.tangent_batch_last
        keep = [s for s in range(k) if s != bad]
        assert np.array_equal(by[:, keep], dy[:, keep]) and np.array_equal(bxn[keep], dxn[keep]) and np.array_equal(bxnm1[keep], dxnm1[keep])
        print(f"batched tangent march first order {first_order}, n = {n}, k = {k}: " + ", ".join(f"{a} {v:.3e}" for a, v in out.items()))
        for a, v in out.items():
            assert v <= TOL, f"{a}: {v:.3e} > {TOL:.1e}"
    finally:
        batch_off(square)


def test_batch_state_untouched_and_refusals(square):
    """2. The batched state, the step counters and a further batched step are the same bits with and without a march in between; the
    batched refusals return their codes with the reason."""
    dev, k, n = square.dev, 5, 3
    c = column_inputs(square, n + 1)
    un, unn, pp, u = c["un"][:k], c["unn"][:k], c["pp"][:k], np.ascontiguousarray(c["u"][:, :k])
    batch_on(square, k)
    try:
        def observe(march):
            dev.set_state_batch(un, unn, pp)
            bc.forward_batch(dev, 2, u[:n], tape=True)
            counts = dev.step_counts()
            if march:
                dev.run_tangent_batch(SLOT_BDF2, n, c["du"][:n, :k], c["d0"][:k], c["dm1"][:k])
            assert dev.step_counts() == counts
            state, tape = dev.get_state_batch(), dev.adjoint_tape_states_batch()
            y, _, _ = dev.step_batch(SLOT_BDF2, u[n], compute_energy=False)
            return dict(zip(("u_n", "u_nn", "p_n", "tape", "y of a further step", "its solution"), [*state, tape, y, dev.get_solution_batch()]))

        before, after = observe(False), observe(True)
        for name in before:
            assert np.array_equal(before[name], after[name]), f"{name} differs after a batched tangent march"
        # (the further step was taped: 4 steps on the tape)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="holds 4 steps")
        # a batched step in flight
        dev.step_batch_begin(SLOT_BDF2, u[n], compute_energy=False)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="in flight")
        dev.step_batch_end()
        dev.set_state_batch(un, unn, pp)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="not begun")
        bc.forward_batch(dev, 2, u[:n], tape=True)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, k, match="ref_col")
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, -2, match="ref_col")
        refused(INV, dev.run_tangent_batch, SLOT_BDF1, n, None, None, None, None, match="first taped step")
        # an explicit right-hand-side operator (Crank-Nicolson) on the slot of the run
        dev.set_rhs_operator(SLOT_BDF2, (0.5 * square.model.M)[:, : 2 * dev.nn])
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="Crank-Nicolson")
        dev.set_rhs_operator(SLOT_BDF2, None)
        dev.run_tangent_batch(SLOT_BDF2, n)
        code = dev.lib.fc_run_tangent_batch(dev._h, SLOT_BDF2, k + 1, n, -1, None, None, None, None, None, None, None)
        assert code == INV and b"k differs" in dev.lib.fc_last_error()
        dev.set_time_scheme(square.dt, False)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="its own tangent")
        dev.set_time_scheme(square.dt, True)
        dev.adjoint_tape_reserve_sparse_batch(6, 2)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="checkpointed")
        dev.adjoint_tape_reserve_sparse_batch(0, 0)
        refused(INV, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="no tape is reserved")
        dev.tangent_reserve(0)
        refused(NOT_READY, dev.run_tangent_batch, SLOT_BDF2, n, None, None, None, None, match="fc_tangent_reserve")
        dev.set_batch(9)  # another width: a reserve made for KB = 8 would not fit KB = 16
        dev.tangent_reserve(1)
        assert dev.tangent_info()["KB"] == 16
        dev.set_batch(k)
        assert not dev.tangent_info()["reserved"]
    finally:
        batch_off(square)


@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_batched_march_with_body_force_actuators(square, first_order, n):
    """2b. With body-force profiles on the actuators the batched forward step enters them in its element loop, the batched march as
    load vectors behind the gather (fc_tan_force_b): k = 5 columns against central differences of the batched device run (eps = 1e-4)
    within 1e-6 and against fc_run_adjoint_batch through the dot-product identity within 1e-8, column by column."""
    from tests.support import step_cases as sc

    dev, k = square.dev, 5
    nn2 = 2 * square.th.nn
    slot = slot_of(first_order)
    c = column_inputs(square, n)
    un, unn, pp = c["un"][:k], c["unn"][:k], c["pp"][:k]
    u, du = np.ascontiguousarray(c["u"][:, :k]), np.ascontiguousarray(c["du"][:, :k])
    d0, dm1 = c["d0"][:k], c["dm1"][:k]
    w, z = np.random.default_rng(73).standard_normal((n, k, dev.n_sens)), np.random.default_rng(79).standard_normal((k, dev.N))
    dev.set_force(sc.force_profiles(square.th, 0))
    bc.batch_on(square, k, tape=6)
    dev.tangent_reserve(1)
    try:
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, first_order, u, tape=True)
        dy, dxn, _ = dev.run_tangent_batch(slot, n, du, d0, dm1)
        g, gx0, gxm1 = dev.run_adjoint_batch(slot, n, w, z)
        terms = np.array([np.einsum("mki,mki->k", w, dy), np.einsum("ki,ki->k", z, dxn), -np.einsum("mka,mka->k", g, du),
                          -np.einsum("ki,ki->k", gx0[:, :nn2], d0[:, :nn2]), -np.einsum("ki,ki->k", gxm1[:, :nn2], dm1[:, :nn2])])
        defect = float(np.max(np.abs(terms.sum(axis=0)) / np.abs(terms).sum(axis=0)))

        def run(sign):
            dev.set_state_batch(un + sign * bc.EPS * d0[:, :nn2], unn + sign * bc.EPS * dm1[:, :nn2], pp)
            yy = bc.forward_batch(dev, first_order, u + sign * bc.EPS * du)
            return yy, dev.get_solution_batch()

        (yp, xp), (ym, xm) = run(1.0), run(-1.0)
        fd_y, fd_x = bc.rel_columns(dy, (yp - ym) / (2 * bc.EPS), 1), bc.rel_columns(dxn, (xp - xm) / (2 * bc.EPS), 0)
        print(f"batched tangent march with body forces, first order {first_order}, n = {n}, k = {k}: identity defect {defect:.3e}, "
              f"device central difference y {fd_y:.3e}, x_n {fd_x:.3e}")
        assert defect <= 1e-8 and fd_y <= bc.TOL_FD and fd_x <= bc.TOL_FD
    finally:
        dev.tangent_reserve(0)
        bc.batch_off(square, refine=0)
        dev.set_force(None)
        square.restart()


def test_floquet_driver_device_against_numpy_backend(square):
    """3. flu.floquet_multipliers on the square (k = 4, 4 blocks, n = 6, about column 0) from the same start block through
    DeviceTangentBlocks and through the numpy backend on the model: the five leading Ritz values agree within 1e-8 relative
    (tests/test_tangent_host.py: they take 1e-13 of apply noise unmoved).  Hessenberg entries are not compared."""
    dev, k, n, blocks = square.dev, 4, 6, 4
    c = column_inputs(square, n)
    batch_on(square, k)
    try:
        dev.set_state_batch(c["un"][:k], c["unn"][:k], c["pp"][:k])
        bc.forward_batch(dev, 2, np.ascontiguousarray(c["u"][:, :k]), tape=True)
        X0 = dev.adjoint_tape_states_batch()[:, 0]
        start = np.random.default_rng(61).standard_normal((2 * dev.N, k))
        back = flu.DeviceTangentBlocks(dev, n, ref_col=0)
        lam_dev = flu.floquet_multipliers(back, n, 5, blocks=blocks, start=start)
        assert back.applies == blocks and dev.tangent_info()["route"] == 4
        lam_np = flu.floquet_multipliers(ModelTangentBlocks(TangentModel(square.model), X0, k), n, 5, blocks=blocks, start=start)
        diff = np.max(np.abs(lam_dev - lam_np) / np.abs(lam_np))
        print(f"Floquet driver on the square: |Ritz| {np.abs(lam_np)}, device against numpy backend {diff:.3e}")
        assert diff <= 1e-8
    finally:
        batch_off(square)
