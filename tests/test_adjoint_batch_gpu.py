"""The batched adjoint march on the MI355X (``fc_set_adjoint_batch``, ``fc_solve_transposed_batch``, ``fc_run_adjoint_batch``,
``fc_adjoint_tape_*_batch``, ``fc_adjoint_batch_info``; csrc/fc_adjoint_batch.hip.h, csrc/fc_adjoint_batch_run.hpp,
flowcontrol_amd/adjoint.py) against the scipy models of tests/support/adjoint_step_model.py and tests/support/adjoint_nl_model.py,
run once per column.

Small problems: the linearised 8 x 8 square (N = 659, two Dirichlet actuators) and the nonlinear 7 x 5 square (N = 378, 70 cells: the
last workgroup of an element launch is partial) of the single-column adjoint tests, with per-column inputs from
tests/support/adjoint_batch_cases.py; the FlowSolver level runs on the cylinder's O1 mesh."""
import tempfile

import numpy as np
import pytest

from flowcontrol_amd import _lib, adjoint
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcDiverged, FcError
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC
from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_nl_child as nl_case
from tests.support import adjoint_step_child as lin_case

pytestmark = pytest.mark.gpu

SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
TOL, EPS, TOL_FD = bc.TOL, bc.EPS, bc.TOL_FD


@pytest.fixture(scope="module")
def lin():
    sq = lin_case.Square()
    assert sq.dev.N == 659
    yield sq
    sq.close()


@pytest.fixture(scope="module")
def nl():
    sq = nl_case.NlSquare()
    assert sq.th.mesh.cells.shape[0] == 70 and sq.dev.N == 378
    yield sq
    sq.close()


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def slot_of(order):
    return SLOT_BDF1 if order == 1 else SLOT_BDF2


def lin_inputs(sq, n, k):
    """Per-column inputs of a linearised march; column 1 has w = 0, z = 0 and the last column repeats column 0 (k >= 3)."""
    u, w, z = bc.column_inputs(n, k, sq.dev.n_act, sq.dev.n_sens, sq.dev.N)
    if k >= 3:
        w[:, 1], z[1] = 0.0, 0.0
        w[:, k - 1], z[k - 1] = w[:, 0], z[0]
    return u, w, z


# ── 1. the transposed block solve ────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("k", [1, 4, 5, 9, 17, 32])
def test_solve_transposed_batch(lin, k):
    """1. solve_transposed_batch against splu(A).solve(b, trans="T"), both slots: every column <= 1e-10 relative; a zero column comes
    back exactly zero, equal columns bit-equal; the direct solve_batch of the same columns is far away and unchanged by the call."""
    dev = lin.dev
    bc.batch_on(lin, k)
    try:
        rng = np.random.default_rng(100 + k)
        b = rng.standard_normal((k, dev.N))
        if k >= 3:
            b[1] = 0.0
            b[k - 1] = b[0]
        for order, s in ((1, SLOT_BDF1), (2, SLOT_BDF2)):
            before = dev.solve_batch(s, b)
            x = dev.solve_transposed_batch(s, b)
            assert np.array_equal(before, dev.solve_batch(s, b))
            worst = 0.0
            for c in range(k):
                if k >= 3 and c == 1:
                    assert not np.any(x[c]), "a zero column did not come back exactly zero"
                    continue
                ref = lin.model.lu[order].solve(b[c], trans="T")
                worst = max(worst, bc.rel(x[c], ref))
                assert bc.rel(before[c], ref) > 1e-3  # (the operator has convection: A^-1 b is not A^-T b)
            print(f"solve_transposed_batch k = {k}, order {order}: worst column {worst:.3e}")
            assert worst <= 1e-10
            if k >= 3:
                assert np.array_equal(x[k - 1], x[0]), "equal columns are not bit-equal"
    finally:
        bc.batch_off(lin)


# ── 2. the linearised march ──────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("k", [5, 32])
@pytest.mark.parametrize("first_order,n", [(1, 12), (2, 3)])
def test_linearised_march(lin, first_order, n, k):
    """2. g, dx0, dxm1 of every column within 1e-8 of the model and of run_adjoint fed that column alone; two marches bit-identical; the
    column with w = 0, z = 0 exactly zero; the two columns with equal inputs bit-equal.  (Measured defects: DESIGN section 5.4.)"""
    linearised_march(lin, first_order, n, k)


@pytest.mark.parametrize("first_order,n", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_shortest_linearised_marches(lin, first_order, n):
    """2a. The edges of the backward schedule -- n = 1 (no later step, one slot, dx0 with one term) and n = 2, from either first slot --
    with the assertions and the bound of test 2, at k = 5 (the smallest width of this file, and no power of two)."""
    linearised_march(lin, first_order, n, 5)


def linearised_march(lin, first_order, n, k):
    dev = lin.dev
    bc.batch_on(lin, k)
    try:
        _, w, z = lin_inputs(lin, n, k)
        slot = slot_of(first_order)
        g, dx0, dxm1 = dev.run_adjoint_batch(slot, n, w, z)
        g2, dx02, dxm12 = dev.run_adjoint_batch(slot, n, w, z)
        assert np.array_equal(g, g2) and np.array_equal(dx0, dx02) and np.array_equal(dxm1, dxm12), "two identical batched marches differ"
        assert g.shape == (n, k, dev.n_act) and dx0.shape == (k, dev.N)
        assert not np.any(g[:, 1]) and not np.any(dx0[1]) and not np.any(dxm1[1]), "the zero column is not exactly zero"
        assert np.array_equal(g[:, k - 1], g[:, 0]) and np.array_equal(dx0[k - 1], dx0[0]) and np.array_equal(dxm1[k - 1], dxm1[0])
        gm, dx0m, dxm1m = bc.model_adjoint_lin(lin.model, first_order, n, w, z)
        worst = {"g": 0.0, "dx0": 0.0, "dxm1": 0.0, "single g": 0.0, "single dx0": 0.0, "single dxm1": 0.0}
        for c in range(k):
            if c == 1:
                continue
            gs, dx0s, dxm1s = dev.run_adjoint(slot, n, w[:, c], z[c])
            worst["g"] = max(worst["g"], bc.rel(g[:, c], gm[:, c]))
            worst["dx0"] = max(worst["dx0"], bc.rel(dx0[c], dx0m[c]))
            worst["single g"] = max(worst["single g"], bc.rel(g[:, c], gs))
            worst["single dx0"] = max(worst["single dx0"], bc.rel(dx0[c], dx0s))
            if first_order == 2:
                worst["dxm1"] = max(worst["dxm1"], bc.rel(dxm1[c], dxm1m[c]))
                worst["single dxm1"] = max(worst["single dxm1"], bc.rel(dxm1[c], dxm1s))
            else:  # a BDF1 first step never reads x_{-1}
                assert not np.any(dxm1[c]) and not np.any(dxm1m[c])
        print(f"batched linearised march first order {first_order}, n = {n}, k = {k}: " + ", ".join(f"{a} {v:.3e}" for a, v in worst.items()))
        for a, v in worst.items():
            assert v <= TOL, f"{a}: {v:.3e} > {TOL:.1e}"
        # columns k .. KB - 1 are padding: a march without state gradients and without weights leaves g at the terminal vector's share alone
        g3, none0, none1 = dev.run_adjoint_batch(slot, n, None, z, state_gradients=False)
        assert none0 is None and none1 is None and np.all(np.isfinite(g3))
        info = dev.adjoint_batch_info(slot)
        assert info["available"] and not info["stale"] and info["run_ms"] > 0.0 and info["tile_bytes"] > 0 and info["march_bytes"] > 0
    finally:
        bc.batch_off(lin)


# ── 3. the nonlinear march over the batched tape ─────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("k", [5, 17])
@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_nonlinear_march_on_the_taped_batched_run(nl, first_order, n, k):
    """3. Initial states and controls different per column.  The taped batched states equal the model's to 1e-8; g, dx0, dxm1 of every
    column within 1e-8 of the model; the directional derivative of every column against central differences of the batched device run
    (eps = 1e-4) <= 1e-6; a batched forward run with a tape reserved is bit-identical to one without.  (Measured defects: DESIGN
    section 5.4.)"""
    dev, model = nl.dev, nl.model
    nn2 = 2 * nl.th.nn
    bc.batch_on(nl, k)
    try:
        un, unn, pp = bc.column_states(nl.u_n, nl.u_nn, nl.p, k)
        x0, xm1 = np.hstack([un, pp]), np.hstack([unn, pp])
        u, w, z = bc.column_inputs(n, k, dev.n_act, dev.n_sens, dev.N)
        slot = slot_of(first_order)
        # without a tape
        dev.set_state_batch(un, unn, pp)
        y_plain = bc.forward_batch(dev, first_order, u)
        end_plain = dev.get_state_batch()
        assert dev.adjoint_batch_info(slot)["tape_bytes"] == 0
        refused(INV, dev.run_adjoint_batch, slot, n, w, z, match="no tape is reserved")
        # taped
        dev.adjoint_tape_reserve_batch(6)
        info = dev.adjoint_tape_info_batch()
        assert info["capacity"] == 6 and info["bytes"] == 8 * dev.N * info["KB"] * 8 and info["KB"] >= k and not info["begun"]
        dev.set_state_batch(un, unn, pp)
        y = bc.forward_batch(dev, first_order, u, tape=True)
        end = dev.get_state_batch()
        assert np.array_equal(y, y_plain) and all(np.array_equal(a, b) for a, b in zip(end, end_plain)), "the tape changed the forward run"
        info = dev.adjoint_tape_info_batch()
        assert info["count"] == n and info["begun"] and not info["overflowed"], info
        X = dev.adjoint_tape_states_batch()  # [n + 2, k, N]
        Xm, ym = bc.model_forward_nl(model, first_order, u, x0, xm1)  # [k, n + 2, N]
        assert np.array_equal(X[0], xm1) and np.array_equal(X[1], x0) and np.array_equal(X[-1], dev.get_solution_batch())
        out = {"forward_X": bc.rel_columns(X, np.swapaxes(Xm, 0, 1), 1), "forward_y": bc.rel_columns(y, ym, 1)}
        g, dx0, dxm1 = dev.run_adjoint_batch(slot, n, w, z)
        g2, dx02, dxm12 = dev.run_adjoint_batch(slot, n, w, z)
        assert np.array_equal(g, g2) and np.array_equal(dx0, dx02) and np.array_equal(dxm1, dxm12), "two identical batched marches differ"
        gm, dx0m, dxm1m = bc.model_adjoint_nl(model, first_order, Xm, w, z)
        out["g"], out["dx0"] = bc.rel_columns(g, gm, 1), bc.rel_columns(dx0, dx0m, 0)
        if first_order == 2:
            out["dxm1"] = bc.rel_columns(dxm1, dxm1m, 0)
        else:
            assert not np.any(dxm1) and not np.any(dxm1m)
        # the derivative of the batched DEVICE run, one direction per column (controls and both velocity levels)
        rng = np.random.default_rng(7)
        du, d0, dm1 = rng.standard_normal(u.shape), rng.standard_normal((k, nn2)), rng.standard_normal((k, nn2))

        def cost(sign):
            dev.set_state_batch(un + sign * EPS * d0, unn + sign * EPS * dm1, pp)
            yy = bc.forward_batch(dev, first_order, u + sign * EPS * du)
            return np.einsum("mki,mki->k", w, yy) + np.einsum("ki,ki->k", z, dev.get_solution_batch())

        fd = (cost(1.0) - cost(-1.0)) / (2 * EPS)
        ad = np.einsum("mka,mka->k", g, du) + np.einsum("ki,ki->k", dx0[:, :nn2], d0) + np.einsum("ki,ki->k", dxm1[:, :nn2], dm1)
        fd_err = float(np.max(np.abs(fd - ad) / np.abs(fd)))
        print(f"batched nonlinear march first order {first_order}, n = {n}, k = {k}: " + ", ".join(f"{a} {v:.3e}" for a, v in out.items()) +
              f", device central difference (worst column) {fd_err:.3e}")
        for a, v in out.items():
            assert v <= TOL, f"{a}: {v:.3e} > {TOL:.1e}"
        assert fd_err <= TOL_FD, f"central difference of the batched device run: {fd_err:.3e} > {TOL_FD:.1e}"
    finally:
        bc.batch_off(nl)
        nl.dev.set_time_scheme(nl.dt, True)


# ── 4. tape semantics ────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_tape_semantics(nl):
    """4. No tape, a count that differs from n_steps, an overflowed tape, a wrong first slot, and set_state_batch or reset_sim_batch
    between the forward and the backward run are each refused with their reason; the single-run tape is still refused with a batch set."""
    dev, k = nl.dev, 5
    refused(NOT_READY, dev.adjoint_tape_reserve_batch, 4)  # no batch
    bc.batch_on(nl, k)
    try:
        un, unn, pp = bc.column_states(nl.u_n, nl.u_nn, nl.p, k)
        u, w, z = bc.column_inputs(8, k, dev.n_act, dev.n_sens, dev.N)
        refused(INV, dev.adjoint_tape_reserve, 4, match="batch set")
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 4, None, z, match="nonlinear")
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 4, None, z, match="no tape is reserved")
        refused(NOT_READY, dev.adjoint_tape_begin_batch)
        dev.adjoint_tape_reserve_batch(6)
        # reserved, not begun: steps are not taped
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, 1, u[:2])
        assert dev.adjoint_tape_info_batch()["count"] == 0
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 2, None, z, match="not begun")
        # count != n_steps, a wrong first slot
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, 1, u[:4], tape=True)
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 6, None, z, match="holds 4 steps")
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 6, None, z, match="fc_adjoint_tape_reserve_batch")
        refused(INV, dev.run_adjoint_batch, SLOT_BDF2, 4, None, z, match="first taped step")
        g, _, _ = dev.run_adjoint_batch(SLOT_BDF1, 4, None, z)
        assert np.all(np.isfinite(g))
        # overflow: the run goes on, nothing more is written, the march is refused
        for m in range(4, 8):
            dev.step_batch(SLOT_BDF2, u[m], compute_energy=False)
        info = dev.adjoint_tape_info_batch()
        assert info["overflowed"] and info["count"] == 6 and info["lost"] == 2
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 8, None, z, match="overflowed")
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 6, None, z, match="overflowed")
        # set_state_batch between the forward and the backward run
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, 1, u[:3], tape=True)
        dev.set_state_batch(un, unn, pp)
        assert not dev.adjoint_tape_info_batch()["begun"]
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 3, None, z, match="not begun")
        # reset_sim_batch between the forward and the backward run
        bc.forward_batch(dev, 1, u[:3], tape=True)
        assert dev.adjoint_tape_info_batch()["count"] == 3
        dev.reset_sim_batch(2)
        assert not dev.adjoint_tape_info_batch()["begun"]
        refused(INV, dev.run_adjoint_batch, SLOT_BDF1, 3, None, z, match="not begun")
        # another batch width ends and releases the tape
        dev.set_batch(k)
        assert dev.adjoint_tape_info_batch()["capacity"] == 6 and not dev.adjoint_tape_info_batch()["begun"]
        dev.set_batch(17)
        assert dev.adjoint_tape_info_batch() == {"capacity": 0, "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0, "KB": 0}
    finally:
        bc.batch_off(nl)
        nl.dev.set_time_scheme(nl.dt, True)
    assert dev.adjoint_batch_info(SLOT_BDF2) == {"available": False, "stale": False, "tile_bytes": 0, "march_bytes": 0, "tape_bytes": 0,
                                                 "repacks": 0, "KB": 0, "run_ms": dev.adjoint_batch_info(SLOT_BDF2)["run_ms"]}


# ── 5. staleness ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_staleness_and_untouched_forward_steps(lin):
    """5. After refactor of a slot the next march repacks (adjoint_batch_info counts it) and still meets 1e-8; after update_operator it is
    refused FC_ERR_NOT_READY until set_adjoint_factors(slot, 1) is called again; forward batched steps before and after
    set_adjoint_batch(+-1) are bit-identical."""
    dev, k, n = lin.dev, 5, 3
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(k)
    try:
        un, unn, pp = bc.column_states(lin.u_n, lin.u_nn, lin.p, k)
        u, w, z = lin_inputs(lin, n, k)

        def series():
            dev.set_state_batch(un, unn, pp)
            return bc.forward_batch(dev, 1, u), dev.get_state_batch()

        def same(a, b):
            return np.array_equal(a[0], b[0]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))

        before = series()
        refused(NOT_READY, dev.set_adjoint_batch, SLOT_BDF2, 1)  # no transposed factors yet
        for s in SLOTS:
            dev.set_adjoint_factors(s, 1)
            dev.set_adjoint_batch(s, 1)
        assert same(before, series())
        gm, dx0m, dxm1m = bc.model_adjoint_lin(lin.model, 2, n, w, z)
        live = [c for c in range(k) if c != 1]

        def march_defect():
            g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF2, n, w, z)
            return max(bc.rel(g[:, live], gm[:, live]), bc.rel(dx0[live], dx0m[live]), bc.rel(dxm1[live], dxm1m[live]))

        assert march_defect() <= TOL
        assert same(before, series())  # (the march left the ring, the tiled factors and the step counter alone)
        assert dev.adjoint_batch_info(SLOT_BDF2)["repacks"] == 1
        dev.refactor(SLOT_BDF2)
        info = dev.adjoint_batch_info(SLOT_BDF2)
        assert info["stale"] and info["repacks"] == 1
        d = march_defect()
        info = dev.adjoint_batch_info(SLOT_BDF2)
        print(f"batched march after refactor: {d:.3e}, repacks {info['repacks']}")
        assert d <= TOL and info["repacks"] == 2 and not info["stale"]
        assert march_defect() <= TOL and dev.adjoint_batch_info(SLOT_BDF2)["repacks"] == 2
        dev.update_operator(SLOT_BDF2)
        refused(NOT_READY, dev.run_adjoint_batch, SLOT_BDF2, n, w, z, match="stale")
        refused(NOT_READY, dev.solve_transposed_batch, SLOT_BDF2, z, match="stale")
        dev.set_adjoint_factors(SLOT_BDF2, 1)
        assert march_defect() <= TOL and dev.adjoint_batch_info(SLOT_BDF2)["repacks"] == 3
        assert same(before, series())
        for s in SLOTS:
            dev.set_adjoint_batch(s, -1)
        info = dev.adjoint_batch_info(SLOT_BDF2)
        assert not info["available"] and info["tile_bytes"] == 0 and info["march_bytes"] == 0
        refused(NOT_READY, dev.run_adjoint_batch, SLOT_BDF2, n, w, z, match="fc_set_adjoint_batch")
        assert same(before, series())
    finally:
        bc.batch_off(lin)


def test_set_bc_apply_bc_and_another_k_between_marches():
    """5b. The other staleness events.  set_bc with ONE MORE actuator column on the same Dirichlet dofs (the batch stays), then
    assemble + apply_bc + refactor: the next march lays its partials out for three actuators, repacks both slots and meets 1e-8 against
    the three-actuator model.  Then set_batch with another k of the same width (5 -> 6, KB = 8): stale, repacked, 1e-8 again."""
    from tests.support import adjoint_step_model as am

    sq = lin_case.Square(refine=0)
    try:
        dev, n = sq.dev, 3
        bc.batch_on(sq, 5)
        _, w, z = lin_inputs(sq, n, 5)
        g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF1, n, w, z)
        gm, dx0m, _ = bc.model_adjoint_lin(sq.model, 1, n, w, z)
        live = [0, 2, 3, 4]
        assert g.shape == (n, 5, 2) and max(bc.rel(g[:, live], gm[:, live]), bc.rel(dx0[live], dx0m[live])) <= TOL
        before = {s: dev.adjoint_batch_info(s) for s in SLOTS}
        # one more actuator
        prof3 = np.c_[sq.prof, np.cos(1.3 * np.arange(len(sq.dofs)) + 0.2)]
        dev.set_bc(sq.dofs, prof3)
        assert dev.batch_k == 5 and all(dev.adjoint_batch_info(s)["stale"] for s in SLOTS)
        refused(NOT_READY, dev.run_adjoint_batch, SLOT_BDF1, n, w, z)
        raw, A = {}, {}
        for order, slot, c in ((1, SLOT_BDF1, 1.0 / sq.dt), (2, SLOT_BDF2, 1.5 / sq.dt)):
            dev.assemble_matrix(slot, mass=c, nu=1.0 / sq.Re, adv=sq.U0, lin=sq.U0)
            raw[order] = dev.matrix(slot)
            dev.apply_bc(slot)
            A[order] = dev.matrix(slot)
            dev.refactor(slot)
            dev.set_adjoint_factors(slot, 1)
        G = np.zeros((dev.N, 3))
        G[sq.dofs] = prof3
        model3 = am.StepModel(A[1], A[2], sq.M, sq.dofs, prof3, raw[1] @ G, raw[2] @ G, sq.model.C, sq.dt)
        g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF1, n, w, z)
        gm, dx0m, _ = bc.model_adjoint_lin(model3, 1, n, w, z)
        d = max(bc.rel(g[:, live], gm[:, live]), bc.rel(dx0[live], dx0m[live]))
        after = {s: dev.adjoint_batch_info(s) for s in SLOTS}
        print(f"batched march after set_bc with a third actuator: {d:.3e}; march bytes {before[SLOT_BDF2]['march_bytes']} -> {after[SLOT_BDF2]['march_bytes']}")
        assert g.shape == (n, 5, 3) and np.any(g[:, 0, 2]) and d <= TOL and not np.any(g[:, 1])
        assert all(after[s]["repacks"] == before[s]["repacks"] + 1 and not after[s]["stale"] for s in SLOTS)
        assert after[SLOT_BDF2]["march_bytes"] > before[SLOT_BDF2]["march_bytes"]
        # another k of the same width
        dev.set_batch(6)
        info = dev.adjoint_batch_info(SLOT_BDF2)
        assert info["available"] and info["stale"] and info["KB"] == 8
        _, w6, z6 = lin_inputs(sq, n, 6)
        g6, dx06, _ = dev.run_adjoint_batch(SLOT_BDF1, n, w6, z6)
        gm6, dx0m6, _ = bc.model_adjoint_lin(model3, 1, n, w6, z6)
        live6 = [0, 2, 3, 4, 5]
        d6 = max(bc.rel(g6[:, live6], gm6[:, live6]), bc.rel(dx06[live6], dx0m6[live6]))
        print(f"batched march after set_batch(6): {d6:.3e}")
        assert d6 <= TOL and all(dev.adjoint_batch_info(s)["repacks"] == after[s]["repacks"] + 1 for s in SLOTS)
    finally:
        sq.close()


def test_overlapped_forward_steps_are_taped(nl):
    """5c. The overlapped form of the batched step (step_batch_begin / step_batch_end_early, what BatchedFlowSolver.step runs) tapes
    the same trajectory: the taped states equal the model's to 1e-8, and the march over them meets 1e-8."""
    dev, model, k, n = nl.dev, nl.model, 5, 4
    bc.batch_on(nl, k, tape=6)
    try:
        un, unn, pp = bc.column_states(nl.u_n, nl.u_nn, nl.p, k)
        x0, xm1 = np.hstack([un, pp]), np.hstack([unn, pp])
        u, w, z = bc.column_inputs(n, k, dev.n_act, dev.n_sens, dev.N)
        dev.set_state_batch(un, unn, pp)
        dev.adjoint_tape_begin_batch()
        y = np.empty((n, k, dev.n_sens))
        for m in range(n):
            dev.step_batch_begin(SLOT_BDF1 if m == 0 else SLOT_BDF2, u[m], compute_energy=False)
            y[m], flags = dev.step_batch_end_early()
            assert not np.any(flags)
        dev.step_batch_collect()
        assert dev.adjoint_tape_info_batch()["count"] == n
        X = dev.adjoint_tape_states_batch()
        Xm, ym = bc.model_forward_nl(model, 1, u, x0, xm1)
        assert np.array_equal(X[-1], dev.get_solution_batch())
        g, dx0, _ = dev.run_adjoint_batch(SLOT_BDF1, n, w, z)
        gm, dx0m, _ = bc.model_adjoint_nl(model, 1, Xm, w, z)
        out = {"forward_X": bc.rel_columns(X, np.swapaxes(Xm, 0, 1), 1), "forward_y": bc.rel_columns(y, ym, 1),
               "g": bc.rel_columns(g, gm, 1), "dx0": bc.rel_columns(dx0, dx0m, 0)}
        print("overlapped batched steps onto the tape: " + ", ".join(f"{a} {v:.3e}" for a, v in out.items()))
        for a, v in out.items():
            assert v <= TOL, f"{a}: {v:.3e} > {TOL:.1e}"
    finally:
        bc.batch_off(nl)
        nl.dev.set_time_scheme(nl.dt, True)


# ── 6. a non-finite column ───────────────────────────────────────────────────────────────────────────────────────────────────────
def test_a_nan_column_stays_alone(lin):
    """6. A NaN in one column's terminal vector gives FC_ERR_DIVERGED and that column's flag only; the other columns are within 1e-8."""
    dev, k, n, bad = lin.dev, 9, 3, 4
    bc.batch_on(lin, k)
    try:
        _, w, z = lin_inputs(lin, n, k)
        gm, dx0m, dxm1m = bc.model_adjoint_lin(lin.model, 2, n, w, z)
        z[bad, 17] = np.nan
        with pytest.raises(FcDiverged):
            dev.run_adjoint_batch(SLOT_BDF2, n, w, z)
        flags = dev.adjoint_batch_flags
        assert flags.tolist() == [1 if c == bad else 0 for c in range(k)], flags
        g, dx0, dxm1 = dev.adjoint_batch_last
        good = [c for c in range(k) if c not in (bad, 1)]
        assert np.all(np.isfinite(g[:, good])) and not np.any(g[:, 1])
        d = max(bc.rel(g[:, good], gm[:, good]), bc.rel(dx0[good], dx0m[good]), bc.rel(dxm1[good], dxm1m[good]))
        print(f"NaN in column {bad}: the other columns against the model {d:.3e}")
        assert d <= TOL
        # ... and the next march is clean again
        z[bad, 17] = 0.0
        dev.run_adjoint_batch(SLOT_BDF2, n, w, z)
        assert not np.any(dev.adjoint_batch_flags)
    finally:
        bc.batch_off(lin)


# ── 7. FlowSolver level: the nonlinear cylinder on O1 ────────────────────────────────────────────────────────────────────────────
def test_batched_flowsolver_cost_gradient(golden_dir):
    """7. O1, nonlinear, k = 4, 20 steps: BatchedFlowSolver.cost_gradient against central differences of the batched forward cost in two
    random directions <= 1e-6 for every column, and column s within 1e-8 of FlowSolver.cost_gradient of run s alone.  The batched state
    is left where it was and everything is released.  (Measured defects: DESIGN section 5.4.)"""
    from flowcontrol_amd.batch import BatchedFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_solver.is_eq_nonlinear = True
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    k, n = 4, 20
    try:
        bfs = BatchedFlowSolver(fs, k)
        bfs.initialize_time_stepping(ics=[ParamIC(xloc=2.0 + 0.3 * s, yloc=0.1 * s, radius=0.5, amplitude=1.0 - 0.1 * s) for s in range(k)])
        dev = bfs.dev
        rng = np.random.default_rng(20)
        u = 0.5 * rng.standard_normal((n, k, dev.n_act))
        Q = np.diag(1.0 + np.arange(dev.n_sens))
        R = 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state_batch()]

        def cost(uu):
            y = bc.forward_batch(dev, 1, uu)
            dev.set_state_batch(*state0)
            return 0.5 * (np.einsum("mki,ij,mkj->k", y, Q, y) + np.einsum("mki,ij,mkj->k", uu, R, uu))

        J, grad, dx0 = bfs.cost_gradient(u, Q, R, state_gradient=True)
        assert J.shape == (k,) and grad.shape == (n, k, dev.n_act) and dx0.shape == (k, dev.N)
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state_batch()))
        info = dev.adjoint_batch_info(SLOT_BDF2)
        assert info["tile_bytes"] == 0 and info["march_bytes"] == 0 and info["tape_bytes"] == 0
        assert all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
        assert np.all(np.abs(J - cost(u)) <= 1e-12 * np.abs(J))
        worst = 0.0
        for q in range(2):
            d = rng.standard_normal(u.shape)
            fd = (cost(u + EPS * d) - cost(u - EPS * d)) / (2 * EPS)
            ad = np.einsum("mka,mka->k", grad, d)
            err = np.abs(fd - ad) / np.abs(fd)
            worst = max(worst, float(err.max()))
            print(f"O1 nonlinear, k = {k}, {n} steps, direction {q}: central differences {fd}, adjoint {ad}, relative {err}")
        assert worst <= TOL_FD
        # column s against the single run s
        bfs.close()
        single = 0.0
        with adjoint.AdjointRun(fs, tape=n) as run:
            for s in range(k):
                Js, gs = adjoint.quadratic_cost_gradient(fs, u[:, s], Q, R, x0=(state0[0][s], state0[1][s], state0[2][s]), adjoint=run)
                single = max(single, bc.rel(grad[:, s], gs), abs(J[s] - Js) / abs(Js))
        print(f"O1 nonlinear, k = {k}: batched columns against the single runs {single:.3e}")
        assert single <= TOL
    finally:
        fs.th.release_device()
