"""The tangent of the energy on the MI355X (``fc_tangent_set_energy``, ``fc_get_tangent_energy``, ``fc_tangent_energy_info``;
csrc/fc_tangent_energy.hip.h, csrc/fc_tangent_energy_run.hpp) in the open-loop marches: against the model of
tests/support/tangent_energy_cases.py, against central differences of the device's own energy series, the batched march against the
single one column by column, the opt-in, and the refusals.

The nonlinear 7 x 5 square (N = 378, 70 cells): fc_tan_energy runs three workgroups, the last with 6 cells; fc_tan_energy_b at KB = 4
two, the second partial, at KB = 32 nine, the last with 6 cells.  The closed loops are in tests/test_tangent_energy_loop_gpu.py."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcDiverged, FcError
from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_energy_cases as ec
from tests.support import adjoint_nl_child as nl_case
from tests.support import adjoint_nl_model as nm
from tests.support import tangent_child as case
from tests.support import tangent_energy_cases as te

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
KMAX = 17
#: a batched column's rows against the single march of that column
TOL_BATCH = 1e-14


def slot_of(first_order):
    return SLOT_BDF1 if first_order == 1 else SLOT_BDF2


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


@pytest.fixture(scope="module")
def square():
    sq = nl_case.NlSquare()
    yield sq
    sq.close()


@pytest.fixture()
def tan(square):
    """A tape of 6 steps and the tangent buffers with the energy option for one test; all released afterwards."""
    dev = square.dev
    dev.adjoint_tape_reserve(6)
    dev.tangent_reserve(1)
    dev.tangent_set_energy(1)
    yield square
    dev.set_adjoint_energy(None)
    dev.tangent_tape_reserve(0)
    dev.tangent_reserve(0)
    dev.adjoint_tape_reserve(0)
    for s in SLOTS:
        dev.set_adjoint_factors(s, -1)
    dev.set_time_scheme(square.dt, True)
    square.restart()


@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_single_march_against_the_model(tan, first_order, n):
    """1. dde within 1e-8 relative of the model; two marches bit-identical; against central differences of the device's own dE series
    (eps = 1e-4) within the bound of tangent_energy_cases.fd_tol; the info reports fc_tan_energy on three workgroups."""
    dev = tan.dev
    assert tan.th.mesh.cells.shape[0] == 70 and dev.N == 378
    tm = te.TangentEnergyModel(tan.model)
    nn2 = 2 * tan.th.nn
    slot = slot_of(first_order)
    rng = np.random.default_rng(9)
    u, du = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    X, _ = case.taped_run(tan, first_order, n, u)
    out = dev.run_tangent(slot, n, du, d0, dm1)
    dde = dev.tangent_energy()
    again = dev.run_tangent(slot, n, du, d0, dm1)
    assert dde.shape == (n,) and np.array_equal(dde, dev.tangent_energy()) and all(np.array_equal(a, b) for a, b in zip(out, again))
    info = dev.tangent_energy_info()
    assert info == {"on": True, "have": True, "kernel": 1, "grid": 3, "steps": n, "k": 0, "launches": n, "bytes": 8 * (3 * n + n)}, info
    _, _, dde_m = tm.tangent_energy(first_order, X, du, d0, dm1)
    err = nm.rel(dde, dde_m)
    # the two mistakes of DESIGN section 5.4 are far outside the tolerance
    wrong = {w: nm.rel(tm.tangent_energy(first_order, X, du, d0, dm1, wrong=w)[2], dde_m) for w in ("x_masked", "mask_out")}

    def series(sign):
        dev.set_state(tan.u_n + sign * te.EPS * d0[:nn2], tan.u_nn + sign * te.EPS * dm1[:nn2], tan.p)
        return dev.run(slot, n, u + sign * te.EPS * du, compute_energy=True)[1]

    fd = nm.rel(dde, (series(1.0) - series(-1.0)) / (2 * te.EPS))
    tan.restart()
    print(f"tangent energy, first order {first_order}, n = {n}: against the model {err:.3e}, device central difference {fd:.3e}, "
          f"model with x masked {wrong['x_masked']:.3e}, with dx masked {wrong['mask_out']:.3e}")
    assert err <= te.TOL
    assert fd <= te.fd_tol("nl", "open")
    assert min(wrong.values()) > 1e4 * te.TOL


def test_opt_in(tan):
    """2. With the option on, dy, dx_n, dx_{n-1} are the bits of the march without it; with it off the bytes and the route row are
    those of a handle that never set it; fc_get_tangent_energy refuses after a march without the option; the option goes with the
    reserve."""
    dev = tan.dev
    n = 4
    rng = np.random.default_rng(17)
    u, du = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    z = rng.standard_normal(dev.N)
    case.taped_run(tan, 1, n, u)
    on = dev.run_tangent(SLOT_BDF1, n, du, z, z)
    route_on, bytes_on = dev.tangent_route().copy(), dev.tangent_info()["bytes"]
    assert dev.tangent_energy().shape == (n,)
    dev.tangent_set_energy(0)
    assert dev.tangent_energy_info() == {"on": False, "have": False, "kernel": 0, "grid": 0, "steps": 0, "k": 0, "launches": 0, "bytes": 0}
    off = dev.run_tangent(SLOT_BDF1, n, du, z, z)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    assert np.array_equal(route_on, dev.tangent_route())
    bytes_off = dev.tangent_info()["bytes"]
    assert bytes_on - bytes_off == 8 * (3 * n + n)
    refused(NOT_READY, dev.tangent_energy, match="without the energy option")
    # a reserve that never saw the option: the same bytes, the same bits
    dev.tangent_reserve(0)
    dev.tangent_reserve(1)
    assert not dev.tangent_energy_info()["on"]
    never = dev.run_tangent(SLOT_BDF1, n, du, z, z)
    assert dev.tangent_info()["bytes"] == bytes_off and all(np.array_equal(a, b) for a, b in zip(on, never))
    # on again; freed and laid out again: dropped
    dev.tangent_set_energy(1)
    dev.run_tangent(SLOT_BDF1, n, du, z, z)
    first = dev.tangent_energy()
    refused(INV, lambda: _lib.check(dev.lib.fc_get_tangent_energy(dev._h, n + 1, 0, np.zeros(n + 1))), match="the last march had n_steps = 4")
    refused(INV, lambda: _lib.check(dev.lib.fc_get_tangent_energy(dev._h, n, 4, np.zeros(4 * n))), match="k = 0")
    dev.tangent_reserve(1)
    assert not dev.tangent_energy_info()["on"] and dev.tangent_info()["bytes"] < bytes_off  # (du / dy are sized by the next march)
    refused(NOT_READY, dev.tangent_energy)
    dev.tangent_set_energy(1)
    dev.run_tangent(SLOT_BDF1, n, du, z, z)
    assert np.array_equal(first, dev.tangent_energy())
    # a FRESH handle that never calls a new entry point: it steps and marches to the same bits, and holds the same bytes
    y_on, x_on = case.taped_run(tan, 1, n, u)[1], dev.get_solution()
    fresh = nl_case.NlSquare()
    try:
        fresh.dev.adjoint_tape_reserve(6)
        fresh.dev.tangent_reserve(1)
        _, y_fresh = case.taped_run(fresh, 1, n, u)
        assert np.array_equal(y_fresh, y_on) and np.array_equal(fresh.dev.get_solution(), x_on)
        never = fresh.dev.run_tangent(SLOT_BDF1, n, du, z, z)
        assert all(np.array_equal(a, b) for a, b in zip(on, never)) and fresh.dev.tangent_info()["bytes"] == bytes_off
        assert np.array_equal(fresh.dev.tangent_route(), route_on)
        y1, _, _ = fresh.dev.step(SLOT_BDF2, u[0], compute_energy=False)
        y2, _, _ = dev.step(SLOT_BDF2, u[0], compute_energy=False)
        assert np.array_equal(y1, y2) and np.array_equal(fresh.dev.get_solution(), dev.get_solution())
    finally:
        fresh.close()


def test_refusals(tan):
    """7. The option without a reserve and with a bad value; a march whose tape does not hold the run enqueues nothing and leaves no
    rows; the march counter is unchanged by every refusal."""
    dev = tan.dev
    marches = dev.tangent_info()["marches"]
    refused(INV, dev.tangent_set_energy, 2, match="on must be 1 or 0")
    refused(INV, dev.run_tangent, SLOT_BDF1, 3, match="not begun")
    refused(NOT_READY, dev.tangent_energy)
    dev.tangent_reserve(0)
    refused(NOT_READY, dev.tangent_set_energy, 1, match="fc_tangent_reserve")
    assert not dev.tangent_energy_info()["on"] and dev.tangent_energy_info()["bytes"] == 0
    dev.tangent_reserve(1)
    assert dev.tangent_info()["marches"] == marches


def test_partitioned_handles_are_refused():
    """7b. A handle with an exchange (a thread-rank partition through fc_set_host_exchange, in a child process) is refused."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "tangent_energy_child.py"), "partitioned"], env=env, capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, f"child: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK partitioned" in out.stdout


@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_dot_product_identity_with_the_device_adjoint(tan, first_order, n):
    """3. sum e_m dde_m + sum w . dy + z . dx_n = <g, du> + <g_x0, dx_0> + <g_xm1, dx_{-1}> between the device tangent and the device
    adjoint with set_adjoint_energy(e) on the SAME tape: the defect is at most 1e-8 of the sum of the absolute terms.  The first check
    of the EN instantiation of fc_adj_elem_nl that does not go through numpy."""
    dev = tan.dev
    nn2 = 2 * tan.th.nn
    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    slot = slot_of(first_order)
    rng = np.random.default_rng(13)
    u, du = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    w, z, e = rng.standard_normal((n, dev.n_sens)), rng.standard_normal(dev.N), ec.weights(n)
    case.taped_run(tan, first_order, n, u)
    dy, dxn, _ = dev.run_tangent(slot, n, du, d0, dm1)
    dde = dev.tangent_energy()
    dev.set_adjoint_energy(e)
    try:
        g, gx0, gxm1 = dev.run_adjoint(slot, n, w, z)
        assert int(dev.adjoint_route()[0]) == ec.ELEM_NL_EN
    finally:
        dev.set_adjoint_energy(None)
    terms = [np.sum(e * dde), np.sum(w * dy), z @ dxn, -np.sum(g * du), -(gx0[:nn2] @ d0[:nn2]), -(gxm1[:nn2] @ dm1[:nn2])]
    defect = abs(sum(terms)) / sum(abs(t) for t in terms)
    print(f"device tangent x device adjoint with energy weights, first order {first_order}, n = {n}: energy term {terms[0]:.6e} of "
          f"{sum(abs(t) for t in terms):.6e}, identity defect {defect:.3e}")
    assert abs(terms[0]) > 1e-3 * sum(abs(t) for t in terms), "the energy term does not act"
    assert defect <= 1e-8


def test_tangent_tape(tan):
    """5. Column n - 1 of the tangent tape is the returned dx_n bit for bit, every column within 1e-8 of the model, bytes = 8 N n; the
    forward state, the state tape, the step counters, the march's results and a further forward step are the same bits with and
    without the tape; a longer march keeps nothing."""
    dev = tan.dev
    tm = te.TangentEnergyModel(tan.model)
    n = 4
    rng = np.random.default_rng(23)
    u, du = rng.standard_normal((n + 1, dev.n_act)), rng.standard_normal((n, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)

    def observe(tape):
        dev.tangent_tape_reserve(n if tape else 0)
        X, _ = case.taped_run(tan, 2, n, u[:n])
        count = dev.step_counts()
        out = dev.run_tangent(SLOT_BDF2, n, du, d0, dm1)
        kept = dev.tangent_tape_states() if tape else None
        assert dev.step_counts() == count
        seen = dict(zip(("dy", "dxn", "dxnm1", "dde", "tape", "solution"), [*out, dev.tangent_energy(), dev.adjoint_tape_states(), dev.get_solution()]))
        y, _, _ = dev.step(SLOT_BDF2, u[n], compute_energy=False)
        seen["y of a further step"], seen["its solution"] = y, dev.get_solution()
        return seen, kept, X

    before, _, _ = observe(False)
    assert dev.tangent_tape_info() == {"capacity": 0, "count": 0, "first_slot": -1, "bytes": 0}
    after, kept, X = observe(True)
    for name in before:
        assert np.array_equal(before[name], after[name]), f"{name} differs with the tangent tape"
    assert dev.tangent_tape_info() == {"capacity": n, "count": n, "first_slot": SLOT_BDF2, "bytes": 8 * dev.N * n}
    assert kept.shape == (n, dev.N) and np.array_equal(kept[n - 1], after["dxn"]) and np.array_equal(kept[n - 2], after["dxnm1"])
    D = tm.tangent(2, X, du, d0, dm1)[0]
    worst = max(nm.rel(kept[m - 1], D[m + 1]) for m in range(1, n + 1))
    print(f"tangent tape, n = {n}: columns against the model {worst:.3e}")
    assert worst <= te.TOL
    # a march longer than the tape keeps nothing; the tape is its own reserve
    dev.tangent_tape_reserve(n - 1)
    case.taped_run(tan, 2, n, u[:n])
    dev.run_tangent(SLOT_BDF2, n, du)
    assert dev.tangent_tape_info()["count"] == 0
    dev.tangent_reserve(0)
    assert dev.tangent_tape_info()["capacity"] == n - 1
    dev.tangent_reserve(1)
    dev.tangent_tape_reserve(0)
    assert dev.tangent_tape_info()["bytes"] == 0


def test_energy_source_refusals(tan):
    """7. Source 1: without a tangent tape, with a tape of another n or first slot, on a checkpointed state tape, on a batched march, in
    fc_step_adjoint; the tangent tape with a batch set -- each with its code and reason, and with the counters of everything a march
    would move read before and after EACH refusal: the energy steps of the adjoint marches (fc_adjoint_energy_info: a march with rows
    held starts it over), the tangent marches, the forward steps, the state of the tangent tape.  The source falls back to 0 with the
    rows and with the tape; a refused reserve leaves the tape and the source as they are."""
    dev = tan.dev

    def counters():
        return (dev.adjoint_energy_info()["steps"], dev.tangent_info()["marches"], dev.step_counts(), dev.tangent_tape_info(), dev.adjoint_energy_source())

    def refused_idle(code, fn, *args, match):
        before = counters()
        refused(code, fn, *args, match=match)
        assert counters() == before, (match, before, counters())

    for s in SLOTS:
        dev.set_adjoint_factors(s, 1)
    n = 3
    rng = np.random.default_rng(37)
    u, w = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_sens))
    e = ec.weights(n)
    refused(INV, dev.set_adjoint_energy_source, 2, match="source must be 0")
    case.taped_run(tan, 2, n, u)
    dev.set_adjoint_energy(e)
    dev.set_adjoint_energy_source(1)
    assert dev.adjoint_energy_source() == 1
    # (a march WITHOUT the source first, so that the energy-step counter stands at n, not at 0, when the refusals are counted)
    dev.set_adjoint_energy_source(0)
    dev.run_adjoint(SLOT_BDF2, n, w)
    assert dev.adjoint_energy_info()["steps"] == n
    dev.set_adjoint_energy_source(1)
    refused_idle(INV, dev.run_adjoint, SLOT_BDF2, n, w, match="no tangent tape is reserved")
    dev.tangent_tape_reserve(n)
    refused_idle(INV, dev.run_adjoint, SLOT_BDF2, n, w, match="it holds a march of 0 steps")
    dev.run_tangent(SLOT_BDF2, n, u)
    g1 = dev.run_adjoint(SLOT_BDF2, n, w)[0]
    assert int(dev.adjoint_route()[0]) == 15 and dev.adjoint_energy_info()["steps"] == n
    refused_idle(INV, dev.step_adjoint, SLOT_BDF2, 1.0, 0.0, None, match="the energy source is the tangent tape")
    refused_idle(INV, dev.tangent_tape_reserve, -1, match="n_steps must be in")  # (the tape holding the march and the source stay)
    assert dev.tangent_tape_info()["count"] == n and dev.adjoint_energy_source() == 1
    # another n, another first slot
    case.taped_run(tan, 2, n - 1, u[: n - 1])
    dev.run_tangent(SLOT_BDF2, n - 1, u[: n - 1])
    case.taped_run(tan, 2, n, u)
    refused_idle(INV, dev.run_adjoint, SLOT_BDF2, n, w, match="it holds a march of 2 steps")
    case.taped_run(tan, 1, n, u)
    dev.run_tangent(SLOT_BDF1, n, u)
    case.taped_run(tan, 2, n, u)
    refused_idle(INV, dev.run_adjoint, SLOT_BDF2, n, w, match="its march started on order slot 0")
    # the rows cleared: source 0; source 0 is the gradient of the energy again
    dev.set_adjoint_energy(None)
    assert dev.adjoint_energy_source() == 0
    dev.set_adjoint_energy(e)
    g0 = dev.run_adjoint(SLOT_BDF2, n, w)[0]
    assert int(dev.adjoint_route()[0]) == ec.ELEM_NL_EN and not np.array_equal(g0, g1)
    # the tape freed: source 0
    dev.set_adjoint_energy_source(1)
    dev.tangent_tape_reserve(0)
    assert dev.adjoint_energy_source() == 0
    dev.set_adjoint_energy(None)
    # a checkpointed state tape
    dev.adjoint_tape_reserve_sparse(6, 2)
    try:
        dev.tangent_tape_reserve(n)
        tan.restart()
        dev.adjoint_tape_begin()
        dev.run(SLOT_BDF2, n, u, compute_energy=False)
        dev.set_adjoint_energy(e)
        dev.set_adjoint_energy_source(1)
        refused_idle(INV, dev.run_adjoint, SLOT_BDF2, n, w, match="checkpointed")
    finally:
        dev.set_adjoint_energy(None)
        dev.tangent_tape_reserve(0)
        dev.adjoint_tape_reserve_sparse(0, 0)
        dev.adjoint_tape_reserve(6)
    # a batch: no tangent tape, and the batched march refuses source 1
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(4)
    try:
        refused_idle(INV, dev.tangent_tape_reserve, n, match="batch set")
        for s in SLOTS:
            dev.set_adjoint_batch(s, 1)
        dev.adjoint_tape_reserve_batch(6)
        dev.set_state_batch(*bc.column_states(tan.u_n, tan.u_nn, tan.p, 4))
        bc.forward_batch(dev, 2, rng.standard_normal((n, 4, dev.n_act)), tape=True)
        dev.set_adjoint_energy(np.ones((n, 4)))
        dev.set_adjoint_energy_source(1)
        refused_idle(INV, dev.run_adjoint_batch, SLOT_BDF2, n, rng.standard_normal((n, 4, dev.n_sens)), match="a batched product is not built")
    finally:
        dev.set_adjoint_energy(None)
        dev.adjoint_tape_reserve_batch(0)
        for s in SLOTS:
            dev.set_adjoint_batch(s, -1)
        dev.set_batch(0)
        dev.set_solver_options(refine=1, check_residual=1)
    assert dev.adjoint_energy_source() == 0


def test_gauss_newton_product_with_energy(tan):
    """6. flu.gauss_newton_product(energy=e) on the square against the model's J^T Q J v + R v + H_E v within 1e-8; symmetric to 1e-10
    in two random directions and v . H v >= 0 for e >= 0; energy=None is the call without the keyword bit for bit; with Q = R = 0 and
    e = (0, .., 0, 1), v . H v = dx_n^T M_s dx_n of the tangent's dx_n (the row indexing); rows, source and tapes are what they were."""
    from flowcontrol_amd import utils as flu

    dev, model = tan.dev, ec.with_energy(tan.model)
    tm = te.TangentEnergyModel(model)
    rng = np.random.default_rng(29)
    n = 5
    u = rng.standard_normal((n, dev.n_act))
    v, v2 = rng.standard_normal((n, dev.n_act)), rng.standard_normal((n, dev.n_act))
    Q, R = np.array([[2.5]]), np.array([[0.3, 0.1], [0.0, 0.2]])
    Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    e = 40.0 * (0.5 + rng.random(n))
    last = np.zeros(n)
    last[-1] = 1.0
    dev.adjoint_tape_reserve(0)
    dev.tangent_reserve(0)
    try:
        with flu.AdjointRun(dev, tape=6) as adj:
            tan.restart()
            Gv = flu.gauss_newton_product(dev, u, Q, R, v, adjoint=adj, energy=e)
            assert np.array_equal(dev.get_solution(), tan.x0) and not dev.adjoint_tape_info()["begun"]
            Gv2 = flu.gauss_newton_product(dev, u, Q, R, v2, adjoint=adj, energy=e)
            plain = flu.gauss_newton_product(dev, u, Q, R, v, adjoint=adj)
            none = flu.gauss_newton_product(dev, u, Q, R, v, adjoint=adj, energy=None)
            pin = flu.gauss_newton_product(dev, u, 0 * Q, 0 * R, v, adjoint=adj, energy=last)
            assert dev.adjoint_energy_info()["n_steps"] == 0 and dev.adjoint_energy_source() == 0
            assert dev.tangent_tape_info()["bytes"] == 0 and dev.tangent_info()["bytes"] == 0
            dev.tangent_reserve(1)
            adj.forward(u, first_order=2, compute_energy=False)
            dxn = dev.run_tangent(SLOT_BDF2, n, v)[1]
            dev.tangent_reserve(0)
    finally:
        dev.adjoint_tape_reserve(6)
        dev.tangent_reserve(1)
    X, _ = model.forward(2, u, tan.x0, tan.xm1)
    dym = tm.tangent(2, X, v)[1]
    G0 = model.adjoint(2, X, dym @ Qs)[0] + v @ Rs
    Gm = G0 + tm.energy_product(2, X, e, v)
    err, sym = nm.rel(Gv, Gm), abs(np.sum(v2 * Gv) - np.sum(v * Gv2)) / abs(np.sum(v2 * Gv))
    share = abs(np.sum(v * (Gm - G0))) / abs(np.sum(v * Gm))
    pinned, want = float(np.sum(v * pin)), float(dxn @ (ec.msym(model.M) @ dxn))
    print(f"gauss_newton_product(energy=) on the square: against the model {err:.3e}, v.Gv = {np.sum(v * Gv):.6e} (energy share {share:.2e}), "
          f"symmetry defect {sym:.3e}; e = (0,..,1): v.Hv = {pinned:.12e}, dx_n.M dx_n = {want:.12e}")
    assert np.array_equal(plain, none) and nm.rel(plain, G0) <= te.TOL
    assert share > 1e-3, "the energy term does not act on the product"
    assert err <= te.TOL and np.sum(v * Gv) >= 0.0 and sym <= 1e-10
    assert abs(pinned - want) <= 1e-8 * abs(want)
    tan.restart()


# ── the public functions on the nonlinear cylinder, O1 ───────────────────────────────────────────────────────────────────────────
def test_public_functions_on_the_cylinder(golden_dir):
    """8. O1, nonlinear, 20 steps: flu.tangent_run(energy=True) against central differences of the logged dE (eps = 1e-4) within the
    bound of item 1; the energy product in two directions symmetric (1e-10) and non-negative; state, log, tapes, rows and source are as
    they were.  O1 has 384 partials per step: the only place the fold runs with more partials than a workgroup has threads."""
    import tempfile

    from flowcontrol_amd import utils as flu
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
        assert -(-fs.th.mesh.cells.shape[0] // 32) > 256
        rng = np.random.default_rng(31)
        u = 0.5 * rng.standard_normal((n, dev.n_act))
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        log0 = len(fs.timeseries) if hasattr(fs, "timeseries") else None
        slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2

        def series(uu, a=0.0, b=0.0):
            dev.set_state(state0[0] + a, state0[1] + b, *state0[2:])
            dE = dev.run(slot, n, uu, compute_energy=True)[1]
            dev.set_state(*state0)
            return dE

        du, d0, dm1 = rng.standard_normal(u.shape), np.zeros(dev.N), np.zeros(dev.N)
        d0[:nn2], dm1[:nn2] = rng.standard_normal(nn2), rng.standard_normal(nn2)
        dy, dxn, _, dde = flu.tangent_run(fs, u, du, d0, dm1, energy=True)
        plain = flu.tangent_run(fs, u, du, d0, dm1)
        assert np.array_equal(plain[0], dy) and np.array_equal(plain[1], dxn) and dde.shape == (n,)
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state()))
        assert dev.adjoint_tape_info()["bytes"] == 0 and dev.tangent_info()["bytes"] == 0 and not dev.tangent_energy_info()["on"]
        eps = te.EPS
        fd = nm.rel(dde, (series(u + eps * du, eps * d0[:nn2], eps * dm1[:nn2]) - series(u - eps * du, -eps * d0[:nn2], -eps * dm1[:nn2])) / (2 * eps))
        Q, R = np.zeros((dev.n_sens, dev.n_sens)), np.zeros((dev.n_act, dev.n_act))
        e = 1.0 + rng.random(n)
        v, v2 = rng.standard_normal(u.shape), rng.standard_normal(u.shape)
        Hv, Hv2 = (flu.gauss_newton_product(fs, u, Q, R, q, energy=e) for q in (v, v2))
        sym = abs(np.sum(v2 * Hv) - np.sum(v * Hv2)) / abs(np.sum(v2 * Hv))
        print(f"O1 nonlinear, 20 steps: tangent_run(energy=True) against central differences of dE {fd:.3e}; energy product v.Hv = {np.sum(v * Hv):.6e}, "
              f"v2.Hv2 = {np.sum(v2 * Hv2):.6e}, symmetry defect {sym:.3e}")
        assert fd <= te.fd_tol("nl", "open")
        assert sym <= 1e-10 and np.sum(v * Hv) >= 0.0 and np.sum(v2 * Hv2) >= 0.0
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state()))
        assert dev.adjoint_tape_info()["bytes"] == 0 and dev.tangent_info()["bytes"] == 0 and dev.tangent_tape_info()["bytes"] == 0
        assert dev.adjoint_energy_info()["n_steps"] == 0 and dev.adjoint_energy_source() == 0
        assert log0 is None or len(fs.timeseries) == log0
    finally:
        fs.th.release_device()


# ── batched ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def column_inputs(sq, n):
    """Per column, the same for every k: start states, controls and the three perturbations (all different per column)."""
    un, unn, pp = bc.column_states(sq.u_n, sq.u_nn, sq.p, KMAX)
    rng = np.random.default_rng(53)
    na, N = sq.dev.n_act, sq.dev.N
    return {"un": un, "unn": unn, "pp": pp, "u": rng.standard_normal((n, KMAX, na)), "du": rng.standard_normal((n, KMAX, na)),
            "d0": rng.standard_normal((KMAX, N)), "dm1": rng.standard_normal((KMAX, N))}


@pytest.fixture(scope="module")
def square0():
    """The square without refinement sweeps: what a batched solve does."""
    sq = nl_case.NlSquare(refine=0)
    yield sq
    sq.close()


@pytest.fixture(scope="module")
def singles(square0):
    """The single march of every column's run, and of every column's direction about the run of column 2, once per case:
    {(first order, n): (own [n, K], about2 [n, K], about0 [n, K])}."""
    dev = square0.dev
    dev.adjoint_tape_reserve(6)
    dev.tangent_reserve(1)
    dev.tangent_set_energy(1)
    out = {}
    for first_order, n in nl_case.CASES:
        c = column_inputs(square0, n)
        slot = slot_of(first_order)

        def march(run, s):
            dev.set_state(c["un"][run], c["unn"][run], c["pp"][run])
            dev.adjoint_tape_begin()
            dev.run(slot, n, c["u"][:, run], compute_energy=False)
            dev.run_tangent(slot, n, c["du"][:, s], c["d0"][s], c["dm1"][s])
            return dev.tangent_energy()

        out[(first_order, n)] = tuple(np.stack([march(s if ref is None else ref, s) for s in range(KMAX)], axis=1) for ref in (None, 2, 0))
    dev.tangent_reserve(0)
    dev.adjoint_tape_reserve(0)
    square0.restart()
    return out


@pytest.mark.parametrize("k", [1, 5, 9, 17])
@pytest.mark.parametrize("first_order,n", nl_case.CASES)
def test_batched_march(square0, singles, first_order, n, k):
    """4. Each column about its own run, and every column about the run of column 2 (0 for k = 1): dde of every column within 1e-14
    relative of the single march of that column; two marches bit-identical; a NaN planted in one column's dx0 leaves the other
    columns' rows the clean march's bits and marks that column."""
    dev = square0.dev
    slot = slot_of(first_order)
    c = column_inputs(square0, n)
    un, unn, pp = c["un"][:k], c["unn"][:k], c["pp"][:k]
    u, du = np.ascontiguousarray(c["u"][:, :k]), np.ascontiguousarray(c["du"][:, :k])
    d0, dm1 = c["d0"][:k], c["dm1"][:k]
    own, about2, about0 = singles[(first_order, n)]
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(k)
    dev.adjoint_tape_reserve_batch(6)
    dev.tangent_reserve(1)
    dev.tangent_set_energy(1)
    try:
        KB = {1: 4, 5: 8, 9: 16, 17: 32}[k]
        G = -(-70 // (256 // KB))
        dev.set_state_batch(un, unn, pp)
        bc.forward_batch(dev, first_order, u, tape=True)
        plain = dev.run_tangent_batch(slot, n, du, d0, dm1)
        dde = dev.tangent_energy()
        info = dev.tangent_energy_info()
        assert info == {"on": True, "have": True, "kernel": 2, "grid": G, "steps": n, "k": k, "launches": n, "bytes": 8 * (n * G * KB + n * k)}, info
        again = dev.run_tangent_batch(slot, n, du, d0, dm1)
        assert dde.shape == (n, k) and np.array_equal(dde, dev.tangent_energy()) and all(np.array_equal(a, b) for a, b in zip(plain, again))
        rc = 2 if k > 2 else 0
        dev.run_tangent_batch(slot, n, du, d0, dm1, rc)
        shared = dev.tangent_energy()
        assert dev.tangent_energy_info()["kernel"] == 3
        e_own = bc.rel_columns(dde, own[:, :k], 1)
        e_shared = bc.rel_columns(shared, (about2 if rc == 2 else about0)[:, :k], 1)
        # a NaN in one column
        bad = min(1, k - 1)
        d0_bad = d0.copy()
        d0_bad[bad, 7] = np.nan
        with pytest.raises(FcDiverged):
            dev.run_tangent_batch(slot, n, du, d0_bad, dm1)
        assert dev.tangent_batch_flags[bad] == 1 and dev.tangent_batch_flags.sum() == 1
        keep = [s for s in range(k) if s != bad]
        marked = dev.tangent_energy()
        assert np.array_equal(marked[:, keep], dde[:, keep]) and not np.all(np.isfinite(marked[:, bad]))
        print(f"batched tangent energy first order {first_order}, n = {n}, k = {k}: own run {e_own:.3e}, about column {rc} {e_shared:.3e}")
        assert e_own <= TOL_BATCH and e_shared <= TOL_BATCH
    finally:
        dev.tangent_reserve(0)
        dev.adjoint_tape_reserve_batch(0)
        dev.set_batch(0)
        dev.set_solver_options(refine=0, check_residual=1)
        square0.restart()
