"""The adjoint of k lock-step closed loops on the MI355X (``fc_adjoint_loop_reserve_batch`` / ``_begin_batch`` / ``_info_batch``,
``fc_run_adjoint_closed_loop_batch``; csrc/fc_adjoint_loop_batch.hip.h, csrc/fc_adjoint_loop_batch_run.hpp, flowcontrol_amd/adjoint.py)
against the numpy / scipy model of tests/support/adjoint_loop_model.py run once per column, against the device's own single closed-loop
march and open-loop batched march, and against central differences of the device's own batched closed-loop runs.

Small problems: the linearised 8 x 8 square (N = 659, two Dirichlet actuators) and the nonlinear 7 x 5 square, each with two sensors;
the FlowSolver level runs on the cylinder's O1 mesh.  Every column has its own initial state, bank, signals, limits and weights
(tests/support/adjoint_loop_batch_cases.py); tests/test_adjoint_loop_batch_host.py checks without a GPU that every column's limits clamp
part of its controls, that the model alone meets 1e-7 for the inputs and step of the central differences here, and that a column given
its neighbour's inputs would be found out."""
import tempfile

import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcDiverged, FcError
from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_loop_batch_cases as lbc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm

pytestmark = pytest.mark.gpu

SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
#: the project's series tolerance against its oracle
TOL = 1e-8
CAPACITY = 16
OUT = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "ubar", "dx0", "dxm1")
#: groups whose arrays lead with the step index: column s is [:, s]
BY_STEP = ("w_y", "w_u", "ubar")


@pytest.fixture(scope="module")
def plant():
    p = lc.DevicePlant(False)
    yield p
    p.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    yield p
    p.close()


def slot_of(first_order):
    return SLOT_BDF1 if first_order == 1 else SLOT_BDF2


def use_batch(p, k):
    """The plant's handle with a batch of k as tests/support/adjoint_batch_cases.batch_on sets it (a nonlinear plant: with the batched
    state tape)."""
    if p.dev.batch_k != k:
        if p.dev._ctrl_bank is not None:
            p.dev.set_controllers(None, p.sq.dt)
        bc.batch_on(p.sq, k, tape=CAPACITY if p.nonlinear else 0)


def column(g, grp, s):
    return None if g[grp] is None else (g[grp][:, s] if grp in BY_STEP else g[grp][s])


def same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in OUT)


def forward(p, loops, cuts=None, tape=True):
    """The device's batched closed-loop run of the columns from their own initial states, taped: (y [n, k, .], u [n, k, .], bad [k])."""
    dev = p.dev
    lbc.put_loops(dev, loops, 2 * p.th.nn)
    if tape:
        if dev.adjoint_loop_info_batch()["capacity"] != CAPACITY:
            dev.adjoint_loop_reserve_batch(CAPACITY)
        if p.nonlinear:
            dev.adjoint_tape_begin_batch()
        dev.adjoint_loop_begin_batch()
    ys, us, y_last, order, bad = [], [], np.array([q.y0 for q in loops]), loops[0].first_order, None
    for n in cuts or (loops[0].n,):
        y, u, _, bad, _ = dev.run_closed_loop_batch(slot_of(order), n, y_last, compute_energy=False)
        ys.append(y), us.append(u)
        y_last, order = y[-1], 2
    return np.concatenate(ys), np.concatenate(us), bad


def march(p, cols, **kw):
    w, r, z = lbc.stack_inputs(cols)
    return p.dev.run_adjoint_closed_loop_batch(slot_of(cols[0][0].first_order), cols[0][0].n, w, r, z, **kw)


def device_costs(p, cols):
    """J_s = sum w . y + sum r . u + z . x_n of every column from an untaped run of the device."""
    w, r, z = lbc.stack_inputs(cols)
    y, u, _ = forward(p, [c[0] for c in cols], tape=False)
    return np.einsum("mks,mks->k", w, y) + np.einsum("mka,mka->k", r, u) + np.einsum("kn,kn->k", z, p.dev.get_solution_batch())


def column_against_model(g, y, u, s, col, label, skip=()):
    """Forward rows and every gradient group of column s against that column's model; returns the model's gradients."""
    loop, w, r, z = col
    f = loop.forward()
    gm = loop.adjoint(f, w, r, z)
    out = {"forward_y": lm.rel(y[:, s], f["y"][1:]), "forward_u": lm.rel(u[:, s], f["u"])}
    for grp in lm.GROUPS + ("ubar",):
        if grp in skip:
            continue
        if not np.any(gm[grp]):  # (nx = 0: no state; a BDF1 first step never reads x_{-1})
            assert not np.any(column(g, grp, s)), (label, s, grp)
            continue
        out[grp] = lm.rel(column(g, grp, s), gm[grp])
    print(f"{label}, column {s}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()), flush=True)
    for k, v in out.items():
        assert v <= TOL, f"{label}, column {s}: {k}: {v:.3e} > {TOL:.1e}"
    if loop.lo is not None:  # the device's clamp pattern is the model's mask
        at_limit = (u[:, s] == loop.lo) | (u[:, s] == loop.hi)
        assert np.array_equal(at_limit, gm["mask"] == 0.0), (s, at_limit, gm["mask"])
        assert np.array_equal(g["w_u"][:, s] == 0.0, at_limit)
    return gm


def against_model(p, cols, label):
    y, u, bad = forward(p, [c[0] for c in cols])
    assert np.all(bad == -1)
    g = march(p, cols)
    for s, col in enumerate(cols):
        column_against_model(g, y, u, s, col, label)
    return g


def main_columns(p, k, first_order, n):
    return lbc.columns(p.model, p.x0, p.xm1, 2 * p.th.nn, k, first_order, n)


# ── against the model ────────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("k,first_order,n", lbc.MAIN_CASES)
def test_gradients_against_the_model(plant, k, first_order, n):
    """Forward y, u and every gradient group of every column within 1e-8 of that column's model; the clamp pattern is the model's mask
    per column; two marches are bit-identical.  k = 3 and 5: padding columns exist."""
    use_batch(plant, k)
    cols = main_columns(plant, k, first_order, n)
    g = against_model(plant, cols, f"batched closed-loop adjoint, k = {k}, first order {first_order}, n = {n}")
    assert same(g, march(plant, cols)), "two identical marches differ"


@pytest.mark.parametrize("k,first_order,n", lbc.NL_CASES)
def test_nonlinear_plant_against_the_model(nl_plant, k, first_order, n):
    """The nonlinear 7 x 5 square: the closed-loop run advances the batched state tape, the march reads it."""
    use_batch(nl_plant, k)
    cols = main_columns(nl_plant, k, first_order, n)
    g = against_model(nl_plant, cols, f"nonlinear plant, k = {k}, first order {first_order}, n = {n}")
    assert nl_plant.dev.adjoint_tape_info_batch()["count"] == n
    assert same(g, march(nl_plant, cols)), "two identical marches differ"


@pytest.mark.parametrize("case", lbc.SHAPE_CASES, ids=lc.case_id)
def test_shapes(plant, case):
    """Every branch of the kernels at k = 3: nx = 0, 1, 13, 65, 256; nyc = 1, 2; nuc = 1 (fanned out) and n_act; with and without
    signals and limits; n = 1, 2, 3."""
    use_batch(plant, lbc.SHAPE_K)
    cols = lbc.shape_columns(plant.model, plant.x0, plant.xm1, 2 * plant.th.nn, case)
    against_model(plant, cols, lc.case_id(case))


# ── against the device's own single paths ────────────────────────────────────────────────────────────────────────────────────────
def test_columns_against_the_single_march(plant):
    """Each column of a k = 3 batch against the device's own run_closed_loop + run_adjoint_closed_loop of that column's loop on the
    same handle with the batch off: 1e-8 (measured: DESIGN section 5.4)."""
    dev, nn2 = plant.dev, 2 * plant.th.nn
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 12)
    yb, ub, _ = forward(plant, [c[0] for c in cols])
    g = march(plant, cols)
    dev.adjoint_loop_reserve_batch(0)
    dev.set_controllers(None, plant.sq.dt)
    dev.set_batch(0)  # (the solver options stay: both paths apply the factors directly)
    worst = 0.0
    try:
        for s, (loop, w, r, z) in enumerate(cols):
            dev.set_state(loop.x0[:nn2], loop.xm1[:nn2], loop.x0[nn2:])
            lc.put_loop(dev, loop)
            dev.adjoint_loop_reserve(CAPACITY)
            dev.adjoint_loop_begin()
            y, u, _ = dev.run_closed_loop(SLOT_BDF1, loop.n, loop.y0, compute_energy=False)
            gs = dev.run_adjoint_closed_loop(SLOT_BDF1, loop.n, w, r, z)
            d = {"y": lm.rel(yb[:, s], y), "u": lm.rel(ub[:, s], u)}
            for grp in OUT:
                if np.any(gs[grp]):
                    d[grp] = lm.rel(column(g, grp, s), gs[grp])
                else:
                    assert not np.any(column(g, grp, s)), grp
            worst = max(worst, *d.values())
            print(f"column {s} against the single march: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()), flush=True)
    finally:
        dev.adjoint_loop_reserve(0)
        dev.set_controllers(None, plant.sq.dt)
    print(f"batched closed-loop march against the single march, worst defect {worst:.3e}", flush=True)
    assert worst <= TOL


def test_equal_columns_are_bit_equal(plant):
    """Two columns given identical inputs have bit-equal outputs."""
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 12)
    cols[2] = (cols[0][0].clone(), *cols[0][1:])
    y, u, _ = forward(plant, [c[0] for c in cols])
    g = march(plant, cols)
    assert np.array_equal(y[:, 0], y[:, 2]) and np.array_equal(u[:, 0], u[:, 2])
    for grp in OUT:
        assert np.array_equal(column(g, grp, 0), column(g, grp, 2)), grp
        assert not np.array_equal(column(g, grp, 0), column(g, grp, 1)) or not np.any(column(g, grp, 0)), grp


def test_zero_controllers_are_the_open_loop_batched_march(plant, monkeypatch):
    """C = 0, D = 0 and no limits in every column: u = w_u, so dJ/dw_u and ubar are run_adjoint_batch's g for the same w and z bit for
    bit, dx0 / dxm1 are equal bit for bit and the gradients of Ad, Bd, w_y and y0 are exactly 0.  The same march with the g reduction
    inside the controller launch (FC_ADJ_LOOP_FUSE=1, the measured alternative) gives the same bits."""
    use_batch(plant, 3)
    cols = lbc.columns(plant.model, plant.x0, plant.xm1, 2 * plant.th.nn, 3, 1, 12, nx=13, limits=False)
    for loop, *_ in cols:
        loop.bank["C"][:] = 0.0
        loop.bank["D"][:] = 0.0
    _, u, _ = forward(plant, [c[0] for c in cols])
    assert np.array_equal(u, np.stack([c[0].w_u for c in cols], axis=1))
    w, _, z = lbc.stack_inputs(cols)
    g = plant.dev.run_adjoint_closed_loop_batch(SLOT_BDF1, 12, w, None, z)
    g_open, dx0, dxm1 = plant.dev.run_adjoint_batch(SLOT_BDF1, 12, w, z)
    assert np.array_equal(g["w_u"], g_open) and np.array_equal(g["ubar"], g_open)
    assert np.array_equal(g["dx0"], dx0) and np.array_equal(g["dxm1"], dxm1)
    assert not np.any(g["Ad"]) and not np.any(g["Bd"]) and not np.any(g["w_y"]) and not np.any(g["y0"])
    assert np.any(g["C"]) and np.any(g["D"])
    monkeypatch.setenv("FC_ADJ_LOOP_FUSE", "1")
    assert same(g, plant.dev.run_adjoint_closed_loop_batch(SLOT_BDF1, 12, w, None, z))


# ── against central differences ──────────────────────────────────────────────────────────────────────────────────────────────────
def central_differences(p, cols, label):
    """One random direction per group applied to one column at a time: the directional derivative of that column's cost against
    central differences of the device's own batched run; the other columns' costs do not move at all."""
    nn2, k = 2 * p.th.nn, len(cols)
    forward(p, [c[0] for c in cols])
    g = march(p, cols)
    base = device_costs(p, cols)
    for s in range(k):
        loop = cols[s][0]
        others = [q for q in range(k) if q != s]
        for grp in lm.GROUPS:
            ad_grp = column(g, grp, s)
            if not np.any(ad_grp):
                continue
            d = lc.fd_direction(grp, ad_grp.shape, seed=s, nn2=nn2)
            J = []
            for sign in (1.0, -1.0):
                moved = list(cols)
                moved[s] = (loop.perturbed(grp, d, sign * lc.FD_EPS), *cols[s][1:])
                J.append(device_costs(p, moved))
                assert np.array_equal(J[-1][others], base[others]), f"{label}: moving {grp} of column {s} moved another column's cost"
            fd = (J[0][s] - J[1][s]) / (2 * lc.FD_EPS)
            ad = float(np.sum(ad_grp * d))
            err = abs(fd - ad) / abs(fd)
            print(f"{label}, column {s}, {grp}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.2e}", flush=True)
            assert err <= lc.FD_TOL, f"{label}: column {s}: {grp}: {err:.3e} > {lc.FD_TOL:.1e}"


@pytest.mark.parametrize("first_order,n", lc.MAIN_CASES)
def test_central_differences_of_the_device_run(plant, first_order, n):
    use_batch(plant, 3)
    central_differences(plant, main_columns(plant, 3, first_order, n), f"k = 3, first order {first_order}, n = {n}")


@pytest.mark.parametrize("first_order,n", lc.NL_CASES)
def test_central_differences_on_the_nonlinear_plant(nl_plant, first_order, n):
    use_batch(nl_plant, 3)
    central_differences(nl_plant, main_columns(nl_plant, 3, first_order, n), f"nonlinear plant, k = 3, first order {first_order}, n = {n}")


# ── tape behaviour ───────────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_a_cut_run_is_one_tape(plant):
    """A forward run cut into 5 + 7 steps gives the gradients of the uncut run bit for bit; info_batch reports 12 steps."""
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 12)
    loops = [c[0] for c in cols]
    y, u, _ = forward(plant, loops)
    g = march(plant, cols)
    y2, u2, _ = forward(plant, loops, cuts=(5, 7))
    assert np.array_equal(y, y2) and np.array_equal(u, u2)
    info = plant.dev.adjoint_loop_info_batch()
    assert info["count"] == 12 and info["begun"] and not info["overflowed"] and info["bad"] == 0, info
    assert same(g, march(plant, cols))


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def test_nothing_moves_without_a_reserve(plant):
    """y, u and the final state of run_closed_loop_batch are bit-equal before a reserve, with the tape on and after reserve_batch(0);
    fc_adjoint_batch_info's bytes do not change; without a reserve the march answers FC_ERR_NOT_READY."""
    dev = plant.dev
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 12)
    loops = [c[0] for c in cols]
    w, r, z = lbc.stack_inputs(cols)
    dev.adjoint_loop_reserve_batch(0)
    held = lambda: [(i["tile_bytes"], i["march_bytes"], i["tape_bytes"]) for i in map(dev.adjoint_batch_info, SLOTS)]  # noqa: E731
    bytes0 = held()
    y0, u0, _ = forward(plant, loops, tape=False)
    x0 = dev.get_solution_batch()
    assert dev.adjoint_loop_info_batch() == {"capacity": 0, "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0, "bad": 0, "row": 0}
    refused(NOT_READY, dev.run_adjoint_closed_loop_batch, SLOT_BDF1, 12, w, r, z, match="no loop tape")
    refused(NOT_READY, dev.adjoint_loop_begin_batch, match="no loop tape")
    y1, u1, _ = forward(plant, loops)  # taped
    x1 = dev.get_solution_batch()
    info = dev.adjoint_loop_info_batch()
    assert info["capacity"] == CAPACITY and info["count"] == 12 and info["row"] == loops[0].bank["nx"] + 2 + 2
    assert info["bytes"] == 8 * 3 * (CAPACITY * info["row"] + int(np.size(lbc.stack_bank(loops)["Ad"][0]) + sum(np.size(loops[0].bank[q][0]) for q in ("Bd", "C", "D", "G", "g0", "S"))))
    assert held() == bytes0
    dev.adjoint_loop_reserve_batch(0)
    assert dev.adjoint_loop_info_batch()["bytes"] == 0 and dev.adjoint_loop_info_batch()["capacity"] == 0
    y2, u2, _ = forward(plant, loops, tape=False)
    x2 = dev.get_solution_batch()
    for a, b, c in ((y0, y1, y2), (u0, u1, u2), (x0, x1, x2)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    refused(NOT_READY, dev.run_adjoint_closed_loop_batch, SLOT_BDF1, 12, w, r, z, match="no loop tape")


# ── refusals and divergence ──────────────────────────────────────────────────────────────────────────────────────────────────────
def test_refusals(plant):
    """Every refusal returns its code and a word of its reason; the march that follows refused calls is the march of a clean handle."""
    dev = plant.dev
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 6)
    loops = [c[0] for c in cols]
    w, r, z = lbc.stack_inputs(cols)
    args = (SLOT_BDF1, 6, w, r, z)
    run = dev.run_adjoint_closed_loop_batch
    forward(plant, loops)
    ref = run(*args)
    # the tape does not hold this run: step count, first slot
    refused(INV, run, SLOT_BDF1, 5, w[:5], r[:5], z, match="holds 6 steps")
    refused(INV, run, SLOT_BDF2, 6, w, r, z, match="first taped step")
    refused(INV, run, SLOT_BDF1, 0, None, None, z, match="positive")
    assert same(ref, run(*args))
    # whatever changes the loops or the state ends the tape
    bank = lbc.stack_bank(loops)
    state = (np.array([q.x0[: 2 * plant.th.nn] for q in loops]), np.array([q.xm1[: 2 * plant.th.nn] for q in loops]))
    enders = {"fc_set_controller_state": lambda: dev.controller_state(bank["x0"]),
              "fc_set_loop_signals": lambda: dev.set_loop_signals(np.stack([q.w_y for q in loops], axis=1), np.stack([q.w_u for q in loops], axis=1)),
              "fc_set_control_limits": lambda: dev.set_control_limits(np.array([q.lo for q in loops]), np.array([q.hi for q in loops])),
              "fc_set_controllers": lambda: lbc.put_bank(dev, bank),
              "the flow state": lambda: dev.set_state_batch(*state),
              "fc_reset_sim_batch": lambda: dev.reset_sim_batch(1),
              "outside the closed loop": lambda: dev.step_batch(SLOT_BDF2, np.zeros((3, 2)), compute_energy=False)}
    for word, end in enders.items():
        forward(plant, loops)
        end()
        refused(INV, run, *args, match=word)
        assert not dev.adjoint_loop_info_batch()["begun"]
    # fc_set_batch frees everything
    forward(plant, loops)
    dev.set_controllers(None, plant.sq.dt)
    dev.set_batch(0)
    assert dev.adjoint_loop_info_batch()["bytes"] == 0 and dev.adjoint_loop_info_batch()["capacity"] == 0
    refused(NOT_READY, dev.adjoint_loop_reserve_batch, 4, match="fc_set_batch")
    use_batch(plant, 3)
    refused(NOT_READY, dev.adjoint_loop_reserve_batch, 4, match="no controller bank")
    refused(INV, dev.adjoint_loop_reserve_batch, -1, match="capacity")
    # reserved, not begun
    lbc.put_loops(dev, loops, 2 * plant.th.nn)
    dev.adjoint_loop_reserve_batch(CAPACITY)
    refused(INV, run, *args, match="not begun")
    # overflow: nothing is written beyond the capacity
    dev.adjoint_loop_reserve_batch(4)
    dev.adjoint_loop_begin_batch()
    dev.run_closed_loop_batch(SLOT_BDF1, 6, np.array([q.y0 for q in loops]), compute_energy=False)
    info = dev.adjoint_loop_info_batch()
    assert info["overflowed"] and info["count"] == 4 and info["lost"] == 2, info
    refused(INV, run, *args, match="overflowed")
    dev.adjoint_loop_reserve_batch(CAPACITY)
    # a bank of another k than the batch's: the reserve goes, the march names the mismatch
    forward(plant, loops)
    lbc.put_bank(dev, lbc.stack_bank(loops[:2]))
    assert dev.adjoint_loop_info_batch()["capacity"] == 0
    refused(INV, run, *args, match="ctl.k != bat.k")
    refused(INV, dev.adjoint_loop_reserve_batch, 4, match="k = 2")
    # what fc_run_adjoint_batch refuses: transposed factors switched off
    forward(plant, loops)
    dev.set_adjoint_factors(SLOT_BDF2, 0)
    refused(NOT_READY, run, *args, match="switched off")
    dev.set_adjoint_factors(SLOT_BDF2, 1)
    assert same(ref, run(*args))


def test_nonlinear_handle_without_the_state_tape(nl_plant):
    """A nonlinear handle's march needs the batched state tape of the same run."""
    dev = nl_plant.dev
    use_batch(nl_plant, 3)
    cols = main_columns(nl_plant, 3, 1, 6)
    loops = [c[0] for c in cols]
    w, r, z = lbc.stack_inputs(cols)
    forward(nl_plant, loops)
    ref = march(nl_plant, cols)
    # the state tape not begun for this run: the closed loop advances nothing
    lbc.put_loops(dev, loops, 2 * nl_plant.th.nn)
    dev.adjoint_loop_begin_batch()
    dev.run_closed_loop_batch(SLOT_BDF1, 6, np.array([q.y0 for q in loops]), compute_energy=False)
    refused(INV, dev.run_adjoint_closed_loop_batch, SLOT_BDF1, 6, w, r, z, match="state tape")
    # no state tape at all
    dev.adjoint_tape_reserve_batch(0)
    refused(INV, dev.run_adjoint_closed_loop_batch, SLOT_BDF1, 6, w, r, z, match="state tape")
    dev.adjoint_tape_reserve_batch(CAPACITY)
    forward(nl_plant, loops)
    assert same(ref, march(nl_plant, cols))


def test_a_non_finite_column_stays_alone(plant):
    """Column 1 starts from an inf in a free velocity dof: flags_out marks column 1 only, its outputs are NaN, columns 0 and 2 match
    their models."""
    dev, nn2 = plant.dev, 2 * plant.th.nn
    use_batch(plant, 3)
    cols = main_columns(plant, 3, 1, 6)
    loops = [c[0].clone() for c in cols]
    loops[1].x0[np.flatnonzero(plant.model.free[:nn2])[40]] = np.inf  # (a free velocity dof: the mass term carries it into the right-hand side)
    y, u, bad = forward(plant, loops)
    assert bad[1] >= 0 and bad[0] == -1 and bad[2] == -1, bad
    assert dev.adjoint_loop_info_batch()["bad"] == 0b010
    with pytest.raises(FcDiverged):
        march(plant, cols)
    assert dev.adjoint_batch_flags.tolist() == [0, 1, 0]
    g = dev.adjoint_loop_batch_last
    for grp in OUT:
        a = column(g, grp, 1)
        assert a.size == 0 or np.all(np.isnan(a)), grp
    for s in (0, 2):
        column_against_model(g, y, u, s, cols[s], "beside a non-finite column")
    # ... and the next run of the three columns is clean again
    forward(plant, [c[0] for c in cols])
    march(plant, cols)
    assert not np.any(dev.adjoint_batch_flags)


# ── FlowSolver level: the cylinder on O1 with k perturbed copies of the shipped controller ────────────────────────────────────────
def test_cost_gradients_of_any_number_of_candidates(golden_dir):
    """optim.closed_loop_cost_gradients: five candidates in chunks of two (the last chunk is filled up and the filler dropped) give the
    costs and gradients of one batch of five."""
    from pathlib import Path

    import flowcontrol_amd
    from flowcontrol_amd import optim
    from flowcontrol_amd.controller import Controller
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_solver.is_eq_nonlinear = False
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    K0 = Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat")
    rng = np.random.default_rng(5)
    Ks = [Controller(*(M * (1.0 + 0.05 * rng.standard_normal(M.shape)) for M in (K0.A, K0.B, K0.C, K0.D)), x0=0.1 * rng.standard_normal(K0.nstates))
          for _ in range(5)]
    Q, R = np.eye(3), 0.1 * np.eye(2)
    try:
        J, g = optim.closed_loop_cost_gradients(fs, Ks, 8, Q, R, batch=2)
        J5, g5 = optim.closed_loop_cost_gradients(fs, Ks, 8, Q, R, batch=8)
        assert J.shape == (5,) and len(g) == 5 and len(g5) == 5
        assert np.all(np.abs(J - J5) <= TOL * np.abs(J5))
        for a, b in zip(g, g5):
            assert set(a) == set(b)
            for q in a:
                assert lm.rel(a[q], b[q]) <= TOL, q
        assert len({float(v) for v in J}) == 5  # (five candidates, five costs: no filler among them)
    finally:
        fs.th.release_device()


@pytest.mark.parametrize("nonlinear", [False, True])
def test_batched_closed_loop_gradient_on_the_cylinder(golden_dir, nonlinear):
    """batched_closed_loop_gradient on O1, k = 4 copies of the shipped 13-state controller with perturbed matrices and states, 10 steps:
    J equals the cost of bfs.run_closed_loop to 1e-12, two random directions over (A, B, C, D) of one controller against central
    differences at 1e-6; the batched state and the controllers' states are put back; every tape byte counter is 0 afterwards."""
    from pathlib import Path

    import flowcontrol_amd
    import flowcontrol_amd.utils as flu
    from flowcontrol_amd.batch import BatchedFlowSolver
    from flowcontrol_amd.controller import Controller
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_solver.is_eq_nonlinear = nonlinear
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    K0 = Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat")
    k, n = 4, 10
    try:
        bfs = BatchedFlowSolver(fs, k)
        bfs.initialize_time_stepping(ics=[ParamIC(xloc=2.0 + 0.3 * s, yloc=0.1 * s, radius=0.5, amplitude=1.0 - 0.1 * s) for s in range(k)])
        dev = bfs.dev
        rng = np.random.default_rng(37)
        mats = [[M * (1.0 + 0.05 * rng.standard_normal(M.shape)) for M in (K0.A, K0.B, K0.C, K0.D)] for _ in range(k)]
        xc0 = 0.1 * rng.standard_normal((k, K0.nstates))
        make = lambda ms: [Controller(*m, x0=xc0[s]) for s, m in enumerate(ms)]  # noqa: E731
        Q = np.diag(1.0 + np.arange(dev.n_sens))
        R = 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state_batch()]
        y_start = np.array(bfs.y_meas, dtype=float)
        slot = SLOT_BDF1 if bfs.order == 1 else SLOT_BDF2

        def cost(ms):
            dev.set_controllers(make(ms), fs.params_time.dt)
            y, u, _, _, _ = dev.run_closed_loop_batch(slot, n, y_start, compute_energy=False)
            dev.set_state_batch(*state0)
            dev.set_controllers(None, fs.params_time.dt)
            return 0.5 * (np.einsum("mki,ij,mkj->k", y, Q, y) + np.einsum("mki,ij,mkj->k", u, R, u))

        Ks = make(mats)
        J, g = flu.batched_closed_loop_gradient(bfs, Ks, n, Q, R)
        J2, g2 = bfs.closed_loop_gradient(Ks, n, Q, R)
        assert np.array_equal(J, J2) and all(np.array_equal(g[s][q], g2[s][q]) for s in range(k) for q in g[s])
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state_batch()))
        assert all(np.array_equal(K.x, xc0[s]) for s, K in enumerate(Ks))
        assert dev.adjoint_loop_info_batch()["bytes"] == 0 and dev.adjoint_loop_info()["bytes"] == 0 and dev.adjoint_tape_info_batch()["bytes"] == 0
        assert all(dev.adjoint_batch_info(s)["tape_bytes"] == 0 and dev.adjoint_batch_info(s)["march_bytes"] == 0 for s in SLOTS)
        assert all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
        assert len(g) == k and set(g[0]) == {"Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "A", "B"}
        assert g[0]["A"].shape == (13, 13) and g[0]["w_u"].shape == (n, dev.n_act)
        assert np.all(np.abs(J - cost(mats)) <= 1e-12 * np.abs(J))
        for q in range(2):
            s = q + 1  # the controller that moves
            d = [rng.standard_normal(M.shape) * np.abs(M).max() for M in mats[s]]
            eps = lc.FD_EPS
            moved = lambda sign: [[M + sign * eps * dm for M, dm in zip(ms, d)] if c == s else ms for c, ms in enumerate(mats)]  # noqa: E731
            Jp, Jm = cost(moved(1.0)), cost(moved(-1.0))
            others = [c for c in range(k) if c != s]
            assert np.array_equal(Jp[others], Jm[others])
            fd = (Jp[s] - Jm[s]) / (2 * eps)
            ad = float(sum(np.sum(g[s][name] * dm) for name, dm in zip(("A", "B", "C", "D"), d)))
            err = abs(fd - ad) / abs(fd)
            print(f"O1 {'nonlinear' if nonlinear else 'linearised'}, k = {k}, {n} steps, controller {s}: central difference {fd:.12e}, "
                  f"adjoint {ad:.12e}, relative {err:.3e}", flush=True)
            assert err <= 1e-6
        # J is the cost of the BatchedFlowSolver's own closed loop (last: it books its log and advances the runs)
        yb, ub, _ = bfs.run_closed_loop(n, make(mats))
        Jb = 0.5 * (np.einsum("mki,ij,mkj->k", yb, Q, yb) + np.einsum("mki,ij,mkj->k", ub, R, ub))
        assert np.all(np.abs(J - Jb) <= 1e-12 * np.abs(J)), (J, Jb)
    finally:
        fs.th.release_device()
