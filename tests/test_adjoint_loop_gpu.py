"""The adjoint of a closed loop on the MI355X (``fc_adjoint_loop_reserve`` / ``_begin``, ``fc_run_adjoint_closed_loop``;
csrc/fc_adjoint_loop.hip.h, csrc/fc_adjoint_loop_run.hpp, flowcontrol_amd/adjoint.py) against the numpy / scipy model of
tests/support/adjoint_loop_model.py and against central differences of the device's own closed-loop runs.

Small problems: the linearised 8 x 8 square (N = 659, two Dirichlet actuators) and the nonlinear 7 x 5 square, each with two sensors;
the FlowSolver level runs on the cylinder's O1 mesh.  The inputs of every case (bank, signals, limits, weights) come from
tests/support/adjoint_loop_cases.py; tests/test_adjoint_loop_host.py checks without a GPU that their limits clamp part of the controls
and that the model alone meets 1e-7 for the inputs and step of the central differences here."""
import tempfile

import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcDiverged, FcError
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm

pytestmark = pytest.mark.gpu

SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
#: the project's series tolerance against its oracle
TOL = 1e-8
CAPACITY = 16
OUT = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "ubar", "dx0", "dxm1")


@pytest.fixture(scope="module")
def plant():
    p = lc.DevicePlant(False)
    yield p
    p.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    p.dev.adjoint_tape_reserve(CAPACITY)
    yield p
    p.close()


def slot_of(first_order):
    return SLOT_BDF1 if first_order == 1 else SLOT_BDF2


def forward(p, loop, cuts=None, tape=True):
    """The device closed-loop run of ``loop`` from its own initial state, taped: (y [n], u [n])."""
    dev, nn2 = p.dev, 2 * p.th.nn
    dev.set_state(loop.x0[:nn2], loop.xm1[:nn2], loop.x0[nn2:])
    lc.put_loop(dev, loop)
    if tape:
        if dev.adjoint_loop_info()["capacity"] != CAPACITY:
            dev.adjoint_loop_reserve(CAPACITY)
        if p.nonlinear:
            dev.adjoint_tape_begin()
        dev.adjoint_loop_begin()
    ys, us, y_last, order = [], [], loop.y0, loop.first_order
    for n in cuts or (loop.n,):
        y, u, _ = dev.run_closed_loop(slot_of(order), n, y_last, compute_energy=False)
        ys.append(y), us.append(u)
        y_last, order = y[-1], 2
    return np.vstack(ys), np.vstack(us)


def device_cost(p, loop, w, r, z):
    y, u = forward(p, loop, tape=False)
    return float(np.sum(w * y) + np.sum(r * u) + z @ p.dev.get_solution())


def same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in OUT)


def against_model(p, loop, w, r, z, label):
    """Forward run and every gradient group of the device against the model; returns (device gradients, model gradients)."""
    y, u = forward(p, loop)
    f = loop.forward()
    g = p.dev.run_adjoint_closed_loop(slot_of(loop.first_order), loop.n, w, r, z)
    gm = loop.adjoint(f, w, r, z)
    out = {"forward_y": lm.rel(y, f["y"][1:]), "forward_u": lm.rel(u, f["u"])}
    for grp in lm.GROUPS + ("ubar",):
        if not np.any(gm[grp]):  # (nx = 0: no state; a BDF1 first step never reads x_{-1})
            assert not np.any(g[grp]), grp
            continue
        out[grp] = lm.rel(g[grp], gm[grp])
    print(f"{label}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()), flush=True)
    for k, v in out.items():
        assert v <= TOL, f"{label}: {k}: {v:.3e} > {TOL:.1e}"
    if loop.lo is not None:  # the device's clamp pattern is the model's mask
        lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
        at_limit = (u == loop.lo) | (u == loop.hi)
        assert np.array_equal(at_limit, gm["mask"] == 0.0), (at_limit, gm["mask"])
        assert np.array_equal(g["w_u"] == 0.0, at_limit)
    return g, gm


@pytest.mark.parametrize("first_order,n", lc.MAIN_CASES)
def test_gradients_against_the_model(plant, first_order, n):
    """Every gradient group within 1e-8 relative of the model, n = 12 from BDF1 and n = 3 from BDF2, with signals and limits that clamp
    part of the controls; the clamp pattern of u_seq is the model's mask; two marches are bit-identical."""
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, first_order, n)
    g, _ = against_model(plant, loop, w, r, z, f"closed-loop adjoint, first order {first_order}, n = {n}")
    g2 = plant.dev.run_adjoint_closed_loop(slot_of(first_order), n, w, r, z)
    assert same(g, g2), "two identical marches differ"


@pytest.mark.parametrize("case", lc.SHAPE_CASES + lc.SHORT_CASES, ids=lc.case_id)
def test_shapes(plant, case):
    """Every branch of the two kernels: nx = 0, 1, 13, 65, 256; nyc = 1, 2; nuc = 1 (fanned out) and n_act; with and without signals
    and limits; n = 1, 2, 3."""
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, **case)
    against_model(plant, loop, w, r, z, lc.case_id(case))


def test_zero_controller_is_the_open_loop_march(plant):
    """C = 0 and D = 0 without limits: u = w_u, so dJ/dw_u is fc_run_adjoint's g for the same w and z bit for bit, and the gradients
    of Ad and Bd are exactly 0."""
    loop, w, _, z = lc.make_case(plant.model, plant.x0, plant.xm1, 1, 12, nx=13, limits=False)
    loop.bank["C"][:] = 0.0
    loop.bank["D"][:] = 0.0
    _, u = forward(plant, loop)
    assert np.array_equal(u, loop.w_u)
    g = plant.dev.run_adjoint_closed_loop(SLOT_BDF1, 12, w, None, z)
    g_open, dx0, dxm1 = plant.dev.run_adjoint(SLOT_BDF1, 12, w, z)
    assert np.array_equal(g["w_u"], g_open) and np.array_equal(g["ubar"], g_open)
    assert np.array_equal(g["dx0"], dx0) and np.array_equal(g["dxm1"], dxm1)
    assert not np.any(g["Ad"]) and not np.any(g["Bd"]) and not np.any(g["w_y"]) and not np.any(g["y0"])
    assert np.any(g["C"]) and np.any(g["D"])


def central_differences(p, loop, w, r, z, g, label):
    nn2 = 2 * p.th.nn
    worst = 0.0
    for grp in lm.GROUPS:
        if not np.any(g[grp]):
            continue
        d = lc.fd_direction(grp, g[grp].shape, nn2=nn2)
        fd = (device_cost(p, loop.perturbed(grp, d, lc.FD_EPS), w, r, z) - device_cost(p, loop.perturbed(grp, d, -lc.FD_EPS), w, r, z)) / (2 * lc.FD_EPS)
        ad = float(np.sum(g[grp] * d))
        err = abs(fd - ad) / abs(fd)
        worst = max(worst, err)
        print(f"{label}, {grp}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.2e}", flush=True)
        assert err <= lc.FD_TOL, f"{label}: {grp}: {err:.3e} > {lc.FD_TOL:.1e}"
    return worst


@pytest.mark.parametrize("first_order,n", lc.MAIN_CASES)
def test_central_differences_of_the_device_run(plant, first_order, n):
    """The directional derivative along one random direction per group against central differences of the device's own
    run_closed_loop cost at the step of tests/support/adjoint_loop_cases.py: 1e-6."""
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, first_order, n)
    forward(plant, loop)
    g = plant.dev.run_adjoint_closed_loop(slot_of(first_order), n, w, r, z)
    central_differences(plant, loop, w, r, z, g, f"first order {first_order}, n = {n}")


@pytest.mark.parametrize("first_order,n", lc.NL_CASES)
def test_nonlinear_plant(nl_plant, first_order, n):
    """The nonlinear 7 x 5 square with the state tape of the same run: against the model at 1e-8 and against central differences."""
    loop, w, r, z = lc.make_case(nl_plant.model, nl_plant.x0, nl_plant.xm1, first_order, n)
    g, _ = against_model(nl_plant, loop, w, r, z, f"nonlinear plant, first order {first_order}, n = {n}")
    central_differences(nl_plant, loop, w, r, z, g, f"nonlinear plant, first order {first_order}, n = {n}")


def test_a_cut_run_is_one_tape(plant):
    """A forward run cut into 5 + 7 steps gives the gradients of the uncut run bit for bit."""
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, 1, 12)
    y, u = forward(plant, loop)
    g = plant.dev.run_adjoint_closed_loop(SLOT_BDF1, 12, w, r, z)
    y2, u2 = forward(plant, loop, cuts=(5, 7))
    assert np.array_equal(y, y2) and np.array_equal(u, u2)
    info = plant.dev.adjoint_loop_info()
    assert info["count"] == 12 and info["begun"] and not info["overflowed"] and not info["bad"], info
    g2 = plant.dev.run_adjoint_closed_loop(SLOT_BDF1, 12, w, r, z)
    assert same(g, g2)


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def test_nothing_moves_without_a_reserve(plant):
    """Without a reserve the closed-loop trajectory is bit-identical to a run with the tape on, fc_adjoint_info's bytes do not change
    and the new entry point answers FC_ERR_NOT_READY; after reserve(0) the handle is as before."""
    dev = plant.dev
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, 1, 12)
    dev.adjoint_loop_reserve(0)
    bytes0 = [dev.adjoint_info(s)["bytes"] for s in SLOTS]
    y0, u0 = forward(plant, loop, tape=False)
    x0 = dev.get_solution()
    assert dev.adjoint_loop_info() == {"capacity": 0, "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0, "bad": False, "row": 0}
    refused(NOT_READY, dev.run_adjoint_closed_loop, SLOT_BDF1, 12, w, r, z, match="no loop tape")
    refused(NOT_READY, dev.adjoint_loop_begin, match="no loop tape")
    y1, u1 = forward(plant, loop)  # taped
    x1 = dev.get_solution()
    info = dev.adjoint_loop_info()
    assert info["capacity"] == CAPACITY and info["count"] == 12 and info["bytes"] > 0 and info["row"] == loop.bank["nx"] + 2 + 2
    assert [dev.adjoint_info(s)["bytes"] for s in SLOTS] == bytes0
    dev.adjoint_loop_reserve(0)
    assert dev.adjoint_loop_info()["bytes"] == 0 and dev.adjoint_loop_info()["capacity"] == 0
    y2, u2 = forward(plant, loop, tape=False)
    x2 = dev.get_solution()
    for a, b, c in ((y0, y1, y2), (u0, u1, u2), (x0, x1, x2)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    refused(NOT_READY, dev.run_adjoint_closed_loop, SLOT_BDF1, 12, w, r, z, match="no loop tape")


def test_refusals(plant):
    """Every refusal returns its code and reason; the march that follows a refused call is the march of a clean handle."""
    dev = plant.dev
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, 1, 6)
    args = (SLOT_BDF1, 6, w, r, z)
    forward(plant, loop)
    ref = dev.run_adjoint_closed_loop(*args)
    # the tape does not hold this run: step count, first slot
    refused(INV, dev.run_adjoint_closed_loop, SLOT_BDF1, 5, w[:5], r[:5], z, match="holds 6 steps")
    refused(INV, dev.run_adjoint_closed_loop, SLOT_BDF2, 6, w, r, z, match="first taped step")
    refused(INV, dev.run_adjoint_closed_loop, SLOT_BDF1, 0, None, None, z, match="positive")
    assert same(ref, dev.run_adjoint_closed_loop(*args))
    # whatever changes the loop or the state ends the tape
    enders = {"fc_set_controller_state": lambda: dev.controller_state(loop.bank["x0"]),
              "fc_set_loop_signals": lambda: dev.set_loop_signals(loop.w_y, loop.w_u),
              "fc_set_control_limits": lambda: dev.set_control_limits(loop.lo, loop.hi),
              "fc_set_controllers": lambda: lc.put_bank(dev, loop.bank),
              "the flow state": plant.restart}
    for word, end in enders.items():
        forward(plant, loop)
        end()
        refused(INV, dev.run_adjoint_closed_loop, *args, match=word)
        assert not dev.adjoint_loop_info()["begun"]
    # a step outside the closed loop
    y, _ = forward(plant, loop, cuts=(5,))
    dev.step(SLOT_BDF2, np.zeros(2), compute_energy=False)
    dev.run_closed_loop(SLOT_BDF2, 1, y[-1], compute_energy=False)
    refused(INV, dev.run_adjoint_closed_loop, *args, match="outside the closed loop")
    # reserved, not begun
    dev.adjoint_loop_reserve(CAPACITY)
    refused(INV, dev.run_adjoint_closed_loop, *args, match="not begun")
    # overflow: nothing is written beyond the capacity
    dev.adjoint_loop_reserve(4)
    plant.restart()
    lc.put_loop(dev, loop)
    dev.adjoint_loop_begin()
    dev.run_closed_loop(SLOT_BDF1, 6, loop.y0, compute_energy=False)
    info = dev.adjoint_loop_info()
    assert info["overflowed"] and info["count"] == 4 and info["lost"] == 2, info
    refused(INV, dev.run_adjoint_closed_loop, *args, match="overflowed")
    dev.adjoint_loop_reserve(CAPACITY)
    # a forward run that went non-finite
    nn2 = 2 * plant.th.nn
    bad = loop.x0[:nn2].copy()
    bad[np.flatnonzero(plant.model.free[:nn2])[40]] = np.inf  # (a free velocity dof: the mass term carries it into the right-hand side)
    dev.set_state(bad, loop.xm1[:nn2], loop.x0[nn2:])
    lc.put_loop(dev, loop)
    dev.adjoint_loop_begin()
    with pytest.raises(FcDiverged):
        dev.run_closed_loop(SLOT_BDF1, 6, loop.y0, compute_energy=False)
    assert dev.adjoint_loop_info()["bad"]
    refused(INV, dev.run_adjoint_closed_loop, *args, match="non-finite")
    # what fc_run_adjoint refuses: transposed factors switched off
    forward(plant, loop)
    dev.set_adjoint_factors(SLOT_BDF2, 0)
    refused(NOT_READY, dev.run_adjoint_closed_loop, *args, match="switched off")
    dev.set_adjoint_factors(SLOT_BDF2, 1)
    assert same(ref, dev.run_adjoint_closed_loop(*args))
    # k != 1: a batch, and a bank of two
    dev.set_batch(2)
    refused(INV, dev.adjoint_loop_begin, match="batch")
    two = lm.copy_bank(loop.bank)
    for k in ("Ad", "Bd", "C", "D", "x0", "G", "g0", "S"):
        two[k] = np.concatenate([two[k], two[k]])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    keep = [f(two[k]) for k in ("Ad", "Bd", "C", "D", "x0", "G", "g0", "S")]
    _lib.check(dev.lib.fc_set_controllers(dev._h, 2, two["nx"], two["nyc"], two["nuc"], *(_lib.ptr(a) for a in keep)))
    assert dev.adjoint_loop_info()["capacity"] == 0  # (the reserve went with the single controller)
    refused(INV, dev.run_adjoint_closed_loop, *args, match="k = 2")
    refused(INV, dev.adjoint_loop_reserve, 4, match="batch")
    dev.set_controllers(None, plant.sq.dt)
    dev.set_batch(0)
    refused(NOT_READY, dev.adjoint_loop_reserve, 4, match="no controller bank")
    # ... and the handle still does what it did
    forward(plant, loop)
    assert same(ref, dev.run_adjoint_closed_loop(*args))


# ── FlowSolver level: the cylinder on O1 with the shipped controller ──────────────────────────────────────────────────────────────
@pytest.mark.parametrize("nonlinear", [False, True])
def test_closed_loop_gradient_on_the_cylinder(golden_dir, nonlinear):
    """closed_loop_gradient on the cylinder's O1 mesh with the shipped 13-state controller, 20 steps, against central differences of the
    device's own closed-loop cost in two random directions over the controller's continuous-time matrices: 1e-6.  The flow state and
    the controller state are left where they were; the tapes and the adjoint setup are released."""
    from pathlib import Path

    import flowcontrol_amd
    import flowcontrol_amd.utils as flu
    from flowcontrol_amd.controller import Controller
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.params_solver.is_eq_nonlinear = nonlinear
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    K = Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat")
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        n, dt = 20, fs.params_time.dt
        rng = np.random.default_rng(31)
        K.x = 0.1 * rng.standard_normal(K.nstates)
        Q = np.diag(1.0 + np.arange(dev.n_sens))
        R = 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        xc0 = K.x.copy()
        slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2
        y_start = np.array(fs.y_meas, dtype=float)

        def cost(A, B, C, D):
            dev.set_controllers([Controller(A, B, C, D, x0=xc0)], dt)
            y, u, _ = dev.run_closed_loop(slot, n, y_start, compute_energy=False)
            dev.set_state(*state0)
            dev.set_controllers(None, dt)
            return 0.5 * (np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", u, R, u))

        J, g = flu.closed_loop_gradient(fs, K, n, Q, R)
        J2, g2 = fs.closed_loop_gradient(K, n, Q, R)
        assert J == J2 and all(np.array_equal(g[k], g2[k]) for k in g)
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state())) and np.array_equal(K.x, xc0)
        assert dev.adjoint_loop_info()["bytes"] == 0 and dev.adjoint_tape_info()["bytes"] == 0 and all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
        assert abs(J - cost(K.A, K.B, K.C, K.D)) <= 1e-12 * abs(J)
        assert set(g) == {"Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "A", "B"}
        assert g["A"].shape == (13, 13) and g["B"].shape == K.B.shape and g["w_u"].shape == (n, dev.n_act)
        for k in range(2):
            # a direction over (A, B, C, D), each matrix moved by 2e-5 of its largest entry
            d = [rng.standard_normal(M.shape) * np.abs(M).max() for M in (K.A, K.B, K.C, K.D)]
            eps = lc.FD_EPS
            fd = (cost(*(M + eps * dm for M, dm in zip((K.A, K.B, K.C, K.D), d))) - cost(*(M - eps * dm for M, dm in zip((K.A, K.B, K.C, K.D), d)))) / (2 * eps)
            ad = float(sum(np.sum(g[name] * dm) for name, dm in zip(("A", "B", "C", "D"), d)))
            err = abs(fd - ad) / abs(fd)
            print(f"O1 {'nonlinear' if nonlinear else 'linearised'}, 20 steps: J = {J:.6e}, direction {k}: central difference {fd:.12e}, "
                  f"adjoint {ad:.12e}, relative {err:.3e}", flush=True)
            assert err <= 1e-6
    finally:
        fs.th.release_device()
