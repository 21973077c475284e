"""The tangent of a closed loop on the MI355X (``fc_run_tangent_closed_loop``; csrc/fc_tangent_loop.hip.h,
csrc/fc_tangent_loop_run.hpp, flowcontrol_amd/tangent.py) against the numpy model of tests/support/tangent_loop_model.py, against the
device's own closed-loop ADJOINT through the dot-product identity, and against central differences of the device's own closed-loop runs.

The problems are those of tests/test_adjoint_loop_gpu.py (tests/support/adjoint_loop_cases.py): the linearised 8 x 8 square (N = 659)
and the nonlinear 7 x 5 square, two sensors, two Dirichlet actuators; the public level runs on the cylinder's O1 mesh.
tests/test_tangent_loop_host.py pins the model without a GPU.

Measured on the MI355X (DESIGN §5.6 "Closed loop"): against the model <= 1.4e-13; identity with the device adjoint 8.2e-16 / 2.9e-16
(linearised square) and 1.4e-16 / 2.8e-16 (nonlinear square); central differences <= 2.5e-8; Gauss-Newton product against the model
<= 2.2e-14, symmetry 1.6e-14; identity on O1 3.2e-16."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import flowcontrol_amd.utils as flu
from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import tangent_loop_model as tm
from tests.test_adjoint_loop_gpu import CAPACITY, TOL, forward, refused, slot_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
#: the bound of the dot-product identity between two device marches (tests/test_tangent_gpu.py's): a share of the summed absolute terms
IDENTITY = 1e-8
OUT = ("dy", "du", "xi", "dxn", "dxnm1")
LOOP_KEYS = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u")


@pytest.fixture(scope="module")
def plant():
    p = lc.DevicePlant(False)
    p.dev.tangent_reserve(1)
    yield p
    p.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    p.dev.adjoint_tape_reserve(CAPACITY)
    p.dev.tangent_reserve(1)
    yield p
    p.close()


def march(p, loop, d):
    """The device's closed-loop tangent over the tapes of the last ``forward(p, loop)`` along the groups of ``d`` that are set."""
    direction = {k: d[k] for k in LOOP_KEYS if d.get(k) is not None}
    return p.dev.run_tangent_closed_loop(slot_of(loop.first_order), loop.n, direction or None, d.get("dx0"), d.get("dxm1"))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in OUT)


def case_of(p, first_order, n, **kw):
    """(loop, model forward, model gradients, directions, w, r, z) of one case; state directions move velocity entries only."""
    loop, w, r, z = lc.make_case(p.model, p.x0, p.xm1, first_order, n, **kw)
    f = loop.forward()
    g = loop.adjoint(f, w, r, z)
    return loop, f, g, tm.directions(g, nn2=2 * p.th.nn), w, r, z


def against_model(p, loop, f, d, label):
    t, m = march(p, loop, d), tm.tangent(loop, f, d)
    errs = {k: lm.rel(t[k], m[k]) for k in OUT}
    print(f"{label}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    for k, v in errs.items():
        assert v <= TOL, f"{label}: {k}: {v:.3e} > {TOL:.1e}"
    return t


def main_cases(plant, nl_plant):
    return [(plant, c) for c in lc.MAIN_CASES] + [(nl_plant, c) for c in lc.NL_CASES]


def test_against_the_model(plant, nl_plant):
    """1. dy, du, xi_n, dx_n, dx_{n-1} within 1e-8 relative of the model on the main cases (linearised plant) and the nonlinear cases:
    all groups at once, then each group alone with the rest NULL; two marches are bit-identical; du is exactly 0 where the forward u
    sits at a limit and nowhere else."""
    for p, (first_order, n) in main_cases(plant, nl_plant):
        loop, f, g, d, *_ = case_of(p, first_order, n)
        label = f"{'nonlinear' if p.nonlinear else 'linearised'} plant, first order {first_order}, n = {n}"
        _, u = forward(p, loop)
        t = against_model(p, loop, f, d, label + ", all groups")
        assert same(t, march(p, loop, d)), "two identical marches differ"
        lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
        at_limit = (u == loop.lo) | (u == loop.hi)
        assert np.array_equal(t["du"] == 0.0, at_limit), (t["du"], at_limit)
        for grp in lm.GROUPS:
            against_model(p, loop, f, {grp: d[grp]}, f"{label}, {grp} alone")


@pytest.mark.parametrize("case", lc.SHAPE_CASES + lc.SHORT_CASES, ids=lc.case_id)
def test_shapes(plant, case):
    """2. Every branch of the kernel: nx = 0, 1, 13, 65 (partial second pass), 256; nyc 1, 2; nuc fanned out and per actuator; with and
    without signals and limits; n = 1, 2, 3 from both first orders."""
    loop, w, r, z = lc.make_case(plant.model, plant.x0, plant.xm1, **case)
    f = loop.forward()
    d = tm.directions(loop.adjoint(f, w, r, z), nn2=2 * plant.th.nn)
    forward(plant, loop)
    against_model(plant, loop, f, d, lc.case_id(case))


def test_identity_with_the_device_adjoint(plant, nl_plant):
    """3. sum w . dy + sum r . du + z . dx_n = sum_groups <g, d> between the device tangent and the device's run_adjoint_closed_loop on
    the SAME tapes: a defect of at most 1e-8 of the summed absolute terms, on both plants and the main cases."""
    for p, (first_order, n) in main_cases(plant, nl_plant):
        loop, f, _, d, w, r, z = case_of(p, first_order, n)
        forward(p, loop)
        t = march(p, loop, d)
        g = p.dev.run_adjoint_closed_loop(slot_of(first_order), n, w, r, z)
        lhs, rhs, scale = tm.identity_terms(t, g, d, w, r, z)
        defect = abs(lhs - rhs) / scale
        print(f"{'nonlinear' if p.nonlinear else 'linearised'} plant, first order {first_order}, n = {n}: tangent {lhs:.15e}, adjoint {rhs:.15e}, "
              f"identity defect {defect:.2e}", flush=True)
        assert defect <= IDENTITY


def test_central_differences_of_the_device_run(plant, nl_plant):
    """4. dy, du, xi_n and dx_n against central differences of the device's own closed-loop runs at ``FD_EPS``, all groups moved at
    once: within ``FD_TOL``."""
    for p, (first_order, n) in main_cases(plant, nl_plant):
        loop, f, _, d, *_ = case_of(p, first_order, n)
        forward(p, loop)
        t = march(p, loop, d)

        def run(sign):
            y, u = forward(p, tm.perturbed(loop, d, sign * lc.FD_EPS), tape=False)
            return {"dy": y, "du": u, "xi": p.dev.controller_state()[0], "dxn": p.dev.get_solution()}

        plus, minus = run(1.0), run(-1.0)
        errs = {k: lm.rel(t[k], (plus[k] - minus[k]) / (2 * lc.FD_EPS)) for k in plus}
        print(f"{'nonlinear' if p.nonlinear else 'linearised'} plant, first order {first_order}, n = {n}, central differences: "
              + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
        for k, v in errs.items():
            assert v <= lc.FD_TOL, (k, v)


def test_zero_controller_is_the_open_loop_march(nl_plant):
    """5. C = D = 0 without limits, direction w_u (and the two state levels): du is dw_u, and dy, dx_n, dx_{n-1} are fc_run_tangent's
    for du = dw_u on the same state tape, bit for bit."""
    p, n = nl_plant, 6
    loop, f, g, d, *_ = case_of(p, 1, n, nx=13, limits=False)
    loop.bank["C"][:] = 0.0
    loop.bank["D"][:] = 0.0
    forward(p, loop)
    t = march(p, loop, {k: d[k] for k in ("w_u", "dx0", "dxm1")})
    dy, dxn, dxnm1 = p.dev.run_tangent(SLOT_BDF1, n, d["w_u"], d["dx0"], d["dxm1"])
    assert np.array_equal(t["du"], d["w_u"])
    assert np.array_equal(t["dy"], dy) and np.array_equal(t["dxn"], dxn) and np.array_equal(t["dxnm1"], dxnm1)
    assert np.any(dy) and np.any(t["xi"])  # (dxi = Bd G dy: the controller's state still listens)


def test_the_march_leaves_the_handle_alone(nl_plant):
    """6. Flow state, controller state, loop cursor, loop-tape and state-tape info, step counter, a following run_adjoint_closed_loop
    and a following closed-loop step: the same bits with and without a march in between."""
    p, dev = nl_plant, nl_plant.dev
    loop, f, g, d, w, r, z = case_of(p, 1, 7)  # (seven rows of signals: six taped steps and the further one)
    w, r = w[:6], r[:6]
    direction = {k: (d[k][:6] if k in ("w_y", "w_u") else d[k]) for k in LOOP_KEYS}

    def observe(with_march):
        y, _ = forward(p, loop, cuts=(6,))
        # (counters and tape info across the march itself: the step counter runs on from test to test, and the loop tape's bytes hold
        # the adjoint's rows from the first backward march on)
        counted, info = np.array(dev.step_counts()), (dev.adjoint_loop_info(), dev.adjoint_tape_info())
        if with_march:
            assert np.any(dev.run_tangent_closed_loop(SLOT_BDF1, 6, direction, d["dx0"], d["dxm1"])["dy"])
        assert (dev.adjoint_loop_info(), dev.adjoint_tape_info()) == info and np.array_equal(dev.step_counts(), counted)
        seen = {"state": np.concatenate(dev.get_state()), "controller state": dev.controller_state(), "cursor": np.array(dev.loop_cursor())}
        grads = dev.run_adjoint_closed_loop(SLOT_BDF1, 6, w, r, z)
        seen.update({f"gradient {k}": v for k, v in grads.items()})
        y1, u1, _ = dev.run_closed_loop(SLOT_BDF2, 1, y[-1], compute_energy=False)
        seen.update({"y of a further step": y1, "u of a further step": u1, "its solution": dev.get_solution()})
        return seen

    before, after = observe(False), observe(True)
    for name in before:
        assert np.array_equal(before[name], after[name]), f"{name} differs after a closed-loop tangent march"


def test_refusals(nl_plant):
    """7. Every refusal returns its code and reason and the march counter does not move."""
    p, dev = nl_plant, nl_plant.dev
    loop, f, g, d, *_ = case_of(p, 1, 6)
    args = (SLOT_BDF1, 6, {"C": d["C"]})
    forward(p, loop)
    ref = dev.run_tangent_closed_loop(*args)
    marches = dev.tangent_info()["marches"]
    # the loop tape does not hold this run; a bad call
    refused(INV, dev.run_tangent_closed_loop, SLOT_BDF1, 5, match="holds 6 steps")
    refused(INV, dev.run_tangent_closed_loop, SLOT_BDF2, 6, match="first taped step")
    refused(INV, dev.run_tangent_closed_loop, SLOT_BDF1, 0, match="n_steps")
    dev.controller_state(loop.bank["x0"])
    refused(INV, dev.run_tangent_closed_loop, *args, match="fc_set_controller_state")
    dev.adjoint_loop_reserve(CAPACITY)
    refused(INV, dev.run_tangent_closed_loop, *args, match="not begun")
    dev.adjoint_loop_reserve(0)
    refused(NOT_READY, dev.run_tangent_closed_loop, *args, match="no loop tape")
    # the state tape of a nonlinear plant: another run, checkpointed, none
    forward(p, loop)
    dev.adjoint_tape_begin()
    refused(INV, dev.run_tangent_closed_loop, *args, match="state tape does not hold this run")
    dev.adjoint_tape_reserve_sparse(CAPACITY, 2)
    forward(p, loop)
    refused(INV, dev.run_tangent_closed_loop, *args, match="checkpointed")
    dev.adjoint_tape_reserve_sparse(0, 0)
    refused(INV, dev.run_tangent_closed_loop, *args, match="no tape is reserved")
    dev.adjoint_tape_reserve(CAPACITY)
    forward(p, loop)
    # a step in flight
    y, _ = forward(p, loop)
    dev.step_begin(SLOT_BDF2, np.zeros(dev.n_act))
    refused(INV, dev.run_tangent_closed_loop, *args, match="in flight")
    dev.step_end()
    # Crank-Nicolson, a Krylov method
    forward(p, loop)
    dev.set_rhs_operator(SLOT_BDF2, (0.5 * p.model.M)[:, : 2 * dev.nn])
    refused(INV, dev.run_tangent_closed_loop, *args, match="Crank-Nicolson")
    dev.set_rhs_operator(SLOT_BDF2, None)
    dev.set_solver_options(refine=30, method="gmres")
    try:
        refused(INV, dev.run_tangent_closed_loop, *args, match="Krylov")
    finally:
        dev.set_solver_options(refine=1, check_residual=1)
    # no tangent buffers; a batch
    dev.tangent_reserve(0)
    refused(NOT_READY, dev.run_tangent_closed_loop, *args, match="no tangent buffers")
    dev.tangent_reserve(1)
    assert dev.tangent_info()["marches"] == marches
    # ... and the handle still does what it did
    forward(p, loop)
    assert same(ref, dev.run_tangent_closed_loop(*args))
    assert dev.tangent_info()["marches"] == marches + 1


def test_partitioned_handles_are_refused():
    """7b. A handle with an exchange (fc_set_host_exchange, in a child process) is refused by both marches with FC_ERR_INVALID."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "tangent_loop_child.py"), "partitioned"], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, f"child: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK partitioned" in out.stdout


def test_gauss_newton_product_against_the_model(plant):
    """8. flu.closed_loop_gauss_newton_product on the linearised square with a Controller object, signals and limits that clamp part of
    the controls: against the model (tangent, then Loop.adjoint with w = dy Q_s, r = du R_s) within 1e-8; v . H v >= 0; v2 . H v =
    v . H v2 to 1e-10 in two random directions over the continuous A, B and C, D, x0."""
    from flowcontrol_amd.controller import Controller, pack_controllers

    p, dev, n, first_order = plant, plant.dev, 6, 1
    rng = np.random.default_rng(41)
    ns, na, dt = dev.n_sens, dev.n_act, plant.sq.dt
    A = rng.standard_normal((3, 3))
    A -= (max(np.linalg.eigvals(A).real) + 1.0) * np.eye(3)
    K = Controller(A, rng.standard_normal((3, 2)), rng.standard_normal((na, 3)), rng.standard_normal((na, 2)), x0=0.3 * rng.standard_normal(3))
    feedback = (rng.standard_normal((2, ns)), 0.1 * rng.standard_normal(2))
    w_y, w_u = 0.2 * rng.standard_normal((n, 2)), 0.2 * rng.standard_normal((n, na))
    Q, R = np.array([[2.5, 0.4], [0.0, 1.0]]), np.array([[0.3, 0.1], [0.0, 0.2]])
    Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    y0 = np.asarray(p.model.C @ p.x0).reshape(ns)
    loop = lm.Loop(p.model, pack_controllers([K], dt, ns, na, feedback), first_order, n, p.x0, p.xm1, y0, w_y, w_u)
    c = float(np.median(np.abs(loop.forward()["v"])))
    loop.lo, loop.hi = np.full(na, -c), np.full(na, c)
    f = loop.forward()
    lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
    names = ("A", "B", "C", "D", "x0")
    vs = [{k: rng.standard_normal(np.shape(m)) for k, m in zip(names, (K.A, K.B, K.C, K.D, K.x))} for _ in range(2)]

    def model_product(v):
        tA, tB = K.discrete_tangent(dt, v["A"], v["B"])
        t = tm.tangent(loop, f, {"Ad": tA, "Bd": tB, "C": v["C"], "D": v["D"], "x0": v["x0"]})
        gm = loop.adjoint(f, t["dy"] @ Qs, t["du"] @ Rs)
        gA, gB = K.discrete_gradient(dt, gm["Ad"], gm["Bd"])
        return {"A": gA, "B": gB, "C": gm["C"], "D": gm["D"], "x0": gm["x0"]}

    nn2 = 2 * p.th.nn
    dev.set_state(p.x0[:nn2], p.xm1[:nn2], p.x0[nn2:])
    state0 = np.concatenate(dev.get_state())
    try:
        with flu.AdjointRun(dev, loop=n) as adj:
            Hv = [flu.closed_loop_gauss_newton_product(dev, K, n, Q, R, v, feedback=feedback, w_y=w_y, w_u=w_u, u_limits=(loop.lo, loop.hi), adjoint=adj, dt=dt,
                                                       y0=y0, first_order=first_order) for v in vs]
        assert np.array_equal(state0, np.concatenate(dev.get_state()))
    finally:
        for s in SLOTS:
            dev.set_adjoint_factors(s, 1)
    dot = lambda a, b: float(sum(np.sum(a[k] * b[k]) for k in names))  # noqa: E731
    Hm = model_product(vs[0])
    errs = {k: lm.rel(Hv[0][k], Hm[k]) for k in names}
    sym = abs(dot(vs[1], Hv[0]) - dot(vs[0], Hv[1])) / abs(dot(vs[1], Hv[0]))
    print("closed_loop_gauss_newton_product on the square: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f", v.Hv = {dot(vs[0], Hv[0]):.6e}, symmetry defect {sym:.2e}", flush=True)
    assert all(v <= TOL for v in errs.values()), errs
    assert dot(vs[0], Hv[0]) >= 0.0 and dot(vs[1], Hv[1]) >= 0.0 and sym <= 1e-10


def test_public_functions_on_the_cylinder(golden_dir):
    """9. flu.closed_loop_tangent on the nonlinear cylinder (O1) with the shipped 13-state controller, 10 steps, limits that clamp part
    of the controls, along a random direction over the continuous A, B, C, D and x0: the identity
    sum (y Q_s) . dy + sum (u R_s) . du = sum <grads, direction> with flu.closed_loop_gradient within 1e-8 of the summed absolute terms.
    The state is left where it was; tapes and buffers are released."""
    import flowcontrol_amd
    from flowcontrol_amd.controller import Controller
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.params_solver.is_eq_nonlinear = True
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    K = Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat")
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        n = 10
        rng = np.random.default_rng(37)
        K.x = 0.1 * rng.standard_normal(K.nstates)
        xc0 = K.x.copy()
        Q, R = np.diag(1.0 + np.arange(dev.n_sens)), 0.1 * np.eye(dev.n_act)
        Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        names = ("A", "B", "C", "D", "x0")
        d = {k: rng.standard_normal(np.shape(m)) * max(np.abs(m).max(), 1e-3) for k, m in zip(names, (K.A, K.B, K.C, K.D, K.x))}
        free = flu.closed_loop_tangent(fs, K, n, d)
        c = float(np.median(np.abs(free["u"])))
        limits = (-c, c)
        t = fs.closed_loop_tangent(K, n, d, u_limits=limits)
        assert all(np.array_equal(t[k], v) for k, v in flu.closed_loop_tangent(fs, K, n, d, u_limits=limits).items())
        at_limit = np.abs(t["u"]) == c
        assert np.any(at_limit) and not np.all(at_limit) and np.array_equal(t["du"] == 0.0, at_limit)
        assert lm.rel(t["dy"], free["dy"]) > 1e-3, "the limits do not act on the tangent"
        J, g = flu.closed_loop_gradient(fs, K, n, Q, R, u_limits=limits)
        left = [np.sum((t["y"] @ Qs) * t["dy"]), np.sum((t["u"] @ Rs) * t["du"])]
        right = [np.sum(g[k] * d[k]) for k in names]
        defect = abs(sum(left) - sum(right)) / (sum(abs(x) for x in left) + sum(abs(x) for x in right))
        print(f"O1 nonlinear, 10 steps, {int(at_limit.sum())} of {at_limit.size} controls clamped: J = {J:.6e}, tangent {sum(left):.15e}, "
              f"adjoint {sum(right):.15e}, identity defect {defect:.2e}", flush=True)
        assert defect <= IDENTITY
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state())) and np.array_equal(K.x, xc0)
        assert dev.adjoint_loop_info()["bytes"] == 0 and dev.adjoint_tape_info()["bytes"] == 0
        assert not dev.tangent_info()["reserved"] and dev.tangent_info()["bytes"] == 0
    finally:
        fs.th.release_device()
