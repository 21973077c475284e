"""The tangent of the energy in the closed-loop tangent marches on the MI355X (``fc_tangent_set_energy`` with
``fc_run_tangent_closed_loop`` / ``_batch``), the device tangent against the device adjoint with energy weights on the same tapes, and
``flu.closed_loop_gauss_newton_product(energy=)`` against the model of tests/support/tangent_energy_cases.py.

The problems are those of tests/test_tangent_loop_gpu.py: the linearised 8 x 8 square and the nonlinear 7 x 5 square, two sensors, two
Dirichlet actuators, limits that clamp part of the controls.  With the option a linearised march reads the dense state tape too."""
import numpy as np
import pytest

import flowcontrol_amd.utils as flu
from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from tests.support import adjoint_energy_cases as ec
from tests.support import adjoint_loop_batch_cases as lbc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import tangent_energy_cases as te
from tests.support import tangent_loop_model as tm
from tests.support import adjoint_batch_cases as bc
from tests.test_adjoint_loop_batch_gpu import main_columns, use_batch
from tests.test_adjoint_loop_gpu import CAPACITY, TOL, refused, slot_of
from tests.test_tangent_loop_gpu import IDENTITY, LOOP_KEYS, case_of, march

pytestmark = pytest.mark.gpu

SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY


@pytest.fixture(scope="module")
def plant():
    p = lc.DevicePlant(False)
    p.dev.adjoint_tape_reserve(CAPACITY)
    p.dev.tangent_reserve(1)
    p.dev.tangent_set_energy(1)
    yield p
    p.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    p.dev.adjoint_tape_reserve(CAPACITY)
    p.dev.tangent_reserve(1)
    p.dev.tangent_set_energy(1)
    yield p
    p.close()


def forward(p, loop, tape=True, energy=False):
    """The device closed-loop run of ``loop`` from its own initial state, onto the loop tape AND the state tape (both plants):
    (y, u, dE)."""
    dev, nn2 = p.dev, 2 * p.th.nn
    dev.set_state(loop.x0[:nn2], loop.xm1[:nn2], loop.x0[nn2:])
    lc.put_loop(dev, loop)
    if tape:
        if dev.adjoint_loop_info()["capacity"] != CAPACITY:
            dev.adjoint_loop_reserve(CAPACITY)
        dev.adjoint_tape_begin()
        dev.adjoint_loop_begin()
    return dev.run_closed_loop(slot_of(loop.first_order), loop.n, loop.y0, compute_energy=energy)


def cases(plant, nl_plant):
    return [(plant, "lin", c) for c in lc.MAIN_CASES] + [(nl_plant, "nl", c) for c in lc.NL_CASES]


def test_against_the_model_and_central_differences(plant, nl_plant):
    """1. dde of a clamped loop within 1e-8 of the model on both plants, all groups moved at once; two marches bit-identical; dy, du,
    dx_n are the bits of the march without the option; against central differences of the device's own dE series at FD_EPS within the
    bound of tangent_energy_cases.fd_tol."""
    for p, kind, (first_order, n) in cases(plant, nl_plant):
        dev = p.dev
        loop, f, g, d, *_ = case_of(p, first_order, n)
        lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
        forward(p, loop)
        t = march(p, loop, d)
        dde = dev.tangent_energy()
        t2 = march(p, loop, d)
        assert np.array_equal(dde, dev.tangent_energy()) and all(np.array_equal(t[k], t2[k]) for k in t)
        info = dev.tangent_energy_info()
        assert info["have"] and info["kernel"] == 1 and info["steps"] == n and info["launches"] == n and info["grid"] == -(-p.th.mesh.cells.shape[0] // 32)
        dev.tangent_set_energy(0)
        off = march(p, loop, d)
        dev.tangent_set_energy(1)
        assert all(np.array_equal(t[k], off[k]) for k in t)
        err = lm.rel(dde, te.loop_dde(loop, f, tm.tangent(loop, f, d)))

        def series(sign):
            return forward(p, tm.perturbed(loop, d, sign * lc.FD_EPS), tape=False, energy=True)[2]

        fd = lm.rel(dde, (series(1.0) - series(-1.0)) / (2 * lc.FD_EPS))
        print(f"closed-loop tangent energy, {kind} plant, first order {first_order}, n = {n}: against the model {err:.3e}, device central difference {fd:.3e}")
        assert err <= TOL and fd <= te.fd_tol(kind, "loop")


def test_identity_with_the_device_adjoint(plant, nl_plant):
    """3. sum e_m dde_m + sum w . dy + sum r . du + z . dx_n = sum_groups <g, d> between the device tangent and the device's
    run_adjoint_closed_loop with set_adjoint_energy(e) on the SAME tapes: a defect of at most 1e-8 of the summed absolute terms, with
    part of the controls clamped -- fc_adj_elem_en (linearised) and fc_adj_elem_nl<EN> (nonlinear) without numpy in between."""
    for p, kind, (first_order, n) in cases(plant, nl_plant):
        dev = p.dev
        loop, f, _, d, w, r, z = case_of(p, first_order, n)
        e = ec.weights(n)
        forward(p, loop)
        t = march(p, loop, d)
        dde = dev.tangent_energy()
        dev.set_adjoint_energy(e)
        try:
            g = dev.run_adjoint_closed_loop(slot_of(first_order), n, w, r, z)
            code = int(dev.adjoint_route()[0])
        finally:
            dev.set_adjoint_energy(None)
        assert code == (ec.ELEM_EN if kind == "lin" else ec.ELEM_NL_EN)
        lhs, rhs, scale = tm.identity_terms(t, g, d, w, r, z)
        en = float(np.sum(e * dde))
        defect = abs(lhs + en - rhs) / (scale + abs(en))
        print(f"closed loop, {kind} plant, first order {first_order}, n = {n}: energy term {en:.6e} of {scale + abs(en):.6e}, identity defect {defect:.2e}")
        assert abs(en) > 1e-6 * scale, "the energy term does not act"
        assert defect <= IDENTITY


def test_linearised_march_needs_the_state_tape(plant):
    """7. A linearised closed-loop march with the option and no state tape that holds the run is refused before anything is enqueued;
    without the option the same march runs on the loop tape alone."""
    dev = plant.dev
    loop, f, g, d, *_ = case_of(plant, 1, 12)
    forward(plant, loop)
    marches = dev.tangent_info()["marches"]
    dev.adjoint_tape_reserve(0)
    try:
        refused(INV, dev.run_tangent_closed_loop, SLOT_BDF1, 12, {"C": d["C"]}, match="no tape is reserved")
        dev.adjoint_tape_reserve(CAPACITY)
        refused(INV, dev.run_tangent_closed_loop, SLOT_BDF1, 12, {"C": d["C"]}, match="state tape does not hold this run")
        assert dev.tangent_info()["marches"] == marches
        dev.tangent_set_energy(0)
        dev.run_tangent_closed_loop(SLOT_BDF1, 12, {"C": d["C"]})
        assert dev.tangent_info()["marches"] == marches + 1
    finally:
        dev.tangent_set_energy(1)


@pytest.mark.parametrize("kind", ["lin", "nl"])
def test_batched_columns_against_the_model(plant, nl_plant, kind):
    """4. k = 3 closed loops in lock step (KB = 4: a padding column), every column with its own state, bank, signals and limits: dde of
    every column within 1e-8 of that column's model, about its own loop and about loop 1; two marches bit-identical.  The linearised
    plant tapes its batched states for the option."""
    p = plant if kind == "lin" else nl_plant
    dev, k, first_order, n = p.dev, 3, 2, 3
    use_batch(p, k)
    try:
        if kind == "lin":
            dev.adjoint_tape_reserve_batch(CAPACITY)
        dev.tangent_reserve(1)
        dev.tangent_set_energy(1)
        cols = main_columns(p, k, first_order, n)
        loops = [c[0] for c in cols]
        fs = [q.forward() for q in loops]
        ds = [tm.directions(q.adjoint(f, w, r, z), seed=5 + s, nn2=2 * p.th.nn) for s, ((q, w, r, z), f) in enumerate(zip(cols, fs))]
        lbc.put_loops(dev, loops, 2 * p.th.nn)
        dev.adjoint_loop_reserve_batch(CAPACITY)
        dev.adjoint_tape_begin_batch()
        dev.adjoint_loop_begin_batch()
        bad = dev.run_closed_loop_batch(slot_of(first_order), n, np.array([q.y0 for q in loops]), compute_energy=False)[3]
        assert np.all(bad == -1)
        by_step = ("w_y", "w_u")
        direction = {key: np.stack([d[key] for d in ds], axis=1 if key in by_step else 0) for key in LOOP_KEYS}
        args = (slot_of(first_order), n, direction, np.array([d["dx0"] for d in ds]), np.array([d["dxm1"] for d in ds]))
        dev.run_tangent_closed_loop_batch(*args)
        dde = dev.tangent_energy()
        dev.run_tangent_closed_loop_batch(*args)
        assert dde.shape == (n, k) and np.array_equal(dde, dev.tangent_energy()) and dev.tangent_energy_info()["kernel"] == 2
        dev.run_tangent_closed_loop_batch(*args, ref_col=1)
        shared = dev.tangent_energy()
        assert dev.tangent_energy_info()["kernel"] == 3
        for s in range(k):
            own = lm.rel(dde[:, s], te.loop_dde(loops[s], fs[s], tm.tangent(loops[s], fs[s], ds[s])))
            about = lm.rel(shared[:, s], te.loop_dde(loops[1], fs[1], tm.tangent(loops[1], fs[1], ds[s])))
            print(f"batched closed-loop tangent energy, {kind} plant, column {s}: own loop {own:.3e}, about loop 1 {about:.3e}")
            assert own <= TOL and about <= TOL
    finally:
        dev.tangent_reserve(0)
        dev.adjoint_loop_reserve_batch(0)
        dev.set_controllers(None, p.sq.dt)
        bc.batch_off(p.sq)
        for s in SLOTS:
            dev.set_adjoint_factors(s, 1)
        dev.adjoint_tape_reserve(CAPACITY)
        dev.tangent_reserve(1)
        dev.tangent_set_energy(1)


@pytest.mark.parametrize("kind", ["lin", "nl"])
def test_gauss_newton_product_with_energy(plant, nl_plant, kind):
    """6. flu.closed_loop_gauss_newton_product(energy=e) with a Controller object, signals and limits that clamp part of the controls:
    against the model (tangent that keeps dX, then the adjoint forced with e_m M_s dx_m, w = dy Q_s, r = du R_s) within 1e-8; symmetric
    to 1e-10 in two random directions and v . H v >= 0 for e >= 0; energy=None is the call without the keyword bit for bit; with
    Q = R = 0 and e = (0, .., 0, 1), v . H v = dx_n^T M_s dx_n of the returned dx_n (the row indexing); rows, source, tapes and state
    are what they were."""
    from flowcontrol_amd.controller import Controller, pack_controllers

    p = plant if kind == "lin" else nl_plant
    dev, n, first_order = p.dev, 6, 1
    rng = np.random.default_rng(41)
    ns, na, dt = dev.n_sens, dev.n_act, p.sq.dt
    A = rng.standard_normal((3, 3))
    A -= (max(np.linalg.eigvals(A).real) + 1.0) * np.eye(3)
    K = Controller(A, rng.standard_normal((3, 2)), rng.standard_normal((na, 3)), rng.standard_normal((na, 2)), x0=0.3 * rng.standard_normal(3))
    feedback = (rng.standard_normal((2, ns)), 0.1 * rng.standard_normal(2))
    w_y, w_u = 0.2 * rng.standard_normal((n, 2)), 0.2 * rng.standard_normal((n, na))
    Q, R = np.array([[2.5, 0.4], [0.0, 1.0]]), np.array([[0.3, 0.1], [0.0, 0.2]])
    Qs, Rs = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    e = 40.0 * (0.5 + rng.random(n))
    y0 = np.asarray(p.model.C @ p.x0).reshape(ns)
    loop = lm.Loop(p.model, pack_controllers([K], dt, ns, na, feedback), first_order, n, p.x0, p.xm1, y0, w_y, w_u)
    c = float(np.median(np.abs(loop.forward()["v"])))
    loop.lo, loop.hi = np.full(na, -c), np.full(na, c)
    f = loop.forward()
    lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
    names = ("A", "B", "C", "D", "x0")
    vs = [{k: rng.standard_normal(np.shape(m)) for k, m in zip(names, (K.A, K.B, K.C, K.D, K.x))} for _ in range(2)]

    def model_product(v, Qm, Rm, em):
        tA, tB = K.discrete_tangent(dt, v["A"], v["B"])
        t = tm.tangent(loop, f, {"Ad": tA, "Bd": tB, "C": v["C"], "D": v["D"], "x0": v["x0"]})
        gm = te.ForcedLoop.of(loop, em, t["dX"]).adjoint(f, t["dy"] @ Qm, t["du"] @ Rm)
        gA, gB = K.discrete_gradient(dt, gm["Ad"], gm["Bd"])
        return {"A": gA, "B": gB, "C": gm["C"], "D": gm["D"], "x0": gm["x0"]}, t

    nn2 = 2 * p.th.nn
    dev.tangent_reserve(0)  # (the functions reserve what they need and free it)
    dev.adjoint_tape_reserve(0)
    dev.set_state(p.x0[:nn2], p.xm1[:nn2], p.x0[nn2:])
    state0 = np.concatenate(dev.get_state())
    kw = dict(feedback=feedback, w_y=w_y, w_u=w_u, u_limits=(loop.lo, loop.hi), dt=dt, y0=y0, first_order=first_order)
    last = np.zeros(n)
    last[-1] = 1.0
    try:
        with flu.AdjointRun(dev, loop=n, tape=n) as adj:
            Hv = [flu.closed_loop_gauss_newton_product(dev, K, n, Q, R, v, adjoint=adj, energy=e, **kw) for v in vs]
            plain = flu.closed_loop_gauss_newton_product(dev, K, n, Q, R, vs[0], adjoint=adj, **kw)
            none = flu.closed_loop_gauss_newton_product(dev, K, n, Q, R, vs[0], adjoint=adj, energy=None, **kw)
            pin = flu.closed_loop_gauss_newton_product(dev, K, n, 0 * Q, 0 * R, vs[0], adjoint=adj, energy=last, **kw)
            dxn = flu.closed_loop_tangent(dev, K, n, vs[0], adjoint=adj, **kw)["dxn"]
            assert dev.adjoint_energy_info()["n_steps"] == 0 and dev.adjoint_energy_source() == 0
            assert dev.tangent_tape_info() == {"capacity": 0, "count": 0, "first_slot": -1, "bytes": 0} and dev.tangent_info()["bytes"] == 0
        assert np.array_equal(state0, np.concatenate(dev.get_state()))
    finally:
        for s in SLOTS:
            dev.set_adjoint_factors(s, 1)
        dev.adjoint_tape_reserve(CAPACITY)
        dev.tangent_reserve(1)
        dev.tangent_set_energy(1)
    dot = lambda a, b: float(sum(np.sum(a[k] * b[k]) for k in names))  # noqa: E731
    Hm, _ = model_product(vs[0], Qs, Rs, e)
    H0, _ = model_product(vs[0], Qs, Rs, 0 * e)
    errs = {k: lm.rel(Hv[0][k], Hm[k]) for k in names}
    sym = abs(dot(vs[1], Hv[0]) - dot(vs[0], Hv[1])) / abs(dot(vs[1], Hv[0]))
    share = abs(dot(vs[0], Hm) - dot(vs[0], H0)) / abs(dot(vs[0], Hm))
    Ms = ec.msym(p.model.M)
    pinned = dot(vs[0], pin)
    want = float(dxn @ (Ms @ dxn))
    print(f"closed_loop_gauss_newton_product(energy=), {kind} plant: against the model " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f"; v.Hv = {dot(vs[0], Hv[0]):.6e} (energy share {share:.2e}), symmetry defect {sym:.2e}; e = (0,..,1): v.Hv = {pinned:.12e}, "
          f"dx_n.M dx_n = {want:.12e}")
    assert all(np.array_equal(plain[k], none[k]) for k in names)
    assert share > 1e-3, "the energy term does not act on the product"
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    assert sym <= 1e-10 and dot(vs[0], Hv[0]) >= 0.0
    assert abs(pinned - want) <= 1e-8 * abs(want)


# ── the public drivers with energy=True on the solver objects ────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("kind", ["lin", "nl"])
def test_energy_keyword_on_the_solvers(kind):
    """flu.closed_loop_tangent / FlowSolver.closed_loop_tangent (a FlowSolver that has stepped), flu.batched_tangent_run (nonlinear) and
    flu.batched_closed_loop_tangent (a BatchedFlowSolver of k = 3 that has stepped) with energy=True on the 9 x 9 cavity: `dde` has
    the shape (n,) / (n, k) and equals, bit for bit, the rows of the device-level march the test makes itself with the same calls (the
    marches this file and tests/test_tangent_energy_gpu.py hold against the model); the other results are the bits of the call
    without the keyword; afterwards the state is where it was, no tape, no tangent buffers and no option are left.  On the linearised
    solver the run is taped for the energy alone."""
    from flowcontrol_amd.adjoint import forward_steps_batch
    from flowcontrol_amd.batch import BatchedFlowSolver
    from flowcontrol_amd.flowsolverparameters import ParamIC
    from tests.support.adjoint_energy_child import copies, same, small_controllers, square_flowsolver

    nl, n, k = kind == "nl", 5, 3
    rng = np.random.default_rng(12)

    def clean(dev, batched):
        info = dev.adjoint_tape_info_batch() if batched else dev.adjoint_tape_info()
        loop = dev.adjoint_loop_info_batch() if batched else dev.adjoint_loop_info()
        assert info["bytes"] == 0 and loop["capacity"] == 0 and dev.tangent_info()["bytes"] == 0 and not dev.tangent_energy_info()["on"]

    # one run
    fs = square_flowsolver(9, 9, nonlinear=nl)
    try:
        fs.initialize_time_stepping(ic=None)
        na = fs.params_control.actuator_number
        for j in range(2):
            fs.step(0.05 * (j + 1) * np.ones(na))
        fs._begin_stepping()
        dev, dt = fs.th.device(), fs.params_time.dt
        slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2
        K = small_controllers(1)[0]
        direction = {"C": rng.standard_normal(K.C.shape), "D": rng.standard_normal(K.D.shape), "x0": rng.standard_normal(K.x.shape)}
        state0, y0 = copies(dev.get_state()), np.array(fs.y_meas, dtype=float).reshape(dev.n_sens)
        t = flu.closed_loop_tangent(fs, K, n, direction, energy=True)
        assert same(state0, dev.get_state())
        clean(dev, False)
        tm_ = fs.closed_loop_tangent(K, n, direction, energy=True)
        plain = flu.closed_loop_tangent(fs, K, n, direction)
        assert t["dde"].shape == (n,) and np.any(t["dde"]) and "dde" not in plain
        assert all(np.array_equal(t[q], tm_[q]) for q in t) and all(np.array_equal(t[q], plain[q]) for q in plain)
        # the same calls at the device level
        dev.adjoint_tape_reserve(n)
        dev.set_controllers([K], dt)
        dev.tangent_reserve(1)
        dev.tangent_set_energy(1)
        dev.adjoint_loop_reserve(n)
        dev.adjoint_tape_begin()
        dev.adjoint_loop_begin()
        dev.run_closed_loop(slot, n, y0, compute_energy=False)
        ref = dev.run_tangent_closed_loop(slot, n, direction)
        dde = dev.tangent_energy()
        dev.tangent_reserve(0)
        dev.set_state(*state0)
        dev.set_controllers(None, dt)
        dev.adjoint_tape_reserve(0)
        assert np.array_equal(t["dde"], dde) and np.array_equal(t["dy"], ref["dy"]) and np.array_equal(t["dxn"], ref["dxn"])
        print(f"{kind} FlowSolver: closed_loop_tangent(energy=True) dde = {t['dde'].tolist()}")
    finally:
        fs.th.release_device()
    # k runs
    fs = square_flowsolver(9, 9, nonlinear=nl)
    try:
        bfs = BatchedFlowSolver(fs, k)
        bfs.initialize_time_stepping(ics=[ParamIC(xloc=0.4 + 0.1 * s, yloc=0.5, radius=0.2, amplitude=1.0 - 0.1 * s) for s in range(k)])
        na = fs.params_control.actuator_number
        bfs.step(0.05 * np.ones((k, na)))
        dev, dt = bfs.dev, fs.params_time.dt
        slot, order = (SLOT_BDF1, 1) if bfs.order == 1 else (SLOT_BDF2, 2)
        state0 = copies(dev.get_state_batch())
        Ks = small_controllers(k)
        dirs = [{"C": rng.standard_normal(Ks[s].C.shape), "D": rng.standard_normal(Ks[s].D.shape)} for s in range(k)]
        y0 = np.asarray(bfs.y_meas, dtype=float).reshape(k, dev.n_sens)
        tb = flu.batched_closed_loop_tangent(bfs, Ks, n, dirs, energy=True)
        assert same(state0, dev.get_state_batch())
        clean(dev, True)
        plain = flu.batched_closed_loop_tangent(bfs, Ks, n, dirs)
        assert tb["dde"].shape == (n, k) and np.all(np.any(tb["dde"], axis=0)) and "dde" not in plain
        assert all(np.array_equal(tb[q], plain[q]) for q in plain)
        dev.adjoint_tape_reserve_batch(n)
        dev.set_controllers(Ks, dt)
        dev.tangent_reserve(1)
        dev.tangent_set_energy(1)
        dev.adjoint_loop_reserve_batch(n)
        dev.adjoint_tape_begin_batch()
        dev.adjoint_loop_begin_batch()
        dev.run_closed_loop_batch(slot, n, y0, compute_energy=False)
        ref = dev.run_tangent_closed_loop_batch(slot, n, {q: np.stack([d[q] for d in dirs]) for q in ("C", "D")})
        dde = dev.tangent_energy()
        dev.tangent_reserve(0)
        dev.set_state_batch(*state0)
        dev.set_controllers(None, dt)
        dev.adjoint_tape_reserve_batch(0)
        assert np.array_equal(tb["dde"], dde) and np.array_equal(tb["dy"], ref["dy"])
        if nl:  # (the open-loop march of a linearised solver is refused: its forward run is its own tangent)
            u, du = 0.1 * rng.standard_normal((n, k, na)), rng.standard_normal((n, k, na))
            d0 = rng.standard_normal((k, dev.N))
            out = flu.batched_tangent_run(bfs, u, du, d0, None, energy=True)
            assert same(state0, dev.get_state_batch())
            clean(dev, True)
            plain = flu.batched_tangent_run(bfs, u, du, d0, None)
            assert len(out) == 4 and len(plain) == 3 and out[3].shape == (n, k) and all(np.array_equal(a, b) for a, b in zip(out, plain))
            dev.adjoint_tape_reserve_batch(n)
            dev.tangent_reserve(1)
            dev.tangent_set_energy(1)
            dev.adjoint_tape_begin_batch()
            forward_steps_batch(dev, k, u, order)
            ref = dev.run_tangent_batch(slot, n, du, d0, None)
            dde = dev.tangent_energy()
            dev.tangent_reserve(0)
            dev.set_state_batch(*state0)
            dev.adjoint_tape_reserve_batch(0)
            assert np.array_equal(out[3], dde) and np.array_equal(out[0], ref[0])
        else:
            with pytest.raises(ValueError, match="its own tangent"):
                flu.batched_tangent_run(bfs, np.zeros((n, k, na)), energy=True)
        print(f"{kind} BatchedFlowSolver: batched_closed_loop_tangent(energy=True) dde[-1] = {tb['dde'][-1].tolist()}")
    finally:
        fs.th.release_device()
