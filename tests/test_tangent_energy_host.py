"""The tangent of the energy and the Gauss-Newton product of the energy cost on the host: the models of
tests/support/tangent_energy_cases.py against central differences of their own energy series, the dot-product identity with the energy
adjoint, the model's H_E assembled column by column, the two mistakes of DESIGN section 5.4, and the drivers of
flowcontrol_amd/tangent.py on a recording device (call order and every exit path).  No GPU."""
import numpy as np
import pytest

from flowcontrol_amd import tangent as tan_mod
from flowcontrol_amd._lib import SLOT_BDF2
from flowcontrol_amd.adjoint import AdjointRun
from flowcontrol_amd.controller import Controller
from tests.support import adjoint_energy_cases as ec
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_nl_model as nm
from tests.support import tangent_energy_cases as te
from tests.support import tangent_loop_model as tlm
from tests.support.recording_device import Marker, RecordingDevice, fake_batched, fake_flowsolver, filled

ORDERS_N = [(fo, n) for fo in (1, 2) for n in (1, 2, 5)]


def nn2_of(model):
    """Velocity dofs of a plant model: the rows of its mass matrix that hold entries."""
    return int(np.count_nonzero(np.diff(model.M.tocsr().indptr)))


@pytest.fixture(scope="module")
def nl_square():
    model, th, (u_n, u_nn, p) = nm.host_square()
    return ec.with_energy(model), np.r_[u_n, p], np.r_[u_nn, p], 2 * th.nn


@pytest.fixture(scope="module")
def plants():
    return {kind: lc.host_plant(kind == "nl") for kind in ("lin", "nl")}


def open_case(sq, first_order, n, seed=9):
    model, x0, xm1, nn2 = sq
    rng = np.random.default_rng(seed)
    u, du = rng.standard_normal((n, model.n_act)), rng.standard_normal((n, model.n_act))
    d0, dm1 = np.zeros(model.N), np.zeros(model.N)
    d0[:nn2], dm1[:nn2] = rng.standard_normal(nn2), rng.standard_normal(nn2)
    return u, du, d0, dm1


def loop_case(plants, kind, first_order, n):
    model, x0, xm1 = plants[kind]
    loop, w, r, z = lc.make_case(model, x0, xm1, first_order, n, limits=n > 1, seed=11 + n)
    f = loop.forward()
    if n > 1:
        lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
    d = tlm.directions(loop.adjoint(f, w, r, z), seed=5, nn2=nn2_of(model))
    return loop, f, d, w, r, z


def measured_fd_distance(kind, march, first_order, n, sq, plants):
    if march == "open":
        model, x0, xm1, _ = sq
        u, du, d0, dm1 = open_case(sq, first_order, n)
        X, _ = model.forward(first_order, u, x0, xm1)
        dde = te.TangentEnergyModel(model).tangent_energy(first_order, X, du, d0, dm1)[2]
        series = lambda s: te.energy_series(model.M, model.forward(first_order, u + s * te.EPS * du, x0 + s * te.EPS * d0, xm1 + s * te.EPS * dm1)[0])  # noqa: E731
        return nm.rel(dde, (series(1.0) - series(-1.0)) / (2 * te.EPS))
    loop, f, d, *_ = loop_case(plants, kind, first_order, n)
    dde = te.loop_dde(loop, f, tlm.tangent(loop, f, d))
    fd = (te.loop_energy(tlm.perturbed(loop, d, lc.FD_EPS)) - te.loop_energy(tlm.perturbed(loop, d, -lc.FD_EPS))) / (2 * lc.FD_EPS)
    return lm.rel(dde, fd)


@pytest.mark.parametrize("kind,march", sorted(te.HOST_FD_DISTANCE))
def test_model_dde_matches_central_differences(kind, march, nl_square, plants):
    """dde against central differences of the model's own energy series, first order 1 / 2, n = 1 / 2 / 5: the constant of
    tangent_energy_cases.HOST_FD_DISTANCE bounds what the six cases measure and exceeds it by less than a factor of two."""
    worst = {}
    for first_order, n in ORDERS_N:
        worst[first_order, n] = measured_fd_distance(kind, march, first_order, n, nl_square, plants)
    top = max(worst.values())
    print(f"{kind} {march}: largest distance {top:.3e} at {max(worst, key=worst.get)}; " + ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))
    bound = te.HOST_FD_DISTANCE[kind, march]
    assert top <= bound < 2 * top, (top, bound)
    assert te.fd_tol(kind, march) == (te.TOL_FD if bound < 0.1 * te.TOL_FD else 16 * bound)


@pytest.mark.parametrize("first_order,n", ORDERS_N)
def test_dot_product_identity_open_loop(nl_square, first_order, n):
    """sum e_m dde_m + sum w . dy + z . dx_n = <g, du> + <g_x0, dx_0> + <g_xm1, dx_{-1}> with g from the energy adjoint."""
    model, x0, xm1, _ = nl_square
    u, du, d0, dm1 = open_case(nl_square, first_order, n)
    rng = np.random.default_rng(3)
    w, z, e = rng.standard_normal((n, model.C.shape[0])), rng.standard_normal(model.N), ec.weights(n)
    X, _ = model.forward(first_order, u, x0, xm1)
    D, dy, dde = te.TangentEnergyModel(model).tangent_energy(first_order, X, du, d0, dm1)
    g, gx0, gxm1, _ = model.adjoint_energy(first_order, X, w, z, e)
    terms = [np.sum(e * dde), np.sum(w * dy), z @ D[-1], -np.sum(g * du), -(gx0 @ d0), -(gxm1 @ dm1)]
    assert abs(sum(terms)) <= 1e-12 * sum(abs(t) for t in terms)
    assert abs(np.sum(e * dde)) > 1e-3 * sum(abs(t) for t in terms), "the energy term does not act"


@pytest.mark.parametrize("kind", ["lin", "nl"])
@pytest.mark.parametrize("first_order,n", [(1, 5), (2, 2), (2, 1)])
def test_dot_product_identity_closed_loop(plants, kind, first_order, n):
    loop, f, d, w, r, z = loop_case(plants, kind, first_order, n)
    e = ec.weights(n)
    t = tlm.tangent(loop, f, d)
    dde = te.loop_dde(loop, f, t)
    g = ec.EnergyLoop.of(loop, e).adjoint(f, w, r, z)
    lhs, rhs, scale = tlm.identity_terms(t, g, d, w, r, z)
    lhs += float(np.sum(e * dde))
    assert abs(lhs - rhs) <= 1e-11 * (scale + abs(np.sum(e * dde)))


def test_energy_product_matrix_on_the_small_square():
    """The model's H_E on the 5 x 3 square at n = 2, assembled from the tangents of all unit directions: symmetric, eigenvalues >=
    -round-off for e >= 0, and equal to the product routine column by column."""
    model, th, (u_n, u_nn, p) = nm.host_square(5, 3)
    model = ec.with_energy(model)
    tm = te.TangentEnergyModel(model)
    n, na = 2, model.n_act
    u = np.random.default_rng(1).standard_normal((n, na))
    X, _ = model.forward(2, u, np.r_[u_n, p], np.r_[u_nn, p])
    e = np.array([0.7, 1.9])
    Ms = ec.msym(model.M)
    units = np.eye(n * na).reshape(n * na, n, na)
    Ds = [tm.tangent(2, X, v)[0] for v in units]
    H = np.array([[sum(e[m - 1] * (Di[m + 1] @ (Ms @ Dj[m + 1])) for m in range(1, n + 1)) for Dj in Ds] for Di in Ds])
    scale = np.abs(H).max()
    assert scale > 0 and np.abs(H - H.T).max() <= 1e-14 * scale
    assert np.linalg.eigvalsh(0.5 * (H + H.T)).min() >= -1e-13 * scale
    for j, v in enumerate(units):
        col = tm.energy_product(2, X, e, v).reshape(-1)
        assert np.abs(col - H[:, j]).max() <= 1e-11 * scale, j
    # the same routine with F = X is the gradient of sum e_m dE_m (the two sources of the device's forcing differ in F only)
    g = te.energy_adjoint_of(model, 2, X, X, e)[0]
    assert np.array_equal(g, model.adjoint_energy(2, X, np.zeros((n, model.C.shape[0])), None, e)[0])


def test_the_two_mistakes_are_told_apart(nl_square, plants):
    """Masking x_m, or masking the tangent state, moves dde by orders of magnitude more than the device tolerance (1e-8)."""
    model, x0, xm1, _ = nl_square
    u, du, d0, dm1 = open_case(nl_square, 2, 3)
    X, _ = model.forward(2, u, x0, xm1)
    tm = te.TangentEnergyModel(model)
    right = tm.tangent_energy(2, X, du, d0, dm1)[2]
    for wrong in ("x_masked", "mask_out"):
        assert nm.rel(tm.tangent_energy(2, X, du, d0, dm1, wrong=wrong)[2], right) > 1e4 * te.TOL, wrong
    for kind in ("lin", "nl"):
        loop, f, d, *_ = loop_case(plants, kind, 2, 5)
        t = tlm.tangent(loop, f, d)
        right = te.loop_dde(loop, f, t)
        for wrong in ("x_masked", "mask_out"):
            assert lm.rel(te.loop_dde(loop, f, t, wrong), right) > 1e4 * te.TOL, (kind, wrong)


# ── the drivers on a recording device ────────────────────────────────────────────────────────────────────────────────────────────
N, NS, NA, NSTEPS, DT, K = 6, 2, 1, 3, 0.125, 3
BATCHED = ("btan", "bcltan")
Q = np.array([[2.0, 0.5], [0.25, 3.0]])
R = np.array([[0.75]])
E = np.array([0.5, 0.0, 2.0])


class EnergyDevice(RecordingDevice):
    """RecordingDevice with the entry points of the tangent energy, the tangent tape and the energy source, and the little state the
    tests read back afterwards."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.t_energy, self.t_tape, self.source, self.rows, self.last = False, 0, 0, None, (0, 0)

    def tangent_reserve(self, on=1):
        self.t_energy = False
        super().tangent_reserve(on)

    def tangent_set_energy(self, on=1):
        self._rec("tangent_set_energy", on)  # (a call that fails changes nothing on the handle)
        self.t_energy = bool(on)

    def tangent_energy_info(self):
        self._rec("tangent_energy_info")
        return {"on": self.t_energy, "have": False, "kernel": 0, "grid": 0, "steps": 0, "k": 0, "launches": 0, "bytes": 0}

    def tangent_energy(self):
        self._rec("tangent_energy")
        assert self.t_energy
        n, k = self.last
        return filled("dde", n, k) if k else filled("dde", n)

    def tangent_tape_reserve(self, n):
        self._rec("tangent_tape_reserve", n)
        self.t_tape = int(n)
        if not n:
            self.source = 0

    def set_adjoint_energy(self, e=None, batched=False):
        self._rec("set_adjoint_energy", e)
        self.rows = e
        if e is None:
            self.source = 0

    def set_adjoint_energy_source(self, source=0):
        self._rec("set_adjoint_energy_source", source)
        self.source = int(source)

    def run_tangent(self, slot, n, du=None, dx0=None, dxm1=None):
        self.last = (int(n), 0)
        return super().run_tangent(slot, n, du, dx0, dxm1)

    def run_tangent_batch(self, slot, n, du=None, dx0=None, dxm1=None, ref_col=None):
        self.last = (int(n), self.batch_k)
        return super().run_tangent_batch(slot, n, du, dx0, dxm1, ref_col)

    def run_tangent_closed_loop(self, slot, n, direction=None, dx0=None, dxm1=None):
        self._rec("run_tangent_closed_loop", slot, n, direction, dx0, dxm1)
        self.last = (int(n), 0)
        return {"dy": filled("dy", int(n), self.n_sens), "du": filled("du", int(n), self.n_act), "xi": filled("xi", self._ctrl_bank["nx"]),
                "dxn": filled("dxn", self.N), "dxnm1": filled("dxnm1", self.N)}

    def run_tangent_closed_loop_batch(self, slot, n, direction=None, dx0=None, dxm1=None, ref_col=None):
        self._rec("run_tangent_closed_loop_batch", slot, n, direction, dx0, dxm1, ref_col)
        k = self.batch_k
        self.last = (int(n), k)
        return {"dy": filled("dy", int(n), k, self.n_sens), "du": filled("du", int(n), k, self.n_act), "xi": filled("xi", k, self._ctrl_bank["nx"]),
                "dxn": filled("dxn", k, self.N), "dxnm1": filled("dxnm1", k, self.N)}


def names(dev):
    return [c[0] for c in dev.calls]


def controller():
    return Controller([[-1.0, 0.5], [0.0, -2.0]], [[1.0], [0.5]], [[1.0, 0.25]], [[0.125]], x0=np.array([0.25, 0.5]))


def make(which, nonlinear=True):
    """(device, solver) of a driver: the batched ones get a BatchedFlowSolver of K runs."""
    dev = EnergyDevice(N, NS, NA, K if which in BATCHED else 0)
    return dev, (fake_batched if which in BATCHED else fake_flowsolver)(dev, nonlinear, 2, DT)


def drive(which, fs, **kw):
    u = filled("u_seq", NSTEPS, NA)
    if which == "btan":
        return tan_mod.batched_tangent_run(fs, filled("u_seq", NSTEPS, K, NA), filled("du", NSTEPS, K, NA), **kw)
    if which == "bcltan":
        return tan_mod.batched_closed_loop_tangent(fs, [controller() for _ in range(K)], NSTEPS, [{"C": filled("dC", 1, 2)} for _ in range(K)], **kw)
    if which == "tan":
        return tan_mod.tangent_run(fs, u, filled("du", NSTEPS, NA), **kw)
    if which == "gnp":
        return tan_mod.gauss_newton_product(fs, u, Q, R, filled("v", NSTEPS, NA), **kw)
    if which == "cltan":
        return tan_mod.closed_loop_tangent(fs, controller(), NSTEPS, {"C": filled("dC", 1, 2)}, **kw)
    assert which == "clgnp"
    return tan_mod.closed_loop_gauss_newton_product(fs, controller(), NSTEPS, Q, R, {"C": filled("dC", 1, 2)}, **kw)


ENERGY_KW = {"tan": {"energy": True}, "cltan": {"energy": True}, "btan": {"energy": True}, "bcltan": {"energy": True}, "gnp": {"energy": E},
             "clgnp": {"energy": E}}
FORWARD = {"tan": "run", "gnp": "run", "cltan": "run_closed_loop", "clgnp": "run_closed_loop", "btan": "step_batch", "bcltan": "run_closed_loop_batch"}
MARCH = {"tan": "run_tangent", "gnp": "run_tangent", "cltan": "run_tangent_closed_loop", "clgnp": "run_tangent_closed_loop", "btan": "run_tangent_batch",
         "bcltan": "run_tangent_closed_loop_batch"}


@pytest.mark.parametrize("which,nonlinear", [("tan", True), ("gnp", True), ("cltan", True), ("cltan", False), ("clgnp", True), ("clgnp", False),
                                             ("btan", True), ("bcltan", True), ("bcltan", False)])
def test_call_order_of_the_drivers(which, nonlinear):
    dev, fs = make(which, nonlinear)
    out = drive(which, fs, **ENERGY_KW[which])
    seq = names(dev)
    first = lambda name: seq.index(name)  # noqa: E731
    forward, march = FORWARD[which], MARCH[which]
    batched = which in BATCHED
    begin, reserve = ("adjoint_tape_begin_batch", "adjoint_tape_reserve_batch") if batched else ("adjoint_tape_begin", "adjoint_tape_reserve")
    assert begin in seq and first(reserve) < first(begin) < first(forward) < first(march), seq  # (taped on a linearised solver too)
    if which in ("tan", "cltan", "btan", "bcltan"):
        assert first("tangent_reserve") < first("tangent_set_energy") < first(forward) < first(march) < first("tangent_energy"), seq
        assert seq.count("tangent_set_energy") == 2 and seq.index("tangent_set_energy", first("tangent_energy")) < len(seq) - 1 - seq[::-1].index("tangent_reserve")
        assert [c[1][0] for c in dev.calls if c[0] == "tangent_set_energy"] == [1, 0]
        dde = out[3] if which in ("tan", "btan") else out["dde"]
        assert np.array_equal(dde, filled("dde", NSTEPS, K) if batched else filled("dde", NSTEPS))
        if which == "btan":
            assert len(out) == 4 and out[0].shape == (NSTEPS, K, NS)
        if which == "bcltan":
            assert set(out) == {"y", "u", "dy", "du", "xi", "dxn", "dxnm1", "dde"}
    else:
        adjoint = "run_adjoint" if which == "gnp" else "run_adjoint_closed_loop"
        order = [forward, "tangent_tape_reserve", march, "set_adjoint_energy", "set_adjoint_energy_source", adjoint]
        assert [first(a) for a in order] == sorted(first(a) for a in order), seq
        tail = seq[first(adjoint):]
        assert tail.index("set_adjoint_energy_source") < tail.index("set_adjoint_energy") < tail.index("tangent_tape_reserve") < tail.index("set_state"), seq
        held = [c for c in dev.calls if c[0] == "set_adjoint_energy"]
        assert held[0][1][0] == ("f8", (NSTEPS,), E.tolist()) and held[1][1][0] is None
        assert [c[1][0] for c in dev.calls if c[0] == "tangent_tape_reserve"] == [NSTEPS, 0]
        assert [c[1][0] for c in dev.calls if c[0] == "set_adjoint_energy_source"] == [1, 0]
    assert dev.rows is None and (dev.source, dev.t_tape, dev.t_energy, dev._tangent) == (0, 0, False, False)
    assert dev._tape[False]["capacity"] == 0 and dev._tape[True]["capacity"] == 0 and dev._ctrl_bank is None


@pytest.mark.parametrize("which", ["tan", "gnp", "cltan", "clgnp", "btan", "bcltan"])
def test_without_the_keyword_no_new_call_is_made(which):
    """energy=None / False: the device calls of the call without the keyword, one for one."""
    traces = []
    for kw in ({}, {"energy": None if which in ("gnp", "clgnp") else False}):
        dev, fs = make(which)
        drive(which, fs, **kw)
        traces.append(list(dev.calls))
    assert traces[0] == traces[1]
    new = {"tangent_set_energy", "tangent_energy_info", "tangent_energy", "tangent_tape_reserve", "set_adjoint_energy_source", "set_adjoint_energy"}
    assert not new & {c[0] for c in traces[0]}


STAGES = {"tan": ["tangent_reserve", "tangent_energy_info", "tangent_set_energy", "adjoint_tape_begin", "run", "run_tangent", "tangent_energy"],
          "gnp": ["run", "tangent_tape_reserve", "tangent_reserve", "run_tangent", "set_adjoint_energy", "set_adjoint_energy_source", "run_adjoint"],
          "cltan": ["tangent_set_energy", "run_closed_loop", "run_tangent_closed_loop", "tangent_energy"],
          "clgnp": ["run_closed_loop", "tangent_tape_reserve", "run_tangent_closed_loop", "set_adjoint_energy", "set_adjoint_energy_source",
                    "run_adjoint_closed_loop"],
          "btan": ["tangent_reserve", "tangent_energy_info", "tangent_set_energy", "adjoint_tape_begin_batch", "step_batch", "run_tangent_batch",
                   "tangent_energy"],
          "bcltan": ["tangent_set_energy", "adjoint_tape_begin_batch", "run_closed_loop_batch", "run_tangent_closed_loop_batch", "tangent_energy"]}


@pytest.mark.parametrize("which,stage", [(w, s) for w, stages in STAGES.items() for s in stages])
def test_every_exit_path(which, stage):
    """An exception in each stage leaves no rows held, source 0, no tangent tape, no tangent reserve or option, no state tape, no
    bank, and the state put back."""
    dev, fs = make(which, which not in ("clgnp", "bcltan"))  # (the two on a linearised solver: taped for the energy alone)
    dev.fail = {stage: 1}
    with pytest.raises(Marker, match=stage):
        drive(which, fs, **ENERGY_KW[which])
    dev.fail = {}
    assert dev.rows is None and (dev.source, dev.t_tape, dev.t_energy) == (0, 0, False), (dev.rows, dev.source, dev.t_tape, dev.t_energy)
    if stage != "tangent_reserve":
        assert not dev._tangent
    assert dev._tape[False]["capacity"] == 0 and dev._tape[True]["capacity"] == 0 and dev._ctrl_bank is None
    seq = names(dev)
    getter, setter, lead = ("get_state_batch", "set_state_batch", (K,)) if which in BATCHED else ("get_state", "set_state", ())
    if getter in seq:
        last_set = [c for c in dev.calls if c[0] == setter][-1]
        assert seq.index(getter) < len(seq) - 1 - seq[::-1].index(setter)
        assert last_set[1] == tuple(("f8", tuple(a.shape), a.ravel().tolist()) for a in (filled("u_n", *lead, 4), filled("u_nn", *lead, 4), filled("p_n", *lead, 2)))


def test_refusals_of_the_products():
    dev = EnergyDevice(N, NS, NA)
    fs = fake_flowsolver(dev, True, 2, DT)
    with pytest.raises(ValueError, match=r"energy must be a scalar, \(3,\)"):
        drive("gnp", fs, energy=np.ones(4))
    with AdjointRun(fs, tape=NSTEPS, checkpoint_every=2) as adj:
        with pytest.raises(ValueError, match="checkpointed"):
            drive("gnp", fs, energy=E, adjoint=adj)
    lin = fake_flowsolver(EnergyDevice(N, NS, NA), False, 2, DT)
    with AdjointRun(lin, loop=NSTEPS) as adj:
        with pytest.raises(ValueError, match=r"energy= reads the forward trajectory -- the AdjointRun needs a state tape"):
            drive("clgnp", lin, energy=E, adjoint=adj)
    # a checkpointed tape under the closed-loop product: still refused, with the reason
    dev2 = EnergyDevice(N, NS, NA)
    fs2 = fake_flowsolver(dev2, True, 2, DT)
    with AdjointRun(fs2, tape=NSTEPS, loop=NSTEPS, checkpoint_every=2) as adj:
        del dev2.calls[:]
        with pytest.raises(ValueError, match=r"^closed_loop_gauss_newton_product: a tangent march over a checkpointed tape is not built"):
            drive("clgnp", fs2, energy=E, adjoint=adj)
        assert not {"tangent_tape_reserve", "set_adjoint_energy", "set_adjoint_energy_source", "run_closed_loop"} & set(names(dev2))
    assert SLOT_BDF2 == 1
