"""The checkpointed state tape on the device (``fc_adjoint_tape_reserve_sparse``; DESIGN section 5.4 "Checkpointed tape"): on ONE handle
the same forward run from the same state is taped densely and marched, then taped with spacing c and marched, and every array the march
returns must be ``np.array_equal`` -- no tolerance: a replayed segment is the taped step's own launches on the taped controls, so the
columns a backward step reads are the dense tape's bits.  n = 7 steps; c = 1 (every segment one step), 2 (odd tail), 3 (a boundary
inside the first BDF2 steps), 7 (one segment, no replay), 9 (spacing beyond the run).  Meshes "9x9" (N = 822) and "12x7" (N = 854) of
tests/support/adjoint_march_cases.py.  Then: the replayed columns themselves, the forward state behind a march, refusals, undo,
overflow, memory.  The batched cases are in tests/test_adjoint_ckpt_batch_gpu.py.  The refusal of a partitioned handle needs two GPUs
and is not exercised.  A replayed MIDDLE segment cannot be read between two segments -- a march synchronises once --: what is read
is segment 0 behind the march, which every run of more than c steps has recomputed; the others show in the gradients."""
import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_march_cases as mc
from tests.support import step_cases as sc

pytestmark = pytest.mark.gpu

INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
N_STEPS = 7
SPACINGS = (1, 2, 3, 7, 9)
LOOP_OUT = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "ubar", "dx0", "dxm1")


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def nl():
    """Nonlinear handle on "9x9", two Dirichlet actuators, five sensors, one refinement sweep per solve."""
    from tests.support.adjoint_march_child import Handle

    h = Handle("9x9", 2, "dirichlet", "five", "default", True, 1)
    yield h
    h.close()


@pytest.fixture(scope="module")
def lin():
    """Linearised handle on "12x7", two actuators with body-force profiles, factor apply only (the fused tail)."""
    from tests.support.adjoint_march_child import Handle

    h = Handle("12x7", 2, "mixed", "five", "default", False, 0)
    yield h
    h.close()


def slot_of(first_order):
    return SLOT_BDF1 if first_order == 1 else SLOT_BDF2


def reserve(dev, c, capacity=N_STEPS):
    """c = None: the dense tape."""
    if c is None:
        dev.adjoint_tape_reserve(capacity)
    else:
        dev.adjoint_tape_reserve_sparse(capacity, c)


def inputs(h, seed=5):
    rng = np.random.default_rng(seed)
    w, z = mc.inputs(h.model.N, len(h.model.rows), N_STEPS, seed)
    return 0.1 * rng.standard_normal((N_STEPS, h.dev.n_act)), w, z


def open_loop(h, c, first_order, energy=None):
    """Forward run and march on the tape of spacing c: everything the march returns, and what the handle looked like around it."""
    dev = h.dev
    u, w, z = inputs(h)
    reserve(dev, c)
    dev.set_state(*sc.initial_state(h.th, 1))
    dev.adjoint_tape_begin()
    y, dE = dev.run(slot_of(first_order), N_STEPS, u, compute_energy=True)
    before = (dev.get_state(), dev.step_counts())
    dense_columns = dev.adjoint_tape_states() if c is None else None
    if energy is not None:
        dev.set_adjoint_energy(energy)
    try:
        g, dx0, dxm1 = dev.run_adjoint(slot_of(first_order), N_STEPS, w, z)
    finally:
        if energy is not None:
            dev.set_adjoint_energy(None)
    after = (dev.get_state(), dev.step_counts())
    return {"y": y, "dE": dE, "g": g, "dx0": dx0, "dxm1": dxm1, "before": before, "after": after, "X": dense_columns, "info": dev.adjoint_tape_info()}


def assert_state_kept(out, label):
    (s0, n0), (s1, n1) = out["before"], out["after"]
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1)), f"{label}: the state ring moved"
    assert n0 == n1, f"{label}: the step counter moved: {n0} -> {n1}"


def check_replayed_columns(dev, c, X, label):
    """Behind the march the buffer holds segment 0: its columns are the dense tape's columns 0 .. min(c, n) + 1."""
    seg, S = dev.adjoint_segment_states()
    assert seg == 0, label
    ncol = min(c, N_STEPS) + 2
    for col in range(ncol):
        assert np.array_equal(S[col], X[col]), f"{label}: buffer column {col} differs from the dense tape's"


@pytest.mark.parametrize("first_order", [1, 2])
def test_nonlinear_open_loop(nl, first_order):
    dense = open_loop(nl, None, first_order)
    assert_state_kept(dense, "dense")
    for c in SPACINGS:
        label = f"bdf{first_order} c = {c}"
        got = open_loop(nl, c, first_order)
        assert np.array_equal(got["y"], dense["y"]) and np.array_equal(got["dE"], dense["dE"]), f"{label}: the forward run differs"
        for k in ("g", "dx0", "dxm1"):
            assert np.array_equal(got[k], dense[k]), f"{label}: {k} differs from the dense tape's"
        assert_state_kept(got, label)
        last = N_STEPS - (cdiv(N_STEPS, c) - 1) * c
        assert got["info"]["every"] == c and got["info"]["replayed"] == N_STEPS - last, (label, got["info"])
        check_replayed_columns(nl.dev, c, dense["X"], label)
    nl.dev.adjoint_tape_reserve_sparse(0, 0)


def test_linearised_with_energy(lin):
    e = np.random.default_rng(9).standard_normal(N_STEPS)
    dense = open_loop(lin, None, 1, energy=e)
    for c in SPACINGS:
        got = open_loop(lin, c, 1, energy=e)
        for k in ("y", "dE", "g", "dx0", "dxm1"):
            assert np.array_equal(got[k], dense[k]), f"c = {c}: {k} differs from the dense tape's"
        assert_state_kept(got, f"c = {c}")
        check_replayed_columns(lin.dev, c, dense["X"], f"c = {c}")
    lin.dev.adjoint_tape_reserve_sparse(0, 0)


def test_steps_taken_one_by_one_with_an_early_end(lin):
    """fc_step_begin / fc_step_end without waiting for energy and residual: where the handle overlaps the step's tail with the next
    step, the taped step took the overlapped form of the launches; the replay must still reproduce its state bit for bit."""
    dev = lin.dev
    u, w, z = inputs(lin)
    e = np.random.default_rng(9).standard_normal(N_STEPS)
    out = {}
    for c in (None, 3):
        reserve(dev, c)
        dev.set_state(*sc.initial_state(lin.th, 1))
        dev.adjoint_tape_begin()
        for m in range(N_STEPS):
            dev.step_begin(SLOT_BDF1 if m == 0 else SLOT_BDF2, u[m])
            dev.step_end(early=True)
        dev.step_collect()
        dev.set_adjoint_energy(e)
        try:
            out[c] = dev.run_adjoint(SLOT_BDF1, N_STEPS, w, z)
        finally:
            dev.set_adjoint_energy(None)
    assert all(np.array_equal(a, b) for a, b in zip(out[3], out[None]))
    dev.adjoint_tape_reserve_sparse(0, 0)


def test_a_second_march_replays_every_segment(nl):
    """A march leaves segment 0 in the buffer, which serves no march of several segments: the same run marched again recomputes all
    of them, to the same bits."""
    dev = nl.dev
    first = open_loop(nl, 2, 2)
    u, w, z = inputs(nl)
    g, dx0, dxm1 = dev.run_adjoint(SLOT_BDF2, N_STEPS, w, z)
    assert np.array_equal(g, first["g"]) and np.array_equal(dx0, first["dx0"]) and np.array_equal(dxm1, first["dxm1"])
    assert dev.adjoint_tape_info()["replayed"] == N_STEPS
    dev.adjoint_tape_reserve_sparse(0, 0)


# ── closed loops ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def loop_inputs(h, seed=13):
    rng = np.random.default_rng(seed)
    ns, na = h.dev.n_sens, h.dev.n_act
    bank = lm.random_bank(3, 2, 2, ns, na, seed=seed)
    return {"bank": bank, "y0": 0.1 * rng.standard_normal(ns), "w_y": 0.2 * rng.standard_normal((N_STEPS, 2)), "w_u": 0.2 * rng.standard_normal((N_STEPS, na)),
            "w": rng.standard_normal((N_STEPS, ns)), "r": rng.standard_normal((N_STEPS, na)), "z": rng.standard_normal(h.model.N)}


def closed_loop(h, c, limit, cuts=(N_STEPS,)):
    from tests.support.adjoint_loop_cases import put_bank

    dev, q = h.dev, loop_inputs(h)
    reserve(dev, c)
    dev.set_state(*sc.initial_state(h.th, 1))
    put_bank(dev, q["bank"])
    dev.set_loop_signals(q["w_y"], q["w_u"])
    dev.set_control_limits(None, None) if limit is None else dev.set_control_limits(np.full(dev.n_act, -limit), np.full(dev.n_act, limit))
    dev.adjoint_loop_reserve(N_STEPS)
    dev.adjoint_tape_begin()
    dev.adjoint_loop_begin()
    ys, us, y_last, slot = [], [], q["y0"], SLOT_BDF1
    for n in cuts:
        y, u, _ = dev.run_closed_loop(slot, n, y_last, compute_energy=False)
        ys.append(y), us.append(u)
        y_last, slot = y[-1], SLOT_BDF2
    before = (dev.get_state(), dev.step_counts(), dev.loop_cursor())
    g = dev.run_adjoint_closed_loop(SLOT_BDF1, N_STEPS, q["w"], q["r"], q["z"])
    after = (dev.get_state(), dev.step_counts(), dev.loop_cursor())
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1:] == after[1:], f"c = {c}: the march moved the forward state"
    return np.vstack(ys), np.vstack(us), g


def middle_limit(u):
    mag = np.sort(np.abs(u).ravel())
    return float(np.sqrt(mag[mag.size // 2 - 1] * mag[mag.size // 2]))


def test_closed_loop_with_active_and_inactive_limits(nl):
    dev = nl.dev
    _, u_free, _ = closed_loop(nl, None, None)
    limit = middle_limit(u_free)
    y, u, dense = closed_loop(nl, None, limit)
    clamped = (np.abs(u) == limit).any(axis=1)
    assert clamped.any() and not clamped.all(), f"the limit {limit} is active on steps {np.flatnonzero(clamped)} of {N_STEPS}"
    for c in SPACINGS:
        yc, uc, got = closed_loop(nl, c, limit)
        assert np.array_equal(yc, y) and np.array_equal(uc, u), f"c = {c}: the forward run differs"
        for k in LOOP_OUT:
            assert np.array_equal(got[k], dense[k]), f"c = {c}: {k} differs from the dense tape's"
    dev.adjoint_tape_reserve_sparse(0, 0)
    dev.adjoint_loop_reserve(0)
    dev.set_control_limits(None, None)


def test_closed_loop_cut_inside_a_segment(nl):
    """Two forward calls, 4 + 3 steps: with c = 3 the cut falls inside segment 1, with c = 2 on a boundary, with c = 7 inside the only one."""
    dev = nl.dev
    y, u, dense = closed_loop(nl, None, None, cuts=(4, 3))
    y1, u1, whole = closed_loop(nl, None, None)
    assert np.array_equal(y, y1) and np.array_equal(u, u1) and all(np.array_equal(whole[k], dense[k]) for k in LOOP_OUT)
    for c in (3, 2, 7):
        yc, uc, got = closed_loop(nl, c, None, cuts=(4, 3))
        assert np.array_equal(yc, y) and np.array_equal(uc, u)
        for k in LOOP_OUT:
            assert np.array_equal(got[k], dense[k]), f"c = {c}: {k} differs from the dense tape's"
    dev.adjoint_tape_reserve_sparse(0, 0)
    dev.adjoint_loop_reserve(0)


# ── the forward state behind a march ──────────────────────────────────────────────────────────────────────────────────────────────────
def test_a_following_step_is_what_it_is_without_the_march(nl):
    dev = nl.dev
    u, w, z = inputs(nl)
    results = []
    for march in (False, True):
        dev.adjoint_tape_reserve_sparse(N_STEPS, 3)
        dev.set_state(*sc.initial_state(nl.th, 1))
        dev.adjoint_tape_begin()
        dev.run(SLOT_BDF1, N_STEPS, u, compute_energy=False)
        if march:
            dev.run_adjoint(SLOT_BDF1, N_STEPS, w, z)
        y, dE, info = dev.step(SLOT_BDF2, u[0])
        results.append((y.copy(), dE, np.asarray(info).copy(), dev.get_solution()))
    assert all(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for a, b in zip(*results))
    dev.adjoint_tape_reserve_sparse(0, 0)


# ── refusals, displacement, undo, overflow, memory ────────────────────────────────────────────────────────────────────────────────────
def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def test_refusals(nl, lin):
    dev = nl.dev
    u, w, z = inputs(nl)
    dev.adjoint_tape_reserve_sparse(0, 0)
    refused(INV, dev.adjoint_tape_reserve_sparse, 7, -1, match="every must be in [0, 2^24]")
    refused(INV, dev.adjoint_tape_reserve_sparse, -1, 2, match="capacity must be in [0, 2^24]")
    refused(INV, dev.adjoint_tape_reserve_sparse, (1 << 24) + 1, 2, match="capacity must be in [0, 2^24]")
    # (a reserve beyond free device memory: test_a_reserve_beyond_device_memory_is_refused, on a larger mesh)
    assert dev.adjoint_tape_info()["capacity"] == 0
    dev.set_state(*sc.initial_state(nl.th, 1))
    dev.step_begin(SLOT_BDF2, u[0])
    try:
        refused(INV, dev.adjoint_tape_reserve_sparse, 7, 2, match="a step is in flight")
    finally:
        dev.step_end()
    lin.dev.set_batch(3)
    try:
        refused(INV, lin.dev.adjoint_tape_reserve_sparse, 7, 2, match="the handle has a batch set")
    finally:
        lin.dev.set_batch(0)
    # a tape that does not hold the run: the dense tape's wording
    dev.adjoint_tape_reserve_sparse(N_STEPS, 3)
    refused(INV, dev.run_adjoint, SLOT_BDF1, N_STEPS, w, z, match="the tape is not begun")
    dev.set_state(*sc.initial_state(nl.th, 1))
    dev.adjoint_tape_begin()
    dev.run(SLOT_BDF1, 5, u[:5], compute_energy=False)
    refused(INV, dev.run_adjoint, SLOT_BDF1, N_STEPS, w, z, match="the tape holds 5 steps, the run has 7")
    refused(INV, dev.run_adjoint, SLOT_BDF2, 5, w[:5], z, match="the first taped step ran on order slot 0, not on 1")
    refused(INV, dev.step_adjoint, SLOT_BDF2, 1.0, 0.0, None, match="the time scheme is nonlinear")
    dev.adjoint_tape_reserve_sparse(0, 0)


def test_a_reserve_beyond_device_memory_is_refused():
    """2^24 steps with c = 1 are 2^25 + 3 columns: 5 TB at N = 18 915, beyond any device.  Refused with the bytes named; the handle
    keeps the tape it had."""
    from tests.support.adjoint_march_child import Handle

    h = Handle("64x32", 5, "dirichlet", "on_dirichlet", "default", False, 0)
    try:
        dev = h.dev
        dev.adjoint_tape_reserve_sparse(7, 2)
        refused(INV, dev.adjoint_tape_reserve_sparse, 1 << 24, 1, match="the device has")
        info = dev.adjoint_tape_info()
        assert info["capacity"] == 7 and info["every"] == 2
    finally:
        h.close()


def test_begin_after_the_actuators_changed():
    """The control tape is laid out for the actuators of the reserve: with another number of them _begin is refused, until the tape is
    reserved again.  (A handle of its own: the actuator set is not put back.)"""
    from tests.support.adjoint_march_child import Handle

    h = Handle("9x9", 2, "dirichlet", "five", "default", True, 0)
    try:
        dev = h.dev
        dev.set_state(*sc.initial_state(h.th, 1))
        dev.adjoint_tape_reserve_sparse(N_STEPS, 3)
        dev.adjoint_tape_begin()
        dev.set_bc(h.dofs, mc.profiles(h.th, h.dofs, 3))  # the same Dirichlet dofs, three actuators
        refused(NOT_READY, dev.adjoint_tape_begin, match="the actuators changed since fc_adjoint_tape_reserve_sparse")
        dev.adjoint_tape_reserve_sparse(N_STEPS, 3)
        dev.adjoint_tape_begin()
        assert dev.adjoint_tape_info()["begun"] and dev.adjoint_tape_info()["bytes"] == (2 * 3 + 3 + 2) * 8 * dev.N + 8 * 2 * 3 * N_STEPS
    finally:
        h.close()


def test_the_long_horizon_example_runs(tmp_path):
    """examples/cavity/compute_long_horizon_gradient.py at a tiny horizon: the keys it prints exist, the tape is the checkpointed
    one and the march recomputed all but the last segment."""
    from flowcontrol_amd.examples.cavity.compute_long_horizon_gradient import main

    n = 20
    J, g, info = main(num_steps=n, every=6, path_out=tmp_path)
    assert np.isfinite(J) and all(np.all(np.isfinite(g[k])) for k in ("A", "B", "C", "D"))
    tape = info["tape"]
    assert info["tape_mode"] == "checkpointed" and tape["every"] == 6 and tape["capacity"] == n and tape["replayed"] == n - 2


def test_undo_behind_a_march_and_the_snapshot_bank(nl):
    """fc_undo_step's saved state and the snapshot bank are as the march found them: the step taken last can still be withdrawn, to
    the bits it is withdrawn to without a march, and the bank has counted and captured nothing."""
    dev = nl.dev
    u, w, z = inputs(nl)
    out = []
    for march in (False, True):
        dev.adjoint_tape_reserve_sparse(N_STEPS, 3)
        dev.set_state(*sc.initial_state(nl.th, 1))
        dev.snap_reserve(4, every=2)
        dev.adjoint_tape_begin()
        for m in range(N_STEPS):
            dev.step(SLOT_BDF1 if m == 0 else SLOT_BDF2, u[m])
        snap = dev.snap_info()
        if march:
            dev.run_adjoint(SLOT_BDF1, N_STEPS, w, z)
            assert dev.snap_info() == snap
        dev.undo_step()
        out.append(dev.get_state())
        dev.snap_reserve(0)
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    dev.adjoint_tape_reserve_sparse(0, 0)


def test_dense_and_sparse_reserves_displace_each_other(nl):
    dev, N = nl.dev, nl.dev.N
    dev.adjoint_tape_reserve(5)
    assert dev.adjoint_tape_info() == {"capacity": 5, "count": 0, "overflowed": False, "bytes": 8 * N * 7, "begun": False, "lost": 0}
    dev.adjoint_tape_reserve_sparse(7, 2)
    info = dev.adjoint_tape_info()
    assert info["capacity"] == 7 and info["every"] == 2 and info["bytes"] == 8 * N * (2 * 4 + 2 + 2) + 8 * 2 * dev.n_act * 7
    refused(NOT_READY, dev.adjoint_tape_states)  # (the dense tape's reader finds no dense tape)
    dev.adjoint_tape_reserve(5)
    assert dev.adjoint_tape_info() == {"capacity": 5, "count": 0, "overflowed": False, "bytes": 8 * N * 7, "begun": False, "lost": 0}
    dev.adjoint_tape_reserve_sparse(7, 0)  # every = 0 frees the checkpointed reserve only: the dense tape is not this call's
    assert dev.adjoint_tape_info()["capacity"] == 5
    dev.adjoint_tape_reserve_sparse(7, 2)
    dev.adjoint_tape_reserve_sparse(0, 2)  # capacity = 0 frees it
    assert dev.adjoint_tape_info() == {"capacity": 0, "count": 0, "overflowed": False, "bytes": 0, "begun": False, "lost": 0}


def test_a_handle_that_reserves_nothing_holds_nothing(nl):
    dev = nl.dev
    dev.adjoint_tape_reserve_sparse(0, 0)
    bytes0 = dev.adjoint_info(SLOT_BDF2)["bytes"]
    u, _, _ = inputs(nl)
    dev.set_state(*sc.initial_state(nl.th, 1))
    dev.run(SLOT_BDF1, 3, u[:3], compute_energy=False)
    raw = np.zeros(8, dtype=np.int64)
    _lib.check(dev.lib.fc_adjoint_tape_info(dev._h, raw))
    assert not raw.any(), raw  # zero bytes, zero replays, no spacing
    assert dev.adjoint_info(SLOT_BDF2)["bytes"] == bytes0


def test_undo_inside_a_segment_and_across_a_boundary(nl):
    dev = nl.dev
    u, w, z = inputs(nl)

    def stepped(c, undo_at):
        """Seven taped steps, the step `undo_at` taken twice with an undo in between; then the march."""
        reserve(dev, c)
        dev.set_state(*sc.initial_state(nl.th, 1))
        dev.adjoint_tape_begin()
        for m in range(1, N_STEPS + 1):
            dev.step(SLOT_BDF1 if m == 1 else SLOT_BDF2, u[m - 1])
            if m == undo_at:
                dev.undo_step()
                if not dev.adjoint_tape_info()["begun"]:
                    return None
                dev.step(SLOT_BDF1 if m == 1 else SLOT_BDF2, u[m - 1])
        return dev.run_adjoint(SLOT_BDF1, N_STEPS, w, z)

    dense = stepped(None, 5)
    got = stepped(3, 5)  # step 5 is the second of segment 1: its column is withdrawn and written again
    assert got is not None and all(np.array_equal(a, b) for a, b in zip(got, dense))
    assert stepped(3, 4) is None  # step 4 opened segment 1: withdrawing it ends the tape
    refused(INV, dev.run_adjoint, SLOT_BDF1, N_STEPS, w, z, match="the tape is not begun")
    dev.adjoint_tape_reserve_sparse(0, 0)


def test_overflow(nl):
    dev = nl.dev
    u, w, z = inputs(nl)
    dev.adjoint_tape_reserve_sparse(5, 2)
    dev.set_state(*sc.initial_state(nl.th, 1))
    dev.adjoint_tape_begin()
    dev.run(SLOT_BDF1, N_STEPS, u, compute_energy=False)
    info = dev.adjoint_tape_info()
    assert info["overflowed"] and info["count"] == 5 and info["lost"] == 2
    refused(INV, dev.run_adjoint, SLOT_BDF1, N_STEPS, w, z, match="the tape overflowed: 7 steps since it was begun, capacity 5")
    dev.adjoint_tape_reserve_sparse(0, 0)


def test_memory(nl):
    """n = 1000: the bytes reported are (2 ceil(n / c) + c + 2) 8 N plus the control tape; with "auto" below a tenth of the dense tape's."""
    from flowcontrol_amd.adjoint import checkpoint_spacing

    dev, N, n = nl.dev, nl.dev.N, 1000
    auto = checkpoint_spacing("auto", n)
    assert auto == 45
    for c in (1, 7, auto, 1000, 1002):
        dev.adjoint_tape_reserve_sparse(n, c)
        assert dev.adjoint_tape_info()["bytes"] == (2 * cdiv(n, c) + c + 2) * 8 * N + 8 * 2 * dev.n_act * n, c
    dev.adjoint_tape_reserve_sparse(n, auto)
    sparse = dev.adjoint_tape_info()["bytes"]
    dev.adjoint_tape_reserve(n)
    dense = dev.adjoint_tape_info()["bytes"]
    assert dense == (n + 2) * 8 * N and sparse < dense / 10, (sparse, dense)
    dev.adjoint_tape_reserve(0)
