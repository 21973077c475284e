"""The checkpointed form of the BATCHED state tape (``fc_adjoint_tape_reserve_sparse_batch``; DESIGN section 5.4 "Checkpointed tape"),
held to the dense batched tape as tests/test_adjoint_ckpt_gpu.py holds the single one: the same batched forward run from the same
batched state, taped densely and with spacing c = 1, 2, 3, 7, 9 over n = 7 steps, and every array the march returns
``np.array_equal``.  Batched nonlinear runs of k = 1 and k = 5 (both padded: KB = 4 and 8) on "9x9"; k = 3 closed loops with
controllers of two orders on "12x7".  A replayed middle segment cannot be read between two segments (a march synchronises once): what is
read is segment 0 behind the march, the others show in the gradients."""
import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from tests.support import adjoint_loop_batch_cases as lbc
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


def handle(mesh, k, nonlinear=True):
    from tests.support.adjoint_march_child import Handle

    return Handle(mesh, 2, "dirichlet", "five", "default", nonlinear, 0, k=k)


@pytest.fixture(scope="module", params=[1, 5], ids=["k1", "k5"])
def nlb(request):
    h = handle("9x9", request.param)
    yield h
    h.close()


@pytest.fixture(scope="module")
def loops():
    h = handle("12x7", 3)
    yield h
    h.close()


def reserve(dev, c, capacity=N_STEPS):
    if c is None:
        dev.adjoint_tape_reserve_batch(capacity)
    else:
        dev.adjoint_tape_reserve_sparse_batch(capacity, c)


def batch_state(h, k):
    cols = [sc.initial_state(h.th, 1 + s) for s in range(k)]
    return tuple(np.array([c[i] for c in cols]) for i in range(3))


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def open_loop(h, c, first_order, early=False):
    dev, k = h.dev, h.dev.batch_k
    rng = np.random.default_rng(5)
    u = 0.1 * rng.standard_normal((N_STEPS, k, dev.n_act))
    w, z = mc.inputs(h.model.N, len(h.model.rows), N_STEPS, 5, k=max(k, 3))
    w, z = np.ascontiguousarray(w[:, :k]), np.ascontiguousarray(z[:k])
    reserve(dev, c)
    dev.set_state_batch(*batch_state(h, k))
    dev.adjoint_tape_begin_batch()
    ys = []
    for m in range(N_STEPS):
        slot = SLOT_BDF1 if (m == 0 and first_order == 1) else SLOT_BDF2
        if early:  # the overlapped form of the batched step, where the handle takes it
            dev.step_batch_begin(slot, u[m], compute_energy=False)
            ys.append(dev.step_batch_end_early()[0])
        else:
            ys.append(dev.step_batch(slot, u[m], compute_energy=False)[0])
    if early:
        dev.step_batch_collect()
    before = (dev.get_state_batch(), dev.step_counts())
    X = dev.adjoint_tape_states_batch() if c is None else None
    g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, N_STEPS, w, z)
    after = (dev.get_state_batch(), dev.step_counts())
    assert same_state(before[0], after[0]) and before[1] == after[1], f"c = {c}: the march moved the batched forward state"
    return {"y": np.array(ys), "g": g, "dx0": dx0, "dxm1": dxm1, "X": X, "info": dev.adjoint_tape_info_batch()}


@pytest.mark.parametrize("first_order", [1, 2])
def test_batched_nonlinear(nlb, first_order):
    dev = nlb.dev
    dense = open_loop(nlb, None, first_order)
    for c in SPACINGS:
        label = f"k = {dev.batch_k} bdf{first_order} c = {c}"
        got = open_loop(nlb, c, first_order)
        for key in ("y", "g", "dx0", "dxm1"):
            assert np.array_equal(got[key], dense[key]), f"{label}: {key} differs from the dense tape's"
        last = N_STEPS - (cdiv(N_STEPS, c) - 1) * c
        assert got["info"]["every"] == c and got["info"]["replayed"] == N_STEPS - last, (label, got["info"])
        seg, S = dev.adjoint_segment_states_batch()
        assert seg == 0
        for col in range(min(c, N_STEPS) + 2):
            assert np.array_equal(S[col], dense["X"][col]), f"{label}: buffer column {col} differs from the dense tape's"
    dev.adjoint_tape_reserve_sparse_batch(0, 0)


def test_batched_steps_with_an_early_end(nlb):
    dense = open_loop(nlb, None, 2, early=True)
    got = open_loop(nlb, 3, 2, early=True)
    for key in ("y", "g", "dx0", "dxm1"):
        assert np.array_equal(got[key], dense[key]), key
    nlb.dev.adjoint_tape_reserve_sparse_batch(0, 0)


def test_a_following_batched_step_is_what_it_is_without_the_march(nlb):
    dev, k = nlb.dev, nlb.dev.batch_k
    u = 0.1 * np.random.default_rng(5).standard_normal((N_STEPS, k, dev.n_act))
    w, z = mc.inputs(nlb.model.N, len(nlb.model.rows), N_STEPS, 5, k=max(k, 3))
    out = []
    for march in (False, True):
        dev.adjoint_tape_reserve_sparse_batch(N_STEPS, 3)
        dev.set_state_batch(*batch_state(nlb, k))
        dev.adjoint_tape_begin_batch()
        for m in range(N_STEPS):
            dev.step_batch(SLOT_BDF2, u[m], compute_energy=False)
        if march:
            dev.run_adjoint_batch(SLOT_BDF2, N_STEPS, np.ascontiguousarray(w[:, :k]), np.ascontiguousarray(z[:k]))
        y, dE, info = dev.step_batch(SLOT_BDF2, u[0], compute_energy=True)
        out.append((y.copy(), dE.copy(), np.asarray(info).copy(), dev.get_solution_batch()))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(*out))
    dev.adjoint_tape_reserve_sparse_batch(0, 0)


# ── k = 3 closed loops, controllers of two orders ─────────────────────────────────────────────────────────────────────────────────────
def bank_of_three(ns, na):
    banks = [lm.random_bank(3, 2, 2, ns, na, seed=31 + s) for s in range(3)]
    b = banks[1]  # column 1: a controller of order 2 in the zero-padded bank of order 3
    b["Ad"][0, 2, :], b["Ad"][0, :, 2], b["Bd"][0, 2, :], b["C"][0, :, 2], b["x0"][0, 2] = 0.0, 0.0, 0.0, 0.0, 0.0
    b["sizes"] = [(2, 2)]

    class Q:
        pass

    loops = []
    for bk in banks:
        q = Q()
        q.bank = bk
        loops.append(q)
    return lbc.stack_bank(loops)


def closed_loops(h, c, limit):
    dev, k = h.dev, 3
    rng = np.random.default_rng(17)
    ns, na = dev.n_sens, dev.n_act
    y0 = 0.1 * rng.standard_normal((k, ns))
    w, r, z = rng.standard_normal((N_STEPS, k, ns)), rng.standard_normal((N_STEPS, k, na)), rng.standard_normal((k, h.model.N))
    reserve(dev, c)
    dev.set_state_batch(*batch_state(h, k))
    lbc.put_bank(dev, bank_of_three(ns, na))
    dev.set_control_limits(None, None) if limit is None else dev.set_control_limits(np.full((k, na), -limit), np.full((k, na), limit))
    dev.adjoint_loop_reserve_batch(N_STEPS)
    dev.adjoint_tape_begin_batch()
    dev.adjoint_loop_begin_batch()
    y, u, _, bad, _ = dev.run_closed_loop_batch(SLOT_BDF1, N_STEPS, y0, compute_energy=False)
    assert np.all(bad < 0)
    before = (dev.get_state_batch(), dev.step_counts(), dev.loop_cursor())
    g = dev.run_adjoint_closed_loop_batch(SLOT_BDF1, N_STEPS, w, r, z)
    after = (dev.get_state_batch(), dev.step_counts(), dev.loop_cursor())
    assert same_state(before[0], after[0]) and before[1:] == after[1:], f"c = {c}: the march moved the batched forward state"
    return y, u, g


def test_batched_closed_loops_of_two_orders(loops):
    dev = loops.dev
    _, u_free, _ = closed_loops(loops, None, None)
    mag = np.sort(np.abs(u_free).ravel())
    limit = float(np.sqrt(mag[mag.size // 2 - 1] * mag[mag.size // 2]))
    y, u, dense = closed_loops(loops, None, limit)
    clamped = (np.abs(u) == limit).any(axis=(1, 2))
    assert clamped.any() and not (np.abs(u) == limit).all(), "the limit must clamp some control values and leave others free"
    for c in SPACINGS:
        yc, uc, got = closed_loops(loops, c, limit)
        assert np.array_equal(yc, y) and np.array_equal(uc, u), f"c = {c}: the forward run differs"
        for key in LOOP_OUT:
            assert np.array_equal(got[key], dense[key]), f"c = {c}: {key} differs from the dense tape's"
    dev.adjoint_tape_reserve_sparse_batch(0, 0)
    dev.adjoint_loop_reserve_batch(0)
    dev.set_control_limits(None, None)


# ── memory, displacement, refusals ────────────────────────────────────────────────────────────────────────────────────────────────────
def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def test_memory_and_displacement(nlb):
    """n = 1000: (2 ceil(n / c) + c + 2) 8 N KB plus the control tape; "auto" below a tenth of the dense tape's; the two reserves
    displace each other; a reserve beyond free device memory is refused with the bytes named."""
    from flowcontrol_amd.adjoint import checkpoint_spacing

    dev, N, n = nlb.dev, nlb.dev.N, 1000
    KB = mc.kb_of(dev.batch_k)
    auto = checkpoint_spacing("auto", n)
    for c in (1, 7, auto, 1002):
        dev.adjoint_tape_reserve_sparse_batch(n, c)
        info = dev.adjoint_tape_info_batch()
        assert info["bytes"] == (2 * cdiv(n, c) + c + 2) * 8 * N * KB + 8 * 2 * dev.n_act * KB * n and info["KB"] == KB and info["every"] == c, (c, info)
    dev.adjoint_tape_reserve_sparse_batch(n, auto)
    sparse = dev.adjoint_tape_info_batch()["bytes"]
    dev.adjoint_tape_reserve_batch(n)  # the dense reserve frees the checkpointed one
    info = dev.adjoint_tape_info_batch()
    assert "every" not in info and info["bytes"] == (n + 2) * 8 * N * KB and sparse < info["bytes"] / 10, (sparse, info)
    dev.adjoint_tape_reserve_sparse_batch(n, 0)  # every = 0 frees the checkpointed reserve only
    assert dev.adjoint_tape_info_batch()["capacity"] == n
    dev.adjoint_tape_reserve_sparse_batch(7, 2)  # ... and the checkpointed reserve frees the dense one
    assert dev.adjoint_tape_info_batch()["bytes"] == (2 * 4 + 2 + 2) * 8 * N * KB + 8 * 2 * dev.n_act * KB * 7
    refused(NOT_READY, dev.adjoint_tape_states_batch)
    # 2^25 + 3 columns of N KB doubles: 0.9 TB and more at N = 822 -- beyond any device; the handle keeps the reserve it had
    refused(INV, dev.adjoint_tape_reserve_sparse_batch, 1 << 24, 1, match="the device has")
    assert dev.adjoint_tape_info_batch()["capacity"] == 7
    dev.adjoint_tape_reserve_sparse_batch(0, 2)
    raw = np.zeros(8, dtype=np.int64)
    _lib.check(dev.lib.fc_adjoint_tape_info_batch(dev._h, raw))
    assert not raw[[0, 1, 2, 3, 4, 5, 7]].any(), raw  # zero bytes, no spacing
    assert dev.adjoint_batch_info(SLOT_BDF2)["tape_bytes"] == 0


def test_refusals_overflow_and_a_tape_that_does_not_hold_the_run(nlb):
    dev, k = nlb.dev, nlb.dev.batch_k
    u = 0.1 * np.random.default_rng(5).standard_normal((N_STEPS, k, dev.n_act))
    refused(INV, dev.adjoint_tape_reserve_sparse_batch, 7, -1, match="every must be in [0, 2^24]")
    refused(INV, dev.adjoint_tape_reserve_sparse_batch, -1, 2, match="capacity must be in [0, 2^24]")
    refused(INV, dev.adjoint_tape_reserve_sparse_batch, (1 << 24) + 1, 2, match="capacity must be in [0, 2^24]")
    dev.set_state_batch(*batch_state(nlb, k))
    dev.step_batch_begin(SLOT_BDF2, u[0], compute_energy=False)
    try:
        refused(INV, dev.adjoint_tape_reserve_sparse_batch, 7, 2, match="a step is in flight")
    finally:
        dev.step_batch_end()
    dev.adjoint_tape_reserve_sparse_batch(5, 2)
    refused(INV, dev.run_adjoint_batch, SLOT_BDF2, N_STEPS, None, None, match="the tape is not begun")
    dev.set_state_batch(*batch_state(nlb, k))
    dev.adjoint_tape_begin_batch()
    for m in range(N_STEPS):
        dev.step_batch(SLOT_BDF2, u[m], compute_energy=False)
    info = dev.adjoint_tape_info_batch()
    assert info["overflowed"] and info["count"] == 5 and info["lost"] == 2
    refused(INV, dev.run_adjoint_batch, SLOT_BDF2, N_STEPS, None, None, match="the tape overflowed: 7 steps since it was begun, capacity 5")
    dev.adjoint_tape_reserve_sparse_batch(0, 0)


def test_begin_batch_after_the_actuators_changed():
    """As the single tape's: the control tape holds KB rows of the reserve's actuators."""
    h = handle("9x9", 3)
    try:
        dev = h.dev
        dev.set_state_batch(*batch_state(h, 3))
        dev.adjoint_tape_reserve_sparse_batch(N_STEPS, 3)
        dev.adjoint_tape_begin_batch()
        dev.set_bc(h.dofs, mc.profiles(h.th, h.dofs, 3))
        refused(NOT_READY, dev.adjoint_tape_begin_batch, match="the actuators changed since fc_adjoint_tape_reserve_sparse_batch")
    finally:
        h.close()


def test_batch_info_counts_the_whole_checkpointed_tape(nlb):
    """fc_adjoint_batch_info's tape bytes are _info_batch's: buffer, pairs and control tape; the buffers a replay borrows (the ring's
    copy, a record page, the flags) exist from the reserve on and are part of the march bytes."""
    dev = nlb.dev
    dev.adjoint_tape_reserve_sparse_batch(0, 0)
    march0 = dev.adjoint_batch_info(SLOT_BDF2)["march_bytes"]
    dev.adjoint_tape_reserve_sparse_batch(N_STEPS, 3)
    info = dev.adjoint_batch_info(SLOT_BDF2)
    assert info["tape_bytes"] == dev.adjoint_tape_info_batch()["bytes"] > 0
    assert info["march_bytes"] > march0
    dev.adjoint_tape_reserve_sparse_batch(0, 0)
    assert dev.adjoint_batch_info(SLOT_BDF2)["march_bytes"] == march0


def test_the_batched_reserve_needs_a_batch():
    """Last in the module: it takes the batch of a handle of its own away."""
    h = handle("9x9", 3)
    try:
        h.dev.set_batch(0)
        refused(NOT_READY, h.dev.adjoint_tape_reserve_sparse_batch, 7, 2, match="fc_set_batch not called")
    finally:
        h.close()
