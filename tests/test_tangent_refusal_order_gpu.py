"""Which refusal of a tangent march wins where several conditions hold at once, and which order slots a march consults
(``fc_run_tangent``, ``fc_run_tangent_batch``, ``fc_run_tangent_closed_loop``; the shared preamble of csrc/fc_tangent_march.hpp, DESIGN
§5.6 "One skeleton").  The refusal tests of tests/test_tangent_gpu.py, _batch_gpu and _loop_gpu hold one condition at a time; a shared
preamble can change the order of two checks without any of them noticing.  The expectations are read off the entry points as they stood
before the four marches shared a preamble, and a library built from that commit (``FC_LIB_PATH``) passes the file as well.

The nonlinear 7 x 5 square of tests/support/adjoint_nl_child.py and the nonlinear closed-loop plant of tests/test_tangent_loop_gpu.py.
Every refused call leaves ``tangent_info()["marches"]`` as it was."""
import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_nl_child as nl_case
from tests.support import tangent_child as case

pytestmark = pytest.mark.gpu

INV, NOT_READY = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
K = 3


@pytest.fixture(scope="module")
def square():
    sq = nl_case.NlSquare()
    yield sq
    sq.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    yield p
    p.close()


def refused(dev, code, match, fn, *args):
    marches = dev.tangent_info()["marches"]
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code and match in str(e.value), str(e.value)
    assert dev.tangent_info()["marches"] == marches, "a refused call counted as a march"


def test_single_march(square):
    """fc_run_tangent: the reserve before the call's arguments, the arguments before the scheme, the scheme before the tape, the tape
    and the slots' right-hand-side operator before the solver method -- and a march of ONE step from BDF1 never looks at BDF2."""
    dev = square.dev
    rng = np.random.default_rng(23)
    u, du = rng.standard_normal((3, dev.n_act)), rng.standard_normal((1, dev.n_act))
    d0, dm1 = rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    rhs_operator = (0.5 * square.model.M)[:, : 2 * dev.nn]
    dev.adjoint_tape_reserve(6)
    try:
        # the reserve freed, and n_steps = 0
        refused(dev, NOT_READY, "no tangent buffers", dev.run_tangent, SLOT_BDF1, 0)
        dev.tangent_reserve(1)
        # a linearised scheme: n_steps = 0; the state tape not begun
        dev.set_time_scheme(square.dt, False)
        refused(dev, INV, "n_steps must be positive", dev.run_tangent, SLOT_BDF1, 0)
        assert not dev.adjoint_tape_info()["begun"]
        refused(dev, INV, "its own tangent", dev.run_tangent, SLOT_BDF1, 3)
        dev.set_time_scheme(square.dt, True)
        try:
            # nonlinear, the tape not begun, and a Krylov method selected
            dev.set_solver_options(refine=30, method="gmres")
            assert not dev.adjoint_tape_info()["begun"]
            refused(dev, INV, "not begun", dev.run_tangent, SLOT_BDF1, 3)
            # an explicit right-hand-side operator on BDF2, and the Krylov method, n = 3
            dev.set_solver_options(refine=1, check_residual=1)
            case.taped_run(square, 1, 3, u)
            dev.set_rhs_operator(SLOT_BDF2, rhs_operator)
            dev.set_solver_options(refine=30, method="gmres")
            refused(dev, INV, "Crank-Nicolson", dev.run_tangent, SLOT_BDF1, 3)
        finally:
            dev.set_solver_options(refine=1, check_residual=1)
            dev.set_rhs_operator(SLOT_BDF2, None)
        # a taped run of ONE step from BDF1 while BDF2 carries the operator: accepted, and the march without the operator's bits
        case.taped_run(square, 1, 1, u[:1])
        plain = dev.run_tangent(SLOT_BDF1, 1, du, d0, dm1)
        dev.set_rhs_operator(SLOT_BDF2, rhs_operator)
        try:
            marches = dev.tangent_info()["marches"]
            with_operator = dev.run_tangent(SLOT_BDF1, 1, du, d0, dm1)
            assert dev.tangent_info()["marches"] == marches + 1
        finally:
            dev.set_rhs_operator(SLOT_BDF2, None)
        assert np.any(plain[0]) and all(np.array_equal(a, b) for a, b in zip(plain, with_operator))
    finally:
        dev.tangent_reserve(0)
        dev.adjoint_tape_reserve(0)
        dev.set_time_scheme(square.dt, True)
        square.restart()


def test_closed_loop_march(nl_plant):
    """fc_run_tangent_closed_loop: the call's arguments before the loop tape, the loop tape before the state tape of a nonlinear plant."""
    p, dev = nl_plant, nl_plant.dev
    loop, *_ = lc.make_case(p.model, p.x0, p.xm1, 1, 3, limits=False)
    lc.put_loop(dev, loop)
    dev.tangent_reserve(1)
    try:
        dev.adjoint_loop_reserve(0)
        dev.adjoint_tape_reserve(0)
        assert dev.adjoint_loop_info()["capacity"] == 0 and dev.adjoint_tape_info()["bytes"] == 0
        refused(dev, INV, "n_steps", dev.run_tangent_closed_loop, SLOT_BDF1, 0)
        refused(dev, NOT_READY, "no loop tape", dev.run_tangent_closed_loop, SLOT_BDF1, 3)
    finally:
        dev.tangent_reserve(0)


def test_batched_march(square):
    """fc_run_tangent_batch, k = 3: the range of ref_col before the batched state tape; the reserve before the range of ref_col.

    The second case was meant to hold buffers reserved for the single mode against a batch -- FC_ERR_NOT_READY, "reserved for another mode" --
    but no sequence of calls leaves such a reserve: fc_set_batch drops the buffers of the mode it ends, so the handle answers
    FC_ERR_NOT_READY, "no tangent buffers".  The code and the condition it wins against (ref_col = k) are pinned as asked."""
    dev = square.dev
    args = (SLOT_BDF2, 3, None, None, None, K)  # ref_col = k
    dev.set_solver_options(refine=0, check_residual=1)
    try:
        dev.set_batch(K)
        dev.adjoint_tape_reserve_batch(6)
        dev.tangent_reserve(1)
        assert dev.tangent_info()["KB"] == 4 and not dev.adjoint_tape_info_batch()["begun"]
        refused(dev, INV, "ref_col", dev.run_tangent_batch, *args)
        # buffers reserved for the single mode, then the batch
        dev.adjoint_tape_reserve_batch(0)
        dev.set_batch(0)
        dev.tangent_reserve(1)
        assert dev.tangent_info()["reserved"] and dev.tangent_info()["KB"] == 0
        dev.set_batch(K)
        refused(dev, NOT_READY, "no tangent buffers", dev.run_tangent_batch, *args)
    finally:
        dev.tangent_reserve(0)
        dev.adjoint_tape_reserve_batch(0)
        dev.set_batch(0)
        dev.set_solver_options(refine=1, check_residual=1)
        square.restart()
