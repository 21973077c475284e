"""The adjoint of the NONLINEAR stepper on the MI355X (``fc_adjoint_tape_reserve`` / ``_begin``, ``fc_run_adjoint`` on a taped run;
csrc/fc_adjoint_nl.hip.h, csrc/fc_adjoint_segments.hpp, flowcontrol_amd/adjoint.py) against the scipy model of
tests/support/adjoint_nl_model.py.

Small problem: the nonlinear 7 x 5 square (N = 378, 70 cells, two Dirichlet actuators, one point sensor) with both order slots set
up; the FlowSolver level runs on the cylinder's O1 mesh."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, FcError
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.flowsolverparameters import ParamIC
from tests.support import adjoint_nl_child as case

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SLOTS = (SLOT_BDF1, SLOT_BDF2)
INV = _lib.FC_ERR_INVALID


@pytest.fixture(scope="module")
def square():
    sq = case.NlSquare()
    yield sq
    sq.close()


@pytest.fixture()
def adj(square):
    """Transposed factors of both slots for one test; they and whatever tape the test reserved are released afterwards."""
    for s in SLOTS:
        square.dev.set_adjoint_factors(s, 1)
    yield square
    square.dev.adjoint_tape_reserve(0)
    for s in SLOTS:
        square.dev.set_adjoint_factors(s, -1)
    square.dev.set_time_scheme(square.dt, True)
    square.restart()


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


@pytest.mark.parametrize("first_order,n", case.CASES)
def test_taped_run_and_adjoint_against_the_model(adj, first_order, n):
    """1. The taped device forward run equals the model's to 1e-8; g, dx0, dxm1 within 1e-8 relative of the model; the directional
    derivative against central differences of the device's own forward run (eps = 1e-4) <= 1e-6; two identical marches bit-identical.
    70 cells: the last workgroup of the eight-lane kernel is partial.  (Measured defects: DESIGN section 5.4.)"""
    assert adj.th.mesh.cells.shape[0] == 70 and adj.dev.N == 378
    adj.dev.adjoint_tape_reserve(6)
    out = case.compare_run(adj, first_order, n)
    if first_order == 2:
        assert out["dxm1"] > 0.0


def test_thread_per_cell_kernel():
    """2. The same comparison in a fresh child process with FC_ELEM_REG_MIN=1: the march runs fc_adj_elem_nl_reg."""
    env = dict(os.environ, FC_ELEM_REG_MIN="1", PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "adjoint_nl_child.py"), "reg"], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    for ln in out.stdout.splitlines():
        if ln.startswith("nonlinear adjoint run"):
            print(ln)
    assert out.returncode == 0, f"child: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK reg" in out.stdout


def test_tape_semantics(adj):
    """3. No tape, a count that differs from n_steps, an overflowed tape, a wrong first slot and a set_state between the forward and
    the backward run are each refused with their reason; step + undo_step + step tapes the columns of two clean steps."""
    dev = adj.dev
    rng = np.random.default_rng(3)
    u = rng.standard_normal((8, dev.n_act))
    z = rng.standard_normal(dev.N)
    refused(INV, dev.run_adjoint, SLOT_BDF1, 4, None, z, match="nonlinear")  # no tape
    refused(_lib.FC_ERR_NOT_READY, dev.adjoint_tape_begin)
    refused(INV, dev.step_adjoint, SLOT_BDF2, 1.0, 0.0, match="nonlinear")
    dev.adjoint_tape_reserve(6)
    assert dev.adjoint_tape_info() == {"capacity": 6, "count": 0, "overflowed": False, "bytes": 8 * dev.N * 8, "begun": False, "lost": 0}
    # reserved, not begun: steps are not taped
    dev.run(SLOT_BDF1, 2, u[:2])
    assert dev.adjoint_tape_info()["count"] == 0
    refused(INV, dev.run_adjoint, SLOT_BDF1, 2, None, z, match="not begun")
    # count != n_steps
    adj.restart()
    dev.adjoint_tape_begin()
    dev.run(SLOT_BDF1, 4, u[:4])
    refused(INV, dev.run_adjoint, SLOT_BDF1, 6, None, z, match="holds 4 steps")
    refused(INV, dev.run_adjoint, SLOT_BDF1, 6, None, z, match="nonlinear")
    refused(INV, dev.run_adjoint, SLOT_BDF1, 6, None, z, match="fc_adjoint_tape_reserve")
    # a wrong first slot
    refused(INV, dev.run_adjoint, SLOT_BDF2, 4, None, z, match="first taped step")
    dev.run_adjoint(SLOT_BDF1, 4, None, z)
    # overflow: the run goes on, nothing more is written, the march is refused
    dev.run(SLOT_BDF2, 4, u[4:])
    info = dev.adjoint_tape_info()
    assert info["overflowed"] and info["count"] == 6 and info["lost"] == 2
    refused(INV, dev.run_adjoint, SLOT_BDF1, 8, None, z, match="overflowed")
    refused(INV, dev.run_adjoint, SLOT_BDF1, 6, None, z, match="overflowed")
    # a set_state between the forward and the backward run
    adj.restart()
    dev.adjoint_tape_begin()
    dev.run(SLOT_BDF1, 3, u[:3])
    adj.restart()
    assert not dev.adjoint_tape_info()["begun"]
    refused(INV, dev.run_adjoint, SLOT_BDF1, 3, None, z, match="not begun")
    # step + undo_step + step
    dev.adjoint_tape_begin()
    dev.step(SLOT_BDF1, u[0])
    dev.step(SLOT_BDF2, u[1])
    clean = dev.adjoint_tape_states()
    adj.restart()
    dev.adjoint_tape_begin()
    dev.step(SLOT_BDF1, u[0])
    dev.step(SLOT_BDF2, u[5])
    assert dev.adjoint_tape_info()["count"] == 2
    dev.undo_step()
    assert dev.adjoint_tape_info()["count"] == 1
    dev.step(SLOT_BDF2, u[1])
    again = dev.adjoint_tape_states()
    assert again.shape == (4, dev.N) and np.array_equal(again, clean)
    assert not np.array_equal(clean[2], clean[3])
    g1 = dev.run_adjoint(SLOT_BDF1, 2, None, z)
    assert np.all(np.isfinite(g1[0]))


def test_nothing_else_moved(square):
    """4. A nonlinear forward series (y, dE, state) is bit-identical without a tape, with a tape that records it, and after the release;
    a linearised run_adjoint is bit-identical with and without a reserved tape; the bytes the info calls report return to zero."""
    dev = square.dev
    u = np.random.default_rng(4).standard_normal((9, dev.n_act))

    def series(begin=False):
        square.restart()
        if begin:
            dev.adjoint_tape_begin()
        y, dE = dev.run(SLOT_BDF1, 5, u[:5])
        y2, dE2, _ = dev.step(SLOT_BDF2, u[5])
        y3, dE3 = dev.run(SLOT_BDF2, 3, u[6:])
        return np.vstack([y, y2[None, :], y3]), np.r_[dE, dE2, dE3], [np.array(a, copy=True) for a in dev.get_state()]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))

    before = series()
    assert dev.adjoint_tape_info()["bytes"] == 0 and all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
    dev.adjoint_tape_reserve(9)
    try:
        assert dev.adjoint_tape_info()["bytes"] == 8 * dev.N * 11
        assert dev.adjoint_info(SLOT_BDF2)["shared_bytes"] == 8 * dev.N * 11  # (no march buffers yet: the tape alone)
        assert same(before, series(begin=True))
        assert dev.adjoint_tape_info()["count"] == 9
        assert same(before, series(begin=False))  # reserved, ended by the set_state: nothing is taped
        assert dev.adjoint_tape_info()["count"] == 0
    finally:
        dev.adjoint_tape_reserve(0)
    assert dev.adjoint_tape_info()["bytes"] == 0 and dev.adjoint_info(SLOT_BDF2)["bytes"] == 0
    assert same(before, series())
    # the linearised march does not see the tape
    rng = np.random.default_rng(6)
    w, z = rng.standard_normal((5, dev.n_sens)), rng.standard_normal(dev.N)
    dev.set_time_scheme(square.dt, False)
    try:
        for s in SLOTS:
            dev.set_adjoint_factors(s, 1)
        plain = dev.run_adjoint(SLOT_BDF1, 5, w, z)
        dev.adjoint_tape_reserve(3)
        dev.adjoint_tape_begin()
        dev.run(SLOT_BDF1, 2, u[:2])
        taped = dev.run_adjoint(SLOT_BDF1, 5, w, z)  # (a tape of another run: a linearised march never asks)
        assert all(np.array_equal(a, b) for a, b in zip(plain, taped))
    finally:
        dev.adjoint_tape_reserve(0)
        for s in SLOTS:
            dev.set_adjoint_factors(s, -1)
        dev.set_time_scheme(square.dt, True)
        square.restart()
    assert dev.adjoint_tape_info()["bytes"] == 0 and all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)


# ── FlowSolver level: the nonlinear cylinder on O1 ──────────────────────────────────────────────────────────────────────────────
def test_flowsolver_cost_gradient_against_central_differences(golden_dir):
    """5. FlowSolver.cost_gradient on the nonlinear cylinder (O1, 20 steps) against central differences of the forward device run in
    three random directions at eps = 1e-4: 1e-6 relative (J is not quadratic in u: truncation error remains).  The state is left where
    it was, the tape and the adjoint setup are released.  (Measured defects: DESIGN section 5.4.)"""
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.params_solver.is_eq_nonlinear = True
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        n = 20
        rng = np.random.default_rng(20)
        u = 0.5 * rng.standard_normal((n, dev.n_act))
        Q = np.diag(1.0 + np.arange(dev.n_sens))
        R = 0.1 * np.eye(dev.n_act)
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2

        def cost(uu):
            y, _ = dev.run(slot, n, uu, compute_energy=False)
            dev.set_state(*state0)
            return 0.5 * (np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", uu, R, uu))

        J, grad = fs.cost_gradient(u, Q, R)
        assert all(np.array_equal(a, b) for a, b in zip(state0, dev.get_state()))
        assert dev.adjoint_tape_info()["bytes"] == 0 and all(dev.adjoint_info(s)["bytes"] == 0 for s in SLOTS)
        assert abs(J - cost(u)) <= 1e-12 * abs(J)
        eps, worst = 1e-4, 0.0
        for k in range(3):
            d = rng.standard_normal(u.shape)
            fd = (cost(u + eps * d) - cost(u - eps * d)) / (2 * eps)
            ad = float(np.sum(grad * d))
            err = abs(fd - ad) / abs(fd)
            worst = max(worst, err)
            print(f"O1 nonlinear, 20 steps: J = {J:.6e}, direction {k}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.3e}")
        assert worst <= 1e-6
        # the linear adjoint is not this gradient: the convective term acts on O1 too
        assert np.linalg.norm(grad) > 0.0
    finally:
        fs.th.release_device()
