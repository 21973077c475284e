"""The energy term of the adjoint marches' cost on the MI355X (``fc_set_adjoint_energy``; csrc/fc_adjoint_energy.hip.h and the EN
instantiations of csrc/fc_adjoint_nl.hip.h / csrc/fc_adjoint_batch.hip.h): every check runs tests/support/adjoint_energy_child.py in a
fresh child process on the small squares of tests/support/adjoint_march_cases.py -- "5x3" (30 cells: one ragged workgroup of the lanes
kernel), "9x9" (162 cells: a ragged last workgroup at 32 and at 8 cells per workgroup) and "12x7".

Bounds.  ``b``: 16 x HOST_ADJ_EN_RHS_ERROR (2-norm, max-norm over the velocity rows), the bound tests/test_adjoint_march_gpu.py uses for
``b`` fed with the constant tests/test_adjoint_energy_host.py measures for the three-operand right-hand side.  Central differences of the
device's own cost: the step and the 1e-6 of the sibling test of each march (open loop 1e-4, closed loop 2e-5) -- larger than ten times the
host-measured model distance everywhere but on the nonlinear closed loop, where ten times that distance, 4.6e-6, is used
(adjoint_energy_cases.fd_tol).  A batched column against the single march of that run: the sibling tests' 1e-8."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _child(*args, env=None):
    e = dict(os.environ, PYTHONPATH=str(ROOT))
    e.pop("FC_ELEM_REG_MIN", None)  # (the handle sets of adjoint_march_cases set it themselves, per handle)
    e.update(env or {})
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "adjoint_energy_child.py"), *args], env=e, capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    print(out.stdout[-4000:])
    assert out.returncode == 0, f"child {args}: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert "CHILD OK " + " ".join(args) in out.stdout


@pytest.mark.parametrize("kind", ["lin", "nl"])
@pytest.mark.parametrize("route", ["lanes", "reg", "b4", "b16", "b32"])
def test_one_backward_step_per_route(route, kind):
    """1. The last backward step of a three-step march with weights held -- both masked levels live, cm_n mu_2 + cm_nn mu_3, next to
    e_1 x_1: lanes, thread per cell (FC_ELEM_REG_MIN=1), batched at KB 4 / 16 / 32 (k = 3, 9, 32), linearised and nonlinear.  ``b`` of
    fc_debug_get_adjoint_stage against the longdouble model fed the device's own two masked levels and taped state (every column of a
    batch), route entry [0] the new code with the old grids, fc_adjoint_energy_info the rows, bytes and step count; the model with the
    older level or the term left out, or with the mask on x, misses by 1e6 bounds."""
    _child("step", route, kind)


@pytest.mark.parametrize("kind", ["lin", "nl"])
@pytest.mark.parametrize("march", ["single", "batch", "loop", "loopb"])
def test_gradient_against_central_differences_of_the_device_cost(march, kind):
    """2. Each of the four marches on "9x9": n = 5 from a BDF1 first step, two actuators, distinct e_m with one zero, Q and R non-zero.
    The gradient (open loop: controls and initial state; closed loop: every matrix of the bank, the feedback map and the controller's
    initial state) against central differences of the device's own forward cost, its dE series included; every batched column (k = 3)
    against the single march of that run on a handle without a batch; two identical marches bit-identical."""
    _child("e2e", march, kind)


def test_opt_in():
    """3. On a handle that never set weights, and again after clearing them, g / dx0 / dxm1 are bit-identical to a march made before the
    weights were set; route [0] shows the old codes; fc_adjoint_energy_info reports 0 bytes; the device state, the tape's step count and
    the forward run that follows are untouched by the march with weights.  (The solvers' step counter and log, which a device handle
    does not have: test_energy_keyword_on_the_solvers.)"""
    _child("optin")


@pytest.mark.parametrize("kind", ["lin", "nl"])
@pytest.mark.parametrize("solver", ["single", "batched"])
def test_energy_keyword_on_the_solvers(solver, kind):
    """3 (continued) and the Python layer.  On a linearised and a nonlinear FlowSolver / BatchedFlowSolver (k = 3) of the 9 x 9 cavity that
    has stepped, so that it has a counter and a log: cost_gradient and closed_loop_gradient, the four flu functions and the AdjointRun.run*
    marches with ``energy=`` (per step, per column, a scalar, one row set for all columns).  J equals the device's own forward cost,
    its dE series included, to 1e-12; the gradients equal, bit for bit, the device-level march with the rows held (the march section 2
    holds against central differences) and differ from the march without weights; ``energy=None`` is the call without the keyword bit for
    bit; after every call the state, the iteration counter, the time, the order, the time-series log and the controllers' states are
    what they were, fc_adjoint_energy_info reports 0 bytes and no tape is left reserved -- on the linearised solver too, whose run
    was taped for the call.  The single solver also runs two iterations of the descent example on the reference's J (cost="energy")."""
    _child("solver", solver, kind)


def test_refusals():
    """4. Rows with another n_steps or k, rows of the other kind, a linearised handle without a covering tape (none, not begun, another
    length), fc_step_adjoint with rows held, a non-finite weight: FC_ERR_INVALID (FC_ERR_NOT_READY without a batch) and the message."""
    _child("refusals")


def test_partitioned_handle_is_refused():
    """4 (continued). A thread-rank (host exchange) handle takes no energy rows."""
    _child("partitioned")


def test_cost_helper_equals_closed_loop_costs():
    """5. optim.closed_loop_cost_gradients(signal="dE") on a 9 x 9 square with two candidates, both criteria, u_penalty = 0.3: J equals
    closed_loop_costs(on_device=True) to 1e-12 relative (both are sums of the same device series), the initial row's share included."""
    _child("cost")
