"""The backward (adjoint) march on every kernel route, single and batched -- the right-hand side in front of the transposed sweeps (the
forward element loops on the two masked levels, fc_adj_elem_nl / _reg / _b, fc_adj_rhs_gather, fc_adj_rhs_gather_b), the control columns
(fc_adj_control_columns) and the tail behind the sweeps (fc_adj_tail, fc_adj_tail_b, fc_adj_reduce, fc_adj_reduce_b) -- kernel by kernel
against a host model in np.longdouble that is fed the device's OWN inputs (fc_debug_get_adjoint_stage), so that no error of the solve
leaks into a kernel's tolerance.

The meshes, actuator sets, sensor sets and runs are those of tests/support/adjoint_march_cases.py; tests/test_adjoint_march_cases_host.py
shows that together they reach every branch label outside UNREACHED.  fc_get_adjoint_route tells what a backward step launched: a route
the host model predicts and the device did not take fails the test.  Handle knobs (FC_ELEM_REG_MIN) and the tape knob (FC_ADJ_TAPE_NT) are
read when a handle / a tape is made: a fresh handle per run, in this process.

Tolerances, per quantity (tests/support/adjoint_march_child.py holds the checks):
  route       equal to the prediction
  bt          Dirichlet rows: the profile, bit for bit; elsewhere 2 eps (|lift| + |F|) on the device's own lift and load vectors (the one
              add; in fact bit for bit their fp64 sum); those operands: (L + 2) eps sum |a g| (the lifting's row sum, any order) and
              16 x HOST_RHS_ERROR max-norm (the step tests' tolerance of a device load vector)
  b           16 x HOST_ADJ_RHS_ERROR (2-norm, max-norm over the velocity rows), measured by tests/test_adjoint_march_cases_host.py; rows
              where only C^T w and the terminal vector contribute: (n_entries + 2) eps (sum |c w| + |term|) -- derived; on a first
              backward step (both levels zero) every row is the sensor table's chain of adds in the order the source states, bit for bit
  mu          16 x HOST_BLOCK_SOLVE_ERROR of tests/test_batch_apply_gpu.py, against a refined transposed host solve of the device's b
  zm          the masked mu, bit for bit; padding columns of a batch exactly zero
  partial     2 (rows in the share + 8) eps sum |bt| |mu| -- derived, holds for any summation order
  g           2 (N + 2) eps sum |bt| |mu| against the longdouble dot product; bit for bit the fold of the downloaded partials in the
              order the source states (lane l takes l, l + 64, .., then the shuffle tree)"""
import numpy as np
import pytest

from tests.support import adjoint_march_cases as mc
from tests.test_batch_apply_gpu import HOST_BLOCK_SOLVE_ERROR
from tests.test_step_routes_gpu import HOST_RHS_ERROR

pytestmark = pytest.mark.gpu

# The device may miss a host constant by 16 times: the project's margin for another fixed summation order.
TOLERANCES = {"rhs": [16 * mc.HOST_ADJ_RHS_ERROR[0], 16 * mc.HOST_ADJ_RHS_ERROR[1]], "solve": 16 * HOST_BLOCK_SOLVE_ERROR, "load": 16 * HOST_RHS_ERROR[1]}


@pytest.fixture(scope="module")
def worst():
    from tests.support import adjoint_march_child as child

    child.TOL.update(TOLERANCES)
    w = child.Worst()
    yield w
    w.report()
    child.report_elem_pairs()


@pytest.mark.parametrize("run", mc.SINGLE_RUNS, ids=mc.run_name)
def test_single_march_against_the_longdouble_host_model(run, worst):
    """Every backward step of the run: route, bt, b, mu, zm, partial, g; two identical marches bit-identical; FC_ADJ_TAPE_NT=0 and the
    default bit-equal (nonlinear runs); a NaN in the terminal vector raises the flag and zm is still written (linearised runs)."""
    from tests.support import adjoint_march_child as child

    child.check_single(run, worst)


@pytest.mark.parametrize("run", mc.BATCH_RUNS, ids=mc.run_name)
def test_batched_march_against_the_longdouble_host_model(run, worst):
    """The last backward step of the marches of every length, column by column against the same model within the same bounds as the
    single march, and every column against the single march of the same inputs on a handle without a batch (the inputs' differences
    carried through the model); two identical batched marches bit-identical; equal columns bit-equal; padding columns exactly zero and
    without output; a NaN column raises its own flag alone."""
    from tests.support import adjoint_march_child as child

    child.check_batch(run, worst)


def test_the_two_test_aids_error_paths():
    """fc_get_adjoint_route / fc_debug_get_adjoint_stage: status codes for a null handle, a null or short buffer and a handle that has
    not marched yet; nothing is written on an error; a mass product makes the stage's right-hand side FC_ERR_NOT_READY and leaves the
    route alone; releasing the transposed factors ends the record."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY, FcError, ptr
    from flowcontrol_amd.device import DeviceSolver
    from tests.support import adjoint_march_child as child

    h = child.Handle("5x3", 2, "dirichlet", "one", "default", False, 0)
    try:
        dev = h.dev
        lib, hd = dev.lib, dev._h
        n = len(DeviceSolver.ADJ_ROUTE_COLS)
        assert DeviceSolver.ADJ_ROUTE_COLS == mc.ROUTE_COLS and DeviceSolver.ADJ_ELEM == mc.ELEM_NAMES and n == 12
        buf = np.full(16, -7, dtype=np.int32)
        assert lib.fc_get_adjoint_route(None, buf.size, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_adjoint_route(hd, buf.size, None) == FC_ERR_INVALID
        assert lib.fc_get_adjoint_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert b"no backward step yet" in lib.fc_last_error()
        assert lib.fc_debug_get_adjoint_stage(hd, 0, 1, *([None] * 11)) == FC_ERR_NOT_READY
        assert lib.fc_debug_get_adjoint_stage(None, 0, 1, *([None] * 11)) == FC_ERR_INVALID
        dev.adjoint_reset(np.ones(dev.N))
        assert lib.fc_get_adjoint_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # a reset alone is no step
        dev.step_adjoint(h.slot_of[2], 0.0, 0.0, np.ones(1))
        assert lib.fc_get_adjoint_route(hd, n - 1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_adjoint_route(hd, -1, ptr(buf)) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error
        assert lib.fc_get_adjoint_route(hd, buf.size, ptr(buf)) == 0 and np.all(buf[n:] == -7)
        want = mc.predicted_route("5x3", 2, 1, {}, False, True, True)
        assert np.array_equal(dev.adjoint_route(), want) and np.array_equal(buf[:n], want)
        assert lib.fc_debug_get_adjoint_stage(hd, 0, 2, *([None] * 11)) == FC_ERR_INVALID  # gx is not the step's
        assert lib.fc_debug_get_adjoint_stage(hd, 4, 1, *([None] * 11)) == FC_ERR_INVALID  # nor is the width
        st = dev.adjoint_stage()
        assert st["b"].shape == (dev.N,) and st["partial"].shape == (2, 1) and st["bt"].shape == (2, dev.N) and not st["refined"]
        assert st["lift"].shape == (2, dev.N) and st["fvec"] is None
        dev.adjoint_mass_product(1.0, 0.0)  # overwrites the right-hand side: the stage says so, the route stays the step's
        assert np.array_equal(dev.adjoint_route(), want)
        with pytest.raises(FcError) as e:
            dev.adjoint_stage()
        assert e.value.code == FC_ERR_NOT_READY and "mass product" in str(e.value)
        again = dev.adjoint_stage(rhs=False)
        assert again["b"] is None and all(np.array_equal(again[q], st[q]) for q in ("mu", "zm", "zm_prev", "partial", "bt", "lift"))
        for s in h.slot_of.values():
            dev.set_adjoint_factors(s, -1)
        assert lib.fc_debug_get_adjoint_stage(hd, 0, 1, *([None] * 11)) == FC_ERR_NOT_READY
    finally:
        h.close()
