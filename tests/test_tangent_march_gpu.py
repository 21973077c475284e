"""The tangent-linear march on every kernel route, single and batched -- the element loops fc_tan_elem_nl / _reg / _b<KB, SHARED>, the
forward step's gathers with the control columns (fc_rhs_gather, fc_rhs_gather_b<KB>, fc_tan_force_b<KB>) and the tails fc_tan_tail /
fc_tan_tail_b<KB> -- kernel by kernel against a host model in np.longdouble that is fed the device's OWN inputs
(fc_debug_get_tangent_stage, the state tape), so that no error of a solve leaks into a kernel's tolerance.

The meshes, actuator sets, sensor sets and runs are those of tests/support/tangent_march_cases.py; tests/test_tangent_march_cases_host.py
shows that together they reach every label outside UNREACHED.  fc_get_tangent_route tells what a tangent step launched: a route the host
model predicts and the device did not take fails the test.  FC_ELEM_REG_MIN is read when a handle is made: a fresh handle per run, in
this process.

Tolerances, per quantity (tests/support/tangent_march_child.py holds the checks):
  route       equal to the prediction
  ev, b       16 x HOST_TAN_RHS_ERROR (2-norm, max-norm; b over the velocity rows, on the device's own lift and load vectors), measured by
              tests/test_tangent_march_cases_host.py; Dirichlet rows of b: (n_act + 2) eps sum |prof| |du| -- derived; free rows against
              the sum of the device's own element vectors, lift and load-vector terms: (cells + 2 n_act + 2) eps sum |terms| -- derived,
              any order; pressure rows exactly 0 without controls (they hold -lift du otherwise, inside the bound above); the operands:
              lift (L + 2) eps sum |a g| against the device's raw operator, load vectors 16 x HOST_RHS_ERROR max-norm
  x           16 x HOST_BLOCK_SOLVE_ERROR of tests/test_batch_apply_gpu.py, against a refined host solve of the device's b (the y half of
              the work buffer is the sweeps' input and is consumed by them: a y that is not b shows here)
  new level   x + dx (one fp64 add) or x, bit for bit, Dirichlet and pressure rows included; the other level is left alone
  dy          (entries + 2) eps sum |c| |x + dx| per sensor -- derived; no row without sensors
  batched     every column within the same bounds of the single model of its inputs; equal columns bit-equal; padding columns exactly
              zero in ev, b, x, the levels and du, and without a row in dy; SHARED: the model fed column ref_col's trajectory, and at
              least 1000 x the tolerance away from the model fed the column's own; a NaN column raises its own flag alone
  elem forms  eight-lane against thread-per-cell, single against batched on the same inputs: printed in ulps, not asserted"""
import numpy as np
import pytest

from tests.support import tangent_march_cases as tc
from tests.test_batch_apply_gpu import HOST_BLOCK_SOLVE_ERROR
from tests.test_step_routes_gpu import HOST_RHS_ERROR

pytestmark = pytest.mark.gpu

# The device may miss a host constant by 16 times: the project's margin for another fixed summation order.
TOLERANCES = {"rhs": [16 * tc.HOST_TAN_RHS_ERROR[0], 16 * tc.HOST_TAN_RHS_ERROR[1]], "solve": 16 * HOST_BLOCK_SOLVE_ERROR, "load": 16 * HOST_RHS_ERROR[1]}


@pytest.fixture(scope="module")
def worst():
    from tests.support import tangent_march_child as child

    child.TOL.update(TOLERANCES)
    w = child.Worst()
    yield w
    w.report()
    child.report_elem_pairs()


@pytest.mark.parametrize("run", tc.SINGLE_RUNS, ids=tc.run_name)
def test_single_march_against_the_longdouble_host_model(run, worst):
    """The last step of the marches of every length: route, operands, ev, b, x, the new level, dy; two identical marches bit-identical."""
    from tests.support import tangent_march_child as child

    child.check_single(run, worst)


@pytest.mark.parametrize("run", tc.BATCH_RUNS, ids=tc.run_name)
def test_batched_march_against_the_longdouble_host_model(run, worst):
    """The same column by column within the single model's bounds; equal columns bit-equal; padding columns exactly zero; SHARED reads
    ref_col's trajectory; a NaN column raises its own flag alone and the others keep their bits."""
    from tests.support import tangent_march_child as child

    child.check_batch(run, worst)


def test_the_tail_reads_the_correction_of_a_refined_solve(worst):
    """fc_tan_tail's level and its sensors both read x + dx, on a dx that is no rounding effect (operator replaced behind its factors)."""
    from tests.support import tangent_march_child as child

    child.check_tail_reads_dx(worst)


def test_the_two_test_aids_error_paths():
    """fc_get_tangent_route / fc_debug_get_tangent_stage: status codes for a null handle, a null or short buffer, a handle that has not
    marched yet and another width; nothing is written on an error; fc_tangent_reserve ends the record."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY, ptr
    from flowcontrol_amd.device import DeviceSolver
    from tests.support import step_cases as sc
    from tests.support import tangent_march_child as child

    h = child.Handle("5x3", 2, "dirichlet", "one", "default", 0, 1)
    try:
        dev = h.dev
        lib, hd = dev.lib, dev._h
        n = len(DeviceSolver.TAN_ROUTE_COLS)
        assert DeviceSolver.TAN_ROUTE_COLS == tc.ROUTE_COLS and n == 14
        buf = np.full(20, -7, dtype=np.int32)
        none13 = [None] * 13
        assert lib.fc_get_tangent_route(None, buf.size, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_tangent_route(hd, buf.size, None) == FC_ERR_INVALID
        assert lib.fc_get_tangent_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert b"no tangent step yet" in lib.fc_last_error()
        assert lib.fc_debug_get_tangent_stage(hd, 0, *none13) == FC_ERR_NOT_READY
        assert lib.fc_debug_get_tangent_stage(None, 0, *none13) == FC_ERR_INVALID
        dev.set_state(*sc.initial_state(h.th, 1))
        dev.adjoint_tape_begin()
        dev.run(h.slot_of[2], 1, np.zeros((1, 2)), compute_energy=False)
        assert lib.fc_get_tangent_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # a taped forward run is no tangent step
        dy, dxn, dxnm1 = dev.run_tangent(h.slot_of[2], 1, np.ones((1, 2)), np.ones(dev.N), None)
        assert lib.fc_get_tangent_route(hd, n - 1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_tangent_route(hd, -1, ptr(buf)) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error
        assert lib.fc_get_tangent_route(hd, buf.size, ptr(buf)) == 0 and np.all(buf[n:] == -7)
        want = tc.predicted_route("5x3", 2, "dirichlet", {}, 2)
        assert np.array_equal(dev.tangent_route(), want) and np.array_equal(buf[:n], want)
        assert dev.tangent_info()["route"] == want[0]
        assert lib.fc_debug_get_tangent_stage(hd, 4, *none13) == FC_ERR_INVALID  # the width is not the step's
        assert lib.fc_debug_get_tangent_stage(hd, 0, *none13) == 0  # every output may be null
        st = dev.tangent_stage()
        nc = h.th.mesh.cells.shape[0]
        assert st["ev"].shape == (12, nc) and st["b"].shape == (dev.N,) and st["du"].shape == (2,) and st["dy"].shape == (1,) and not st["refined"]
        assert st["lift"].shape == (2, dev.N) and st["fvec"] is None and st["dx"] is None and st["flags"].shape == (32,)
        assert np.array_equal(st["dy"], dy[0]) and np.array_equal(h.to_w(st["new"]), dxn) and np.array_equal(h.to_w(st["other"]), dxnm1)
        assert np.array_equal(dxnm1, np.ones(dev.N))  # the level the step did not own, pressure and Dirichlet rows as the caller gave them
        dev.tangent_reserve(1)  # lays the buffers out again: the record ends
        assert lib.fc_get_tangent_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert lib.fc_debug_get_tangent_stage(hd, 0, *none13) == FC_ERR_NOT_READY
        dev.tangent_reserve(0)
        assert lib.fc_get_tangent_route(hd, buf.size, ptr(buf)) == FC_ERR_NOT_READY
    finally:
        h.close()


def test_a_handle_that_never_calls_the_aids_marches_the_same():
    """The record costs no launch and changes no bit: a march read through both aids and a march nobody looks at return the same arrays,
    leave the same tangent_info route and the same sweep_launches; a march behind the aids' calls is again the same."""
    from tests.support import step_cases as sc
    from tests.support import tangent_march_child as child

    def observe(look: bool):
        h = child.Handle("9x9", 2, "mixed", "five", "default", 1, 3)
        try:
            dev = h.dev
            du, d0, dm1 = tc.inputs(dev.N, 2, 3, 11)
            u = 0.1 * np.random.default_rng(1).standard_normal((3, 2))
            outs = []
            for rep in range(2):
                dev.set_state(*sc.initial_state(h.th, 1))
                dev.adjoint_tape_begin()
                y, _ = dev.run(h.slot_of[1], 3, u, compute_energy=False)
                outs += [y, *dev.run_tangent(h.slot_of[1], 3, du, d0, dm1), dev.get_solution()]
                if look:
                    dev.tangent_route()
                    dev.tangent_stage()
            return outs, [dev.sweep_launches(s).copy() for s in h.slot_of.values()], dev.tangent_info()["route"], dev.step_counts()
        finally:
            h.close()

    plain, looked = observe(False), observe(True)
    assert all(np.array_equal(a, b) for a, b in zip(plain[0], looked[0])), "the aids changed a march's bits"
    assert all(np.array_equal(a, b) for a, b in zip(plain[1], looked[1])), "the aids changed sweep_launches"
    assert plain[2:] == looked[2:]
    n = len(plain[0]) // 2
    assert all(np.array_equal(a, b) for a, b in zip(looked[0][:n], looked[0][n:])), "a march behind the aids' calls differs from the one in front"
