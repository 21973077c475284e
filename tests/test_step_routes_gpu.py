"""The half of a time step around the factor sweeps -- the right-hand side in front of them (csrc/fc_kernels.hip.h: fc_rhs_elem,
fc_rhs_elem_reg, fc_rhs_gather, fc_force_rows) and the tail behind them (fc_tail<false|true>, fc_finish, fc_final, fc_early, fc_wait_solved,
fc_final_late; dispatched by enqueue_rhs, launch_tail, enqueue_step_launches and step_enqueue_overlapped of csrc/fc_hip.hip) -- on every
kernel route, against a host model in np.longdouble.

The cases, knob sets and runs are those of tests/support/step_cases.py; tests/test_step_cases_host.py shows that together they reach every
branch label outside step_cases.UNREACHED.  Knobs read once per process make a child process each (tests/support/step_child.py), one after
the other; inside a child every run gets a fresh handle, created under the run's handle-level knobs.  fc_get_step_route tells what a step
launched: a route the host model predicts and the device did not take fails the test.

Tolerances, per quantity:
  right-hand side    16 x HOST_RHS_ERROR (2-norm, max-norm), measured by tests/test_step_cases_host.py
  solution           16 x HOST_BLOCK_SOLVE_ERROR of tests/test_batch_apply_gpu.py, against batch_cases.refined_solve on the device's operator and b
  state              u_n = velocity part of the solution, u_nn = the previous u_n: bit for bit
  sensors            2 (n_s + 6) eps sum |w_k x_k|: a 64-lane partial and a 6-level shuffle tree, times 2 -- derived, nothing measured
  energy             16 x HOST_ENERGY_ERROR, measured by tests/test_step_cases_host.py
  |r|_2              2 (L + 2) eps | |b| + |A| |x| |_2, L the longest row: running error bound of the row sums, times 2 -- derived
  |b|_2              1e-14 relative
  fused final, speculation   records equal to the default child's bit for bit"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.support import step_cases as sc
from tests.test_batch_apply_gpu import HOST_BLOCK_SOLVE_ERROR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# Largest relative distance of the fp64 numpy oracle (oracle/ns_oracle.py: TimeStepper.rhs for both orders, nonlinear on and off, with and
# without force profiles; TimeStepperCN.rhs with the explicit operator C) from the np.longdouble right-hand side of step_cases.HostModel,
# in the 2-norm / in the max-norm, and of the fp64 1/2 u^T M u (velocity_mass) from the longdouble energy; measured per case by
# tests/test_step_cases_host.py::test_longdouble_model_against_the_fp64_oracle_and_the_constants, which asserts that these constants
# bound what it measures and exceed it by less than a factor of two:
#              rhs 2-norm / max-norm     energy
#   5x3        1.60e-16 / 3.63e-16       2.49e-16
#   9x9        1.22e-16 / 2.45e-16       1.30e-16
#   12x7       1.07e-16 / 2.35e-16       3.44e-16
#   12x11      9.28e-17 / 1.53e-16       3.70e-16
#   23x12      6.50e-17 / 8.01e-17       3.25e-16
HOST_RHS_ERROR = (1.61e-16, 3.63e-16)
HOST_ENERGY_ERROR = 3.71e-16
# The device may miss the reference by 16 times that, the project's margin for another fixed summation order: the 7 quadrature points of
# a cell are exchanged by shuffles, the element contributions of a row summed in list order, the energy by cell quadrature in shuffle and
# LDS trees (fc_tail) or by rows of the mass matrix (fc_finish).
TOLERANCES = {"rhs": [16 * HOST_RHS_ERROR[0], 16 * HOST_RHS_ERROR[1]], "energy": 16 * HOST_ENERGY_ERROR, "solve": 16 * HOST_BLOCK_SOLVE_ERROR, "bnorm": 1e-14}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """Per case: the operators as a default handle assembles them -- both BDF orders without and with boundary conditions, and the
    lagged operator of the residual-monitor runs -- written once to one file that every child reads and compares its own with; the
    handle is closed before the first child starts."""
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, SLOT_SCRATCH, DeviceSolver

    out = {}
    for case in sc.CASES:
        th, dofs, prof = sc.host_case(case)
        dev = DeviceSolver(th)
        try:
            dev.set_bc(dofs, prof)
            dev.set_time_scheme(sc.DT, True)
            for order, slot in ((1, SLOT_BDF1), (2, SLOT_BDF2)):
                dev.assemble_matrix(SLOT_SCRATCH, **sc.operator_args(th, order))
                out[f"{case}/full{order}"] = dev.matrix(SLOT_SCRATCH).data
                dev.assemble_matrix(slot, **sc.operator_args(th, order))
                dev.apply_bc(slot)
                out[f"{case}/bc{order}"] = dev.matrix(slot).data
                dev.assemble_matrix(slot, **sc.operator_args(th, order, lagged=True))
                dev.apply_bc(slot)
                out[f"{case}/lagged{order}"] = dev.matrix(slot).data
        finally:
            dev.close()
    d = tmp_path_factory.mktemp("step_routes")
    np.savez(d / "reference.npz", **out)
    return d


def test_every_route_of_the_step_rhs_and_tail_against_the_longdouble_host_model(reference):
    """One child per process-level knob set, strictly one after the other; the first that fails (assertion, fault, abort, timeout) ends
    the sequence.  Then the records of the children that must agree bit for bit are compared: the fused final against the separate
    fc_final launch (y, dE, |r| / |b|, |b| and the solution of every step), the speculated element loop against FC_SPECULATE=0."""
    for kn, knobs in sc.KNOB_SETS.items():
        env = {k: v for k, v in os.environ.items() if k not in sc.PROCESS_KNOBS + sc.HANDLE_KNOBS}
        env.update(knobs, PYTHONPATH=str(ROOT))
        out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "step_child.py"), str(reference / "reference.npz"), kn, json.dumps(TOLERANCES),
                              str(reference / f"records_{kn}.npz")], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        for ln in out.stdout.splitlines():
            if ln.startswith(("WORST", "RUN OK", "ELEM KERNELS", "CHILD OK")):
                print(ln)
        assert out.returncode == 0, f"knob set {kn} {knobs}: exit status {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
        assert f"CHILD OK {kn}" in out.stdout
    for a, b in sc.BITWISE_PAIRS:
        ra, rb = np.load(reference / f"records_{a}.npz"), np.load(reference / f"records_{b}.npz")
        shared = [sc.run_name(r) for r in sc.RUNS[a] if r in sc.RUNS[b]]
        keys = sorted(k for k in ra.files if k.rsplit("/", 2)[0] in shared and not k.rsplit("/", 1)[1].startswith("b"))
        assert keys and all(k in rb.files for k in keys), f"{a} / {b}: the children did not record the same steps"
        for k in keys:
            assert np.array_equal(ra[k], rb[k], equal_nan=True), f"{k}: the children {a} and {b} differ: {ra[k][-3:]} / {rb[k][-3:]}"
        print(f"BITWISE {a} == {b}: {len(keys)} records of {len(shared)} runs")


def test_more_than_64_sensor_rows_are_refused_and_route_getter_error_paths():
    """fc_set_sensors refuses a 65th row with a status code (the kernels park the readings in ysh[64]).  fc_get_step_route: status codes
    for a null handle, a null buffer, a handle that has not stepped yet and a short buffer; nothing is written on an error; the getter
    reports the step that ran."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY, ptr
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver

    case = "5x3"
    th, dofs, prof = sc.host_case(case)
    env = {k: os.environ[k] for k in sc.PROCESS_KNOBS + sc.HANDLE_KNOBS if k in os.environ}
    dev = DeviceSolver(th, 0)
    try:
        lib, h = dev.lib, dev._h
        n = len(DeviceSolver.STEP_ROUTE_COLS)
        assert DeviceSolver.STEP_ROUTE_COLS == sc.ROUTE_COLS and n == 9
        buf = np.full(16, -7, dtype=np.int32)
        assert lib.fc_get_step_route(None, buf.size, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_step_route(h, buf.size, None) == FC_ERR_INVALID
        assert lib.fc_get_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert b"no time step yet" in lib.fc_last_error()
        dev.set_bc(dofs, prof)
        dev.set_time_scheme(sc.DT, True)
        dev.assemble_matrix(SLOT_BDF2, **sc.operator_args(th, 2))
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2)
        rows = sc.sensor_rows(th, "limit64")
        one_more = rows + [rows[0]]
        rp = np.cumsum([0] + [len(i) for i, _ in one_more]).astype(np.int32)
        idx, w = np.concatenate([i for i, _ in one_more]).astype(np.int32), np.concatenate([w for _, w in one_more])
        assert lib.fc_set_sensors(h, len(one_more), ptr(rp), ptr(idx), ptr(w)) == FC_ERR_INVALID
        dev.set_sensors(rows)
        dev.set_state(*sc.initial_state(th, 1))
        assert lib.fc_get_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # set up, not stepped
        assert dev.assemble_rhs(SLOT_BDF2, sc.CONTROLS[0]).shape == (dev.N,)
        assert lib.fc_get_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # a right-hand side alone is no step
        hist = sc.History()
        hist.ready[0] = False  # (the BDF1 slot is not set up: nothing is speculated for it, BDF2 follows anyway)
        settings = dict(order=2, energy=True, blocking=True, **sc.DEFAULT_OPTS)
        want = sc.predicted_route(case, env, settings, hist)
        y, dE, info = dev.step(SLOT_BDF2, sc.CONTROLS[0])
        assert y.shape == (64,) and np.isfinite(dE) and info[3] == 0
        assert lib.fc_get_step_route(h, n - 1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_step_route(h, -1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_step_route(h, 0, ptr(buf)) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error
        assert lib.fc_get_step_route(h, buf.size, ptr(buf)) == 0
        assert np.all(buf[n:] == -7)
        got = dev.step_route()
        assert np.array_equal(got, buf[:n])
        assert np.array_equal(got, want), f"route not taken: predicted {want.tolist()}, reported {got.tolist()}"
        sc.advance(hist, want)
        dev.assemble_rhs(SLOT_BDF2, sc.CONTROLS[1])  # a right-hand side in between leaves the last step's record alone
        assert np.array_equal(dev.step_route(), want)
    finally:
        dev.close()
