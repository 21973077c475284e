"""The forward batched step (csrc/fc_batch.hip.h: fc_rhs_elem_breg<KB, FORCE>, fc_rhs_elem_b<KB>, fc_rhs_gather_b, fc_rhs_ctrl_b,
fc_tail_b with its row blocks and fc_energy_b_block, fc_final_b, fc_early_b, fc_wait_solved_b, fc_final_late_b, fc_b_interleave,
fc_b_zero_column; dispatched by batch_enqueue, batch_launches, batch_launches_side, build_tail_blocks and build_ctrl_rows of
csrc/fc_hip.hip) on every kernel route, step by step and column by column, against a host model in np.longdouble.

The meshes, widths, knob sets, scenarios and runs are those of tests/support/batch_step_cases.py; tests/test_batch_step_cases_host.py
shows that together they reach every branch label outside batch_step_cases.UNREACHED.  Knobs read once per process make a child process
each (tests/support/batch_step_child.py), one after the other; inside a child every run gets a fresh handle, created under the run's
handle-level knobs.  fc_get_batch_step_route tells what a batched step launched: a route the host model predicts and the device did not
take fails the test.  fc_debug_capture_batch_rhs hands back the right-hand side the solve consumed.

Tolerances, per quantity, per step and per column:
  right-hand side    16 x HOST_RHS_ERROR (2-norm, max-norm) of tests/test_step_routes_gpu.py, on the star too
  solution           16 x HOST_BLOCK_SOLVE_ERROR of tests/test_batch_apply_gpu.py, against batch_cases.refined_solve (step_cases.Refined) on the
                     device's operator and the captured right-hand side
  state              u_n = velocity part of the solution, u_nn = the previous u_n: bit for bit
  sensors            2 (n_s + 6) eps sum |w_k x_k|: a 64-lane partial and a 6-level shuffle tree, times 2 -- derived, nothing measured
  energy             16 x HOST_ENERGY_ERROR of tests/test_step_routes_gpu.py
  |r|_2              2 (L + 2) eps | |b| + |A| |x| |_2, L the longest row: running error bound of the row sums, times 2 -- derived (the batched
                     tail splits a row over 16 / (KB / 2) lanes and folds them by shuffles: fewer additions in a chain, the bound holds)
  |b|_2              1e-14 relative
  off the cadence    NaN in the info;  flags: set for the non-finite column only
  bit for bit        gather ahead against FC_SPECULATE_GATHER=0 and FC_SPECULATE=0, FC_LATE_GATE=0 and FC_BATCH_GRAPH=1 against the default,
                     capture on against off, the same scenario in two columns, columns 0 to 2 of k = 3 against k = 4, the other columns of a
                     batch with and without a non-finite one
No tolerance is taken from the device's own output."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.support import batch_step_cases as bs
from tests.support import step_cases as sc
from tests.test_batch_apply_gpu import HOST_BLOCK_SOLVE_ERROR
from tests.test_step_routes_gpu import HOST_ENERGY_ERROR, HOST_RHS_ERROR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# The constants are those of tests/test_step_routes_gpu.py, measured there on the structured meshes; the star stays within them
# (tests/test_batch_step_cases_host.py::test_longdouble_model_against_the_fp64_oracle_on_the_star: rhs 1.29e-16 / 3.35e-16, energy 2.08e-16).
# The device may miss the reference by 16 times that, the project's margin for another fixed summation order.
TOLERANCES = {"rhs": [16 * HOST_RHS_ERROR[0], 16 * HOST_RHS_ERROR[1]], "energy": 16 * HOST_ENERGY_ERROR, "solve": 16 * HOST_BLOCK_SOLVE_ERROR, "bnorm": 1e-14}
CHILD_TIMEOUT = 120


def _shared_keys(ra, a: str, b: str):
    shared = [bs.run_name(r) for r in bs.RUNS[a] if r in bs.RUNS[b]]
    return shared, sorted(k for k in ra.files if k.rsplit("/", 2)[0] in shared)


def test_every_route_of_the_batched_step_against_the_longdouble_host_model(tmp_path):
    """One child per process-level knob set, strictly one after the other; the first that fails (assertion, fault, abort, timeout) ends
    the sequence.  Then the records of the children that must agree bit for bit are compared: right-hand side, solution, y, dE, |r| / |b|
    and |b| of every step and column."""
    for kn, knobs in bs.KNOB_SETS.items():
        env = {k: v for k, v in os.environ.items() if k not in bs.PROCESS_KNOBS + bs.HANDLE_KNOBS}
        env.update(knobs, PYTHONPATH=str(ROOT))
        out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "batch_step_child.py"), kn, json.dumps(TOLERANCES), str(tmp_path / f"records_{kn}.npz")],
                             env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
        for ln in out.stdout.splitlines():
            if ln.startswith(("WORST", "RUN OK", "BITWISE", "REFUSED", "CHILD OK")):
                print(ln)
        assert out.returncode == 0, f"knob set {kn} {knobs}: exit status {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
        assert f"CHILD OK {kn}" in out.stdout
    for a, b in bs.BITWISE_PAIRS:
        ra, rb = np.load(tmp_path / f"records_{a}.npz"), np.load(tmp_path / f"records_{b}.npz")
        shared, keys = _shared_keys(ra, a, b)
        assert keys and all(k in rb.files for k in keys), f"{a} / {b}: the children did not record the same steps"
        for k in keys:
            assert np.array_equal(ra[k], rb[k], equal_nan=True), f"{k}: the children {a} and {b} differ"
        print(f"BITWISE {a} == {b}: {len(keys)} records of {len(shared)} runs")
    # fc_rhs_elem_b against fc_rhs_elem_breg on the steps that start from a state the host has set (the first of a run, the one behind
    # fc_set_state_batch: the same inputs in both children; later steps start from solutions that already differ).  The same sums in the
    # same order, but not the same bits: the compiler fuses multiply-adds at different places of the scalar and of the two-wide chains.
    # Said, not asserted bit for bit; each child holds these right-hand sides to the model, so the two differ by at most twice that.
    a, b = bs.ELEM_PAIR
    ra, rb = np.load(tmp_path / f"records_{a}.npz"), np.load(tmp_path / f"records_{b}.npz")
    keys = []
    for run in (r for r in bs.RUNS[a] if r in bs.RUNS[b]):
        n, fresh = 0, True
        for op in bs.scenario(run[0]):
            if op[0] == "set_state":
                fresh = True
            elif op[0] == "step":
                if fresh:
                    keys.append(f"{bs.run_name(run)}/{n}/b")
                n, fresh = n + 1, False
            elif op[0] == "nonfinite":
                n, fresh = n + 2, False
    assert len(keys) >= 8 and all(k in ra.files and k in rb.files for k in keys)
    same = sum(bool(np.array_equal(ra[k], rb[k])) for k in keys)
    diff = max(float(np.max(np.abs(ra[k] - rb[k]).max(axis=1) / np.abs(ra[k]).max(axis=1))) for k in keys)
    print(f"ELEM KERNELS: fc_rhs_elem_b and fc_rhs_elem_breg agree bit for bit on {same} of {len(keys)} right-hand sides from the same state "
          f"(largest difference {diff:.1e} of a column's largest entry)")
    assert diff <= 2 * TOLERANCES["rhs"][1]


def test_route_and_capture_getters_error_paths():
    """fc_get_batch_step_route: status codes for a null handle, a null buffer, a handle without a batched step and a short buffer; nothing
    is written on an error; the getter reports the step that ran, and fc_set_batch forgets it.  fc_debug_get_batch_rhs: not ready without
    a batch, without capture and before the first captured step; a null buffer and another k are refused; the capture cannot be
    switched while a step is in flight."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY, ptr
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver

    mesh, k = "5x3", 3
    th, dofs, prof = bs.host_case(mesh)
    env = {name: os.environ[name] for name in bs.PROCESS_KNOBS + bs.HANDLE_KNOBS if name in os.environ}
    dev = DeviceSolver(th, 0)
    try:
        lib, h = dev.lib, dev._h
        n = len(DeviceSolver.BATCH_ROUTE_COLS)
        assert DeviceSolver.BATCH_ROUTE_COLS == bs.ROUTE_COLS and n == 13
        buf = np.full(20, -7, dtype=np.int32)
        out = np.full((k, th.N), -7.0)
        assert lib.fc_get_batch_step_route(None, buf.size, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_batch_step_route(h, buf.size, None) == FC_ERR_INVALID
        assert lib.fc_get_batch_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert b"no batched step yet" in lib.fc_last_error()
        assert lib.fc_debug_capture_batch_rhs(None, 1) == FC_ERR_INVALID
        assert lib.fc_debug_get_batch_rhs(None, k, ptr(out)) == FC_ERR_INVALID
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY  # no batch
        dev.set_bc(dofs, prof)
        dev.set_time_scheme(sc.DT, True)
        dev.assemble_matrix(SLOT_BDF2, **sc.operator_args(th, 2))
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2)
        dev.set_solver_options(refine=0, check_residual=1)
        dev.set_sensors(sc.sensor_rows(th, "single_entry"))
        dev.set_batch(k)
        cols = [bs.column_state(th, s, k, 1) for s in range(k)]
        dev.set_state_batch(np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols]))
        assert lib.fc_get_batch_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # a batch, no step
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY  # no capture
        dev.step_batch(SLOT_BDF2, bs.controls(k, 0))
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY  # a step without capture
        assert b"no captured right-hand side" in lib.fc_last_error()
        # (DeviceSolver.step_batch is fc_step_batch_begin + _end: overlapped unless the handle runs on one stream)
        hist, settings = bs.History(), dict(order=2, energy=True, mode="early", check=1)
        bs.advance(hist, bs.predicted_route(mesh, k, env, settings, hist))
        dev.capture_batch_rhs(True)
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY  # capture on, no captured step yet
        dev.step_batch_begin(SLOT_BDF2, bs.controls(k, 1))
        assert lib.fc_debug_capture_batch_rhs(h, 0) == FC_ERR_INVALID  # a step is in flight
        y, dE, info = dev.step_batch_end()
        assert np.all(info[:, 3] == 0) and np.all(np.isfinite(dE))
        assert lib.fc_get_batch_step_route(h, n - 1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_batch_step_route(h, -1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_batch_step_route(h, 0, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_debug_get_batch_rhs(h, k, None) == FC_ERR_INVALID
        assert lib.fc_debug_get_batch_rhs(h, k + 1, ptr(out)) == FC_ERR_INVALID
        assert np.all(buf == -7) and np.all(out == -7.0)  # nothing written on an error
        assert lib.fc_get_batch_step_route(h, buf.size, ptr(buf)) == 0 and np.all(buf[n:] == -7)
        got = dev.batch_step_route()
        assert np.array_equal(got, buf[:n])
        want = bs.predicted_route(mesh, k, env, settings, hist)
        want[11] = got[11]  # (the count of control rows is the child's to check, from the device's own operator)
        assert np.array_equal(got, want), f"route not taken: predicted {want.tolist()}, reported {got.tolist()}"
        b = dev.batch_rhs()
        assert b.shape == (k, th.N) and np.all(np.isfinite(b)) and not np.array_equal(b[0], b[1])
        dev.set_batch(k)  # a new batch: the record and the captured right-hand side are the old batch's
        assert lib.fc_get_batch_step_route(h, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY
        dev.set_batch(0)
        assert lib.fc_debug_get_batch_rhs(h, k, ptr(out)) == FC_ERR_NOT_READY
    finally:
        dev.close()
