"""The single-vector factor apply (csrc/fc_kernels.hip.h: fc_nd_sweep, fc_nd_down_block, fc_nd_flat_block, fc_nd_fold1; dispatched by
launch_sweep / launch_flat / launch_up_column of csrc/fc_hip.hip) on every kernel route, against a host apply of higher precision.

The cases, knob sets and runs are those of tests/support/sweep_cases.py; tests/test_sweep_cases_host.py shows that together they reach
every template instance and every branch label outside sweep_cases.UNREACHED.  Knobs read once per process make a child process each
(tests/support/sweep_apply_child.py), one after the other; inside a child every (handle-level knob set, storage width, case) gets a fresh
handle.  fc_get_sweep_launches tells what was launched: a route the host model predicts and the device did not take fails the test.

References.  (1) The same operation in higher precision, for every storage width: the stage-by-stage apply with products and sums in
np.longdouble (sweep_cases.apply_longdouble) on the factor values the device holds (DeviceSolver.factor_values, rounded to the storage
width as fc_pack rounds them) -- this isolates the sweeps from the elimination.  (2) End to end, fp64 storage and default knobs only:
the operator the device assembled, solved with LAPACK and refined in np.longdouble (batch_cases.refined_solve).

A solve with refine = 0 and method "refine" is the bare apply on a compressed slot too: solve_once turns to GMRES only for a Krylov
method or through KrylovOverride, which is on for slots with inexact fp64 factors alone; compressed slots are never marked inexact."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.support import batch_cases as bc
from tests.support import front_cases as fcs
from tests.support import sweep_cases as sc
from tests.test_batch_apply_gpu import HOST_BLOCK_SOLVE_ERROR

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# Largest relative distance between the HOST fp64 nd_numeric.block_solve (numpy sums) and the longdouble apply on the same values -- host
# factors of batch_cases.host_operator by nd_numeric.factorize_blocks, both operators, the 8 right-hand sides of the pool -- in the
# 2-norm / in the max-norm, per storage width (values rounded to nearest even as fc_pack does).  Measured per case, worst of bdf1 / bdf2:
#                  fp64                 fp32                 bf16
#   square8        6.1e-16 / 5.9e-16    4.9e-16 / 5.3e-16    8.5e-16 / 7.5e-16
#   wide16x9       7.0e-16 / 6.5e-16    7.8e-16 / 8.7e-16    9.3e-16 / 7.5e-16
#   huge20x9       8.5e-16 / 1.1e-15    6.8e-16 / 1.1e-15    4.7e-16 / 1.0e-15
#   huge16x16      1.7e-15 / 1.3e-15    9.1e-16 / 1.2e-15    1.3e-15 / 1.3e-15
#   deep8x6        5.0e-16 / 5.4e-16    6.0e-16 / 6.8e-16    4.8e-16 / 5.4e-16
#   bin8x6         5.3e-16 / 4.9e-16    9.9e-16 / 4.6e-16    7.2e-16 / 3.8e-16
#   twoleaf22x20   1.8e-15 / 1.4e-15    4.2e-15 / 3.2e-15    1.8e-15 / 1.8e-15
#   bin32x16       1.2e-15 / 1.0e-15    8.2e-16 / 9.1e-16    6.8e-16 / 1.1e-15
HOST_APPLY_ERROR = {64: (1.810e-15, 1.432e-15), 32: (4.205e-15, 3.183e-15), 16: (1.811e-15, 1.832e-15)}
# The device may miss the reference by 16 times that, as in the batched test and for the same reason: another fixed summation order
# (four partial sums per lane, shuffle trees over 8 ... 64 lanes, LDS sums of four waves, tiles of 2048 operands).
TOLERANCES = {str(b): (16 * e2, 16 * ei) for b, (e2, ei) in HOST_APPLY_ERROR.items()}
TOLERANCES["end_to_end"] = 16 * HOST_BLOCK_SOLVE_ERROR


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """Per case and operator: the matrix and the factor values as a default handle computes them, the right-hand sides, the longdouble
    apply for every storage width a run uses and the refined solve: computed once, written to one file that every child reads.  The
    handle is closed before the first child starts."""
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, DeviceSolver
    from tests.support import ndsolver

    widths = {}
    for runs in sc.RUNS.values():
        for _, bits, case in runs:
            widths.setdefault(case, set()).add(bits)
    out = {}
    for ci, (case, nx, ny, tbits, depth, merge) in enumerate(sc.cases()):
        th, dofs, tree = fcs.host_case(nx, ny, tbits)
        fac = ndsolver.factorize_blocks(None, tree)
        dev = DeviceSolver(th)
        try:
            U0 = bc.smooth_advection(th)
            dev.set_bc(dofs, np.zeros((dofs.size, 1)))
            dev.set_time_scheme(0.005, True)
            for op, slot in (("bdf1", SLOT_BDF1), ("bdf2", SLOT_BDF2)):
                dev.assemble_matrix(slot, mass=bc.OPERATORS[op], nu=bc.NU, adv=U0, lin=U0)
                dev.apply_bc(slot)
                dev.setup_solver(slot, depth=depth, merge=merge)
                assert np.array_equal(ndsolver.tree_of(dev).perm, tree.perm)
                A, V = dev.matrix(slot), dev.factor_values(slot)
                assert V.size == fac.vals.size
                B = sc.rhs_set(tree, bc.rhs_pool(dev.N, 1000 + ci), dofs)
                E = bc.refined_solve(A, B)
                res = np.linalg.norm(bc.residual_longdouble(A, E, B).astype(np.float64), axis=1) / np.linalg.norm(B, axis=1)
                assert res.max() < 1e-14
                out[f"{case}/{op}/V"], out[f"{case}/{op}/B"], out[f"{case}/{op}/E"] = V, B, E
                for bits in sorted(widths[case]):
                    X = sc.apply_longdouble(fac, sc.round_values(V, bits), B)
                    out[f"{case}/{op}/X{bits}"] = X
                    d = max(np.linalg.norm(X[j] - E[j]) / np.linalg.norm(E[j]) for j in range(len(B)))
                    print(f"{case} {op}: N {dev.N}, longdouble apply of the {bits}-bit factor values against the refined solve {d:.2e}")
        finally:
            dev.close()
    path = tmp_path_factory.mktemp("sweep_apply") / "reference.npz"
    np.savez(path, **out)
    return path


def test_every_route_of_the_single_vector_apply_against_the_longdouble_host_apply(reference):
    """One child per process-level knob set, strictly one after the other; the first that fails (assertion, fault, abort, timeout) ends
    the sequence."""
    for kn, knobs in sc.KNOB_SETS.items():
        env = {k: v for k, v in os.environ.items() if k not in sc.PROCESS_KNOBS + sc.HANDLE_KNOBS}
        env.update(knobs, PYTHONPATH=str(ROOT))
        out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "sweep_apply_child.py"), str(reference), kn, json.dumps(TOLERANCES)],
                             env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        for ln in out.stdout.splitlines():
            if ln.startswith(("WORST", "[")):
                print(ln)
        assert out.returncode == 0, f"knob set {kn} {knobs}: exit status {out.returncode}\n{out.stdout[-2500:]}\n{out.stderr[-3000:]}"
        assert f"CHILD OK {kn}" in out.stdout


def test_sweep_geometry_without_an_instance_is_refused():
    """FC_SWEEP_GEOM = 8:2 on the first stage, segment kernel on every level: launch_sweep has no fc_nd_sweep<8, 2>, so the solve returns
    FC_ERR_INVALID ("unsupported (lanes, sub) combination") from the check in front of the launch -- it neither launches another
    instance nor skips the stage silently -- and the child ends as any other."""
    env = {k: v for k, v in os.environ.items() if k not in sc.PROCESS_KNOBS + sc.HANDLE_KNOBS}
    env.update(PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "sweep_apply_child.py"), "refusal"], env=env, capture_output=True,
                         text=True, timeout=120, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, f"exit status {out.returncode}\n{out.stdout[-2500:]}\n{out.stderr[-3000:]}"
    assert out.stdout.count("REFUSED") == 2 and "CHILD OK refusal" in out.stdout


def test_sweep_launch_getter_error_paths():
    """fc_get_sweep_launches: status codes for a null handle, a slot without factors, a bad slot and a short buffer; nothing written; the
    count for n = 0; the rows DeviceSolver.sweep_launches returns are the model's."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY, ptr
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from tests.support import ndsolver

    th = TaylorHood(Mesh.unit_square(4, 4))
    dev = DeviceSolver(th, 0)
    try:
        lib, h = dev.lib, dev._h
        buf = np.full(512, -7, dtype=np.int32)
        assert lib.fc_get_sweep_launches(None, SLOT_BDF2, buf.size, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, buf.size, ptr(buf)) == FC_ERR_NOT_READY
        assert b"fc_solver_setup" in lib.fc_last_error()
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, 0, None) == FC_ERR_NOT_READY
        dofs = fcs.dirichlet_dofs(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.01, True)
        dev.assemble_matrix(SLOT_BDF2, mass=150.0, nu=0.01)
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2)
        assert lib.fc_get_sweep_launches(h, SLOT_BDF1, buf.size, ptr(buf)) == FC_ERR_NOT_READY  # the other slot has no factors
        count = lib.fc_get_sweep_launches(h, SLOT_BDF2, 0, None)
        n = len(DeviceSolver.SWEEP_LAUNCH_COLS) * count
        assert len(DeviceSolver.SWEEP_LAUNCH_COLS) == 8 and 0 < n <= buf.size
        assert count == dev.bench_sweeps(SLOT_BDF2, reps=1)[1]  # the launches an apply really makes
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, n - 1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_sweep_launches(h, 2, n, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_sweep_launches(h, -1, n, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, -1, ptr(buf)) == FC_ERR_INVALID
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, n, None) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error, nor by the count
        assert lib.fc_get_sweep_launches(h, SLOT_BDF2, n, ptr(buf)) == 0
        assert np.all(buf[:n] >= 0) and np.all(buf[n:] == -7)
        rows = dev.sweep_launches(SLOT_BDF2)
        assert np.array_equal(rows.reshape(-1), buf[:n])
        knobs = {k: v for k, v in os.environ.items() if k in sc.PROCESS_KNOBS + sc.HANDLE_KNOBS}
        want = sc.predicted_launches(sc.model(ndsolver.tree_of(dev), knobs))
        assert np.array_equal(rows, want), f"route not taken: predicted {want.tolist()}, reported {rows.tolist()}"
    finally:
        dev.close()
