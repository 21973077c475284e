"""The batched factor apply (csrc/fc_batch.hip.h: fc_nd_block_b<KB, NT>, fc_nd_fold_b<KB>, fc_b_repack, the tables of
build_batch_tables) on every kernel route, against a host solve of higher precision.

The cases are the small meshes of tests/support/batch_cases.py (the stress meshes of the front-elimination test and one deep tree);
tests/test_batch_cases_host.py shows that they and the knob sets below reach every branch label.  The knobs are read once per process,
so every knob set is a child process (tests/support/batch_apply_child.py), one after the other.  fc_get_batch_launches tells what was
launched: a route the host model predicts and the device did not take fails the test.

The reference: the operator the device assembled (mass 200 / 300, nu 0.01, smooth advection, Dirichlet rows), taken back to the host,
solved with LAPACK in fp64 and refined twice with the residual in np.longdouble."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import batch_cases as bc
from tests.support import front_cases as fcs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# Largest relative error |x - x_ref| / |x_ref| of the HOST multifrontal nd_numeric.block_solve (fp64, the device's factor layout, numpy
# sums) against the refined reference, over the five cases, both operators assembled by the numpy oracle (batch_cases.host_operator) and
# the first 8 right-hand sides of the pool.  Measured per case (bdf1 / bdf2):
#   square8 1.1e-15 / 3.4e-15   wide16x9 3.8e-15 / 4.6e-15   huge20x9 7.5e-15 / 1.7e-14   huge16x16 1.5e-14 / 3.1e-14   deep8x6 1.9e-15 / 2.4e-15
# (1-norm condition estimates 1.3e4 ... 4.7e4; two and three refinement sweeps of the reference agree to 1e-16.)
HOST_BLOCK_SOLVE_ERROR = 3.081e-14
# The device may miss the reference by 16 times that: its matrix-core sums run over up to 21 chunks of 32 columns, and over the parts
# of split tiles, in another order than numpy's pairwise sums.
TOLERANCE = 16 * HOST_BLOCK_SOLVE_ERROR


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """Operators of every case as the device assembles them, the right-hand side pool and its refined solutions: computed once, written
    to one file that every child reads.  The handle is closed before the first child starts."""
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, DeviceSolver
    from tests.support import nd_numeric

    out = {}
    for ci, (case, nx, ny, bits, depth, merge) in enumerate(bc.cases()):
        th, dofs, tree = fcs.host_case(nx, ny, bits)
        dev = DeviceSolver(th)
        try:
            U0 = bc.smooth_advection(th)
            dev.set_bc(dofs, np.zeros((dofs.size, 1)))
            dev.set_time_scheme(0.005, True)
            for op, slot in (("bdf1", SLOT_BDF1), ("bdf2", SLOT_BDF2)):
                dev.assemble_matrix(slot, mass=bc.OPERATORS[op], nu=bc.NU, adv=U0, lin=U0)
                dev.apply_bc(slot)
                A = dev.matrix(slot)
                pool = bc.rhs_pool(dev.N, 1000 + ci)
                X = bc.refined_solve(A, pool)
                res = np.linalg.norm(bc.residual_longdouble(A, X, pool).astype(np.float64), axis=1) / np.linalg.norm(pool, axis=1)
                assert res.max() < 1e-14
                fac = nd_numeric.factorize_blocks(A, tree)
                host = max(np.linalg.norm(nd_numeric.block_solve(fac, pool[j]) - X[j]) / np.linalg.norm(X[j]) for j in range(2))
                print(f"{case} {op}: N {dev.N} cond_1(A) ~ {bc.cond1_estimate(A):.3g}, reference residual {res.max():.1e}, host block_solve error {host:.2e}")
                out[f"{case}/{op}/A"], out[f"{case}/{op}/B"], out[f"{case}/{op}/X"] = A.data, pool, X
        finally:
            dev.close()
    path = tmp_path_factory.mktemp("batch_apply") / "reference.npz"
    np.savez(path, **out)
    return path


def test_every_route_of_the_batched_apply_against_the_refined_host_solve(reference):
    """One child per knob set, strictly one after the other; the first that fails (assertion, fault, abort, timeout) ends the sequence."""
    for kn, knobs in bc.KNOB_SETS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith(("FC_BATCH_", "FC_NT_BYTES"))}
        env.update(knobs, PYTHONPATH=str(ROOT))
        out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "batch_apply_child.py"), str(reference), kn, repr(TOLERANCE)],
                             env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        for ln in out.stdout.splitlines():
            if ln.startswith(("WORST", "LAUNCHES")):
                print(ln)
        assert out.returncode == 0, f"knob set {kn} {knobs}: exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
        assert f"CHILD OK {kn}" in out.stdout


def test_batch_launch_getter_error_paths():
    """fc_get_batch_launches: status codes for a null handle, a handle without a batch, a bad slot and a short buffer; nothing written."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from tests.support import ndsolver

    th = TaylorHood(Mesh.unit_square(4, 4))
    dev = DeviceSolver(th, 0)
    try:
        lib, h = dev.lib, dev._h
        buf = np.full(256, -7, dtype=np.int32)
        assert lib.fc_get_batch_launches(None, SLOT_BDF2, buf.size, buf) == FC_ERR_INVALID
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, buf.size, buf) == FC_ERR_NOT_READY
        assert b"fc_set_batch" in lib.fc_last_error()
        dofs = fcs.dirichlet_dofs(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.01, True)
        dev.assemble_matrix(SLOT_BDF2, mass=150.0, nu=0.01)
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2)
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, buf.size, buf) == FC_ERR_NOT_READY  # factors, but no batch
        dev.set_batch(3)
        info = dev.batch_info()
        n = 8 * (info["block_launches"] + info["fold_launches"])
        assert 0 < n <= buf.size
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, n - 1, buf) == FC_ERR_INVALID
        assert lib.fc_get_batch_launches(h, 2, n, buf) == FC_ERR_INVALID
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, -1, buf) == FC_ERR_INVALID
        assert np.all(buf == -7)  # nothing written on an error
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, n, buf) == 0
        assert np.all(buf[:n] >= 0) and np.all(buf[n:] == -7)
        rows = dev.batch_launches(SLOT_BDF2)
        assert np.array_equal(rows.reshape(-1), buf[:n])
        knobs = {k: v for k, v in os.environ.items() if k.startswith(("FC_BATCH_", "FC_NT_BYTES"))}
        want = bc.predicted_launches(bc.model(ndsolver.tree_of(dev), knobs), 4, knobs)
        assert np.array_equal(rows, want), f"route not taken: predicted {want.tolist()}, reported {rows.tolist()}"
        dev.set_batch(0)
        assert lib.fc_get_batch_launches(h, SLOT_BDF2, buf.size, buf) == FC_ERR_NOT_READY
    finally:
        dev.close()


@pytest.mark.parametrize("k", [5, 32])
def test_the_batched_residual_monitor_reports_a_residual_that_is_there(k):
    """fc_tail_b / fc_final_b are otherwise only bounded from above (info[:, 1] < 1e-12): a tail that skipped row blocks would pass.
    Here the factors LAG the operator (fc_update_operator after a second assembly), so the batched step solves A0 x = b while the
    monitor forms b - A1 x = (A0 - A1) x: the record must hold exactly that, in the form the library reports it --
    sqrt(sum r^2 / sum b^2), i.e. |b - A1 x|_2 / |b|_2 with b = A0 x (residual_info in csrc/fc_hip.hip) -- to a relative 1e-8."""
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver

    case, nx, ny, bits, depth, merge = [c for c in bc.cases() if c[0] == "huge20x9"][0]
    th, dofs, tree = fcs.host_case(nx, ny, bits)
    dev = DeviceSolver(th)
    try:
        U0 = bc.smooth_advection(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.005, True)
        dev.set_sensors([th.point_eval_row((0.31, 0.42), 1)])
        dev.assemble_matrix(SLOT_BDF2, mass=300.0, nu=0.01, adv=U0, lin=U0)
        dev.apply_bc(SLOT_BDF2)
        dev.setup_solver(SLOT_BDF2, depth=depth, merge=merge)
        A0 = dev.matrix(SLOT_BDF2)
        dev.assemble_matrix(SLOT_BDF2, mass=600.0, nu=0.01, adv=U0, lin=U0, adv_scale=1.6, lin_scale=1.6)  # advection x 1.6, mass doubled
        dev.apply_bc(SLOT_BDF2)
        dev.update_operator(SLOT_BDF2)  # the factors stay those of A0
        A1 = dev.matrix(SLOT_BDF2)
        dev.set_batch(k)
        rng = np.random.default_rng(40 + k)
        u0, u1 = 1e-3 * rng.standard_normal((k, 2 * th.nn)), 1e-3 * rng.standard_normal((k, 2 * th.nn))
        dev.set_state_batch(u0, u1, np.zeros((k, th.nv)))
        _, _, info = dev.step_batch(SLOT_BDF2, np.zeros((k, 1)))
        X = dev.get_solution_batch()
        got = info[:, 1].copy()
        D = sp.csr_matrix(A0 - A1)
        want = np.array([np.linalg.norm(D @ X[s]) / np.linalg.norm(A0 @ X[s]) for s in range(k)])
        print(f"k {k}: monitor {got.min():.6e} ... {got.max():.6e}, worst disagreement {np.abs(got / want - 1).max():.2e}; |b| reported vs |A0 x| "
              f"{np.abs(info[:, 2] / np.array([np.linalg.norm(A0 @ X[s]) for s in range(k)]) - 1).max():.2e}")
        assert np.all(want > 1e-4)  # a residual that is really there
        assert np.all(np.abs(got - want) <= 1e-8 * want), f"reported {got.tolist()}, true {want.tolist()}"
        dev.set_batch(0)
    finally:
        dev.close()
