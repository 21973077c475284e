"""The apply of the factorisation-free preconditioner (``apply_pc`` / ``pc_vcycle`` in ``csrc/fc_hip.hip``, the kernels fc_pc_csr<1|8|16|32>,
fc_pc_dense and fc_pc_final of ``csrc/fc_precond.hip.h``) against the np.longdouble host model ``tests/support/precond_model.py``, launch
list by launch list: ``fc_get_pc_route`` must report what the model predicts, so that a kernel, a lane count or an AMG level that silently
did not run fails.

Cases (``precond_model.CASES``): Mesh.unit_square(n, n) for n = 6 and 12 (no sparse AMG level: B writes the dense solve's right-hand
side, the dense kernel with n < 64 and n % 4 != 0, then two and three trips of its column loop), 16 (one sparse level) and 48 (two; G / U
rows of several hundred entries: three trips of the predicated 4 x LANES loop), n = 16 once more as an enclosed flow with the pressure
pinned; 1 to 4 Jacobi sweeps (no matrix, K_F, one further sweep -- the result in u1 --, two -- back in u0); V(1,1) and V(2,2), one fresh
child process each (FC_PC_AMG_SWEEPS is read once per process); once in the permutation the library lays out itself and once in the W
numbering (fc_set_permutation), the permutation of tests/test_precond_model_host.py, which holds the same table to the C++ header on
the CPU.  The level sizes and row lengths follow the permutation (the greedy aggregation runs in row order): in the W numbering the
launch lists reach everything in ``precond_model.REACH`` but ``MISSES`` (on the oracle's matrices: everything).  What no case
reaches is in ``precond_model.UNREACHED``.

Tolerances: 16 x the measured host errors ``precond_model.HOST_ERROR_*`` (float64 folded evaluation of the header's matrices against the
longdouble unfolded model), velocity and pressure parts apart, 2-norm and max-norm; omega to 1e-14; sizes, launch lists and repeated
applies exactly."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests.support import precond_model as pm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


#: what the launch lists that run on the device do not exercise, by permutation.  A single trip of the 4 x LANES loop: on the oracle's
#: matrices B of unit_square(16, 16) (rows of up to 29 entries at 8 lanes) and U_1 of unit_square(48, 48) under V(1,1) (63 at 16 lanes)
#: stay within one trip; the matrix the device assembles stores more non-zero entries per row (B: up to 36, U_1: 66), and every
#: matrix of every case has a row beyond 4 x LANES.  Two trips run the loop body once whole and once predicated: a single trip adds no
#: path of its own.  Three trips: in the library's own permutation level 1 of unit_square(48, 48) has 287 rows (389 in the W
#: numbering) and its G / U rows stay within two.
MISSES = {"tree": {"csr one trip", "csr three trips"}, "identity": {"csr one trip"}}


@pytest.mark.parametrize("perm_kind", ["tree", "identity"])
def test_every_apply_route_against_the_host_model(perm_kind):
    reached = set()
    for amg in pm.AMG_SWEEPS:  # one child after the other; the first that fails ends the test
        env = dict(os.environ, PYTHONPATH=str(ROOT), FC_PC_AMG_SWEEPS=str(amg))
        out = subprocess.run([sys.executable, str(ROOT / "tests" / "support" / "precond_child.py"), str(amg), perm_kind], env=env, capture_output=True, text=True,
                             timeout=240, cwd=ROOT)
        print(out.stdout[-12000:])
        assert out.returncode == 0, f"V({amg},{amg}): exit status {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}"
        assert f"CHILD OK {amg}" in out.stdout
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("REACH ")]
        assert len(line) == 1
        reached |= set(json.loads(line[0][len("REACH "):]))
    want = set(pm.REACH) - MISSES[perm_kind]
    assert reached - set(pm.UNREACHED) == want, (sorted(want - reached), sorted(reached - want - set(pm.UNREACHED)))
