"""Child process of tests/test_krylov_free_gpu.py::test_graph_replay_equals_plain_launches: five open-loop time steps of the cylinder
case (O1) on a factor-free GMRES slot, under whatever FC_KRYLOV_GRAPH the parent put into the environment (the library reads the knob
once per process).

    python krylov_graph_child.py <golden dir> <output dir>

Prints one line ``RESULT <json>``: the GMRES iterations of every step and the SHA-256 of the bits of every step's velocity field and
solve record (iterations, residual)."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np


def main(golden: Path, out: Path) -> None:
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    g = np.load(golden / "cylinder_O1.npz")
    fs = CylinderFlowSolver.make_default(Re=100, path_out=out, num_steps=5)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    fs.krylov_precond, fs.krylov_method, fs.krylov_max_iter, fs.krylov_rtol = "schur_amg", "gmres", 300, 1e-11
    U0, P0 = Function(fs.W, g["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.initialize_time_stepping(ic=None)
    its, bits = [], []
    for _ in range(5):
        fs.step([0.0, 0.0])
        its.append(int(fs.solve_info[0]))
        u = fs.fields.u_.vector().get_local()
        assert np.all(np.isfinite(u))
        state = np.r_[u, np.asarray(fs.solve_info, dtype=float)[:2]]
        bits.append(hashlib.sha256(np.ascontiguousarray(state).tobytes()).hexdigest())
    fs.th.release_device()
    print("RESULT " + json.dumps({"iterations": its, "bits": bits}), flush=True)


if __name__ == "__main__":
    main(Path(sys.argv[1]), Path(sys.argv[2]))
