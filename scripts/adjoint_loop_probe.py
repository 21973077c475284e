"""The adjoint of a closed loop: what the controller costs inside the backward march and what the loop tape costs in the forward run,
steps per second on the shipped cylinder mesh (linearised about the base flow).

    python scripts/adjoint_loop_probe.py [--steps 2000] [--passes 3] [--no-profile]

(a) ``fc_run_adjoint_closed_loop`` against ``fc_run_adjoint`` at the same n, with Kopt_reduced13.mat (13 states) and with a random
    stable controller of 256 states (wall clock around the call, the download of the rows included; best of ``--passes``).
(b) ``fc_run_closed_loop`` with the loop tape begun against the same run without a reserve.
One JSON line with every pass, the best of each and the ratios, plus the mean durations of ``fc_ctrl_adj_step`` and
``fc_ctrl_adj_grads`` from one ``rocprofv3 --kernel-trace --stats`` run of its own (a child process: the 13-state march only)."""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2  # noqa: E402
from flowcontrol_amd.controller import Controller  # noqa: E402
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver  # noqa: E402
from flowcontrol_amd.examples.data import controller_file  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--child", action="store_true", help="(internal) the profiled child: one 13-state forward run and march")
args = ap.parse_args()
n = args.steps

fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=10)
fs.params_solver.is_eq_nonlinear = False
U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
fs._assign_steady_state(U0, P0)
fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.01)
fs.initialize_time_stepping(ic=None)
fs._begin_stepping()
dev = fs.th.device()
dt = fs.params_time.dt
slot = SLOT_BDF1 if fs.order == 1 else SLOT_BDF2
state0 = [np.array(a, copy=True) for a in dev.get_state()]
y0 = np.array(fs.y_meas, dtype=float)
rng = np.random.default_rng(0)
w, r = rng.standard_normal((n, dev.n_sens)), rng.standard_normal((n, dev.n_act))


def controller(nx):
    K0 = Controller.from_file(file=controller_file(), x0=None)
    if nx == K0.nstates:
        return Controller(A=K0.A, B=K0.B, C=0.5 * K0.C, D=0.5 * K0.D)
    A = rng.standard_normal((nx, nx))
    A -= (max(np.linalg.eigvals(A).real) + 1.0) * np.eye(nx)  # stable
    return Controller(A, rng.standard_normal((nx, 1)) / np.sqrt(nx), 1e-3 * rng.standard_normal((1, nx)) / np.sqrt(nx), np.zeros((1, 1)))


def forward(K, tape):
    """steps/s of one closed-loop run from the start state, with or without the loop tape"""
    dev.set_state(*state0)
    dev.set_controllers([K], dt)
    if tape:
        dev.adjoint_loop_reserve(n)
        dev.adjoint_loop_begin()
    t0 = time.perf_counter()
    dev.run_closed_loop(slot, n, y0, compute_energy=False)
    return n / (time.perf_counter() - t0)


def best(fn):
    v = [fn() for _ in range(args.passes)]
    return {"passes": [round(x, 1) for x in v], "best": round(max(v), 1)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return n / (time.perf_counter() - t0)


for s in (SLOT_BDF1, SLOT_BDF2):
    dev.set_adjoint_factors(s, 1)
if args.child:
    forward(controller(13), True)
    dev.run_adjoint_closed_loop(slot, n, w, r, None, state_gradients=False)
    fs.th.release_device()
    sys.exit(0)

out = {"mesh": "cylinder O1", "steps": n, "unit": "steps/s", "march": {}, "forward": {}}
dev.run_adjoint(slot, n, w, None, state_gradients=False)  # (warm-up: the march's buffers)
out["march"]["open_loop"] = best(lambda: timed(lambda: dev.run_adjoint(slot, n, w, None, state_gradients=False)))
for nx in (13, 256):
    K = controller(nx)
    off = best(lambda: forward(K, False))
    dev.adjoint_loop_reserve(0)
    on = best(lambda: forward(K, True))
    out["forward"][f"nx{nx}"] = {"tape_off": off, "tape_on": on, "ratio": round(on["best"] / off["best"], 4), "row_bytes": 8 * dev.adjoint_loop_info()["row"]}
    closed = best(lambda: timed(lambda: dev.run_adjoint_closed_loop(slot, n, w, r, None, state_gradients=False)))
    out["march"][f"closed_loop_nx{nx}"] = dict(closed, ratio=round(closed["best"] / out["march"]["open_loop"]["best"], 4))
    dev.set_controllers(None, dt)
fs.th.release_device()
if not args.no_profile:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, str(Path(__file__).resolve()), "--child",
               "--steps", str(n)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            found = {}
            for f in Path(d).rglob("*_kernel_stats.csv"):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        for name in ("fc_ctrl_adj_step", "fc_ctrl_adj_grads", "fc_ctrl_step"):
                            if row["Name"].startswith(name):
                                found[name] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 3)}
            out["kernels"] = found or {"error": f"no kernel statistics (rocprofv3 exit {res.returncode})"}
        except (OSError, subprocess.TimeoutExpired) as err:
            out["kernels"] = {"error": str(err)}
print(json.dumps(out))
