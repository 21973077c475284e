"""Closed loops: the host loop against the device loop, simulated steps per second on the shipped cylinder mesh with Kopt_reduced13.mat.

    python scripts/closed_loop_probe.py [--steps 500] [--warmup 50] [--passes 3] [--ks 1,8,32] [--no-profile] [--signals]

(a) host loop: ``step`` + ``Controller.step`` (k = 1); the loop of ``optim.closed_loop_costs(on_device=False)`` -- one
    ``Controller.step`` per candidate between two ``BatchedFlowSolver.step`` calls (k > 1).
(b) device loop: ``FlowSolver.run_closed_loop`` (k = 1); ``BatchedFlowSolver.run_closed_loop`` (k > 1).
``--signals``: both loops add an excitation w_u at the plant input, other rows in every column (the device loop reads them from rows
uploaded once, ``fc_set_loop_signals``; the host loop slices them step by step).
Three passes each; one JSON line with every pass, the medians, the ratios (b) / (a) and the spread of (a)'s passes, plus the mean
duration of ``fc_ctrl_step`` from one ``rocprofv3 --kernel-trace --stats`` run of the k = 32 device loop (a child process)."""
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
from flowcontrol_amd.batch import BatchedFlowSolver  # noqa: E402
from flowcontrol_amd.controller import Controller  # noqa: E402
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver  # noqa: E402
from flowcontrol_amd.examples.data import controller_file  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--ks", default="1,8,32")
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--signals", action="store_true", help="add an excitation w_u at the plant input in both loops")
ap.add_argument("--child", action="store_true", help="(internal) the profiled child: k = 32 device loop only")
args = ap.parse_args()

K0 = Controller.from_file(file=controller_file(), x0=None)
# small perturbation, moderate gains: the loops stay finite over the whole run
IC = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.01)


def controllers(k):
    gains = [0.25 + 0.75 * i / max(k - 1, 1) for i in range(k)]
    return [Controller(A=K0.A, B=K0.B, C=a * K0.C, D=a * K0.D) for a in gains]


fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=10)
U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
fs._assign_steady_state(U0, P0)
fs.params_ic = IC
fs.params_solver.throw_error = False
dt = fs.params_time.dt
n_act = fs.params_control.actuator_number


def excitation(n, k):
    """w_u (n, k, n_act): small sinusoids, another period and phase in every column"""
    s, col = np.arange(n)[:, None, None], np.arange(k)[None, :, None]
    return 1e-4 * np.sin(2 * np.pi * s / (40.0 + col) + 0.4 * col + np.arange(n_act)[None, None, :])


def single(device):
    fs.initialize_time_stepping(ic=None)
    K = controllers(1)[0]

    def go(n):
        w = excitation(n, 1)[:, 0] if args.signals else None
        if device:
            assert fs.run_closed_loop(n, K, **({"w_u": w} if args.signals else {})) is not None
            return
        for s in range(n):
            u = K.step(y=-fs.y_meas[0], dt=dt)
            assert fs.step(u_ctrl=np.full(n_act, u[0]) + w[s] if args.signals else [u[0]] * n_act) is not None

    go(args.warmup)
    t0 = time.perf_counter()
    go(args.steps)
    return args.steps / (time.perf_counter() - t0)


def batch(k, device):
    bfs = BatchedFlowSolver(fs, k)
    bfs.initialize_time_stepping(ics=[IC] * k)
    Ks = controllers(k)

    def go(n):
        w = excitation(n, k) if args.signals else None
        if device:
            assert bfs.run_closed_loop(n, Ks, **({"w_u": w} if args.signals else {})) is not None
            return
        for s in range(n):  # the loop of optim.closed_loop_costs
            u = np.zeros((k, n_act))
            for i, K in enumerate(Ks):
                if bfs.diverged[i]:
                    continue
                cmd = np.atleast_1d(np.asarray(K.step(y=-bfs.y_meas[i][0], dt=dt), dtype=float)).ravel()
                u[i] = cmd if cmd.size == n_act else cmd[0]
                if args.signals:
                    u[i] = u[i] + w[s, i]
            assert bfs.step(u) is not None

    go(args.warmup)
    t0 = time.perf_counter()
    go(args.steps)
    rate = k * args.steps / (time.perf_counter() - t0)
    assert not bfs.diverged.any()
    bfs.close()
    return rate


if args.child:
    batch(32, True)
    fs.th.release_device()
    sys.exit(0)

out = {"mesh": "cylinder O1", "controller": "Kopt_reduced13.mat", "signals": bool(args.signals), "steps": args.steps, "warmup": args.warmup, "unit": "simulated steps/s", "k": {}}
for k in [int(v) for v in args.ks.split(",")]:
    host = [single(False) if k == 1 else batch(k, False) for _ in range(args.passes)]
    dev = [single(True) if k == 1 else batch(k, True) for _ in range(args.passes)]
    mh, md = float(np.median(host)), float(np.median(dev))
    out["k"][str(k)] = {"host": [round(v, 1) for v in host], "device": [round(v, 1) for v in dev], "host_median": round(mh, 1),
                        "device_median": round(md, 1), "ratio": round(md / mh, 3), "host_spread": round((max(host) - min(host)) / mh, 3)}
fs.th.release_device()
if not args.no_profile:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, str(Path(__file__).resolve()), "--child",
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            rows = []
            for f in Path(d).rglob("*_kernel_stats.csv"):
                with open(f) as fh:
                    rows += [r for r in csv.DictReader(fh) if "fc_ctrl_step" in r["Name"]]
            if rows:
                out["fc_ctrl_step"] = {"k": 32, "calls": int(rows[0]["Calls"]), "mean_us": round(float(rows[0]["AverageNs"]) / 1e3, 3)}
            else:
                out["fc_ctrl_step"] = {"error": f"no kernel statistics (rocprofv3 exit {res.returncode})"}
        except (OSError, subprocess.TimeoutExpired) as err:
            out["fc_ctrl_step"] = {"error": str(err)}
print(json.dumps(out))
