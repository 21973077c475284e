"""What the closed-loop tangent march costs on the shipped cylinder mesh (O1, nonlinear) with the 13-state controller, BDF2 steps
(DESIGN §5.6 "Closed loop"):

  (a) steps / s of ``fc_run_tangent_closed_loop`` beside ``fc_run_tangent`` over the SAME taped closed-loop run (the open-loop march is
      the code path that existed before the closed-loop one), single march, and columns x steps / s of the two batched marches per
      width -- in one process, alternating the two, the median of the passes, from the HIP events inside the march and by the wall clock,
  (b) the same for the two ADJOINT marches (``fc_run_adjoint`` / ``fc_run_adjoint_closed_loop`` and their batched forms) in the same
      session: what the controller's launch adds per step there,
  (c) bytes the tangent buffers hold after the reserve, after an open-loop march and after a closed-loop march.

    python scripts/tangent_loop_probe.py [--steps 2000] [--batch-steps 400] [--passes 5] [--widths 0,8,32] [--limit 300]

Width 0 is the single march.  One child process per width, each under its own time limit (``--limit`` seconds); the first child that
fails or runs out of time ends the run.  One JSON line per width.  The device time of the controller's kernel alone comes from a kernel
trace of one child in a run of its own (``--child 8 --passes 1`` under the profiler)."""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--batch-steps", type=int, default=400)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--widths", default="0,8,32")
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--child", type=int, default=-1, help="(internal) measure this width in this process")
args = ap.parse_args()

if args.child < 0:
    for k in (int(v) for v in args.widths.split(",")):
        cmd = [sys.executable, __file__, "--child", str(k), "--steps", str(args.steps), "--batch-steps", str(args.batch_steps), "--passes", str(args.passes)]
        try:
            res = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"k = {k}: no result within {args.limit} s; stopping")
        if res.returncode != 0:
            sys.exit(f"k = {k}: exit status {res.returncode}; stopping")
    sys.exit(0)

import numpy as np  # noqa: E402

from flowcontrol_amd._lib import SLOT_BDF2  # noqa: E402
from flowcontrol_amd.controller import Controller  # noqa: E402
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver  # noqa: E402
from flowcontrol_amd.examples.data import controller_file  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402

k = args.child
n = args.batch_steps if k else args.steps
cols = max(k, 1)
fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=10)
fs.params_solver.is_eq_nonlinear = True
U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
fs._assign_steady_state(U0, P0)
fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.01)
fs.initialize_time_stepping(ic=None)
fs._begin_stepping()
dev = fs.th.device()
dt = fs.params_time.dt
dev.set_solver_options(refine=0, check_residual=0)
state0 = [np.array(a, copy=True) for a in dev.get_state()]
rng = np.random.default_rng(0)
K0 = Controller.from_file(file=controller_file(), x0=None)
Ks = [Controller(K0.A, K0.B, K0.C, K0.D, x0=0.01 * rng.standard_normal(K0.nstates)) for _ in range(cols)]
out = {"mesh": "cylinder O1", "N": int(dev.N), "k": k, "steps": n, "passes": args.passes, "controller_states": int(K0.nstates)}
lead = (k,) if k else ()
for s in (0, 1):
    dev.set_adjoint_factors(s, 1)

# one taped closed-loop run: both tangent marches and both adjoint marches read its tapes
if k:
    dev.set_batch(k)
    for s in (0, 1):
        dev.set_adjoint_batch(s, 1)
    dev.set_state_batch(*(np.tile(a, (k, 1)) * (1.0 + 0.1 * np.arange(k))[:, None] for a in state0))
    dev.adjoint_tape_reserve_batch(n)
dev.set_controllers(Ks, dt)
bank = dev._ctrl_bank
if k:
    dev.adjoint_loop_reserve_batch(n)
    dev.adjoint_tape_begin_batch()
    dev.adjoint_loop_begin_batch()
    dev.run_closed_loop_batch(SLOT_BDF2, n, np.zeros((k, dev.n_sens)), compute_energy=False)
else:
    dev.adjoint_tape_reserve(n)
    dev.adjoint_loop_reserve(n)
    dev.adjoint_tape_begin()
    dev.adjoint_loop_begin()
    dev.run_closed_loop(SLOT_BDF2, n, np.zeros(dev.n_sens), compute_energy=False)

du = rng.standard_normal((n, *lead, dev.n_act))
direction = {q: rng.standard_normal((*lead, *np.shape(bank[q][0]))) for q in ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0")}
direction["w_u"] = du
w, r = rng.standard_normal((n, *lead, dev.n_sens)), rng.standard_normal((n, *lead, dev.n_act))
dev.tangent_reserve(1)
held = {"after_reserve": dev.tangent_info()["bytes"]}

tan_ms = lambda: dev.tangent_info()["run_ms"]  # noqa: E731
adj_ms = (lambda: dev.adjoint_batch_info(1)["run_ms"]) if k else (lambda: dev.adjoint_info(1)["run_ms"])
if k:
    marches = {"tangent_open_loop": (lambda: dev.run_tangent_batch(SLOT_BDF2, n, du), tan_ms),
               "tangent_closed_loop": (lambda: dev.run_tangent_closed_loop_batch(SLOT_BDF2, n, direction), tan_ms),
               "adjoint_open_loop": (lambda: dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False), adj_ms),
               "adjoint_closed_loop": (lambda: dev.run_adjoint_closed_loop_batch(SLOT_BDF2, n, w, r, None, state_gradients=False), adj_ms)}
else:
    marches = {"tangent_open_loop": (lambda: dev.run_tangent(SLOT_BDF2, n, du), tan_ms),
               "tangent_closed_loop": (lambda: dev.run_tangent_closed_loop(SLOT_BDF2, n, direction), tan_ms),
               "adjoint_open_loop": (lambda: dev.run_adjoint(SLOT_BDF2, n, w, None, state_gradients=False), adj_ms),
               "adjoint_closed_loop": (lambda: dev.run_adjoint_closed_loop(SLOT_BDF2, n, w, r, None, state_gradients=False), adj_ms)}
times = {name: ([], []) for name in marches}
for name, (run, _) in marches.items():  # (warm-up: every march sizes its buffers)
    run()
    if name == "tangent_open_loop":
        held["after_open_loop_march"] = dev.tangent_info()["bytes"]
    if name == "tangent_closed_loop":
        held["after_closed_loop_march"] = dev.tangent_info()["bytes"]
for _ in range(args.passes):  # alternating, so that drift hits all four alike
    for name, (run, ms) in marches.items():
        t0 = time.perf_counter()
        run()
        times[name][0].append(time.perf_counter() - t0)
        times[name][1].append(1e-3 * ms())
for name, (wall, device) in times.items():
    out[name] = {"rate_device": round(cols * n / float(np.median(device)), 1), "rate_wall": round(cols * n / float(np.median(wall)), 1),
                 "us_per_step_device": round(1e6 * float(np.median(device)) / n, 2)}
for kind in ("tangent", "adjoint"):
    a, b = out[f"{kind}_closed_loop"], out[f"{kind}_open_loop"]
    out[f"{kind}_closed_over_open"] = round(a["rate_device"] / b["rate_device"], 4)
    out[f"{kind}_controller_us_per_step"] = round(a["us_per_step_device"] - b["us_per_step_device"], 2)
held["closed_loop_beyond_open_loop"] = held["after_closed_loop_march"] - held["after_open_loop_march"]
out["tangent_bytes"] = held
fs.th.release_device()
print(json.dumps(out), flush=True)
