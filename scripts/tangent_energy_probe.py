"""What the tangent of the energy costs on the shipped cylinder mesh (O1, nonlinear), BDF2 steps (DESIGN §5.6 "Energy"):

  (a) µs per step of ``fc_run_tangent`` (width 0) and of ``fc_run_tangent_batch`` (widths 8, 32) with the energy option off, with it on,
      and -- single march -- with the tangent tape kept: in one process, alternating, the median of the passes, from the HIP events
      inside the march,
  (b) µs per backward step of ``fc_run_adjoint`` with energy weights held, source 0 (the state tape) against source 1 (the tangent tape),
  (c) one ``closed_loop_gauss_newton_product`` of the 13-state controller with and without ``energy=`` (wall clock, 200 steps),
  (d) the bytes held: tangent buffers without and with the option, the tangent tape.

    python scripts/tangent_energy_probe.py [--steps 2000] [--batch-steps 400] [--passes 5] [--widths 0,8,32] [--limit 300] [--off-only]

``--off-only`` measures (a) with the option off alone, through entry points that existed before the option: run it on the parent commit's
tree and library (one process per build, alternating with this commit's in one session) for the comparison of the off path.  One child
process per width, each under its own time limit; the first child that fails or runs out of time ends the run.  One JSON line per width."""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--batch-steps", type=int, default=400)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--widths", default="0,8,32")
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--tree", type=Path, default=ROOT, help="the source tree whose package is measured (default: this one)")
ap.add_argument("--child", type=int, default=-1, help="(internal) measure this width in this process")
args = ap.parse_args()
sys.path.insert(0, str(args.tree))

if args.child < 0:
    for k in (int(v) for v in args.widths.split(",")):
        cmd = [sys.executable, __file__, "--child", str(k), "--steps", str(args.steps), "--batch-steps", str(args.batch_steps), "--passes", str(args.passes),
               "--tree", str(args.tree)] + (["--off-only"] if args.off_only else [])
        try:
            res = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"k = {k}: no result within {args.limit} s; stopping")
        if res.returncode != 0:
            sys.exit(f"k = {k}: exit status {res.returncode}; stopping")
    sys.exit(0)

import numpy as np  # noqa: E402

from flowcontrol_amd import utils as flu  # noqa: E402
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
dev.set_solver_options(refine=0, check_residual=0)
state0 = [np.array(a, copy=True) for a in dev.get_state()]
rng = np.random.default_rng(0)
out = {"mesh": "cylinder O1", "N": int(dev.N), "k": k, "steps": n, "passes": args.passes, "off_only": bool(args.off_only), "tree": str(args.tree.name)}
lead = (k,) if k else ()
u = 0.01 * rng.standard_normal((n, *lead, dev.n_act))
du = rng.standard_normal((n, *lead, dev.n_act))

# one taped forward run: every march reads its tape
if k:
    dev.set_batch(k)
    dev.set_state_batch(*(np.tile(a, (k, 1)) * (1.0 + 0.1 * np.arange(k))[:, None] for a in state0))
    dev.adjoint_tape_reserve_batch(n)
    dev.adjoint_tape_begin_batch()
    for m in range(n):
        dev.step_batch(SLOT_BDF2, u[m], compute_energy=False)
    tangent = lambda: dev.run_tangent_batch(SLOT_BDF2, n, du)  # noqa: E731
else:
    for s in (0, 1):
        dev.set_adjoint_factors(s, 1)
    dev.adjoint_tape_reserve(n)
    dev.adjoint_tape_begin()
    dev.run(SLOT_BDF2, n, u, compute_energy=False)
    tangent = lambda: dev.run_tangent(SLOT_BDF2, n, du)  # noqa: E731
dev.tangent_reserve(1)
tan_ms = lambda: dev.tangent_info()["run_ms"]  # noqa: E731
held = {}


def set_mode(mode):
    if args.off_only:
        return
    dev.tangent_set_energy(1 if mode in ("on", "on_tape") else 0)
    if not k:
        dev.tangent_tape_reserve(n if mode == "on_tape" else 0)


modes = ["off"] if args.off_only else (["off", "on"] + ([] if k else ["on_tape"]))
times = {m: [] for m in modes}
for m in modes:  # (warm-up: every mode sizes its buffers)
    set_mode(m)
    tangent()
    held[f"tangent_bytes_{m}"] = dev.tangent_info()["bytes"]
    if m == "on_tape":
        held["tangent_tape_bytes"] = dev.tangent_tape_info()["bytes"]
for _ in range(args.passes):  # alternating, so that drift hits all alike
    for m in modes:
        set_mode(m)
        tangent()
        times[m].append(1e-3 * tan_ms())
for m in modes:
    out[f"tangent_{m}_us_per_step"] = round(1e6 * float(np.median(times[m])) / n, 2)
    out[f"tangent_{m}_spread"] = round((max(times[m]) - min(times[m])) / float(np.median(times[m])), 4)
if not args.off_only:
    out["energy_us_per_step"] = round(out["tangent_on_us_per_step"] - out["tangent_off_us_per_step"], 2)
    if not k:
        out["tape_us_per_step"] = round(out["tangent_on_tape_us_per_step"] - out["tangent_on_us_per_step"], 2)
        # (b) the adjoint march with the weights held, the two sources alternating (the tangent tape holds the last march)
        set_mode("on_tape")
        tangent()
        w, e = rng.standard_normal((n, dev.n_sens)), np.full(n, 0.5)
        dev.set_adjoint_energy(e)
        adj = {0: [], 1: []}
        for p in range(args.passes + 1):
            for source in (0, 1):
                dev.set_adjoint_energy_source(source)
                dev.run_adjoint(SLOT_BDF2, n, w, None, state_gradients=False)
                if p:
                    adj[source].append(1e-3 * dev.adjoint_info(1)["run_ms"])
        dev.set_adjoint_energy(None)
        for source in (0, 1):
            out[f"adjoint_source{source}_us_per_step"] = round(1e6 * float(np.median(adj[source])) / n, 2)
        set_mode("off")
        # (c) one closed-loop product with and without the energy weights
        dev.tangent_reserve(0)
        dev.adjoint_tape_reserve(0)
        dev.set_state(*state0)
        K = Controller.from_file(file=controller_file(), x0=None)
        steps = 200
        Q, R = np.eye(dev.n_sens), 1e-3 * np.eye(dev.n_act)
        v = {q: rng.standard_normal(np.shape(getattr(K, q))) for q in ("A", "B", "C", "D")}
        with flu.AdjointRun(fs, tape=steps, loop=steps) as run:
            for name, kw in (("sensors", {}), ("energy", {"energy": np.full(steps, 1.0 / steps)})):
                wall = []
                for p in range(3):
                    t0 = time.perf_counter()
                    flu.closed_loop_gauss_newton_product(fs, K, steps, Q, R, v, adjoint=run, **kw)
                    wall.append(time.perf_counter() - t0)
                out[f"closed_loop_product_{name}_ms"] = round(1e3 * float(np.median(wall[1:])), 2)
out["bytes"] = held
fs.th.release_device()
print(json.dumps(out), flush=True)
