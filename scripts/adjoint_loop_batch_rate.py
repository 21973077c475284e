"""What the batched closed-loop adjoint costs on the shipped cylinder mesh (O1) with k copies of the 13-state controller, BDF2 steps,
linearised and nonlinear (DESIGN §5.4 "Batched closed loops"):

  (a) columns x steps / s of ``fc_run_adjoint_closed_loop_batch`` beside ``fc_run_adjoint_batch`` at the same k on the same run,
  (b) simulated steps / s of ``fc_run_closed_loop_batch`` with the tapes on (loop tape; nonlinear: and the batched state tape) beside
      the untaped rate,
  (c) microseconds per backward step with the g reduction as a launch of its own (the default) and inside the controller launch
      (``FC_ADJ_LOOP_FUSE=1``), from the HIP events inside the march,
  (d) bytes held: loop tape, bank copy, adjoint rows and the rest of the loop buffers.

    python scripts/adjoint_loop_batch_rate.py [--steps 400] [--passes 3] [--widths 8,16,32] [--limit 300] [--baseline]

One child process per width, each under its own time limit (``--limit`` seconds); the first child that fails or runs out of time ends
the run.  ``--baseline`` measures only what existed before the batched closed-loop adjoint -- ``fc_run_adjoint_batch`` and the untaped
``fc_run_closed_loop_batch`` -- so the same script gives the denominators of (a) and (b) on an earlier commit's build.  One JSON line
per width."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--widths", default="8,16,32")
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--child", type=int, default=0, help="(internal) measure this width in this process")
args = ap.parse_args()

if not args.child:
    for k in (int(v) for v in args.widths.split(",")):
        cmd = [sys.executable, __file__, "--child", str(k), "--steps", str(args.steps), "--passes", str(args.passes)] + (["--baseline"] if args.baseline else [])
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

k, n = args.child, args.steps
fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=10)
fs.params_solver.is_eq_nonlinear = False
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
Ks = [Controller(K0.A, K0.B, K0.C, K0.D, x0=0.01 * rng.standard_normal(K0.nstates)) for _ in range(k)]
out = {"mesh": "cylinder O1", "N": int(dev.N), "k": k, "steps": n, "controller_states": int(K0.nstates), "baseline": bool(args.baseline)}


def best(fn, cols):
    """best of the passes: (columns x steps / s by the wall clock, whatever fn returns at that pass)"""
    top = (0.0, None)
    for _ in range(args.passes):
        t0 = time.perf_counter()
        extra = fn()
        r = cols * n / (time.perf_counter() - t0)
        if r > top[0]:
            top = (r, extra)
    return top


dev.set_batch(k)
un, unn, pn = (np.tile(a, (k, 1)) * (1.0 + 0.1 * np.arange(k))[:, None] for a in state0)
y0 = np.zeros((k, dev.n_sens))
w = rng.standard_normal((n, k, dev.n_sens))
r = rng.standard_normal((n, k, dev.n_act))
for s in (0, 1):
    dev.set_adjoint_factors(s, 1)
    dev.set_adjoint_batch(s, 1)
new = not args.baseline and hasattr(dev, "run_adjoint_closed_loop_batch")

for nonlinear in (False, True):
    d = out["nonlinear" if nonlinear else "linearised"] = {}
    dev.set_time_scheme(dt, nonlinear)
    dev.set_controllers(Ks, dt)

    def closed_loop(taped):
        dev.set_state_batch(un, unn, pn)
        dev.controller_state(np.array([K.x for K in Ks]))
        if taped:
            if nonlinear:
                dev.adjoint_tape_begin_batch()
            dev.adjoint_loop_begin_batch()
        t0 = time.perf_counter()
        dev.run_closed_loop_batch(SLOT_BDF2, n, y0, compute_energy=False)
        return time.perf_counter() - t0

    closed_loop(False)  # (warm-up)
    d["closed_loop_untaped"] = round(k * n / min(closed_loop(False) for _ in range(args.passes)), 1)
    # the open-loop batched march of the same k (nonlinear: over the state tape of n open-loop batched steps)
    if nonlinear:
        dev.adjoint_tape_reserve_batch(n)
        dev.set_state_batch(un, unn, pn)
        dev.adjoint_tape_begin_batch()
        for m in range(n):
            dev.step_batch(SLOT_BDF2, np.zeros((k, dev.n_act)), compute_energy=False)
    dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False)  # (warm-up: the march's buffers)
    rate, ms = best(lambda: (dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False), dev.adjoint_batch_info(1)["run_ms"])[1], k)
    d["march_open_loop"] = {"rate": round(rate, 1), "us_per_step": round(1e3 * ms / n, 2)}
    if new:
        dev.adjoint_loop_reserve_batch(n)
        closed_loop(True)  # (warm-up)
        d["closed_loop_taped"] = round(k * n / min(closed_loop(True) for _ in range(args.passes)), 1)
        d["taped_over_untaped"] = round(d["closed_loop_taped"] / d["closed_loop_untaped"], 4)
        for fuse in ("0", "1"):
            os.environ["FC_ADJ_LOOP_FUSE"] = fuse
            march = lambda: (dev.run_adjoint_closed_loop_batch(SLOT_BDF2, n, w, r, None, state_gradients=False), dev.adjoint_batch_info(1)["run_ms"])[1]  # noqa: E731
            march()  # (warm-up)
            rate, ms = best(march, k)
            d["march_closed_loop" if fuse == "0" else "march_closed_loop_fused"] = {"rate": round(rate, 1), "us_per_step": round(1e3 * ms / n, 2)}
        os.environ.pop("FC_ADJ_LOOP_FUSE")
        d["closed_over_open_loop"] = round(d["march_closed_loop"]["rate"] / d["march_open_loop"]["rate"], 3)
        info, bank = dev.adjoint_loop_info_batch(), dev._ctrl_bank
        stride = sum(int(np.size(bank[q][0])) for q in ("Ad", "Bd", "C", "D", "G", "g0", "S"))
        tape_b, bank_b = 8 * n * k * info["row"], 8 * k * stride
        d["bytes"] = {"loop_tape": tape_b, "bank_copy": bank_b, "adjoint_rows_and_buffers": info["bytes"] - tape_b - bank_b,
                      "state_tape": dev.adjoint_tape_info_batch()["bytes"], "per_step_loop_tape": 8 * k * info["row"]}
        dev.adjoint_loop_reserve_batch(0)
    if nonlinear:
        dev.adjoint_tape_reserve_batch(0)
    dev.set_controllers(None, dt)

fs.th.release_device()
print(json.dumps(out), flush=True)
