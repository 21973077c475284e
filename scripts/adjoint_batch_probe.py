"""The batched adjoint march against k single marches, and what the batched state tape costs in the forward run: columns x steps per
second on the shipped cylinder mesh (O1), BDF2 steps, wall clock around the calls and HIP events inside them.

    python scripts/adjoint_batch_probe.py [--steps 2000] [--passes 3] [--widths 8,16,32] [--baseline]

Per pass, alternating: the single ``fc_run_adjoint`` (linearised, then nonlinear over its state tape), then for every k the forward
batched step rate without and with the batched tape, and ``fc_run_adjoint_batch`` linearised and nonlinear.  One JSON line with every
pass, the best of each, the memory held (tiled transposed copy per slot, march buffers, tape at its capacity) and the ratio of the
batched to the single march.  ``--baseline``: only what existed before the batched march (the single march and the untaped forward
batched rate) -- the part that also runs on an earlier build of the library, for a comparison within one session."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowcontrol_amd._lib import SLOT_BDF2  # noqa: E402
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--widths", default="8,16,32")
ap.add_argument("--baseline", action="store_true")
args = ap.parse_args()
n, widths = args.steps, [int(v) for v in args.widths.split(",")]

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
u1 = np.zeros((n, dev.n_act))
w1 = rng.standard_normal((n, dev.n_sens))
out = {"mesh": "cylinder O1", "N": int(dev.N), "steps": n, "unit": "columns x steps / s", "single": {}, "batched": {}, "memory": {}}


def rate(fn, cols=1):
    t0 = time.perf_counter()
    fn()
    return cols * n / (time.perf_counter() - t0)


def note(d, key, v, ms=None):
    e = d.setdefault(key, {"passes": []})
    e["passes"].append(round(v, 1))
    e["best"] = max(e["passes"])
    if ms is not None:
        e["event_ms"] = round(min(ms, e.get("event_ms", ms)), 2)


def single_pass():
    dev.set_batch(0)
    for s in (0, 1):
        dev.set_adjoint_factors(s, 1)
    dev.set_time_scheme(dt, False)
    dev.run_adjoint(SLOT_BDF2, 8, w1[:8], None, state_gradients=False)  # (warm-up: the march's buffers)
    note(out["single"], "march_linearised", rate(lambda: dev.run_adjoint(SLOT_BDF2, n, w1, None, state_gradients=False)), dev.adjoint_info(1)["run_ms"])
    dev.set_time_scheme(dt, True)
    dev.adjoint_tape_reserve(n)
    dev.set_state(*state0)
    dev.adjoint_tape_begin()
    note(out["single"], "forward_taped", rate(lambda: dev.run(SLOT_BDF2, n, u1, compute_energy=False)))
    note(out["single"], "march_nonlinear", rate(lambda: dev.run_adjoint(SLOT_BDF2, n, w1, None, state_gradients=False)), dev.adjoint_info(1)["run_ms"])
    dev.adjoint_tape_reserve(0)
    dev.set_time_scheme(dt, False)
    dev.set_state(*state0)
    note(out["single"], "forward", rate(lambda: dev.run(SLOT_BDF2, n, u1, compute_energy=False)))


def forward_batched(k, u):
    """the stepping loop of BatchedFlowSolver.step: begin, early end"""
    for m in range(n):
        dev.step_batch_begin(SLOT_BDF2, u, compute_energy=False)
        dev.step_batch_end_early()
    dev.step_batch_collect()


def batched_pass(k):
    d = out["batched"].setdefault(f"k{k}", {})
    dev.set_batch(k)
    un, unn, pn = (np.tile(a, (k, 1)) * (1.0 + 0.1 * np.arange(k))[:, None] for a in state0)
    u = np.zeros((k, dev.n_act))
    dev.set_time_scheme(dt, False)
    dev.set_state_batch(un, unn, pn)
    note(d, "forward", rate(lambda: forward_batched(k, u), k))
    if args.baseline:
        return
    w = rng.standard_normal((n, k, dev.n_sens))
    for s in (0, 1):
        dev.set_adjoint_factors(s, 1)
        dev.set_adjoint_batch(s, 1)
    dev.run_adjoint_batch(SLOT_BDF2, 8, w[:8], None, state_gradients=False)  # (warm-up)
    note(d, "march_linearised", rate(lambda: dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False), k), dev.adjoint_batch_info(1)["run_ms"])
    dev.set_time_scheme(dt, True)
    dev.adjoint_tape_reserve_batch(n)
    dev.set_state_batch(un, unn, pn)
    dev.adjoint_tape_begin_batch()
    note(d, "forward_taped", rate(lambda: forward_batched(k, u), k))
    note(d, "march_nonlinear", rate(lambda: dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False), k), dev.adjoint_batch_info(1)["run_ms"])
    info = dev.adjoint_batch_info(1)
    out["memory"][f"k{k}"] = {"tile_bytes_per_slot": info["tile_bytes"], "march_bytes": info["march_bytes"], "tape_bytes": info["tape_bytes"], "KB": info["KB"]}
    dev.adjoint_tape_reserve_batch(0)
    dev.set_time_scheme(dt, False)
    dev.set_state_batch(un, unn, pn)
    note(d, "forward_after", rate(lambda: forward_batched(k, u), k))
    for s in (0, 1):
        dev.set_adjoint_batch(s, -1)


for _ in range(args.passes):
    single_pass()
    for k in widths:
        batched_pass(k)
if not args.baseline:
    for k in widths:
        d = out["batched"][f"k{k}"]
        d["ratio_linearised"] = round(d["march_linearised"]["best"] / out["single"]["march_linearised"]["best"], 2)
        d["ratio_nonlinear"] = round(d["march_nonlinear"]["best"] / out["single"]["march_nonlinear"]["best"], 2)
fs.th.release_device()
print(json.dumps(out))
