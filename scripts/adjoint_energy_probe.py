"""What the energy term of the cost (fc_set_adjoint_energy) costs the adjoint marches, and what taping a linearised run costs the forward
run: device time per backward step on the shipped cylinder mesh (O1), BDF2 steps, single march and batched at the given widths,
linearised and nonlinear, with and without weights.

    python scripts/adjoint_energy_probe.py [--steps 500] [--passes 3] [--widths 8,32] [--baseline]

Device times are the HIP events of ``fc_adjoint_info`` / ``fc_adjoint_batch_info`` (best of the passes), forward rates are wall clock
around the calls.  One JSON line.  ``--baseline``: only what exists without the energy term -- the marches without weights and the untaped
linearised forward run -- which also runs on an earlier build of the library (FC_LIB_PATH), for a comparison within one session."""
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
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--widths", default="8,32")
ap.add_argument("--baseline", action="store_true")
args = ap.parse_args()
n, widths = args.steps, [int(v) for v in args.widths.split(",") if v]

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
out = {"mesh": "cylinder O1", "N": int(dev.N), "steps": n, "unit": "us of device time per backward step (forward: steps x columns / s, wall clock)",
       "baseline": bool(args.baseline), "single": {}, "batched": {}}


def note(d, key, v, best=min):
    e = d.setdefault(key, {"passes": []})
    e["passes"].append(round(v, 2))
    e["best"] = best(e["passes"])


def forward_rate(fn, cols=1):
    t0 = time.perf_counter()
    fn()
    return cols * n / (time.perf_counter() - t0)


def single_pass():
    d = out["single"]
    dev.set_batch(0)
    for s in (0, 1):
        dev.set_adjoint_factors(s, 1)
    u, w = np.zeros((n, dev.n_act)), rng.standard_normal((n, dev.n_sens))
    march = lambda: dev.run_adjoint(SLOT_BDF2, n, w, None, state_gradients=False)  # noqa: E731
    us = lambda: 1e3 * dev.adjoint_info(1)["run_ms"] / n  # noqa: E731
    for nl in (False, True):
        kind = "nonlinear" if nl else "linearised"
        dev.set_time_scheme(dt, nl)
        if not nl:
            dev.set_state(*state0)
            note(d, "forward_linearised_untaped", forward_rate(lambda: dev.run(SLOT_BDF2, n, u, compute_energy=False)), max)
            dev.run_adjoint(SLOT_BDF2, 8, w[:8], None, state_gradients=False)  # (warm-up: the march's buffers)
            march()
            note(d, "march_linearised", us())
            if args.baseline:
                continue
        dev.adjoint_tape_reserve(n)
        dev.set_state(*state0)
        dev.adjoint_tape_begin()
        note(d, f"forward_{kind}_taped", forward_rate(lambda: dev.run(SLOT_BDF2, n, u, compute_energy=False)), max)
        if nl:
            march()
            note(d, "march_nonlinear", us())
        if not args.baseline:
            dev.set_adjoint_energy(np.full(n, 0.7))
            march()
            note(d, f"march_{kind}_energy", us())
            dev.set_adjoint_energy(None)
        dev.adjoint_tape_reserve(0)
    dev.set_time_scheme(dt, False)
    dev.set_state(*state0)


def forward_batched(u):
    for _ in range(n):
        dev.step_batch_begin(SLOT_BDF2, u, compute_energy=False)
        dev.step_batch_end_early()
    dev.step_batch_collect()


def batched_pass(k):
    d = out["batched"].setdefault(f"k{k}", {})
    dev.set_batch(k)
    un, unn, pn = (np.tile(a, (k, 1)) * (1.0 + 0.1 * np.arange(k))[:, None] for a in state0)
    u, w = np.zeros((k, dev.n_act)), rng.standard_normal((n, k, dev.n_sens))
    for s in (0, 1):
        dev.set_adjoint_factors(s, 1)
        dev.set_adjoint_batch(s, 1)
    march = lambda: dev.run_adjoint_batch(SLOT_BDF2, n, w, None, state_gradients=False)  # noqa: E731
    us = lambda: 1e3 * dev.adjoint_batch_info(1)["run_ms"] / n  # noqa: E731
    for nl in (False, True):
        kind = "nonlinear" if nl else "linearised"
        dev.set_time_scheme(dt, nl)
        if not nl:
            dev.set_state_batch(un, unn, pn)
            note(d, "forward_linearised_untaped", forward_rate(lambda: forward_batched(u), k), max)
            dev.run_adjoint_batch(SLOT_BDF2, 8, w[:8], None, state_gradients=False)  # (warm-up)
            march()
            note(d, "march_linearised", us())
            if args.baseline:
                continue
        dev.adjoint_tape_reserve_batch(n)
        dev.set_state_batch(un, unn, pn)
        dev.adjoint_tape_begin_batch()
        note(d, f"forward_{kind}_taped", forward_rate(lambda: forward_batched(u), k), max)
        if nl:
            march()
            note(d, "march_nonlinear", us())
        if not args.baseline:
            dev.set_adjoint_energy(np.full((n, k), 0.7))
            march()
            note(d, f"march_{kind}_energy", us())
            dev.set_adjoint_energy(None)
        dev.adjoint_tape_reserve_batch(0)
    dev.set_time_scheme(dt, False)
    for s in (0, 1):
        dev.set_adjoint_batch(s, -1)


for _ in range(args.passes):
    single_pass()
    for k in widths:
        batched_pass(k)
fs.th.release_device()
print(json.dumps(out))
