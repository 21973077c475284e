"""What the checkpointed state tape costs (DESIGN §5.4 "Checkpointed tape"): the cylinder's O1 mesh, nonlinear equations, n = 1000 steps,
spacing "auto": a single run, then batches of k = 8 and k = 32, printed as ONE JSON line.  One process, `--passes` alternating passes behind a warm-up pass; median and
spread (min, max) per figure.

  forward_ms         wall ms of one fc_run of n steps (one synchronisation, the sensor rows read back at the end, no energy) without a
                     tape, onto the dense tape and onto the checkpointed tape -- the taping cost of either
  march_dense_ms     HIP-event ms of fc_run_adjoint over the dense tape
  march_sparse_ms    HIP-event ms of fc_run_adjoint over the checkpointed tape: the same backward steps plus `replayed` forward steps
  expected_sparse_ms march_dense_ms + forward_ms["none"] * replayed / n -- the expectation to hold march_sparse_ms against
  bytes              held by either tape

The gradients of both marches are compared bit for bit in every pass.  Batched widths ("widths"): the same figures with
fc_run_adjoint_batch; their forward run is the stepping loop of BatchedFlowSolver.step (fc_step_batch_begin, early end: one host
round trip per step), which a replayed step -- enqueued with no host in between -- does not pay, so the expectation is an upper bound there.

    python scripts/adjoint_ckpt_probe.py [--steps 1000] [--passes 5] [--every auto] [--widths 8,32]
"""
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
from flowcontrol_amd.adjoint import AdjointRun, checkpoint_spacing  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402


def _cylinder():
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(prefix="fc_ckpt_"), num_steps=10)
    fs.params_solver.is_eq_nonlinear = True
    U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=0.01)
    fs.initialize_time_stepping(ic=None)
    return fs


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def probe_width(fs, k, n, passes, every):
    """The batch of k: forward stepping loop untaped / dense / checkpointed, the two batched marches, bytes held."""
    from flowcontrol_amd.batch import BatchedFlowSolver

    bfs = BatchedFlowSolver(fs, k)
    fig = {q: [] for q in ("forward_none_ms", "forward_dense_ms", "forward_sparse_ms", "march_dense_ms", "march_sparse_ms")}
    held, replayed = {}, 0
    with AdjointRun(bfs, tape=n) as run:
        dev = run.dev
        start = dev.get_state_batch()
        rng = np.random.default_rng(0)
        u = 1e-3 * rng.standard_normal((k, max(dev.n_act, 1)))
        w = rng.standard_normal((n, k, dev.n_sens))

        def loop():
            for _ in range(n):
                dev.step_batch_begin(SLOT_BDF2, u, compute_energy=False)
                dev.step_batch_end_early()
            dev.step_batch_collect()

        def forward(mode):
            if mode == "none":
                dev.adjoint_tape_reserve_batch(0)
            elif mode == "dense":
                dev.adjoint_tape_reserve_batch(n)
            else:
                dev.adjoint_tape_reserve_sparse_batch(n, every)
            dev.set_state_batch(*start)
            if mode != "none":
                dev.adjoint_tape_begin_batch()
                held[mode] = dev.adjoint_tape_info_batch()["bytes"]
            return wall_ms(loop)[0]

        for p in range(passes + 1):
            t_none = forward("none")
            t_dense = forward("dense")
            g_dense = dev.run_adjoint_batch(SLOT_BDF2, n, w, None)
            m_dense = dev.adjoint_batch_info(SLOT_BDF2)["run_ms"]
            t_sparse = forward("sparse")
            g_sparse = dev.run_adjoint_batch(SLOT_BDF2, n, w, None)
            m_sparse = dev.adjoint_batch_info(SLOT_BDF2)["run_ms"]
            replayed = dev.adjoint_tape_info_batch()["replayed"]
            assert all(np.array_equal(x, y) for x, y in zip(g_dense, g_sparse)), "the checkpointed batched march differs from the dense one"
            if p == 0:
                continue
            for q, v in (("forward_none_ms", t_none), ("forward_dense_ms", t_dense), ("forward_sparse_ms", t_sparse), ("march_dense_ms", m_dense),
                         ("march_sparse_ms", m_sparse)):
                fig[q].append(v)
        dev.adjoint_tape_reserve_sparse_batch(0, 0)
        dev.adjoint_tape_reserve_batch(n)  # (what the AdjointRun releases on the way out)
        dev.set_state_batch(*start)
    bfs.close()
    out = {q: stats(v) for q, v in fig.items()}
    expected = out["march_dense_ms"]["median"] + out["forward_none_ms"]["median"] * replayed / n
    return {"k": k, "replayed": replayed, **out, "expected_sparse_ms": expected, "sparse_over_expected": out["march_sparse_ms"]["median"] / expected,
            "bytes": held, "bytes_ratio": held["sparse"] / held["dense"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--every", default="auto")
    ap.add_argument("--widths", default="8,32")
    a = ap.parse_args()
    n = a.steps
    every = checkpoint_spacing(a.every if a.every == "auto" else int(a.every), n)
    fs = _cylinder()
    fig = {q: [] for q in ("forward_none_ms", "forward_dense_ms", "forward_sparse_ms", "march_dense_ms", "march_sparse_ms")}
    try:
        with AdjointRun(fs, tape=n) as run:
            dev = run.dev
            start = dev.get_state()
            rng = np.random.default_rng(0)
            u = 1e-3 * rng.standard_normal((n, max(dev.n_act, 1)))
            w = rng.standard_normal((n, dev.n_sens))
            held, replayed = {}, 0

            def forward(mode):
                if mode == "none":
                    dev.adjoint_tape_reserve(0)
                elif mode == "dense":
                    dev.adjoint_tape_reserve(n)
                else:
                    dev.adjoint_tape_reserve_sparse(n, every)
                dev.set_state(*start)
                if mode != "none":
                    dev.adjoint_tape_begin()
                    held[mode] = dev.adjoint_tape_info()["bytes"]
                return wall_ms(lambda: dev.run(SLOT_BDF2, n, u, compute_energy=False))[0]

            for p in range(a.passes + 1):  # (pass 0 warms every route up and is dropped)
                t_none = forward("none")
                t_dense = forward("dense")
                g_dense = dev.run_adjoint(SLOT_BDF2, n, w, None)
                m_dense = dev.adjoint_info(SLOT_BDF2)["run_ms"]
                t_sparse = forward("sparse")
                g_sparse = dev.run_adjoint(SLOT_BDF2, n, w, None)
                m_sparse = dev.adjoint_info(SLOT_BDF2)["run_ms"]
                replayed = dev.adjoint_tape_info()["replayed"]
                assert all(np.array_equal(x, y) for x, y in zip(g_dense, g_sparse)), "the checkpointed march differs from the dense one"
                if p == 0:
                    continue
                for q, v in (("forward_none_ms", t_none), ("forward_dense_ms", t_dense), ("forward_sparse_ms", t_sparse), ("march_dense_ms", m_dense),
                             ("march_sparse_ms", m_sparse)):
                    fig[q].append(v)
            dev.set_state(*start)
            N = int(dev.N)
        out = {q: stats(v) for q, v in fig.items()}
        expected = out["march_dense_ms"]["median"] + out["forward_none_ms"]["median"] * replayed / n
        res = {"mesh": "cylinder O1", "nonlinear": True, "N": N, "n_steps": n, "every": every, "passes": a.passes, "replayed": replayed, **out,
               "expected_sparse_ms": expected, "sparse_over_expected": out["march_sparse_ms"]["median"] / expected, "bytes": held,
               "bytes_ratio": held["sparse"] / held["dense"]}
        res["widths"] = [probe_width(fs, int(k), n, a.passes, every) for k in a.widths.split(",") if k]
    finally:
        fs.th.release_device()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
