"""Measurements of the snapshot bank on the cylinder's O1 mesh, printed as ONE JSON line:

  steps: steps/s of fc_run without a bank, with a bank at every = 1 (nontemporal and plain stores: FC_SSNAP_NT), and of the only way to
         get the same snapshots without one -- runs of one step, each followed by fc_get_solution -- in `--passes` alternating passes
         of `--steps` steps each; median and spread (min, max) per mode, and the ratios of the medians
  gram:  X^T M X and X^T X of 256 loaded columns: device ms between HIP events (operator pass, product, reduction), wall ms of the call,
         algorithmic bytes, TFLOP/s; the wall ms of downloading the columns and forming X^T M X with scipy / numpy
  complex_gram (--complex): fc_shifted_snap_gram at the sizes of the 64-frequency reduced model (384 x 256 real, kind E) in the same
         session, for the comparison of the two kernels

    python scripts/modal_probe.py [--steps 1000] [--passes 3] [--complex]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from flowcontrol_amd import linalg, modal  # noqa: E402
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.flowsolverparameters import ParamIC  # noqa: E402


def _cylinder():
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(prefix="fc_modal_"))
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


def probe_steps(dev, state0, n: int, passes: int) -> dict:
    u0 = np.zeros(dev.n_act)

    def timed(mode):
        dev.set_state(*state0)
        bank = None
        if mode in ("bank_nt", "bank_plain"):
            os.environ["FC_SSNAP_NT"] = "1" if mode == "bank_nt" else "0"
            bank = modal.SnapshotBank(dev, n)
        dev.run(SLOT_BDF1, 1, u0)  # (the first step is BDF1; not timed)
        if bank:
            bank.clear()
        t0 = time.perf_counter()
        if mode == "download":
            for _ in range(n):
                dev.run(SLOT_BDF2, 1, u0)
                dev.get_solution()
        else:
            dev.run(SLOT_BDF2, n, u0)
        dt = time.perf_counter() - t0
        if bank:
            assert bank.count == n
            bank.close()
        return n / dt

    modes = ("none", "bank_nt", "bank_plain", "download")
    for m in modes:
        timed(m)  # warm-up: buffers, first-touch of the bank's pages
    rates = {m: [] for m in modes}
    for _ in range(passes):
        for m in modes:
            rates[m].append(timed(m))
    os.environ.pop("FC_SSNAP_NT", None)
    out = {m: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for m, v in rates.items()}
    med = {m: float(np.median(v)) for m, v in rates.items()}
    best = "bank_nt" if med["bank_nt"] >= med["bank_plain"] else "bank_plain"
    out.update(steps=n, passes=passes, faster_store=best, capture_over_download=round(med[best] / med["download"], 2),
               capture_over_none={m: round(med[m] / med["none"], 4) for m in ("bank_nt", "bank_plain")})
    return out


def probe_gram(dev, m: int = 256) -> dict:
    bank = modal.SnapshotBank(dev, m)
    out = {"m": m, "N": dev.N}
    try:
        rng = np.random.default_rng(0)
        for _ in range(0, m, 64):
            bank.load(rng.standard_normal((64, dev.N)), set=0)
        for name, weight in (("XtMX", "energy"), ("XtX", None)):
            bank.gram(weight=weight)  # (the work buffers are sized by the first call)
            t0 = time.perf_counter()
            bank.gram(weight=weight)
            wall = time.perf_counter() - t0
            t = dev.snap_gram_last()
            out[name] = {"ms": round(t["ms"], 4), "wall_ms": round(1e3 * wall, 3), "MB": round(t["bytes"] / 1e6, 1),
                         "TBps": round(t["bytes"] / t["ms"] * 1e-9, 3), "TFLOPs": round(t["flops"] / t["ms"] * 1e-9, 3)}
        M = dev.matrix(SLOT_MASS)
        t0 = time.perf_counter()
        X = bank.get()
        t_get = time.perf_counter() - t0
        X @ (M @ X.T)
        out["host"] = {"download_ms": round(1e3 * t_get, 2), "total_ms": round(1e3 * (time.perf_counter() - t0), 2)}
        out["bank_bytes"] = bank.info()["bytes"]
    finally:
        bank.close()
    return out


def probe_complex_gram(fs) -> dict:
    from flowcontrol_amd.operatorgetter import OperatorGetter

    A, E, _, _ = OperatorGetter(fs).get_all()
    op = linalg.ShiftedOperator(fs, A.tocsr(), E.tocsr())
    try:
        op.factor(0.77j)
        rng = np.random.default_rng(0)
        for which, ncol in ((0, 128), (1, 192)):
            op.snap_reserve(which, ncol)
            op.snap_load(which, rng.standard_normal((op.n, ncol)) + 1j * rng.standard_normal((op.n, ncol)))
        op.snap_gram(1, 0, 1)
        op.snap_gram(1, 0, 1)
        t = op.snap_gram_timing()
        return {"shape": [384, 256], "kind": "E", "ms": round(t["ms"], 4), "TFLOPs": round(t["TFLOPs"], 3), "TBps": round(t["TBps"], 3)}
    finally:
        op.release()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--complex", action="store_true", help="also time the complex kernel (one shifted factorisation)")
    args = ap.parse_args()
    fs = _cylinder()
    res = {"probe": "modal", "case": "O1"}
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        state0 = [np.array(a, copy=True) for a in dev.get_state()]
        res["steps"] = probe_steps(dev, state0, args.steps, args.passes)
        res["gram"] = probe_gram(dev)
        if args.complex:
            res["complex_gram"] = probe_complex_gram(fs)
    finally:
        fs.th.release_device()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
