"""Cost of the device linear analysis (flowcontrol_amd.linalg) on the cylinder (O1, golden base flow) and on
cavity_fine (a few Picard sweeps from rest: a throughput run, as bench.py's other_configs), printed as ONE JSON line:

  per case: order of the real-equivalent system, factor bytes, first setup (symbolic + first numeric phase) seconds, per frequency
  (median of 5): wall ms, device ms of the numeric factorisation, ms of the nu solves + C X, refactor GFLOP/s (trailing-update flops
  of the fp64 MFMA elimination / device time), us per Arnoldi step (operator apply + 2 Gram-Schmidt passes); O1: wall seconds of the
  cylinder eigen solve of compute_eigenvalues.py (n = 2, target 0.1 + 0.8j, tol 1e-10) and its leading eigenvalue.

  --lagged adds, per case, the frequency sweep on lagged factors (64-point log grid over [1e-1, 1e1], refactor_every = 1, 4, 16, GMRES
  rtol 1e-10): ms per frequency, GMRES iterations per solve (median / max over the lagged frequencies), numeric factorisations
  (above the planned ones: a GMRES that missed its tolerance fell back to refactorising), max |dH| / max |H| against
  refactor_every = 1.  The case "lidcavity" is the stability study of examples/lidcavity/eig_compute_lidcavity.py at Re = 8000
  (continuation in Re first): wall seconds of each of the four targets and whether a solve needed the GMRES rescue.

  --block runs the same grid with the frequencies of a group solved side by side (frequency_response(block=True)) at
  (refactor_every, block) = (1, off), (8, on), (16, on), (32, on): ms per frequency, numeric factorisations, GMRES iterations per
  column (min / median / max over the groups' columns), lock-step iterations and cycles, the wall time of solve_block per factor
  apply (host side included: upload, the whole iteration's kernels, record reads), and HIP-event times with algorithmic bytes and
  TB/s of one batched factor apply and one fc_shifted_spmv_b at the block's width next to their single-column counterparts
  (fc_bench_shifted_block), max |dH| / max |H| against (1, off).  --block-settings 8:on picks a subset.

  --adjoint: the adjoint side on the held factors (fc_shifted_set_adjoint): device ms of the numeric factorisation next to device ms,
  algorithmic bytes and TB/s of the transposed export that stands in for a second one (medians over 5 shifts), device bytes with
  and without the adjoint side, ms per frequency of resolvent_gains (ncv = 20; n = 1 at tol 1e-10, n = 3 at tol 1e-8) on the 64-point
  grid, and the wall time of get_mat_vp(left=True) next to two right eigen solves.

  --rom: balanced reduced models from frequency snapshots (flowcontrol_amd.rom): 64 Gauss-Legendre nodes in log w on [0.05, 20]; ms per
  frequency of the sweep (factorisation, direct solves, C X, adjoint solves, two pushes), device ms of the numeric factorisation
  (median), HIP-event ms with algorithmic MB, TB/s and TFLOP/s of the three Gram calls, their sum against one factorisation, bytes
  held by the sets; O1: the Hankel singular values, r for tol = 1e-3, the distance of the reduced model's leading eigenvalue from the
  full operator's and the error of the reduced response at the nodes (examples/cylinder/compute_reduced_model.py's figures).

    python scripts/linalg_probe.py [--cases O1,cavity_fine,lidcavity] [--lagged | --block | --adjoint | --rom]
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

from flowcontrol_amd import linalg  # noqa: E402
from flowcontrol_amd.examples.data import mesh_file  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402
from flowcontrol_amd.operatorgetter import OperatorGetter  # noqa: E402


def _cylinder():
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(prefix="fc_linalg_"))
    U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


def _cavity_fine():
    from flowcontrol_amd.examples.cavity.cavityflowsolver import CavityFlowSolver

    fs = CavityFlowSolver.make_default(Re=7500, path_out=tempfile.mkdtemp(prefix="fc_linalg_"), meshpath=mesh_file("cavity_fine"))
    fs.compute_steady_state(method="picard", max_iter=4, tol=1e-7, u_ctrl=[0.0])
    return fs


def probe(fs, eig: bool) -> dict:
    A, E, B, Cm = OperatorGetter(fs).get_all()
    B, Cm = np.asarray(B, dtype=float), np.asarray(Cm, dtype=float)
    op = linalg.ShiftedOperator(fs, A, E)
    out = {"N": int(A.shape[0]), "nu": int(B.shape[1]), "ny": int(Cm.shape[0])}
    t0 = time.perf_counter()
    op.factor(0.77j)
    out["first_setup_s"] = round(time.perf_counter() - t0, 3)
    info = op.info()
    out.update(order=info["order"], factor_bytes=info["factor_bytes"], device_bytes=info["device_bytes"])
    wall, dev, solve, gfs = [], [], [], []
    for w in (0.05, 0.3, 0.77, 2.0, 10.0):
        t0 = time.perf_counter()
        op.factor(1j * w)
        t1 = time.perf_counter()
        op.transfer(B, Cm)
        t2 = time.perf_counter()
        i = op.info()
        wall.append(1e3 * (t2 - t0))
        dev.append(i["refactor_ms"])
        solve.append(1e3 * (t2 - t1))
        gfs.append(i["refactor_flops"] / (1e6 * i["refactor_ms"]))
    out.update(ms_per_frequency=round(float(np.median(wall)), 2), refactor_ms=round(float(np.median(dev)), 2),
               solves_ms=round(float(np.median(solve)), 2), refactor_gflops=round(float(np.median(gfs)), 1),
               refactor_gflop=round(op.info()["refactor_flops"] / 1e9, 1))
    op.factor(0.1 + 0.8j)
    kry = linalg.DeviceKrylov(op)
    m = 20
    rng = np.random.default_rng(0)
    kry.start(m, rng.standard_normal(op.n) + 1j * rng.standard_normal(op.n))
    t0 = time.perf_counter()
    for j in range(m):
        kry.step(j)
    out["arnoldi_step_us"] = round(1e6 * (time.perf_counter() - t0) / m, 1)
    op.release()
    if eig:
        t0 = time.perf_counter()
        valp, _ = linalg.get_mat_vp(A, E, n=2, target=0.1 + 0.8j, tol=1e-10, flowsolver=fs)
        out["eig_solve_s"] = round(time.perf_counter() - t0, 3)
        out["eig_leading"] = [float(valp[0].real), float(valp[0].imag)]
    return out


def probe_lagged(fs) -> dict:
    A, E, B, Cm = OperatorGetter(fs).get_all()
    B, Cm = np.asarray(B, dtype=float), np.asarray(Cm, dtype=float)
    ww = np.logspace(-1, 1, 64)
    out, Href = {}, None
    for every in (1, 4, 16):
        op = linalg.ShiftedOperator(fs, A, E, krylov={"max_iter": 300, "restart": 60, "rtol": 1e-10} if every > 1 else None)
        iters = []
        transfer = op.transfer

        def counted(Bm, Cmat, transfer=transfer, op=op, iters=iters):
            H = transfer(Bm, Cmat)
            if op.sigma != op.factored_sigma:
                iters.extend(int(i) for i in op.last_iterations)
            return H

        op.transfer = counted
        try:
            op.factor(1j * ww[0])  # (the symbolic phase is not part of the sweep's time)
            t0 = time.perf_counter()
            H, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=every)
            ms = 1e3 * (time.perf_counter() - t0) / ww.size
            nfac = op.krylov_info()["refactorisations"] - 1
        finally:
            op.release()
        if Href is None:
            Href = H
        out[f"every_{every}"] = {"ms_per_frequency": round(ms, 2), "refactorisations": nfac, "planned": int(np.ceil(ww.size / every)),
                                 "gmres_iterations_median": float(np.median(iters)) if iters else 0.0,
                                 "gmres_iterations_max": int(max(iters)) if iters else 0,
                                 "max_dH_rel": float(np.max(np.abs(H - Href)) / np.max(np.abs(Href)))}
    return out


def probe_block(fs, settings) -> dict:
    A, E, B, Cm = OperatorGetter(fs).get_all()
    B, Cm = np.asarray(B, dtype=float), np.asarray(Cm, dtype=float)
    ww = np.logspace(-1, 1, 64)
    out, Href = {"nu": int(B.shape[1])}, None
    for every, block in settings:
        op = linalg.ShiftedOperator(fs, A, E, krylov={"max_iter": 300, "restart": 60, "rtol": 1e-10} if block else None)
        iters, apply_ms, lock = [], [], [0, 0]
        if block:
            solve_block = op.solve_block

            def counted(b, sigmas, download=True, solve_block=solve_block, op=op, iters=iters, apply_ms=apply_ms, lock=lock):
                a0 = op.krylov_info()["applies"]
                t0 = time.perf_counter()
                try:
                    return solve_block(b, sigmas, download)
                except Exception:
                    lock.append(1)  # (a block that missed its tolerance: the sweep falls back for its group)
                    raise
                finally:
                    dt = 1e3 * (time.perf_counter() - t0)
                    iters.extend(int(i) for i in op.last_iterations)
                    apply_ms.append(dt / max(1, op.krylov_info()["applies"] - a0))  # (wall time of the call, host work included)
                    bi = op.block_info()
                    lock[0] += bi["lockstep_iterations"]
                    lock[1] += bi["cycles"]

            op.solve_block = counted
        try:
            op.factor(1j * ww[0])  # (the symbolic phase is not part of the sweep's time)
            if block:
                op.set_block(min(linalg.MAX_BLOCK, every * B.shape[1]))  # (nor are the block's tables)
            t0 = time.perf_counter()
            H, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=every, block=block or None)
            ms = 1e3 * (time.perf_counter() - t0) / ww.size
            info = op.krylov_info()
            dev_bytes = op.info()["device_bytes"]
            bench = None
            if block:
                op.set_block(min(linalg.MAX_BLOCK, every * B.shape[1]))
                bench = {k: {"ms": round(v["ms"], 4), "MB": round(v["bytes"] / 1e6, 1), "TBps": round(v["TBps"], 3)}
                         for k, v in op.bench_block(20).items()}
        finally:
            op.release()
        if Href is None:
            Href = H
        out[f"every_{every}_{'block' if block else 'off'}"] = {
            "ms_per_frequency": round(ms, 2), "refactorisations": info["refactorisations"] - 1, "planned": int(np.ceil(ww.size / every)),
            "applies": info["applies"], "matvecs": info["matvecs"],
            "iterations_min_median_max": [int(min(iters)), float(np.median(iters)), int(max(iters))] if iters else [0, 0.0, 0],
            "lockstep_iterations": lock[0], "cycles": lock[1], "block_solves": len(apply_ms), "failed_block_solves": len(lock) - 2,
            "solve_block_wall_ms_per_apply": round(float(np.median(apply_ms)), 3) if apply_ms else 0.0, "bench": bench,
            "device_bytes": dev_bytes, "max_dH_rel": float(np.max(np.abs(H - Href)) / np.max(np.abs(Href)))}
    return out


def probe_adjoint(fs, gains: bool = True) -> dict:
    A, E, _, _ = OperatorGetter(fs).get_all()
    op = linalg.ShiftedOperator(fs, A, E)
    out = {"N": int(A.shape[0])}
    try:
        op.factor(0.77j)
        out["device_bytes_direct"] = op.info()["device_bytes"]
        op.set_adjoint(True)
        op.set_adjoint(False)
        out.update(device_bytes=op.info()["device_bytes"], adjoint_bytes=op.adjoint_info()["bytes"], factor_bytes=op.info()["factor_bytes"])
        fac, exp, tbps = [], [], []
        for w in (0.05, 0.3, 0.77, 2.0, 10.0):
            op.factor(1j * w)
            a = op.adjoint_info()
            fac.append(op.info()["refactor_ms"])
            exp.append(a["export_ms"])
            tbps.append(a["export_TBps"])
        out.update(refactor_ms=round(float(np.median(fac)), 3), export_ms=round(float(np.median(exp)), 4),
                   export_MB=round(op.adjoint_info()["export_bytes"] / 1e6, 1), export_TBps=round(float(np.median(tbps)), 3),
                   exports=op.adjoint_info()["exports"])
        b = np.random.default_rng(0).standard_normal(op.n)
        t0 = time.perf_counter()
        op.solve(b)
        t1 = time.perf_counter()
        op.solve(b, adjoint=True)
        out.update(solve_ms=round(1e3 * (t1 - t0), 2), adjoint_solve_ms=round(1e3 * (time.perf_counter() - t1), 2))
    finally:
        op.release()
    if gains:
        ww = np.logspace(-1, 1, 64)
        linalg.resolvent_gains(A, E, ww[:1], n=1, flowsolver=fs)  # (the symbolic phase is not part of the sweep's time)
        for name, kw in (("gains_n1", {"n": 1, "tol": 1e-10}), ("gains_n3", {"n": 3, "tol": 1e-8})):
            try:  # (a sweep that misses its tolerance is reported in the line, the rest still runs)
                t0 = time.perf_counter()
                g = linalg.resolvent_gains(A, E, ww, flowsolver=fs, **kw)
                wall = time.perf_counter() - t0
                i = int(np.argmax(g[0]))
                out[name] = {"tol": kw["tol"], "ms_per_frequency": round(1e3 * wall / ww.size, 2), "gain_max": float(g[0, i]),
                             "gain_max_w": round(float(ww[i]), 4)}
            except RuntimeError as e:
                out[name] = {"tol": kw["tol"], "error": str(e)[:200]}
        kw = dict(n=2, target=0.1 + 0.8j, tol=1e-10, flowsolver=fs)
        t0 = time.perf_counter()
        linalg.get_mat_vp(A, E, **kw)
        t1 = time.perf_counter()
        linalg.get_mat_vp(A, E, left=True, **kw)
        t2 = time.perf_counter()
        out.update(eig_right_s=round(t1 - t0, 3), eig_left_right_s=round(t2 - t1, 3), two_right_solves_s=round(2 * (t1 - t0), 3))
    return out


def probe_rom(fs, quality: bool) -> dict:
    from flowcontrol_amd import rom

    A, E, B, Cm = OperatorGetter(fs).get_all()
    B, Cm = np.asarray(B, dtype=float).reshape(A.shape[0], -1), np.asarray(Cm, dtype=float)
    ww, weights = rom.log_quadrature(0.05, 20.0, 64)
    nu, ny = B.shape[1], Cm.shape[0]
    out = {"N": int(A.shape[0]), "nu": nu, "ny": ny, "nq": int(ww.size)}
    op = linalg.ShiftedOperator(fs, A, E)
    try:
        op.factor(1j * ww[0])  # (the symbolic phase and the adjoint side's set-up are not part of the sweep's time)
        op.set_adjoint(True)
        op.set_adjoint(False)
        fac = []
        t0 = time.perf_counter()
        H, CXs = rom.snapshot_sweep(op, B, Cm, ww, weights, verbose=False, on_factor=lambda j, o: fac.append(o.info()["refactor_ms"]))
        out["sweep_ms_per_frequency"] = round(1e3 * (time.perf_counter() - t0) / ww.size, 2)
        out["refactor_ms"] = round(float(np.median(fac)), 3)
        op.snap_reserve(2, nu)
        op.snap_load(2, B)
        grams, total = {}, 0.0
        mats = {}
        for name, (left, right, kind) in (("ZtEX", (1, 0, 1)), ("ZtAX", (1, 0, 2)), ("ZtB", (1, 2, 0))):
            op.snap_gram(left, right, kind)  # (warm-up: the work buffers are sized by the first call)
            mats[name] = op.snap_gram(left, right, kind)
            t = op.snap_gram_timing()
            total += t["ms"]
            grams[name] = {"shape": list(mats[name].shape), "ms": round(t["ms"], 4), "MB": round(t["bytes"] / 1e6, 1), "TBps": round(t["TBps"], 3),
                           "TFLOPs": round(t["TFLOPs"], 3)}
        info = op.snap_info()
        out.update(grams=grams, grams_ms=round(total, 4), grams_below_one_factorisation=bool(total < float(np.median(fac))),
                   set_bytes=info["bytes"], columns=info["columns"], device_bytes=op.info()["device_bytes"])
    finally:
        op.release()
    if quality:
        from flowcontrol_amd.examples.cylinder import compute_reduced_model

        red = rom.reduced_from_grams(mats["ZtEX"], mats["ZtAX"], mats["ZtB"][:, 0::2], CXs, ww, weights, H=H, tol=1e-3)
        q = compute_reduced_model.summary(red)
        out.update(hsv=[float(f"{v:.4e}") for v in red.hsv[:24]], r=q["r"], error_bound=q["error_bound"],
                   leading=[q["leading"].real, q["leading"].imag], leading_distance=q["leading_distance"], node_error_rel=q["node_error_rel"])
    return out


def probe_lidcavity() -> dict:
    from flowcontrol_amd.examples.lidcavity import eig_compute_lidcavity, eig_compute_operators_lidcavity
    from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver

    out_dir = Path(tempfile.mkdtemp(prefix="fc_linalg_lid_"))
    t0 = time.perf_counter()
    A, E = eig_compute_operators_lidcavity.main(out_dir)
    res = {"N": int(A.shape[0]), "operators_s": round(time.perf_counter() - t0, 1)}
    fs = LidCavityFlowSolver.make_default(Re=8000, path_out=out_dir)
    try:
        lam, _, stats = eig_compute_lidcavity.compute(fs, A, E)
    finally:
        fs.th.release_device()
    res["targets"] = [{"target": [s["target"].real, s["target"].imag], "seconds": round(s["seconds"], 3), "rescued": bool(s["rescued"])}
                      for s in stats]
    res["eigenvalues"] = [[float(v.real), float(v.imag)] for v in lam]
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", default="O1,cavity_fine")
    ap.add_argument("--lagged", action="store_true", help="the sweep on lagged factors instead of the per-frequency costs")
    ap.add_argument("--block", action="store_true", help="the sweep with the frequencies of a group solved as blocks")
    ap.add_argument("--adjoint", action="store_true", help="the transposed export, resolvent gains and left modes on the held factors")
    ap.add_argument("--rom", action="store_true", help="balanced reduced models: the snapshot sweep and the Gram calls")
    ap.add_argument("--block-settings", default="1:off,8:on,16:on,32:on", help="refactor_every:on|off pairs of --block")
    args = ap.parse_args()
    settings = [(int(a), b == "on") for a, b in (item.split(":") for item in args.block_settings.split(","))]
    res = {"probe": "linalg_rom" if args.rom else "linalg_adjoint" if args.adjoint else "linalg_block" if args.block else ("linalg_lagged" if args.lagged else "linalg")}
    for case in args.cases.split(","):
        if case == "lidcavity":
            try:
                res[case] = probe_lidcavity()
            except Exception as e:  # noqa: BLE001
                res[case] = {"error": f"{type(e).__name__}: {e}"}
            continue
        fs = _cylinder() if case == "O1" else _cavity_fine()
        try:
            if args.rom:
                res[case] = probe_rom(fs, quality=case == "O1")
            elif args.adjoint:
                res[case] = probe_adjoint(fs, gains=case == "O1")
            else:
                res[case] = probe_block(fs, settings) if args.block else (probe_lagged(fs) if args.lagged else probe(fs, eig=case == "O1"))
        except Exception as e:  # noqa: BLE001  (one case's failure is reported in the line, the other case still runs)
            res[case] = {"error": f"{type(e).__name__}: {e}"}
        finally:
            fs.th.release_device()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
