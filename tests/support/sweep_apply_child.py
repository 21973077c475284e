"""Child process of tests/test_sweep_apply_gpu.py: the single-vector factor apply under ONE set of process-level knobs (the library
reads them once per process), every run of sweep_cases.RUNS for it -- a fresh handle per (handle-level knob set, storage width, case) --
both slots, against the reference file the parent wrote.

    python sweep_apply_child.py <reference.npz> <knob set> <tolerances as JSON>
    python sweep_apply_child.py refusal        a sweep geometry without a template instance must be refused (refusal())

Prints one line per (run, operator) and exits non-zero with the failed assertion."""
import json
import os
import sys
import time

import numpy as np


def main(ref_path: str, kn: str, tol: dict) -> None:
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, DeviceSolver
    from tests.support import batch_cases as bc
    from tests.support import front_cases as fcs
    from tests.support import ndsolver
    from tests.support import sweep_cases as sc

    knobs = sc.KNOB_SETS[kn]
    for name in sc.PROCESS_KNOBS:
        assert os.environ.get(name) == knobs.get(name), f"{name} in the environment is not the knob set's"
    ref = np.load(ref_path)
    slots = {"bdf1": SLOT_BDF1, "bdf2": SLOT_BDF2}
    cases = {c[0]: c for c in sc.cases()}
    host = {}
    worst = {}
    for hs, bits, case in sc.RUNS[kn]:
        t0 = time.time()
        _, nx, ny, tbits, depth, merge = cases[case]
        if case not in host:
            host[case] = fcs.host_case(nx, ny, tbits)
        th, dofs, tree = host[case]
        hk = sc.handle_knobs(hs, 2 * tree.depth + 1)
        for name in sc.HANDLE_KNOBS:  # read when the handle is created and when it lays out its tables
            os.environ.pop(name, None)
        os.environ.update(hk)
        m = sc.model(tree, {**knobs, **hk}, bits)
        want = sc.predicted_launches(m)
        dev = DeviceSolver(th)
        try:
            if bits != 64:
                dev.set_factor_precision(bits)
            U0 = bc.smooth_advection(th)
            dev.set_bc(dofs, np.zeros((dofs.size, 1)))
            dev.set_time_scheme(0.005, True)
            for op, slot in slots.items():
                dev.assemble_matrix(slot, mass=bc.OPERATORS[op], nu=bc.NU, adv=U0, lin=U0)
                dev.apply_bc(slot)
                dev.setup_solver(slot, depth=depth, merge=merge)
                assert not dev.factors_inexact[slot]
            assert tuple(dev.tree_info()["bits"]) == tuple(tbits)
            assert np.array_equal(ndsolver.tree_of(dev).perm, tree.perm)
            dev.set_solver_options(refine=0, method="refine")  # solve = the bare apply (+ the residual monitor), whatever the storage width
            for op, slot in slots.items():
                assert dev.factor_storage(slot)[0] == bits
                took = dev.sweep_launches(slot)
                assert took.shape == want.shape and np.array_equal(took, want), (
                    f"route not taken: {kn} / {hs} / {bits} bits / {case} expects launches {sc.LAUNCH_COLS}\n{want.tolist()}\nthe device reports\n{took.tolist()}")
                vals = dev.factor_values(slot)
                assert np.array_equal(vals, sc.round_values(ref[f"{case}/{op}/V"], bits)), "the factor values differ from the ones the reference was applied with"
                B, Xr = ref[f"{case}/{op}/B"], ref[f"{case}/{op}/X{bits}"]
                X = np.array([dev.solve(slot, b)[0] for b in B])
                e2 = max(np.linalg.norm(X[j] - Xr[j]) / np.linalg.norm(Xr[j]) for j in range(len(B)))
                ei = max(np.abs(X[j] - Xr[j]).max() / np.abs(Xr[j]).max() for j in range(len(B)))
                t2, ti = tol[str(bits)]
                w = worst.setdefault(bits, [0.0, 0.0])
                w[0], w[1] = max(w[0], e2 / t2 * 16), max(w[1], ei / ti * 16)
                line = f"[{kn}] {hs} {bits} {case} {op}: 2-norm {e2:.2e} ({e2 / t2 * 16:.1f} x host) max-norm {ei:.2e} ({ei / ti * 16:.1f} x host)"
                if kn == "default" and hs == "default" and bits == 64:  # end to end: the operator's own inverse
                    Xe = ref[f"{case}/{op}/E"]
                    ee = max(np.linalg.norm(X[j] - Xe[j]) / np.linalg.norm(Xe[j]) for j in range(len(B)))
                    line += f" end to end {ee:.2e}"
                    print(line, flush=True)
                    assert ee <= tol["end_to_end"], f"{case} {op}: error against the refined host solve {ee:.3e} > {tol['end_to_end']:.3e}"
                else:
                    print(line, flush=True)
                assert e2 <= t2, f"{hs} {bits} {case} {op}: 2-norm error {e2:.3e} > {t2:.3e}\n{took.tolist()}"
                assert ei <= ti, f"{hs} {bits} {case} {op}: max-norm error {ei:.3e} > {ti:.3e}\n{took.tolist()}"
                # bit-wise properties: a fixed summation order without atomics
                for _ in range(2):
                    assert np.array_equal(dev.solve(slot, B[0])[0], X[0]), "the apply is not reproducible from call to call"
                assert np.array_equal(dev.solve(slot, 2.0**40 * B[0])[0], 2.0**40 * X[0]), "the apply of 2^40 b is not 2^40 times the apply of b, bit for bit"
                assert not dev.solve(slot, np.zeros(dev.N))[0].any(), "a zero right-hand side did not come back exactly zero"
            print(f"LAUNCHES {kn} {hs} {bits} {case} {want.tolist()} ({time.time() - t0:.1f} s)", flush=True)
        finally:
            dev.close()
    for bits, (a, b) in sorted(worst.items()):
        print(f"WORST {kn} {bits} bits: {a:.2f} x host (2-norm) {b:.2f} x host (max-norm), 16 allowed", flush=True)
    print("CHILD OK", kn, flush=True)


def refusal() -> None:
    """A (lanes, sub) geometry without a template instance on the first stage of the smallest case: the solve is refused with
    FC_ERR_INVALID by the argument check in front of the launch, and the handle closes as usual."""
    from flowcontrol_amd._lib import FC_ERR_INVALID, FcError
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from tests.support import batch_cases as bc
    from tests.support import front_cases as fcs
    from tests.support import sweep_cases as sc

    geom = (8, 2)
    assert geom not in sc.SWEEP_KEYS
    _, nx, ny, tbits, depth, merge = min(sc.cases(), key=lambda c: c[1] * c[2])
    th, dofs, tree = fcs.host_case(nx, ny, tbits)
    for name in sc.HANDLE_KNOBS:
        os.environ.pop(name, None)
    os.environ.update({"FC_SWEEP_GEOM": sc.sweep_geom([geom]), "FC_BLOCK_KERNEL": "0", "FC_UP_FORM": "row"})
    dev = DeviceSolver(th)
    try:
        U0 = bc.smooth_advection(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        dev.set_time_scheme(0.005, True)
        dev.assemble_matrix(SLOT_BDF2, mass=bc.OPERATORS["bdf2"], nu=bc.NU, adv=U0, lin=U0)
        dev.apply_bc(SLOT_BDF2)

        def refused(what, call):
            try:
                call()
            except FcError as e:
                print(f"REFUSED {what}: {e}", flush=True)
                assert e.code == FC_ERR_INVALID and "unsupported (lanes, sub) combination" in str(e)
            else:
                raise AssertionError(f"{what}: a sweep geometry without an instance was not refused")

        # the factors are computed and held; the solve that accepts them at the end of the setup is the first to be refused ...
        refused("acceptance solve of the setup", lambda: dev.setup_solver(SLOT_BDF2, depth=depth, merge=merge))
        # ... and so is every solve of the caller's
        refused("solve", lambda: dev.solve(SLOT_BDF2, bc.rhs_pool(dev.N, 1000)[0]))
    finally:
        dev.close()
    print("CHILD OK refusal", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "refusal":
        refusal()
    else:
        main(sys.argv[1], sys.argv[2], json.loads(sys.argv[3]))
