"""Child process of tests/test_batch_apply_gpu.py: the batched factor apply under ONE knob set (the library reads the knobs once per
process), every case of batch_cases.cases(), both slots, k = 1 ... 32, against the reference file the parent wrote.

    python batch_apply_child.py <reference.npz> <knob set> <tolerance>

Prints one line per (case, batch width) and exits non-zero with the failed assertion."""
import os
import sys

import numpy as np
import scipy.sparse as sp


def main(ref_path: str, kn: str, tol: float) -> None:
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, DeviceSolver
    from tests.support import batch_cases as bc
    from tests.support import front_cases as fcs
    from tests.support import ndsolver

    knobs = bc.KNOB_SETS[kn]
    for name in ("FC_BATCH_CG", "FC_BATCH_CPW", "FC_BATCH_SPLIT", "FC_BATCH_XCD", "FC_NT_BYTES", "FC_BATCH_SPLIT_CPW"):
        assert os.environ.get(name) == knobs.get(name), f"{name} in the environment is not the knob set's"
    ref = np.load(ref_path)
    slots = {"bdf1": SLOT_BDF1, "bdf2": SLOT_BDF2}
    for ci, (case, nx, ny, bits, depth, merge) in enumerate(bc.cases()):
        th, dofs, tree = fcs.host_case(nx, ny, bits)
        dev = DeviceSolver(th)
        try:
            U0 = bc.smooth_advection(th)
            dev.set_bc(dofs, np.zeros((dofs.size, 1)))
            dev.set_time_scheme(0.005, True)
            A = {}
            for op, slot in slots.items():
                dev.assemble_matrix(slot, mass=bc.OPERATORS[op], nu=bc.NU, adv=U0, lin=U0)
                dev.apply_bc(slot)
                dev.setup_solver(slot, depth=depth, merge=merge)
                assert not dev.factors_inexact[slot]
                vals = dev.matrix(slot).data
                want = ref[f"{case}/{op}/A"]
                assert np.abs(vals - want).max() <= 1e-13 * np.abs(want).max(), "the operator differs from the one the reference was solved for"
                A[op] = sp.csr_matrix((want, dev.colidx.copy(), dev.rowptr.copy()), shape=(dev.N, dev.N))
            assert tuple(dev.tree_info()["bits"]) == tuple(bits)
            assert np.array_equal(ndsolver.tree_of(dev).perm, tree.perm)
            m = bc.model(tree, knobs)
            worst = {}
            col0 = {}
            for k in bc.KS:
                dev.set_batch(k)
                KB = dev.batch_info()["KB"]
                want = bc.predicted_launches(m, KB, knobs)
                for op, slot in slots.items():
                    took = dev.batch_launches(slot)
                    assert took.shape == want.shape and np.array_equal(took, want), (
                        f"route not taken: {case} / {kn} / KB {KB} expects launches {bc.LAUNCH_COLS}\n{want.tolist()}\nthe device reports\n{took.tolist()}")
                    pool, xref = ref[f"{case}/{op}/B"], ref[f"{case}/{op}/X"]
                    B, Xr, zero, twin = bc.batch_rhs(pool, xref, k)
                    X = dev.solve_batch(slot, B)
                    live = [s for s in range(k) if s != zero]
                    err = max(np.linalg.norm(X[s] - Xr[s]) / np.linalg.norm(Xr[s]) for s in live)
                    res = max(np.linalg.norm(A[op] @ X[s] - B[s]) / np.linalg.norm(B[s]) for s in live)
                    w = worst.setdefault(KB, [0.0, 0.0])
                    w[0], w[1] = max(w[0], err), max(w[1], res)
                    print(f"[{kn}] {case} {op} k {k:2d} KB {KB:2d} error {err:.2e} residual {res:.2e}", flush=True)
                    assert err <= tol, f"{case} {op} k {k}: solution error {err:.3e} > {tol:.3e}"
                    assert res < 1e-11, f"{case} {op} k {k}: residual {res:.3e}"
                    if zero is not None:
                        assert not X[zero].any(), "the zero column did not come back exactly zero"
                        s, t = twin
                        assert np.array_equal(X[s], 2.0**40 * X[t]), "the column scaled by 2^40 is not 2^40 times its twin, bit for bit"
                    for _ in range(2):  # three calls in all
                        assert np.array_equal(dev.solve_batch(slot, B), X), "the batched apply is not reproducible from call to call"
                    same = dev.solve_batch(slot, np.tile(pool[0], (k, 1)))
                    assert all(np.array_equal(same[s], same[0]) for s in range(1, k)), "the same right-hand side gives different columns"
                    assert np.array_equal(same[0], X[0])  # ... and what it gave beside other columns
                    if (op, KB) in col0:
                        assert np.array_equal(col0[op, KB][1], same[0]), f"column 0 at k = {col0[op, KB][0]} and at k = {k} (KB {KB}) differ"
                    col0[op, KB] = (k, same[0])
            dev.set_batch(4)
            rows = dev.batch_launches(SLOT_BDF2)
            for KB, (err, res) in sorted(worst.items()):
                print(f"WORST {kn} {case} KB {KB} error {err:.3e} residual {res:.3e}", flush=True)
            print(f"LAUNCHES {kn} {case} KB 4 {rows.tolist()}", flush=True)
            dev.set_batch(0)
        finally:
            dev.close()
    print("CHILD OK", kn, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], float(sys.argv[3]))
