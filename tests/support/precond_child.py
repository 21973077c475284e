"""Child process of tests/test_precond_apply_gpu.py: every case of precond_model.CASES (and the enclosed one) under ONE setting of
FC_PC_AMG_SWEEPS (the library reads it once per process), every sweep count of precond_model.SWEEPS, against the np.longdouble host
model built from the handle's own matrix and permutation.

    python precond_child.py <AMG sweeps> <tree | identity>

``tree``: the permutation fc_setup_krylov lays out itself (its nested-dissection tree); ``identity``: the W numbering, handed in through
fc_set_permutation -- the permutation of tests/test_precond_model_host.py, whose reach table then holds on the device as it stands
(the greedy aggregation follows the row order: another permutation, other level sizes and other row lengths).

Per setup: omega and the sizes of fc_get_krylov_info equal the model's, fc_get_pc_route reports the launch list the model predicts,
fc_debug_apply_pc of the three inputs is within the tolerances of the model (velocity and pressure parts, 2-norm and max-norm), leaves
its input alone, returns the same bits for a after b as for a, and on a second handle.  Prints one line per setup with the worst
ratio to the tolerances, the reach of the launch lists as ``REACH <json>``, and exits non-zero with the failed assertion."""
import json
import os
import sys
import time

import numpy as np


def main(amg: int, perm_kind: str) -> None:
    from flowcontrol_amd import _lib
    from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from tests.support import krylov_model as km
    from tests.support import precond_model as pm

    assert os.environ.get("FC_PC_AMG_SWEEPS") == str(amg), "FC_PC_AMG_SWEEPS in the environment is not the child's setting"
    tol = pm.tolerances()
    reached, worst_all = set(), {}

    def handle(th, dofs, enclosed):
        dev = DeviceSolver(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        if enclosed:
            dev.set_pressure_pin(pm.pin_dof(th), pm.PIN_SHIFT)
        dev.assemble_matrix(SLOT_BDF2, **pm.operator_args(th.node_coords))
        dev.apply_bc(SLOT_BDF2)
        if perm_kind == "identity":
            _lib.check(dev.lib.fc_set_permutation(dev._h, np.arange(th.N, dtype=np.int32)))
        return dev

    for n, enclosed in [(n, False) for n in pm.CASES] + [(pm.ENCLOSED, True)]:
        tag = f"unit_square({n}){' enclosed' if enclosed else ''}"
        th = TaylorHood(Mesh.unit_square(n, n))
        dofs = pm.all_wall_dofs(th) if enclosed else km.wall_dofs(th)
        n_vel = 2 * th.nn
        dev, twin = handle(th, dofs, enclosed), handle(th, dofs, enclosed)
        try:
            spec = None
            for sweeps in pm.SWEEPS:
                t0 = time.time()
                what = f"[V({amg},{amg}) {perm_kind}] {tag} sweeps {sweeps}"
                info = dev.setup_krylov(SLOT_BDF2, sweeps=sweeps, method="gmres", max_iter=60, rtol=1e-10)
                twin.setup_krylov(SLOT_BDF2, sweeps=sweeps, method="gmres", max_iter=60, rtol=1e-10)
                A, perm = dev.matrix(SLOT_BDF2), dev.perm.copy()
                assert np.array_equal(perm, twin.perm) and np.array_equal(A.data, twin.matrix(SLOT_BDF2).data)
                if spec is None:
                    spec = pm.Spec(A, perm, n_vel, pin=(pm.pin_dof(th), pm.PIN_SHIFT) if enclosed else None)
                    A0, perm0 = A, perm
                    assert perm_kind == "tree" or np.array_equal(perm, np.arange(th.N))
                    # the gap condition of the host test, on the device's own matrix: no strength ratio near 1, the aggregates are the model's
                    gaps = [float(np.abs(pm.strength_ratios(V["A"]) - 1.0).min()) for V in spec.levels]
                    assert all(g >= 1e-6 for g in gaps), f"{tag}: a strength ratio within {min(gaps):.1e} of 1"
                    if not enclosed:
                        assert (th.N, spec.np) == pm.CASES[n][:2]
                        assert perm_kind == "tree" or (len(spec.levels), spec.Ac.shape[0]) == pm.CASES[n][2:]
                assert np.array_equal(A.data, A0.data) and np.array_equal(perm, perm0), f"{what}: the setup moved the matrix or the permutation"
                # sizes and damping
                om = spec.omega(sweeps)
                assert abs(info["jacobi_omega"] - om) <= 1e-14 * om, f"{what}: omega {info['jacobi_omega']!r}, the model's {om!r}"
                got = (info["velocity_dofs"], info["pressure_dofs"], info["amg_levels"], info["coarsest_rows"], info["launches_per_apply"], info["jacobi_sweeps"])
                want = (spec.nu, spec.np, len(spec.levels) + 1, spec.Ac.shape[0], spec.launches(sweeps), sweeps)
                assert got == want, f"{what}: fc_get_krylov_info {got}, the model {want}"
                route, rows = spec.route(sweeps, amg)
                xs = pm.inputs(th.N, n_vel, perm)
                outs, ratio = {}, 0.0
                for name, x in xs.items():
                    keep = x.copy()
                    y = dev.debug_apply_pc(SLOT_BDF2, x)
                    assert np.array_equal(x, keep), f"{what} {name}: the input was written"
                    r = dev.pc_route(SLOT_BDF2)
                    assert np.array_equal(r, route), f"route not taken: {what} {name}: predicted {route.tolist()}, reported {r.tolist()}"
                    errs = pm.part_errors(y, spec.apply(x, sweeps, amg), n_vel)
                    for part, e, t in zip(("velocity", "pressure"), errs, tol):
                        for norm, ev, tv in zip(("2-norm", "max-norm"), e, t):
                            ratio = max(ratio, ev / tv)
                            key = f"{part} {norm}"
                            worst_all[key] = max(worst_all.get(key, 0.0), ev)
                            assert ev <= tv, f"{what} {name}: {part} part misses the longdouble model by {ev:.3e} ({norm}), allowed {tv:.3e}"
                    outs[name] = y
                    assert np.array_equal(twin.debug_apply_pc(SLOT_BDF2, x), y), f"{what} {name}: a second handle returns other bits"
                # a, then b, then a again: stale cat / u buffers would show
                again = dev.debug_apply_pc(SLOT_BDF2, xs["random"])
                assert np.array_equal(again, outs["random"]), f"{what}: a after b differs from a"
                reached |= pm.reach(route, rows, sweeps, amg, len(spec.levels), enclosed)
                print(f"{what}: levels {spec.level_rows}, route (kernel, rows, lanes, level, longest row) {[(pm.KERNELS[k], nr, ln, lv, row) for (k, nr, ln, lv), row in zip(route.tolist(), rows)]}, "
                      f"worst {ratio:.3f} x tolerance ({time.time() - t0:.1f} s)", flush=True)
        finally:
            dev.close()
            twin.close()
    for key, v in sorted(worst_all.items()):
        print(f"WORST V({amg},{amg}) {perm_kind} {key}: {v:.3e}", flush=True)
    print("REACH " + json.dumps(sorted(reached)), flush=True)
    print("CHILD OK", amg, flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
