"""Child process of tests/test_step_routes_gpu.py: the runs of step_cases.RUNS for ONE set of process-level knobs (the library reads them
once per process) -- a fresh handle per run, created under the run's handle-level knobs -- against the np.longdouble host model and the
operators in the reference file the parent wrote.

    python step_child.py <reference.npz> <knob set> <tolerances as JSON> <records.npz to write>

After every step fc_get_step_route must report the route the host model predicts.  Prints one line per step, the worst ratio to every
tolerance at the end, and exits non-zero with the failed assertion.  The records (y, dE, residual norms and the solution of every step)
go to the file named last: the parent compares them between children bit for bit."""
import json
import os
import sys
import time

import numpy as np


class Worst:
    def __init__(self):
        self.w = {}

    def see(self, what, value, tol):
        r = float(value) / float(tol) if tol > 0 else (0.0 if value == 0 else np.inf)
        if r > self.w.get(what, (-1.0,))[0]:
            self.w[what] = (r, float(value), float(tol))
        return r


def main(ref_path: str, kn: str, tol: dict, rec_path: str) -> None:
    from flowcontrol_amd._lib import FC_ERR_DIVERGED, FcError
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, SLOT_SCRATCH, DeviceSolver
    from tests.support import step_cases as sc

    knobs = sc.KNOB_SETS[kn]
    for name in sc.PROCESS_KNOBS:
        assert os.environ.get(name) == knobs.get(name), f"{name} in the environment is not the knob set's"
    ref = np.load(ref_path)
    worst, records, models = Worst(), {}, {}
    slot_of = {1: SLOT_BDF1, 2: SLOT_BDF2}

    for run in sc.RUNS[kn]:
        t0 = time.time()
        name, case, hs, sens = run
        tag = sc.run_name(run)
        for k in sc.HANDLE_KNOBS:  # read when the handle is created
            os.environ.pop(k, None)
        os.environ.update(sc.HANDLE_SETS[hs])
        kk = {**knobs, **sc.HANDLE_SETS[hs]}
        m = models.setdefault(case, sc.HostModel(case))
        th, dofs, prof = m.th, m.dofs, m.prof
        nn2 = 2 * th.nn
        rows = sc.sensor_rows(th, sens)
        can_assemble = name != "speculate" or knobs.get("FC_SPECULATE") == "0"  # fc_assemble_rhs resets the speculation, by design
        dev = DeviceSolver(th)
        try:
            st = dict(dt=sc.DT, nl=True, fprof=None, C={1: None, 2: None}, A_full={}, A_fac={}, A_mon={}, solve={}, lagged=False)

            def operators(dt, check_ref):
                for order, slot in slot_of.items():
                    args = sc.operator_args(th, order, dt)
                    dev.assemble_matrix(SLOT_SCRATCH, **args)
                    st["A_full"][order] = dev.matrix(SLOT_SCRATCH)
                    dev.assemble_matrix(slot, **args)
                    dev.apply_bc(slot)
                    dev.setup_solver(slot)
                    assert not dev.factors_inexact[slot]
                    st["A_fac"][order] = st["A_mon"][order] = dev.matrix(slot)
                    st["solve"][order] = None
                    if check_ref:
                        assert np.array_equal(st["A_full"][order].data, ref[f"{case}/full{order}"]) and np.array_equal(st["A_fac"][order].data, ref[f"{case}/bc{order}"]), \
                            "the operators differ from the ones the reference handle assembled"

            def refined(order):
                if st["solve"][order] is None:
                    st["solve"][order] = sc.Refined(st["A_fac"][order])
                return st["solve"][order]

            def apply_opts(o):
                dev.set_solver_options(refine=o["refine"], check_residual=o["check"], method=o["method"], rtol=1e-13)

            dev.set_bc(dofs, prof)
            dev.set_time_scheme(sc.DT, True)
            operators(sc.DT, True)
            dev.set_sensors(rows)
            state = list(sc.initial_state(th, 1))
            dev.set_state(*state)
            hist, opts = sc.History(), dict(sc.DEFAULT_OPTS)
            apply_opts(opts)
            prev_state = None
            n_step = 0
            burst = dict(state=None, ys=[], tail=None, replay=[])  # back-to-back overlapped steps and their replay (ops "mark" ... "same_as_raw")

            def rhs_model(order, uc):
                u_n, u_nn, _ = dev.get_state()
                return m.rhs(order, st["dt"], st["nl"], u_n, u_nn, uc, st["A_full"][order], fprof=st["fprof"], Cmat=st["C"][order])

            def check_rhs(order, uc, what):
                """(a): fc_assemble_rhs against the longdouble right-hand side, 2-norm and max-norm."""
                b = dev.assemble_rhs(slot_of[order], uc)
                sc.apply_op(hist, ("rhs",))
                bl = rhs_model(order, uc)
                e2, ei = sc.rel2(b, bl), sc.relmax(b, bl)
                r2, ri = worst.see("rhs 2-norm", e2, tol["rhs"][0]), worst.see("rhs max-norm", ei, tol["rhs"][1])
                assert r2 <= 1 and ri <= 1, f"{tag} {what}: right-hand side misses the longdouble one by {e2:.3e} / {ei:.3e} (2-norm / max-norm), allowed {tol['rhs']}"
                return b, e2, ei

            def run_step(order, energy, mode, uc, expect_bad=False):
                slot = slot_of[order]
                if mode == "block":
                    try:
                        y, dE, info = dev.step(slot, uc, compute_energy=energy)
                    except FcError as e:
                        assert expect_bad and e.code == FC_ERR_DIVERGED, f"{tag}: {e}"
                        return None, None, dev._step_bufs[3].copy()
                    assert not expect_bad, f"{tag}: a non-finite step was not refused"
                    return y, dE, np.array(info)
                dev.step_begin(slot, uc, compute_energy=energy)
                try:
                    y, _, _ = dev.step_end(early=True)
                except FcError as e:
                    assert expect_bad and e.code == FC_ERR_DIVERGED, f"{tag}: {e}"
                    return None, None, np.array(dev.step_collect()[1])
                assert not expect_bad, f"{tag}: a non-finite step was not refused"
                dE, info = dev.step_collect()
                return y, dE, np.array(info)

            def route_check(settings, what):
                want = sc.predicted_route(case, kk, settings, hist)
                got = dev.step_route()
                assert np.array_equal(got, want), f"route not taken: {tag} {what}: predicted {dict(zip(sc.ROUTE_COLS, want.tolist()))}, reported {dict(zip(sc.ROUTE_COLS, got.tolist()))}"
                sc.advance(hist, want)
                return want

            for i, op in enumerate(sc.scenario(name)):
                kind = op[0]
                what = f"op {i} {op}"
                if kind == "opts":
                    opts = dict(op[1])
                    apply_opts(opts)
                elif kind == "rhs":
                    records[f"{tag}/b{i}"], e2, ei = check_rhs(op[1], sc.CONTROLS[op[2]], what)
                    print(f"[{kn}] {tag} {what}: rhs {e2:.2e} / {ei:.2e}", flush=True)
                elif kind == "step":
                    _, order, energy, mode, ui = op
                    uc = sc.CONTROLS[ui]
                    settings = dict(order=order, energy=energy, blocking=mode == "block", **opts)
                    before = dev.get_state()
                    line = f"[{kn}] {tag} {what}:"
                    if can_assemble:
                        b, e2, ei = check_rhs(order, uc, what)
                        line += f" rhs {e2:.2e} / {ei:.2e}"
                    else:
                        b = None
                    y, dE, info = run_step(order, energy, mode, uc)
                    route = route_check(settings, what)
                    r = dict(zip(sc.ROUTE_COLS, route.tolist()))
                    line += f" route {route.tolist()}"
                    # (b) solution and state
                    x = dev.get_solution()
                    u_n, u_nn, p_n = dev.get_state()
                    assert np.array_equal(u_n, x[:nn2]) and np.array_equal(p_n, x[nn2:]), f"{tag} {what}: the state is not the step's solution, bit for bit"
                    assert np.array_equal(u_nn, before[0]), f"{tag} {what}: u_nn is not the previous u_n, bit for bit"
                    prev_state = before
                    if b is not None:
                        R = refined(order)
                        xr = R(b)
                        if opts["method"] == "refine" and opts["refine"] > 0:  # one refinement sweep on the monitored operator
                            assert opts["refine"] == 1
                            res = np.asarray(np.asarray(b, dtype=sc.L) - sc.spmv_longdouble(st["A_mon"][order], xr), dtype=np.float64)
                            xr = xr + R(res)
                        ex = sc.rel2(x, xr)
                        line += f" solution {ex:.2e}"
                        assert worst.see("solution", ex, tol["solve"]) <= 1, f"{tag} {what}: solution misses the refined host solve by {ex:.3e} > {tol['solve']:.3e}"
                    # (c) sensors
                    assert y.shape == (len(rows),)
                    if rows:
                        yr, bound = m.sensors(rows, x)
                        ratio = max(worst.see("sensors", abs(sc.L(y[s]) - yr[s]), bound[s]) for s in range(len(rows)))
                        line += f" sensors {ratio:.2f} x bound"
                        assert ratio <= 1, f"{tag} {what}: a sensor reading misses its bound: {ratio:.3f} x"
                    # (d) energy
                    if energy:
                        Er = m.energy(x[:nn2])
                        ee = abs(float((sc.L(dE) - Er) / Er))
                        line += f" energy {ee:.2e}"
                        assert worst.see("energy", ee, tol["energy"]) <= 1, f"{tag} {what}: energy misses the longdouble value by {ee:.3e} > {tol['energy']:.3e}"
                    else:
                        assert np.isnan(dE) and r["g_cells"] == 0, f"{tag} {what}: compute_energy off must give NaN and no cell workgroups"
                    # (e) residual monitor
                    r_bound = None
                    assert info[3] == 0, f"{tag} {what}: non-finite flag {info[3]} on a finite step"
                    if r["monitored"]:
                        assert np.isfinite(info[1]) and np.isfinite(info[2]), f"{tag} {what}: a monitored step carries no residual: {info}"
                        if b is not None:
                            xm = x
                            if opts["method"] == "refine" and opts["refine"] > 0:  # the driver's partials are those of the first apply
                                apply_opts({**opts, "refine": 0})
                                xm = dev.solve(slot_of[order], b)[0]
                                apply_opts(opts)
                            rn, bn, bound = m.residual(st["A_mon"][order], xm, b)
                            r_bound = bound
                            eb = abs(float((sc.L(info[2]) - bn) / bn))
                            er = abs(sc.L(info[1]) * sc.L(info[2]) - rn)
                            line += f" |r|/|b| {info[1]:.2e} (true {float(rn / bn):.2e}, {float(er / bound):.2f} x bound) |b| {eb:.1e}"
                            assert worst.see("|b|", eb, tol["bnorm"]) <= 1, f"{tag} {what}: |b| misses by {eb:.3e}"
                            assert worst.see("|r|", er, bound) <= 1, f"{tag} {what}: the monitor's |r| misses the longdouble one by {float(er / bound):.2f} x its bound"
                            if st["lagged"]:
                                assert rn / bn > 1e-6, f"{tag} {what}: the lagged operator leaves no residual to compare: {float(rn / bn):.2e}"
                                worst.see("|r| relative, lagged operator", float(er / rn), float(bound / rn))
                    else:
                        assert np.isnan(info[1]) and np.isnan(info[2]), f"{tag} {what}: an unmonitored step carries a residual: {info}"
                        if r["tail"] != sc.TAIL_FINISH:  # off the cadence: the check workgroups test finiteness instead of the row workgroups
                            assert r["g_rows"] == 0 and (r["tail"] == sc.TAIL_OVERLAPPED or r["g_check"] == sc.cdiv(dev.N, sc.TAIL_CHECK_ROWS))
                    records[f"{tag}/{n_step}/rec"] = np.r_[y, dE, info[1], info[2]]
                    records[f"{tag}/{n_step}/x"] = x
                    burst["replay"].append((y, dE, info, x, route, r_bound))
                    n_step += 1
                    print(line, flush=True)
                elif kind == "mark":
                    burst.update(state=dev.get_state(), ys=[], tail=None)
                elif kind == "raw_step":  # nothing but the step itself: the late tail of this step runs while the next one is enqueued
                    _, order, energy, ui = op
                    dev.step_begin(slot_of[order], sc.CONTROLS[ui], compute_energy=energy)
                    burst["ys"].append(dev.step_end(early=True)[0])
                    burst["route"] = route_check(dict(order=order, energy=energy, blocking=False, **opts), what)
                elif kind == "raw_collect":
                    dE, info = dev.step_collect()
                    burst["tail"] = (dE, np.array(info), dev.get_solution())
                elif kind == "rewind":
                    dev.set_state(*burst["state"])
                    burst["replay"] = []
                    sc.apply_op(hist, op)
                elif kind == "same_as_raw":
                    rp = burst["replay"]
                    assert len(rp) == len(burst["ys"]) > 1
                    for k, rec in enumerate(rp):
                        assert np.array_equal(rec[0], burst["ys"][k]), f"{tag} {what}: sensors of back-to-back step {k} differ from the replay's: {burst['ys'][k]} / {rec[0]}"
                    (dE, info, x), (_, dEr, infor, xr, route_r, r_bound) = burst["tail"], rp[-1]
                    assert np.array_equal(x, xr), f"{tag} {what}: the solution after back-to-back steps differs from the replay's"
                    same_grid = np.array_equal(burst["route"][4:], route_r[4:])  # (the overlapped tail does not read FC_TAIL_REPS: other partials, another fold)
                    if same_grid:
                        assert np.array_equal(np.r_[dE, info[1:]], np.r_[dEr, infor[1:]], equal_nan=True), f"{tag} {what}: late record {dE} {info} against the replay's {dEr} {infor}"
                    else:  # both within their tolerances of the longdouble values, which the replay has been held to
                        assert abs(dE - dEr) <= tol["energy"] * abs(dEr) and abs(info[2] - infor[2]) <= tol["bnorm"] * infor[2], f"{tag} {what}: late record {dE} {info} against the replay's {dEr} {infor}"
                        assert r_bound is not None and abs(sc.L(info[1]) * sc.L(info[2]) - sc.L(infor[1]) * sc.L(infor[2])) <= 2 * r_bound
                    print(f"[{kn}] {tag} {what}: {len(rp)} back-to-back steps equal their replay bit for bit (late record: {'bit for bit' if same_grid else 'within the tolerances, another tail grid'})", flush=True)
                elif kind == "bad_step":
                    _, order, mode, bad = op
                    uc = sc.CONTROLS[1].copy()
                    if bad == "nan_u":
                        u_n, u_nn, p_n = dev.get_state()
                        u_n = u_n.copy()
                        u_n[int(np.setdiff1d(np.arange(nn2), dofs)[nn2 // 3])] = np.nan
                        dev.set_state(u_n, u_nn, p_n)
                        sc.apply_op(hist, ("set_state", 0, None))
                    else:
                        uc[0] = np.inf
                    settings = dict(order=order, energy=True, blocking=mode == "block", **opts)
                    _, _, info = run_step(order, True, mode, uc, expect_bad=True)
                    route = route_check(settings, what)
                    assert info[3] == 1, f"{tag} {what}: FC_ERR_DIVERGED without the flag in info[3]: {info}"
                    print(f"[{kn}] {tag} {what}: refused, flag 1, route {route.tolist()}", flush=True)
                elif kind == "set_state":
                    state = list(sc.initial_state(th, op[1]))
                    if op[2] == "nan_p":
                        state[2][2] = np.nan
                    dev.set_state(*state)
                    sc.apply_op(hist, op)
                elif kind == "time_scheme":
                    _, dt, nl, refactor = op
                    dev.set_time_scheme(dt, nl)
                    st["dt"], st["nl"] = dt, nl
                    if refactor:
                        operators(dt, False)
                        apply_opts(opts)  # (setup_solver sets the options it is given)
                    sc.apply_op(hist, op)
                elif kind == "undo":
                    dev.undo_step()
                    now = dev.get_state()
                    assert all(np.array_equal(a, c) for a, c in zip(now, prev_state)), f"{tag} {what}: undo_step did not bring the state back bit for bit"
                    sc.apply_op(hist, op)
                elif kind == "batch":
                    u_n, u_nn, p_n = dev.get_state()
                    dev.set_batch(2)
                    dev.set_state_batch(np.stack([u_n, u_nn]), np.stack([u_nn, u_n]), np.stack([p_n, p_n]))
                    dev.step_batch(SLOT_BDF2, np.stack([sc.CONTROLS[0], sc.CONTROLS[1]]))
                    dev.set_batch(0)
                    assert all(np.array_equal(a, c) for a, c in zip(dev.get_state(), (u_n, u_nn, p_n))), f"{tag} {what}: a batched step moved the single simulation's state"
                    sc.apply_op(hist, op)
                elif kind == "force":
                    st["fprof"] = None if op[1] is None else sc.force_profiles(th, op[1])
                    dev.set_force(st["fprof"])
                    sc.apply_op(hist, op)
                elif kind == "cop":
                    _, order, on = op
                    if on:
                        dev.assemble_matrix(SLOT_SCRATCH, **sc.cn_operator_args(th))
                        st["C"][order] = dev.matrix(SLOT_SCRATCH)[:, :nn2].tocsr()
                    else:
                        st["C"][order] = None
                    dev.set_rhs_operator(slot_of[order], st["C"][order])
                    sc.apply_op(hist, op)
                elif kind == "solve_energy":
                    bb = np.cos(0.37 * np.arange(dev.N))
                    xs, _ = dev.solve(SLOT_BDF2, bb)
                    assert sc.rel2(xs, refined(2)(bb)) <= tol["solve"]
                    u = dev.get_state()[0]
                    assert abs(float((sc.L(dev.energy(u)) - m.energy(u)) / m.energy(u))) <= tol["energy"]
                    sc.apply_op(hist, op)
                elif kind == "lagged":
                    order = op[1]
                    args = sc.operator_args(th, order, st["dt"], lagged=True)
                    dev.assemble_matrix(SLOT_SCRATCH, **args)
                    st["A_full"][order] = dev.matrix(SLOT_SCRATCH)
                    dev.assemble_matrix(slot_of[order], **args)
                    dev.apply_bc(slot_of[order])
                    dev.update_operator(slot_of[order])  # refreshes the monitor's permuted matrix, leaves the factors of A0
                    st["A_mon"][order] = dev.matrix(slot_of[order])
                    assert np.array_equal(st["A_mon"][order].data, ref[f"{case}/lagged{order}"])
                    st["lagged"] = True
                    sc.apply_op(hist, op)
                else:
                    raise KeyError(kind)
            print(f"RUN OK [{kn}] {tag}: {n_step} steps ({time.time() - t0:.1f} s)", flush=True)
        finally:
            dev.close()
    np.savez(rec_path, **records)
    # the source claims the same summation order for the two element kernels: said, not asserted (the assertion is the tolerance)
    for case in sc.CASES:
        pairs = [(records[k], records[k.replace("/default/", "/reg/")]) for k in sorted(records)
                 if k.startswith(f"rhs/{case}/default/") and k.rsplit("/", 1)[1].startswith("b") and k.replace("/default/", "/reg/") in records]
        if pairs:
            same = sum(bool(np.array_equal(a, c)) for a, c in pairs)
            diff = max(np.abs(a - c).max() / np.abs(a).max() for a, c in pairs)
            print(f"ELEM KERNELS {case}: fc_rhs_elem and fc_rhs_elem_reg agree bit for bit on {same} of {len(pairs)} right-hand sides (largest difference {diff:.1e} of the largest entry)", flush=True)
    for what, (r, v, t) in sorted(worst.w.items()):
        print(f"WORST {kn} {what}: {v:.3e} of {t:.3e} allowed ({r:.3f} x)", flush=True)
    print("CHILD OK", kn, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], json.loads(sys.argv[3]), sys.argv[4])
