"""Child process of tests/test_batch_step_routes_gpu.py: the runs of batch_step_cases.RUNS for ONE set of process-level knobs (the
library reads them once per process) -- a fresh handle per run, created under the run's handle-level knobs -- against the np.longdouble
host model of step_cases.HostModel, column by column and step by step.

    python batch_step_child.py <knob set> <tolerances as JSON> <records.npz to write>

After every step fc_get_batch_step_route must report the route the host model predicts; the right-hand side the solve consumed
(fc_debug_capture_batch_rhs) is held to HostModel.rhs of every column, the solution to a refined host solve of the device's operator and
that right-hand side, the state to the solution bit for bit, sensors, energy and residual norms to the model and its bounds.  Prints one
line per step, the worst ratio to every tolerance at the end, and exits non-zero with the failed assertion.  The records (right-hand side,
solution, y, dE, residual norms of every step and column) go to the file named last: the parent compares them between children bit for
bit."""
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


def main(kn: str, tol: dict, rec_path: str) -> None:
    from flowcontrol_amd._lib import FC_ERR_DIVERGED, FC_ERR_INVALID, FC_ERR_NOT_READY, FcError, ptr
    from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, SLOT_SCRATCH, DeviceSolver
    from tests.support import batch_step_cases as bs
    from tests.support import step_cases as sc

    knobs = bs.KNOB_SETS[kn]
    for name in bs.PROCESS_KNOBS:
        assert os.environ.get(name) == knobs.get(name), f"{name} in the environment is not the knob set's"
    assert DeviceSolver.BATCH_ROUTE_COLS == bs.ROUTE_COLS
    worst, records, models = Worst(), {}, {}
    slot_of = {1: SLOT_BDF1, 2: SLOT_BDF2}
    L = sc.L

    def make_handle(mesh, hs):
        for name in bs.HANDLE_KNOBS:  # read when the handle is created
            os.environ.pop(name, None)
        os.environ.update(bs.HANDLE_SETS[hs])
        th, dofs, prof = bs.host_case(mesh)
        dev = DeviceSolver(th)
        st = dict(A_full={}, A_fac={}, n_ctrl={}, solve={})
        try:
            dev.set_bc(dofs, prof)
            dev.set_time_scheme(sc.DT, True)
            isbc = np.zeros(th.N, dtype=bool)
            isbc[dofs] = True
            for order, slot in slot_of.items():
                args = sc.operator_args(th, order)
                dev.assemble_matrix(SLOT_SCRATCH, **args)
                st["A_full"][order] = dev.matrix(SLOT_SCRATCH)
                dev.assemble_matrix(slot, **args)
                dev.apply_bc(slot)
                dev.setup_solver(slot)
                assert not dev.factors_inexact[slot]
                st["A_fac"][order] = dev.matrix(slot)
                # build_ctrl_rows: the Dirichlet rows and the rows with an entry in a lifting vector A_full g_k (|A| |g|: no cancellation on the host)
                g = np.zeros((th.N, prof.shape[1]))
                g[dofs] = np.abs(prof)
                st["n_ctrl"][order] = int(np.count_nonzero(isbc | ((abs(st["A_full"][order]) @ g) != 0).any(axis=1)))
            dev.set_solver_options(refine=0, check_residual=1, method="refine", rtol=1e-13)
        except BaseException:
            dev.close()
            raise
        return dev, st

    for run, capture in [(r, True) for r in bs.RUNS[kn]] + [(r, False) for r in (bs.UNCAPTURED if kn == "default" else [])]:
        t0 = time.time()
        name, mesh, k, hs, sens = run
        tag = bs.run_name(run) + ("" if capture else "/uncaptured")
        kk = {**knobs, **bs.HANDLE_SETS[hs]}
        if mesh not in models:
            bs.host_case(mesh)
            models[mesh] = sc.HostModel(mesh)
        m = models[mesh]
        th, dofs = m.th, m.dofs
        nn2, N = 2 * th.nn, th.N
        rows = sc.sensor_rows(th, sens)
        rhs_tol = tol["rhs"]
        dev, st = make_handle(mesh, hs)
        try:
            lib, h = dev.lib, dev._h
            dev.set_sensors(rows)
            buf = np.full((k, N), -7.0)
            if capture and k % 2:  # switched on before the batch exists (fc_set_batch allocates the copy) ...
                dev.capture_batch_rhs(True)
            dev.set_batch(k)
            if capture and not k % 2:  # ... or behind it
                dev.capture_batch_rhs(True)
            assert lib.fc_debug_get_batch_rhs(h, k, ptr(buf)) == FC_ERR_NOT_READY and np.all(buf == -7.0), f"{tag}: a captured right-hand side before any step"
            rbuf = np.full(len(bs.ROUTE_COLS), -7, dtype=np.int32)
            assert lib.fc_get_batch_step_route(h, rbuf.size, ptr(rbuf)) == FC_ERR_NOT_READY and np.all(rbuf == -7), f"{tag}: a route before any step"
            cols = [bs.column_state(th, s, k, 1) for s in range(k)]
            dev.set_state_batch(np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols]))
            hist, check = bs.History(), 1
            fprof, Cmat = None, {1: None, 2: None}
            n_step = 0

            def refined(order):
                if order not in st["solve"]:
                    st["solve"][order] = sc.Refined(st["A_fac"][order])
                return st["solve"][order]

            def run_step(order, energy, mode, shift, expect_bad):
                """The step itself: (controls, force amplitudes, y, dE, info, flags)."""
                u = bs.controls(k, shift)
                uf = bs.force_amplitudes(k, shift) if fprof is not None else None
                diverged = False
                if mode == "block":  # fc_step_batch itself (DeviceSolver.step_batch is begin + end: the overlapped form)
                    bu, buf_, by, bdE, binfo, (pu, puf, py, pdE, pinfo) = dev._batch_buffers()
                    bu[:, : dev.n_act] = u
                    if uf is not None:
                        buf_[:, : dev.n_act] = uf
                    code = lib.fc_step_batch(h, slot_of[order], k, pu, puf if uf is not None else None, py, pdE, 1 if energy else 0, pinfo)
                    assert code in (0, FC_ERR_DIVERGED), f"{tag}: fc_step_batch: status {code}: {(lib.fc_last_error() or b'').decode()}"
                    diverged = code == FC_ERR_DIVERGED
                    y, dE, info = by[:, : dev.n_sens].copy(), bdE.copy(), np.array(binfo)
                    flags = info[:, 3].astype(np.int64)
                else:
                    dev.step_batch_begin(slot_of[order], u, compute_energy=energy, u_force=uf)
                    try:
                        y, flags = dev.step_batch_end_early()
                    except FcError as e:
                        assert e.code == FC_ERR_DIVERGED, f"{tag}: {e}"
                        diverged = True
                        y, flags = dev._batch_bufs[2][:, : dev.n_sens].copy(), dev._batch_flags
                    flags = np.array(flags, dtype=np.int64)
                    dE, info = dev.step_batch_collect()
                    info = np.array(info)
                    assert np.all(np.isnan(info[:, 3])), f"{tag}: the flags come with the early end, the late record repeats none"
                assert diverged == expect_bad, f"{tag}: FC_ERR_DIVERGED {'missing' if expect_bad else 'on a finite step'}"
                return u, uf, y, np.array(dE), info, flags

            def full_step(i, op, bad_col=None, clean=None):
                """One step through every check; ``bad_col``: that column's state is non-finite and ``clean`` the records of the same step
                without it."""
                nonlocal n_step
                _, order, energy, mode, shift = op
                what = f"op {i} {op}" + (f" (column {bad_col} non-finite)" if bad_col is not None else "")
                settings = dict(order=order, energy=energy, mode=mode, check=check)
                want = bs.predicted_route(mesh, k, kk, settings, hist, st["n_ctrl"][order])
                before = dev.get_state_batch()
                u, uf, y, dE, info, flags = run_step(order, energy, mode, shift, bad_col is not None)
                got = dev.batch_step_route()
                assert np.array_equal(got, want), f"route not taken: {tag} {what}: predicted {dict(zip(bs.ROUTE_COLS, want.tolist()))}, reported {dict(zip(bs.ROUTE_COLS, got.tolist()))}"
                bs.advance(hist, want)
                r = dict(zip(bs.ROUTE_COLS, want.tolist()))
                x = dev.get_solution_batch()
                after = dev.get_state_batch()
                if capture:
                    b = dev.batch_rhs()
                else:
                    assert lib.fc_debug_get_batch_rhs(h, k, ptr(buf)) == FC_ERR_NOT_READY, f"{tag} {what}: a captured right-hand side without capture"
                    b = None
                good = [s for s in range(k) if s != bad_col]
                # flags: set for the non-finite column only
                assert flags.tolist() == [int(s == bad_col) for s in range(k)], f"{tag} {what}: flags {flags.tolist()}"
                # state: the new u_n is the velocity part of the solution, u_nn the previous u_n, bit for bit
                assert np.array_equal(after[0][good], x[good, :nn2]) and np.array_equal(after[2][good], x[good, nn2:]), f"{tag} {what}: the state is not the step's solution, bit for bit"
                assert np.array_equal(after[1][good], before[0][good]), f"{tag} {what}: u_nn is not the previous u_n, bit for bit"
                assert y.shape == (k, len(rows)) and dE.shape == (k,) and info.shape == (k, 4)
                line = f"[{kn}] {tag} {what}: route {want.tolist()}"
                rec = np.c_[y, dE, info[:, 1], info[:, 2]]
                if clean is not None:  # the other columns of the batch equal the run without the non-finite one, bit for bit
                    cb, cx, crec = clean
                    assert b is None or np.array_equal(b[good], cb[good]), f"{tag} {what}: a non-finite column changed another column's right-hand side"
                    assert np.array_equal(x[good], cx[good]), f"{tag} {what}: a non-finite column changed another column's solution"
                    assert np.array_equal(rec[good], crec[good], equal_nan=True), f"{tag} {what}: a non-finite column changed another column's record"
                    assert not np.all(np.isfinite(x[bad_col, :nn2])), f"{tag} {what}: the non-finite column has a finite velocity"
                    line += f" others equal the clean step bit for bit, flag on column {bad_col} only"
                else:
                    e = dict(rhs2=0.0, rhsi=0.0, sol=0.0, sens=0.0, en=0.0, r=0.0, bn=0.0)
                    R = refined(order)
                    for s in good:
                        where = f"{tag} {what} column {s}"
                        # right-hand side the solve consumed against the longdouble one
                        if b is not None:
                            bl = m.rhs(order, sc.DT, True, before[0][s], before[1][s], u[s], st["A_full"][order], fprof=fprof, uforce=None if uf is None else uf[s],
                                       Cmat=Cmat[order])
                            e2, ei = sc.rel2(b[s], bl), sc.relmax(b[s], bl)
                            e["rhs2"], e["rhsi"] = max(e["rhs2"], e2), max(e["rhsi"], ei)
                            r2, ri = worst.see("rhs 2-norm", e2, rhs_tol[0]), worst.see("rhs max-norm", ei, rhs_tol[1])
                            assert r2 <= 1 and ri <= 1, f"{where}: right-hand side misses the longdouble one by {e2:.3e} / {ei:.3e} (2-norm / max-norm), allowed {rhs_tol}"
                            # solution against the refined host solve of the device's operator and that right-hand side
                            ex = sc.rel2(x[s], R(b[s]))
                            e["sol"] = max(e["sol"], ex)
                            assert worst.see("solution", ex, tol["solve"]) <= 1, f"{where}: solution misses the refined host solve by {ex:.3e} > {tol['solve']:.3e}"
                        if rows:
                            yr, bound = m.sensors(rows, x[s])
                            ratio = max(worst.see("sensors", abs(L(y[s, q]) - yr[q]), bound[q]) for q in range(len(rows)))
                            e["sens"] = max(e["sens"], ratio)
                            assert ratio <= 1, f"{where}: a sensor reading misses its bound: {ratio:.3f} x"
                        if energy:
                            Er = m.energy(x[s, :nn2])
                            ee = abs(float((L(dE[s]) - Er) / Er))
                            e["en"] = max(e["en"], ee)
                            assert worst.see("energy", ee, tol["energy"]) <= 1, f"{where}: energy misses the longdouble value by {ee:.3e} > {tol['energy']:.3e}"
                        else:
                            assert np.isnan(dE[s]), f"{where}: compute_energy off must give NaN"
                        if r["monitored"]:
                            assert np.isfinite(info[s, 1]) and np.isfinite(info[s, 2]), f"{where}: a monitored step carries no residual: {info[s]}"
                            if b is not None:
                                rn, bnorm, bound = m.residual(st["A_fac"][order], x[s], b[s])
                                eb = abs(float((L(info[s, 2]) - bnorm) / bnorm))
                                er = float(abs(L(info[s, 1]) * L(info[s, 2]) - rn) / bound)
                                e["r"], e["bn"] = max(e["r"], er), max(e["bn"], eb)
                                assert worst.see("|b|", eb, tol["bnorm"]) <= 1, f"{where}: |b| misses by {eb:.3e}"
                                assert worst.see("|r|", er, 1.0) <= 1, f"{where}: the monitor's |r| misses the longdouble one by {er:.2f} x its bound"
                        else:  # off the cadence: NaN in the info, as fc_step_batch documents
                            assert np.isnan(info[s, 1]) and np.isnan(info[s, 2]), f"{where}: an unmonitored step carries a residual: {info[s]}"
                    if k >= 4:  # the same scenario in two columns of one batch
                        assert b is None or np.array_equal(b[0], b[k - 1]), f"{tag} {what}: columns 0 and {k - 1} carry the same scenario, their right-hand sides differ"
                        assert np.array_equal(x[0], x[k - 1]) and np.array_equal(rec[0], rec[k - 1], equal_nan=True), f"{tag} {what}: columns 0 and {k - 1} carry the same scenario and differ"
                    line += (f" rhs {e['rhs2']:.2e} / {e['rhsi']:.2e} solution {e['sol']:.2e} sensors {e['sens']:.2f} x bound energy {e['en']:.2e} "
                             f"|r| {e['r']:.2f} x bound |b| {e['bn']:.1e}")
                if b is not None:
                    records[f"{tag}/{n_step}/b"] = b
                records[f"{tag}/{n_step}/x"] = x
                records[f"{tag}/{n_step}/rec"] = rec
                n_step += 1
                print(line, flush=True)
                return b, x, rec

            for i, op in enumerate(bs.scenario(name)):
                kind = op[0]
                if kind == "opts":
                    check = op[1]
                    dev.set_solver_options(refine=0, check_residual=check, method="refine", rtol=1e-13)
                elif kind == "step":
                    full_step(i, op)
                elif kind == "set_state":
                    cols = [bs.column_state(th, s, k, op[1]) for s in range(k)]
                    dev.set_state_batch(np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols]))
                    bs.apply_op(hist, op)
                elif kind == "cop":
                    _, order, on = op
                    if on:
                        dev.assemble_matrix(SLOT_SCRATCH, **sc.cn_operator_args(th))
                        Cmat[order] = dev.matrix(SLOT_SCRATCH)[:, :nn2].tocsr()
                    else:
                        Cmat[order] = None
                    dev.set_rhs_operator(slot_of[order], Cmat[order])
                    bs.apply_op(hist, op)
                elif kind == "force":
                    fprof = None if op[1] is None else sc.force_profiles(th, op[1])
                    dev.set_force(fprof)
                    bs.apply_op(hist, op)
                elif kind == "nonfinite":
                    c = k // 2
                    s0 = dev.get_state_batch()
                    dev.set_state_batch(*s0)
                    bs.apply_op(hist, ("set_state", 0))
                    clean = full_step(i, ("step",) + op[1:])
                    un = s0[0].copy()
                    un[c, int(np.setdiff1d(np.arange(nn2), dofs)[nn2 // 3])] = np.nan
                    dev.set_state_batch(un, s0[1], s0[2])
                    bs.apply_op(hist, ("set_state", 0))
                    full_step(i, ("step",) + op[1:], bad_col=c, clean=clean)
                    # fc_reset_sim_batch: that column's two time levels become zero, nothing else moves
                    s1 = dev.get_state_batch()
                    dev.reset_sim_batch(c)
                    bs.apply_op(hist, ("reset",))
                    s2 = dev.get_state_batch()
                    others = [s for s in range(k) if s != c]
                    assert all(np.all(a[c] == 0.0) for a in s2), f"{tag} op {i}: fc_reset_sim_batch left something in column {c}"
                    assert all(np.array_equal(a[others], d[others]) for a, d in zip(s1, s2)), f"{tag} op {i}: fc_reset_sim_batch moved another column"
                else:
                    raise KeyError(kind)
            if capture:  # switching the capture off frees the copy: the getter is not ready again
                dev.capture_batch_rhs(False)
                assert lib.fc_debug_get_batch_rhs(h, k, ptr(buf)) == FC_ERR_NOT_READY
            print(f"RUN OK [{kn}] {tag}: {n_step} steps ({time.time() - t0:.1f} s)", flush=True)
        finally:
            dev.close()

    # capture on against capture off, and columns 0 to 2 of k = 3 against the same three scenarios at k = 4: bit for bit
    def same(tag_a, tag_b, what, sel=slice(None), with_b=True):
        keys = sorted(key for key in records if key.startswith(tag_a + "/") and key[len(tag_a) + 1:].split("/")[0].isdigit() and (with_b or not key.endswith("/b")))
        assert keys, tag_a
        for key in keys:
            other = tag_b + key[len(tag_a):]
            assert other in records and np.array_equal(records[key][sel], records[other][sel], equal_nan=True), f"{what}: {key} differs from {other}"
        print(f"BITWISE [{kn}] {what}: {len(keys)} records", flush=True)

    if kn == "default":
        for run in bs.UNCAPTURED:
            same(bs.run_name(run) + "/uncaptured", bs.run_name(run), "capture off == capture on", with_b=False)
        r3 = next(r for r in bs.RUNS[kn] if r[2] == 3 and (r[0], r[1], 4) + r[3:] in bs.RUNS[kn])
        same(bs.run_name(r3), bs.run_name((r3[0], r3[1], 4) + r3[3:]), "columns 0-2 of k = 3 == k = 4", sel=slice(0, 3))

    # refusals: fc_set_batch with a row block narrower than a matrix row
    for ks, mesh, k in bs.REFUSED:
        if ks != kn:
            continue
        dev, _ = make_handle(mesh, "overlapped")
        try:
            code = dev.lib.fc_set_batch(dev._h, k)
            msg = (dev.lib.fc_last_error() or b"").decode()
            assert code == FC_ERR_INVALID and bs.REFUSAL in msg, f"fc_set_batch({k}) on {mesh} under {knobs}: status {code}, {msg!r}"
            print(f"REFUSED [{kn}] fc_set_batch({k}) on {mesh}: {msg}", flush=True)
        finally:
            dev.close()
    np.savez(rec_path, **records)
    for what, (r, v, t) in sorted(worst.w.items()):
        print(f"WORST {kn} {what}: {v:.3e} of {t:.3e} allowed ({r:.3f} x)", flush=True)
    print("CHILD OK", kn, flush=True)


if __name__ == "__main__":
    main(sys.argv[1], json.loads(sys.argv[2]), sys.argv[3])
