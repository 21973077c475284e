"""Device side of tests/test_tangent_march_gpu.py: the runs of tests/support/tangent_march_cases.py on the device, the last step of the
marches of every length n = 1 .. steps held to the np.longdouble host model, kernel by kernel, on the device's OWN inputs
(fc_debug_get_tangent_stage, fc_debug_get_adjoint_tape / _batch), and to the route the host model predicts (fc_get_tangent_route).  The
test imports check_single / check_batch / check_tail_reads_dx; as a program

    python tangent_march_child.py single|batch|all

runs every run of the table in one fresh process, goes on past a failed comparison to the next run, prints one line per step and the
worst fraction of every bound at the end, and exits non-zero if a run failed.  No test starts it (no knob here is read per process).

Which inputs a step read.  Step n reads x1 = x_{n-1}, x2 = x_{n-2} from the state tape, d1 = dx_{n-1}, which the stage still holds (the
tail writes over the OLDER level), and d2 = dx_{n-2}: the given dx0 / dxm1 for n <= 2, else the dx_{n-1}' the march of length n - 1
returned as its older level -- two identical marches are bit-identical, which is asserted first."""
import sys
import time

import numpy as np

from tests.support import step_cases as sc
from tests.support import tangent_march_cases as tc
from tests.support.adjoint_march_child import Worst, _ratio, knobs

L = np.longdouble

TOL = {}
# element vectors of the first step of the single runs, by run: the two element kernels of a route are compared in a report
RECORDS = {}


class Handle:
    """A fresh nonlinear handle of a run: operators of both orders (the device's own, downloaded for the host model), actuators,
    sensors; ``k`` > 0: a batch of k.  State tape and tangent buffers reserved for ``steps`` steps."""

    def __init__(self, mesh, n_act, variant, sens, hs, refine, steps, k=0, lagged=False):
        from flowcontrol_amd._lib import check
        from flowcontrol_amd.device import SLOT_BDF1, SLOT_BDF2, SLOT_SCRATCH, DeviceSolver

        self.slot_of = {1: SLOT_BDF1, 2: SLOT_BDF2}
        self.th, self.dofs = tc.host_case(mesh)
        th = self.th
        with knobs(tc.HANDLE_SETS[hs], tc.HANDLE_KNOBS):  # read when the handle is created, by nothing later
            dev = self.dev = DeviceSolver(th)
        try:
            dev.set_bc(self.dofs, tc.profiles(th, self.dofs, n_act))
            dev.set_time_scheme(tc.DT, True)
            A_full, A_bc = {}, {}
            for order, slot in self.slot_of.items():
                args = sc.operator_args(th, order)
                dev.assemble_matrix(SLOT_SCRATCH, **args)
                A_full[order] = dev.matrix(SLOT_SCRATCH)
                dev.assemble_matrix(slot, **args)
                dev.apply_bc(slot)
                dev.setup_solver(slot, refine=refine)
                assert not dev.factors_inexact[slot]
                A_bc[order] = dev.matrix(slot)
            if lagged:  # the BDF2 operator replaced behind its factors: a refinement sweep's dx is no rounding effect then
                dev.assemble_matrix(SLOT_BDF2, **sc.operator_args(th, 2, lagged=True))
                dev.apply_bc(SLOT_BDF2)
                dev.update_operator(SLOT_BDF2)
            self.model = tc.TangentMarchModel(mesh, n_act, variant, sens, A_full)
            if self.model.fprof is not None:
                dev.set_force(self.model.fprof)
            dev.set_sensors(self.model.rows)
            if k:
                dev.set_solver_options(refine=0, check_residual=1)
                dev.set_batch(k)
                dev.adjoint_tape_reserve_batch(steps)
            else:
                dev.adjoint_tape_reserve(steps)
            dev.tangent_reserve(1)
            self.solve = {o: tc.Refined(A_bc[o]) for o in (1, 2)}
            if dev.perm is None:
                dev.perm = np.empty(dev.N, dtype=np.int32)
                check(dev.lib.fc_get_permutation(dev._h, dev.perm))
            self.perm = np.asarray(dev.perm)
        except BaseException:
            dev.close()
            raise

    def to_w(self, v):
        """A vector (or [N][KB] block) of the stage, permuted numbering -> W numbering."""
        out = np.empty_like(v)
        out[self.perm] = v
        return out

    def close(self):
        self.dev.close()


def ulps(a, b) -> float:
    """Largest |a - b| in units of the spacing at the larger of the two."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a == b, 0.0, np.abs(a - b) / np.spacing(m))
    return float(r.max()) if r.size else 0.0


STAGE_ARRAYS = ("ev", "b", "x", "new", "other", "du", "dy", "flags")


def same_stage(a, b) -> bool:
    return all(np.array_equal(a[q], b[q], equal_nan=True) for q in STAGE_ARRAYS) and (a["dx"] is None) == (b["dx"] is None) and \
        (a["dx"] is None or np.array_equal(a["dx"], b["dx"], equal_nan=True))


def check_operands(h: Handle, order, st, worst, tag):
    """The control columns' operands as the device holds them: lift within (L + 2) eps sum |a g| of the longdouble row sum of the
    device's raw operator (any order), the load vectors within 16 x HOST_RHS_ERROR (max-norm) of the longdouble ones; load vectors are
    there exactly when fc_set_force supplied profiles."""
    m = h.model
    if m.n_act == 0:
        return
    _, lift, F, lb = m.control_columns(order)
    un = lambda a: np.stack([h.to_w(c) for c in a])  # noqa: E731
    dl = un(st["lift"])
    assert (st["fvec"] is not None) == (m.fprof is not None), f"{tag}: load vectors {'missing' if st['fvec'] is None else 'present without profiles'}"
    f = m.free
    rl = _ratio((dl - lift)[:, f], lb[:, f])
    assert worst.see("lift", rl, 1.0) <= 1, f"{tag}: the lifting misses the longdouble row sum by {rl:.3f} x its bound"
    if m.fprof is not None:
        df = un(st["fvec"])
        rf = max(float(np.abs(df[k] - F[k])[f].max() / np.abs(F[k]).max()) for k in range(m.n_act))
        assert worst.see("load vectors, max-norm", rf, TOL["load"]) <= 1, f"{tag}: a load vector misses the longdouble one by {rf:.3e} > {TOL['load']:.3e}"
        assert not df[:, m.dofs].any() and not df[:, 2 * m.nn:].any(), f"{tag}: a load vector is not zero on the Dirichlet / pressure rows"


def check_step(h: Handle, order, d1, d2, x1, x2, du, st, dy_ret, worst, tag, col=None, own=None):
    """One tangent step (``col``: column of a batched one) against the model.  d1 / d2, x1 / x2: the tangent levels and taped states
    the step read (W numbering), du: its control row or None, dy_ret: what the march returned for it.  ``own``: (x1, x2) of the column's
    OWN trajectory when the step is SHARED -- the model fed them must miss the device by the seeded-mistake margin."""
    m = h.model
    pick = (lambda a: a) if col is None else (lambda a: np.ascontiguousarray(a[..., col]))
    ev, b_p, x_p, new_p, other_p = (pick(st[q]) for q in ("ev", "b", "x", "new", "other"))
    dx_p = None if st["dx"] is None else pick(st["dx"])
    du_dev, dy_dev = (st["du"], st["dy"]) if col is None else (st["du"][col], st["dy"][col])
    b, nn2, line = h.to_w(b_p), 2 * m.nn, f"{tag}:"
    coeffs = tc.step_coeffs(order)
    duv = np.zeros(m.n_act) if du is None else np.asarray(du, dtype=np.float64)
    assert np.array_equal(du_dev, duv), f"{tag}: the control row on the device is not the given one"
    assert np.array_equal(h.to_w(other_p), d1), f"{tag}: the level the tail does not own was touched (or is not dx of the step before)"
    # ev ---------------------------------------------------------------------------------------------------------------------------
    ev_ref, rows_ref = m.elem_part(d1, d2, x1, x2, coeffs)
    if np.any(ev_ref):
        e2, ei = tc.rel2(ev, ev_ref), tc.relmax(ev, ev_ref)
        r2, ri = worst.see("ev 2-norm", e2, TOL["rhs"][0]), worst.see("ev max-norm", ei, TOL["rhs"][1])
        line += f" ev {e2:.2e} / {ei:.2e},"
        assert r2 <= 1 and ri <= 1, f"{tag}: ev misses the longdouble element vectors by {e2:.3e} / {ei:.3e} (2-norm / max-norm), allowed {TOL['rhs']}"
        if own is not None and (np.any(d1) or np.any(d2)) and not (np.array_equal(own[0], x1) and np.array_equal(own[1], x2)):
            miss = tc.relmax(ev, m.elem_part(d1, d2, own[0], own[1], coeffs)[0]) / TOL["rhs"][1]
            worst.see("ev against the column's OWN trajectory (must exceed 1000)", 1000.0, miss)
            assert miss >= 1000, f"{tag}: SHARED: the model fed the column's own trajectory is only {miss:.1f} x the tolerance away"
    else:
        assert not np.any(ev), f"{tag}: element vectors of zero levels are not zero"
    # b ----------------------------------------------------------------------------------------------------------------------------
    lift = np.stack([h.to_w(c) for c in st["lift"]]) if m.n_act else None
    fvec = np.stack([h.to_w(c) for c in st["fvec"]]) if (m.n_act and st["fvec"] is not None) else None
    ref = m.rhs(rows_ref, duv, order, lift=lift, fvec=fvec)
    if np.any(ref[:nn2]):
        e2, ei = tc.rel2(b[:nn2], ref[:nn2]), tc.relmax(b[:nn2], ref[:nn2])
        r2, ri = worst.see("b 2-norm", e2, TOL["rhs"][0]), worst.see("b max-norm", ei, TOL["rhs"][1])
        line += f" b {e2:.2e} / {ei:.2e},"
        assert r2 <= 1 and ri <= 1, f"{tag}: b misses the longdouble right-hand side by {e2:.3e} / {ei:.3e} (2-norm / max-norm), allowed {TOL['rhs']}"
    else:
        assert not np.any(b[:nn2]), f"{tag}: b of a zero column is not zero"
    rd = _ratio(b[m.dofs] - ref[m.dofs], m.dirichlet_bound(duv))
    assert worst.see("b, Dirichlet rows", rd, 1.0) <= 1, f"{tag}: a Dirichlet row of b misses the profile times du by {rd:.3f} x (n_act + 2) eps sum |prof| |du|"
    # free rows on the device's own element vectors and operands: the row's cells, then n_act products each of lift and fvec -- an fp64
    # sum of (cells + 2 n_act) terms in any order; a pressure row has no cells (exactly 0 without controls)
    cells = np.bincount(np.r_[m.hm.cn.reshape(-1), m.nn + m.hm.cn.reshape(-1)], minlength=m.N)
    mag = m.gather(np.abs(ev))
    own_rows = m.rhs(m.gather(ev), duv, order, lift=lift, fvec=fvec)
    if m.n_act:
        mag = mag + np.abs(duv).astype(L) @ np.abs(lift).astype(L) + (np.abs(duv).astype(L) @ np.abs(fvec).astype(L) if fvec is not None else 0)
    f = m.free
    rr = _ratio((b - own_rows)[f], ((cells + 2 * m.n_act + 2) * sc.EPS * mag)[f])
    assert worst.see("b, free rows from the device's own ev, lift, fvec", rr, 1.0) <= 1, f"{tag}: a free row of b misses its own terms' sum by {rr:.3f} x its bound"
    if not m.n_act or not np.any(duv):
        assert not b[nn2:].any(), f"{tag}: a pressure row of b is not exactly 0"
    # x ----------------------------------------------------------------------------------------------------------------------------
    lev_ref, dy_ref, dy_bound = m.tail(h.to_w(x_p), None if dx_p is None else h.to_w(dx_p))
    if np.all(np.isfinite(b)) and np.any(b):
        ex = tc.rel2(lev_ref, h.solve[order](b))
        line += f" x {ex:.2e},"
        assert worst.see("x", ex, TOL["solve"]) <= 1, f"{tag}: x misses the refined host solve of the device's b by {ex:.3e} > {TOL['solve']:.3e}"
    # the new level, dy --------------------------------------------------------------------------------------------------------------
    assert np.array_equal(h.to_w(new_p), lev_ref, equal_nan=True), f"{tag}: the new level is not x{' + dx' if dx_p is not None else ''}, bit for bit"
    assert np.array_equal(dy_dev, dy_ret), f"{tag}: the returned dy row is not the device's"
    if len(m.rows):
        ry = _ratio(np.asarray(dy_dev, dtype=L) - dy_ref, dy_bound)
        line += f" dy {ry:.3f} x bound"
        assert worst.see("dy", ry, 1.0) <= 1, f"{tag}: dy misses C (x + dx) by {ry:.3f} x (entries + 2) eps sum |c| |x + dx|"
    else:
        assert np.size(dy_dev) == 0 and np.size(dy_ret) == 0
        line += " no sensors"
    print(line, flush=True)


def check_single(run, worst=None):
    """One run of tc.SINGLE_RUNS."""
    worst = worst or Worst()
    mesh, n_act, variant, sens, hs, first, refine, steps, given = run
    tag0 = tc.run_name(run[:-1]) + "/" + "".join(c for c, g in zip("u01", given) if g)
    t0 = time.time()
    h = Handle(mesh, n_act, variant, sens, hs, refine, steps)
    try:
        dev, m = h.dev, h.model
        u = 0.1 * np.random.default_rng(3).standard_normal((steps, n_act))
        du, d0, dm1 = tc.inputs(m.N, n_act, steps, 7)
        du, d0, dm1 = (a if g else None for a, g in zip((du, d0, dm1), given))
        zero = np.zeros(m.N)

        def march(n):
            dev.set_state(*sc.initial_state(h.th, 1))
            dev.adjoint_tape_begin()
            dev.run(h.slot_of[first], n, u[:n], compute_energy=False)
            X = dev.adjoint_tape_states()
            out = dev.run_tangent(h.slot_of[first], n, None if du is None else du[:n], d0, dm1)
            return X, out, dev.tangent_stage(), dev.tangent_route()

        prev = None
        for n, order, want in tc.walk_single(run):
            X, (dy, dxn, dxnm1), st, got = march(n)
            assert np.array_equal(got, want), f"route not taken: {tag0} n = {n}: predicted {dict(zip(tc.ROUTE_COLS, want.tolist()))}, reported {dict(zip(tc.ROUTE_COLS, got.tolist()))}"
            if n == 1:  # two identical marches are bit-identical: what the choice of d2 below rests on
                X2, out2, st2, _ = march(n)
                assert np.array_equal(X, X2) and all(np.array_equal(a, c) for a, c in zip((dy, dxn, dxnm1), out2)) and same_stage(st, st2), f"{tag0}: two identical marches differ"
            d1 = (zero if d0 is None else d0) if n == 1 else prev[0]
            d2 = (zero if dm1 is None else dm1) if n == 1 else (zero if d0 is None else d0) if n == 2 else prev[1]
            assert st["refined"] == bool(refine) and not st["flags"].any()
            check_operands(h, order, st, worst, tag0)
            check_step(h, order, d1, d2, X[n], X[n - 1], None if du is None else du[n - 1], st, dy[n - 1], worst, f"{tag0} n = {n}")
            assert np.array_equal(dxn, h.to_w(st["new"])) and np.array_equal(dxnm1, h.to_w(st["other"])), f"{tag0} n = {n}: the returned levels are not the device's"
            if n == 1:
                RECORDS[tc.run_name(run)] = st["ev"]
            prev = (dxn, dxnm1)
        print(f"RUN OK {tag0} ({time.time() - t0:.1f} s)", flush=True)
    finally:
        h.close()
    return worst


def check_batch(run, worst=None):
    """One run of tc.BATCH_RUNS."""
    from flowcontrol_amd._lib import FC_ERR_DIVERGED, FcError

    worst = worst or Worst()
    mesh, k, n_act, variant, sens, first, steps, ref_col = run
    tag0 = tc.run_name(run)
    t0 = time.time()
    h = Handle(mesh, n_act, variant, sens, "default", 0, steps, k=k)
    hs = None
    try:
        dev, m = h.dev, h.model
        KB = tc.kb_of(k)
        u = 0.1 * np.random.default_rng(4).standard_normal((steps, k, n_act))
        states = [np.stack(c) for c in zip(*(sc.initial_state(h.th, 1 + s) for s in range(k)))]
        if k >= 3:
            u[:, k - 2] = u[:, 0]
            for a in states:
                a[k - 2] = a[0]
        du, d0, dm1 = tc.inputs(m.N, n_act, steps, 9, k=k)
        ref = None if ref_col < 0 else ref_col

        def march(n, dx0=d0):
            dev.set_state_batch(*states)
            dev.adjoint_tape_begin_batch()
            for j in range(n):
                dev.step_batch(h.slot_of[tc.order_of(j + 1, first)], u[j], compute_energy=False)
            X = dev.adjoint_tape_states_batch()
            out = dev.run_tangent_batch(h.slot_of[first], n, du[:n], dx0, dm1, ref_col=ref)
            return X, out, dev.tangent_stage(), dev.tangent_route()

        prev = kept = None
        for n, order, want in tc.walk_batch(run):
            X, (dy, dxn, dxnm1), st, got = march(n)
            assert np.array_equal(got, want), f"route not taken: {tag0} n = {n}: predicted {dict(zip(tc.ROUTE_COLS, want.tolist()))}, reported {dict(zip(tc.ROUTE_COLS, got.tolist()))}"
            if n == 1:
                X2, out2, st2, _ = march(n)
                assert np.array_equal(X, X2) and all(np.array_equal(a, c) for a, c in zip((dy, dxn, dxnm1), out2)) and same_stage(st, st2), f"{tag0}: two identical batched marches differ"
            D1 = d0 if n == 1 else prev[0]
            D2 = dm1 if n == 1 else d0 if n == 2 else prev[1]
            assert not st["refined"] and not st["flags"].any() and st["dy"].shape == (k, len(m.rows)) and dy.shape == (n, k, len(m.rows))
            check_operands(h, order, st, worst, tag0)
            for s in range(k):
                t = s if ref is None else ref
                check_step(h, order, D1[s], D2[s], X[n, t], X[n - 1, t], du[n - 1, s], st, dy[n - 1, s], worst, f"{tag0} n = {n} column {s}", col=s,
                           own=None if ref is None else (X[n, s], X[n - 1, s]))
            assert np.array_equal(dxn, h.to_w(st["new"]).T[:k]) and np.array_equal(dxnm1, h.to_w(st["other"]).T[:k]), f"{tag0} n = {n}: the returned levels are not the device's"
            # padding columns: computed like the others from zero inputs -- exactly zero everywhere; dy has no row for them
            for q in ("ev", "b", "x", "new", "other"):
                assert not st[q][..., k:].any(), f"{tag0} n = {n}: padding columns of {q} are not zero"
            assert not st["du"][k:].any(), f"{tag0} n = {n}: padding rows of du are not zero"
            if k >= 3:  # equal columns are bit-equal; the column without inputs is zero
                for q in ("ev", "b", "x", "new"):
                    assert np.array_equal(st[q][..., 0], st[q][..., k - 2]), f"{tag0} n = {n}: equal columns differ in {q}"
                assert np.array_equal(dy[:, 0], dy[:, k - 2])
            assert not st["x"][:, k - 1].any() and not dy[:, k - 1].any(), f"{tag0} n = {n}: the zero column is not zero"
            prev, kept = (dxn, dxnm1), (dy, dxn, dxnm1)
            if n == 1 and ref is None:
                hs = hs or Handle(mesh, n_act, variant, sens, "default", 0, 1)
                report_single_against_batched(h, hs, run, st, u, states, du, d0, dm1)
        # a NaN entry in one column's dx0: FC_ERR_DIVERGED, that column's flag alone, the other columns keep their bits
        if k >= 2:
            bad = d0.copy()
            bad[1, int(np.flatnonzero(m.free)[m.N // 3])] = np.nan
            try:
                march(steps, bad)
            except FcError as e:
                assert e.code == FC_ERR_DIVERGED, str(e)
            else:
                raise AssertionError(f"{tag0}: a NaN in a column's dx0 was not flagged")
            flags = np.asarray(dev.tangent_batch_flags)
            assert flags.tolist() == [int(s == 1) for s in range(k)], f"{tag0}: flags {flags.tolist()}"
            others = [s for s in range(k) if s != 1]
            assert all(np.array_equal(a[..., others, :], c[..., others, :]) for a, c in zip(dev.tangent_batch_last, kept)), f"{tag0}: a NaN column moved the others"
        print(f"RUN OK {tag0} ({time.time() - t0:.1f} s)", flush=True)
    finally:
        h.close()
        if hs is not None:
            hs.close()
    return worst


def report_single_against_batched(h, hs, run, st, u, states, du, d0, dm1):
    """Said, not asserted: the first step of column 0 through the single march's element kernel on a handle without a batch -- the same
    inputs bit for bit (the initial states, dx0, dxm1) -- against the batched kernel's column, in ulps of the element vectors."""
    first = run[5]
    d1 = hs.dev
    d1.set_state(*(a[0] for a in states))
    d1.adjoint_tape_begin()
    d1.run(hs.slot_of[first], 1, u[:1, 0], compute_energy=False)
    d1.run_tangent(hs.slot_of[first], 1, du[:1, 0], d0[0], dm1[0])
    ev1 = d1.tangent_stage()["ev"]
    print(f"ELEM FORMS {tc.run_name(run)}: fc_tan_elem_nl against fc_tan_elem_nl_b<{tc.kb_of(run[1])}> on column 0, first step: largest difference "
          f"{ulps(ev1, st['ev'][..., 0]):.1f} ulp", flush=True)


def check_tail_reads_dx(worst=None):
    """fc_tan_tail on a correction that is no rounding effect: the BDF2 operator replaced behind its factors, one refinement sweep.  The
    new level is x + dx bit for bit, dy = C (x + dx) within its bound, and sensors read from x alone would miss it by at least 1000 x
    that bound (the seeded mistake, on the device's own x and dx)."""
    worst = worst or Worst()
    h = Handle("12x7", 5, "mixed", "five", "default", 1, 1, lagged=True)
    try:
        dev, m = h.dev, h.model
        du, d0, dm1 = tc.inputs(m.N, 5, 1, 7)
        dev.set_state(*sc.initial_state(h.th, 1))
        dev.adjoint_tape_begin()
        dev.run(h.slot_of[2], 1, 0.1 * np.ones((1, 5)), compute_energy=False)
        dy, dxn, _ = dev.run_tangent(h.slot_of[2], 1, du, d0, dm1)
        st = dev.tangent_stage()
        assert st["refined"] and st["dx"] is not None and np.all(np.isfinite(st["x"])) and np.all(np.isfinite(st["dx"]))
        x, dx = h.to_w(st["x"]), h.to_w(st["dx"])
        lev, ref, bound = m.tail(x, dx)
        assert np.array_equal(h.to_w(st["new"]), lev) and np.array_equal(dxn, lev), "the new level is not x + dx, bit for bit"
        ry = _ratio(np.asarray(dy[0], dtype=L) - ref, bound)
        assert worst.see("dy, lagged operator", ry, 1.0) <= 1, f"dy misses C (x + dx) by {ry:.3f} x its bound"
        miss = np.abs(m.tail(x, dx, wrong="no_dx")[1] - ref) / bound
        print(f"TAIL lagged operator: |dx| / |x| = {np.linalg.norm(dx) / np.linalg.norm(x):.1e}, dy {ry:.3f} x bound; sensors read from x alone would miss by "
              f"{float(miss.min()):.2e} .. {float(miss.max()):.2e} x the bound", flush=True)
        assert miss.min() >= 1000
    finally:
        h.close()
    return worst


def report_elem_pairs() -> None:
    """Said, not asserted (the assertion is the ev tolerance): the eight-lane and the thread-per-cell element kernel on the same
    inputs, the first step of the single runs that differ in the handle knob set only, in ulps."""
    for run in tc.SINGLE_RUNS:
        if run[4] != "default":
            continue
        twin = tc.run_name(run[:4] + ("reg",) + run[5:])
        if tc.run_name(run) in RECORDS and twin in RECORDS:
            print(f"ELEM FORMS {tc.run_name(run)}: fc_tan_elem_nl against fc_tan_elem_nl_reg, first step: largest difference "
                  f"{ulps(RECORDS[tc.run_name(run)], RECORDS[twin]):.1f} ulp", flush=True)


def main(which: str) -> None:
    from tests.test_tangent_march_gpu import TOLERANCES

    TOL.update(TOLERANCES)
    worst, failed = Worst(), []
    todo = [(check_single, r) for r in tc.SINGLE_RUNS if which in ("single", "all")] + [(check_batch, r) for r in tc.BATCH_RUNS if which in ("batch", "all")]
    for fn, run in todo:
        try:
            fn(run, worst)
        except AssertionError as e:  # (a failed comparison: the next run starts on a fresh handle; anything else ends the process)
            failed.append(tc.run_name(run))
            print(f"RUN FAILED {tc.run_name(run)}: {e}", flush=True)
    if which == "all":
        check_tail_reads_dx(worst)
    worst.report()
    report_elem_pairs()
    if failed:
        raise SystemExit(f"{len(failed)} of {len(todo)} runs failed: {failed}")
    print("CHILD OK", which, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
