"""Device side of tests/test_adjoint_energy_gpu.py: the energy term of the adjoint marches' cost (fc_set_adjoint_energy) on the device,
against tests/support/adjoint_energy_cases.py.  As a program

    python adjoint_energy_child.py step <route> <lin|nl> | e2e <single|batch|loop|loopb> <lin|nl> | optin | refusals | partitioned | cost
                                   | solver <single|batched> <lin|nl>

runs one check in a fresh process (the handle knob FC_ELEM_REG_MIN is read when a handle is made) and ends with ``CHILD OK ..``.  The
handles are adjoint_march_child.Handle's: the small squares of adjoint_march_cases.MESHES with two Dirichlet actuators and five sensors."""
import sys

import numpy as np

from tests.support import adjoint_energy_cases as ec
from tests.support import adjoint_loop_batch_cases as lbc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_march_cases as mc
from tests.support import adjoint_march_child as child
from tests.support import step_cases as sc

L = np.longdouble
N_ACT, SENS = 2, "five"
# the device may miss a host constant by 16 times: the bound tests/test_adjoint_march_gpu.py uses for b, fed with the constant measured
# for the three-operand right-hand side
TOL_RHS = (16 * ec.HOST_ADJ_EN_RHS_ERROR[0], 16 * ec.HOST_ADJ_EN_RHS_ERROR[1])
TOL_SINGLE = 1e-8  # a batched column against the single march of that run: tests/test_adjoint_batch_gpu.py, test_adjoint_loop_batch_gpu.py
# route -> (mesh, handle set, k)
ROUTES = {"lanes": ("9x9", "default", 0), "reg": ("9x9", "reg", 0), "b4": ("5x3", "default", 3), "b16": ("12x7", "default", 9), "b32": ("9x9", "default", 32)}


def handle(mesh, hs, nl, k=0):
    h = child.Handle(mesh, N_ACT, "dirichlet", SENS, hs, nl, 0, k=k)
    h.model.__class__ = ec.EnergyMarchModel
    return h


def states(th, k):
    """Initial states of k columns, (k, .) each; column s from seed 1 + s."""
    return [np.stack(c) for c in zip(*(sc.initial_state(th, 1 + s) for s in range(k)))]


# ── 1. one backward step per route ─────────────────────────────────────────────────────────────────────────────────────────────────
def check_b(h, b_w, z1, z2, w, x_taped, e, x, coeffs, tag):
    """One right-hand side (W numbering) against the longdouble model fed the device's own two masked levels and taped state.  Both
    levels are live but in the column of a batch whose sensor weights are all zero (adjoint_march_cases.inputs): there mu_3 = 0, and
    only e_2 x_2 has fed mu_2."""
    m = h.model
    nn2 = 2 * m.nn
    zero = np.zeros(m.N)
    assert coeffs[0] != 0 and coeffs[1] != 0 and np.any(z1) and (np.any(z2) or not np.any(w)), "both levels must be live in this step"
    ref = m.rhs(z1, z2, coeffs, w, None, x_taped, e=e, x_state=x)
    e2, ei = mc.rel2(b_w[:nn2], ref[:nn2]), mc.relmax(b_w[:nn2], ref[:nn2])
    print(f"{tag}: b {e2:.2e} / {ei:.2e} of {TOL_RHS[0]:.2e} / {TOL_RHS[1]:.2e} allowed", flush=True)
    assert e2 <= TOL_RHS[0] and ei <= TOL_RHS[1], f"{tag}: b misses the longdouble right-hand side by {e2:.3e} / {ei:.3e}"
    _, mag, cnt = m.ct_part(w)
    rc = child._ratio((b_w - ref)[nn2:], ((cnt + 2) * sc.EPS * mag)[nn2:])
    assert rc <= 1, f"{tag}: the rows of C^T w alone miss by {rc:.3f} x their bound"
    # the inputs tell the mistakes apart: a device that made one would miss by far more than the bound
    if np.any(z2):
        miss = mc.rel2(m.rhs(z1, zero, coeffs, w, None, x_taped, e=e, x_state=x)[:nn2], ref[:nn2])
        assert miss >= 1e6 * TOL_RHS[0], (tag, "cm_nn z2 left out", miss)
    if e != 0.0:
        for wrong in ("no_energy", "x_masked"):
            miss = mc.rel2(m.rhs(z1, z2, coeffs, w, None, x_taped, wrong=wrong, e=e, x_state=x)[:nn2], ref[:nn2])
            assert miss >= 1e6 * TOL_RHS[0], (tag, wrong, miss)


def run_step(route, kind):
    """Backward step m = 1 of a three-step march: both masked levels are live (cm_n mu_2 + cm_nn mu_3) next to e_1 x_1.  The stage shows
    mu_2's masked copy; mu_3's is that of the march's first backward step run as a one-step march of its own on the BDF2 slot, as
    adjoint_march_child does it -- without weights, because the row of that step is zero here and adds nothing to its right-hand side."""
    mesh, hs, k = ROUTES[route]
    nl = kind == "nl"
    n, first = 3, 1
    rows = [0, 2, 1]  # weights(): row 1 is the zero row -- here it weights dE_3, rows 0 and 1 (dE_1, dE_2) are live
    h = handle(mesh, hs, nl, k)
    try:
        dev, m = h.dev, h.model
        ns = len(m.rows)
        rng = np.random.default_rng(3)
        c = mc.step_coeffs(1, n, nl)
        assert c[0] != 0 and c[1] != 0
        want = ec.route_with_energy(mc.predicted_route(mesh, N_ACT, ns, mc.HANDLE_SETS[hs], nl, True, False, k=k, tape=1))
        if not k:
            u = 0.1 * rng.standard_normal((n, N_ACT))
            w, _ = mc.inputs(m.N, ns, n, 7)
            e = ec.weights(n)[rows]
            assert e[0] != 0 and e[1] != 0 and e[2] == 0
            dev.adjoint_tape_reserve(n)
            dev.set_state(*sc.initial_state(h.th, 1))
            dev.adjoint_tape_begin()
            dev.run(h.slot_of[2], 1, u[:1], compute_energy=False)  # (a nonlinear handle marches over a tape; this step's c is zero)
            dev.run_adjoint(h.slot_of[2], 1, w[n - 1: n], None, state_gradients=False)
            z2 = h.to_w(dev.adjoint_stage()["zm"])
            dev.set_state(*sc.initial_state(h.th, 1))
            dev.adjoint_tape_begin()
            dev.run(h.slot_of[first], n, u, compute_energy=False)
            X = dev.adjoint_tape_states()
            assert np.any(X[2][m.dofs]), "the taped state has no Dirichlet values: the mask on x would not show"
            dev.set_adjoint_energy(e)
            info = dev.adjoint_energy_info()
            assert info["n_steps"] == n and info["k"] == 0 and info["bytes"] == 8 * n and info["KB"] == 0, info
            dev.run_adjoint(h.slot_of[first], n, w, None, state_gradients=False)
            st, got = dev.adjoint_stage(), dev.adjoint_route()
            assert np.array_equal(got, want), f"route not taken: predicted {want.tolist()}, reported {got.tolist()}"
            assert dev.adjoint_energy_info()["steps"] == n
            check_b(h, h.to_w(st["b"]), h.to_w(st["zm_prev"]), z2, w[0], X[2] if nl else None, float(e[0]), X[2], c, f"{route} {kind}")
            # the state gradients carry no energy term and leave the last step's route alone; the step count stays the march's
            dev.run_adjoint(h.slot_of[first], n, w, None, state_gradients=True)
            assert np.array_equal(dev.adjoint_route(), want) and dev.adjoint_energy_info()["steps"] == n
        else:
            KB = mc.kb_of(k)
            u = 0.1 * rng.standard_normal((n, k, N_ACT))
            w, _ = mc.inputs(m.N, ns, n, 9, k=k)
            e = ec.weights(n, k)[rows]
            assert np.all(e[:2] != 0) and not e[2].any()
            dev.adjoint_tape_reserve_batch(n)
            dev.set_state_batch(*states(h.th, k))
            dev.adjoint_tape_begin_batch()
            dev.step_batch(h.slot_of[2], u[0], compute_energy=False)
            dev.run_adjoint_batch(h.slot_of[2], 1, w[n - 1: n], None, state_gradients=False)
            z2w = h.to_w(dev.adjoint_stage()["zm"])
            dev.set_state_batch(*states(h.th, k))
            dev.adjoint_tape_begin_batch()
            for j in range(n):
                dev.step_batch(h.slot_of[first if j == 0 else 2], u[j], compute_energy=False)
            X = dev.adjoint_tape_states_batch()
            dev.set_adjoint_energy(e)
            info = dev.adjoint_energy_info()
            assert info["n_steps"] == n and info["k"] == k and info["KB"] == KB and info["bytes"] == 8 * n * KB, info
            dev.run_adjoint_batch(h.slot_of[first], n, w, None, state_gradients=False)
            st, got = dev.adjoint_stage(), dev.adjoint_route()
            assert np.array_equal(got, want), f"route not taken: predicted {want.tolist()}, reported {got.tolist()}"
            assert dev.adjoint_energy_info()["steps"] == n
            assert not st["b"][:, k:].any(), "padding columns of b are not zero"
            bw, zw = h.to_w(st["b"]), h.to_w(st["zm_prev"])
            assert sum(bool(np.any(z2w[:, s])) for s in range(k)) >= k - 1, "the older level is live in every column but the one without sensor weights"
            for s in range(k):
                check_b(h, np.ascontiguousarray(bw[:, s]), np.ascontiguousarray(zw[:, s]), np.ascontiguousarray(z2w[:, s]), w[0, s], X[2, s] if nl else None,
                        float(e[0, s]), X[2, s], c,
                        f"{route} {kind} column {s}")
    finally:
        h.close()


# ── 2. end to end ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────
N_E2E, K_E2E = 5, 3


def weights_qr(ns, na, seed=2):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((ns, ns))
    return 1e-3 * (A @ A.T) / ns, np.diag(0.5 + rng.random(na))


def quad(y, Q, u, R, axes=""):
    return 0.5 * (np.einsum(f"m{axes}i,ij,m{axes}j->{axes}", y, Q, y) + np.einsum(f"m{axes}i,ij,m{axes}j->{axes}", u, R, u))


def y_of(m, x):
    """The sensors' readings of a state (W numbering)."""
    return np.array([float(np.dot(wt, x[idx])) for idx, wt in m.rows])


def e2e_open(h, hs, nl, k):
    """(fc_run_adjoint | fc_run_adjoint_batch): J(u, x0) = 1/2 sum (y^T Q y + u^T R u) + sum e_m dE_m, the device's own y and dE."""
    dev, m, n = h.dev, h.model, N_E2E
    nn2, ns = 2 * m.nn, len(m.rows)
    Q, R = weights_qr(ns, N_ACT)
    rng = np.random.default_rng(12)
    kk = max(k, 1)
    u = 0.1 * rng.standard_normal((n, kk, N_ACT))
    st0 = states(h.th, kk)
    e = ec.weights(n, kk)
    assert np.count_nonzero(e[:, 0]) == n - 1 and len(set(e[:, 0].tolist())) == n
    du, d0 = rng.standard_normal(u.shape), rng.standard_normal((kk, nn2))

    def forward(dv, uu, s0, batched):
        if batched:
            dv.set_state_batch(*s0)
            dv.adjoint_tape_begin_batch()
            y, dE = np.empty((n, kk, ns)), np.empty((n, kk))
            for j in range(n):
                y[j], dE[j], _ = dv.step_batch(h.slot_of[1 if j == 0 else 2], uu[j], compute_energy=True)
            return y, dE
        dv.set_state(*(a[0] for a in s0))
        dv.adjoint_tape_begin()
        y, dE = dv.run(h.slot_of[1], n, uu[:, 0], compute_energy=True)
        return y[:, None], dE[:, None]

    def cost(dv, uu, s0, batched):
        y, dE = forward(dv, uu, s0, batched)
        return quad(y, Q, uu, R, "k") + np.einsum("mk,mk->k", e[:, : y.shape[1]], dE)

    def gradient(dv, uu, s0, batched, ee):
        y, dE = forward(dv, uu, s0, batched)
        dv.set_adjoint_energy(ee if batched else ee[:, 0])
        try:
            if batched:
                g, dx0, _ = dv.run_adjoint_batch(h.slot_of[1], n, y @ Q, None, True)
            else:
                g, dx0, _ = dv.run_adjoint(h.slot_of[1], n, y[:, 0] @ Q, None, True)
                g, dx0 = g[:, None], dx0[None]
        finally:
            dv.set_adjoint_energy(None)
        return g + uu @ R, dx0

    batched = k > 0
    (dev.adjoint_tape_reserve_batch if batched else dev.adjoint_tape_reserve)(n)
    g, dx0 = gradient(dev, u, st0, batched, e)
    g2, dx02 = gradient(dev, u, st0, batched, e)
    assert np.array_equal(g, g2) and np.array_equal(dx0, dx02), "two identical marches differ"
    hstep = ec.FD_STEP_OPEN
    moved = lambda s: (u + s * hstep * du, [st0[0] + s * hstep * d0, st0[1], st0[2]])  # noqa: E731
    fd = (cost(dev, *moved(1.0), batched) - cost(dev, *moved(-1.0), batched)) / (2 * hstep)
    gd = np.einsum("mki,mki->k", g, du) + np.einsum("ki,ki->k", dx0[:, :nn2], d0)
    tol = ec.fd_tol("nl" if nl else "lin", "open")  # the sibling tests' 1e-6 (larger than ten times the host-measured distance)
    for s in range(kk):
        err = abs(fd[s] - gd[s]) / abs(fd[s])
        print(f"open loop, column {s}: central differences {err:.2e} of {tol:.1e} allowed (difference quotient {fd[s]:.3e})", flush=True)
        assert err <= tol, (s, err)
    # without the weights the same march misses its own central differences with them: the test sees the term
    dev.set_adjoint_energy(None)
    y, _ = forward(dev, u, st0, batched)
    gp = (dev.run_adjoint_batch(h.slot_of[1], n, y @ Q, None, False)[0] if batched else dev.run_adjoint(h.slot_of[1], n, y[:, 0] @ Q, None, False)[0][:, None]) + u @ R
    share = lm.rel(gp, g)
    print(f"the march without the weights differs by {share:.2e} of the gradient", flush=True)
    assert share > 100 * tol
    if batched:  # every column against the single march of that run, on a handle without a batch
        hs.dev.adjoint_tape_reserve(n)
        for s in range(kk):
            gs, dxs = gradient(hs.dev, u[:, s: s + 1], [a[s: s + 1] for a in st0], False, e[:, s: s + 1])
            d = max(lm.rel(g[:, s], gs[:, 0]), lm.rel(dx0[s, :nn2], dxs[0, :nn2]))
            print(f"column {s} against the single march: {d:.2e}", flush=True)
            assert d <= TOL_SINGLE, (s, d)


def e2e_loop(h, hs, nl, k):
    """(fc_run_adjoint_closed_loop | _batch): J over every matrix of the bank, the feedback map and the controller's initial state."""
    dev, m, n = h.dev, h.model, N_E2E
    ns = len(m.rows)
    Q, R = weights_qr(ns, N_ACT)
    kk = max(k, 1)
    batched = k > 0
    st0 = states(h.th, kk)
    y0 = np.array([y_of(m, np.r_[st0[0][s], st0[2][s]]) for s in range(kk)])
    # (the plant answers a unit control with sensor readings of 1e3: a feedback map of 1e-3 keeps the loop gain below one, so that J
    # stays the low-order polynomial of the bank's entries that central differences at the sibling tests' step resolve)
    banks = [lm.random_bank(3, 2, 2, ns, N_ACT, seed=31 + s, gain=0.3) for s in range(kk)]
    for b in banks:
        b["G"] *= 1e-3
    e = ec.weights(n, kk)
    groups = lm.PARAMS + ("x0",)
    dirs = [{g: lc.fd_direction(g, b[g][0].shape, seed=s) for g in groups} for s, b in enumerate(banks)]
    for d in dirs:
        d["G"] *= 1e-3  # (the direction moves G by the size of G: a step of 2e-5 times O(1) would be 2 % of every entry)

    def stacked(bs):
        out = {"k": len(bs), "nx": 3, "nyc": 2, "nuc": 2, "sizes": [b["sizes"][0] for b in bs]}
        for key in lbc.BANK_KEYS:
            out[key] = np.concatenate([b[key] for b in bs])
        return out

    def forward(dv, bs, cols, as_batch):
        if as_batch:
            lbc.put_bank(dv, stacked(bs))
            dv.adjoint_loop_reserve_batch(n)
            dv.set_state_batch(*st0)
            dv.adjoint_tape_begin_batch()
            dv.adjoint_loop_begin_batch()
            y, u, dE, bad, _ = dv.run_closed_loop_batch(h.slot_of[1], n, y0, compute_energy=True)
            assert np.all(bad < 0)
            return y, u, dE
        s = cols[0]
        lc.put_bank(dv, bs[0])
        dv.adjoint_loop_reserve(n)
        dv.set_state(*(a[s] for a in st0))
        dv.adjoint_tape_begin()
        dv.adjoint_loop_begin()
        y, u, dE = dv.run_closed_loop(h.slot_of[1], n, y0[s], compute_energy=True)
        return y[:, None], u[:, None], dE[:, None]

    def cost(dv, bs, cols, as_batch):
        y, u, dE = forward(dv, bs, cols, as_batch)
        return quad(y, Q, u, R, "k") + np.einsum("mk,mk->k", e[:, cols], dE)

    def gradient(dv, bs, cols, as_batch, with_e=True):
        y, u, dE = forward(dv, bs, cols, as_batch)
        dv.set_adjoint_energy((e[:, cols] if as_batch else e[:, cols[0]]) if with_e else None)
        try:
            if as_batch:
                return dv.run_adjoint_closed_loop_batch(h.slot_of[1], n, y @ Q, u @ R, None, False)
            g = dv.run_adjoint_closed_loop(h.slot_of[1], n, y[:, 0] @ Q, u[:, 0] @ R, None, False)
            return {q: (None if v is None else v[None]) for q, v in g.items()}
        finally:
            dv.set_adjoint_energy(None)

    def moved(sign, hstep):
        out = []
        for b, d in zip(banks, dirs):
            q = lm.copy_bank(b)
            for grp in groups:
                q[grp][0] += sign * hstep * d[grp]
            out.append(q)
        return out

    cols = list(range(kk))
    (dev.adjoint_tape_reserve_batch if batched else dev.adjoint_tape_reserve)(n)
    g = gradient(dev, banks, cols, batched)
    print("closed-loop costs", cost(dev, banks, cols, batched).tolist(), flush=True)
    g2 = gradient(dev, banks, cols, batched)
    assert all(np.array_equal(g[q], g2[q]) for q in groups), "two identical marches differ"
    hstep = ec.FD_STEP_LOOP
    fd = (cost(dev, moved(1.0, hstep), cols, batched) - cost(dev, moved(-1.0, hstep), cols, batched)) / (2 * hstep)
    # the sibling tests' 1e-6; on the nonlinear plant ten times the host-measured distance, 4.6e-6, which is larger
    tol = ec.fd_tol("nl" if nl else "lin", "loop")
    for s in range(kk):
        gd = sum(float(np.sum(g[grp][s] * dirs[s][grp])) for grp in groups)
        err = abs(fd[s] - gd) / abs(fd[s])
        print(f"closed loop, column {s}: central differences {err:.2e} of {tol:.1e} allowed (difference quotient {fd[s]:.3e})", flush=True)
        assert err <= tol, (s, err)
    # without the weights the same march differs by far more than the bound: the test sees the term
    gp = gradient(dev, banks, cols, batched, with_e=False)
    share = min(lm.rel(gp["C"][s], g["C"][s]) for s in range(kk))
    print(f"the march without the weights differs by {share:.2e} of dJ/dC", flush=True)
    assert share > 100 * tol
    if batched:
        hs.dev.adjoint_tape_reserve(n)
        for s in range(kk):
            gs = gradient(hs.dev, [banks[s]], [s], False)
            d = max(lm.rel(g[grp][s], gs[grp][0]) for grp in groups)
            print(f"column {s} against the single march: {d:.2e}", flush=True)
            assert d <= TOL_SINGLE, (s, d)


def run_e2e(march, kind):
    nl = kind == "nl"
    k = K_E2E if march in ("batch", "loopb") else 0
    h = handle("9x9", "default", nl, k)
    hs = handle("9x9", "default", nl) if k else None
    try:
        (e2e_open if march in ("single", "batch") else e2e_loop)(h, hs, nl, k)
    finally:
        h.close()
        if hs is not None:
            hs.close()


# ── 3. opt-in ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def run_optin():
    n = 4
    for nl in (False, True):
        h = handle("9x9", "default", nl)
        try:
            dev, m = h.dev, h.model
            ns = len(m.rows)
            w, z = mc.inputs(m.N, ns, n, 7)
            u = 0.1 * np.random.default_rng(1).standard_normal((n, N_ACT))
            old = mc.predicted_route("9x9", N_ACT, ns, {}, nl, True, False, tape=1 if nl else -1)

            def march():
                out = dev.run_adjoint(h.slot_of[1], n, w, z, True)
                return out, dev.adjoint_route()

            def taped_forward():
                dev.set_state(*sc.initial_state(h.th, 1))
                dev.adjoint_tape_begin()
                return dev.run(h.slot_of[1], n, u, compute_energy=True)

            assert dev.adjoint_energy_info() == {"n_steps": 0, "k": 0, "bytes": 0, "steps": 0, "KB": 0}
            if nl:
                dev.adjoint_tape_reserve(n)
                taped_forward()
            before, route0 = march()  # a handle that never set weights
            assert np.array_equal(route0, old), (route0.tolist(), old.tolist())
            if not nl:
                dev.adjoint_tape_reserve(n)
                old[11] = 1
            fwd = taped_forward()
            state = [np.array(a, copy=True) for a in dev.get_state()]
            count = dev.adjoint_tape_info()["count"]
            dev.set_adjoint_energy(ec.weights(n))
            with_e, route1 = march()
            assert int(route1[0]) == ec.ENERGY_OF[int(old[0])] and not np.array_equal(with_e[0], before[0])
            assert dev.adjoint_energy_info()["bytes"] == 8 * n
            # the state, the tape's step count and the forward run that follows are what they were
            assert all(np.array_equal(a, b) for a, b in zip(state, dev.get_state())) and dev.adjoint_tape_info()["count"] == count
            dev.set_adjoint_energy(None)
            assert dev.adjoint_energy_info() == {"n_steps": 0, "k": 0, "bytes": 0, "steps": n, "KB": 0}
            after, route2 = march()
            assert np.array_equal(route2, old), (route2.tolist(), old.tolist())
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), "g differs after the weights were cleared"
            again = taped_forward()
            assert all(np.array_equal(a, b) for a, b in zip(fwd, again)), "the forward run moved"
            print(f"opt-in {'nonlinear' if nl else 'linearised'}: bit-identical before / after, routes {int(route0[0])} -> {int(route1[0])} -> {int(route2[0])}", flush=True)
        finally:
            h.close()


# ── 4. refusals ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def refused(fn, *args, code, match):
    from flowcontrol_amd._lib import FcError

    try:
        fn(*args)
    except FcError as err:
        assert err.code == code and match in str(err), str(err)
        return
    raise AssertionError(f"not refused: {match}")


def run_refusals():
    from flowcontrol_amd._lib import FC_ERR_INVALID, FC_ERR_NOT_READY

    n, k = 3, 3
    h = handle("5x3", "default", False)
    try:
        dev, m = h.dev, h.model
        s1 = h.slot_of[1]
        w = np.ones((n, len(m.rows)))
        dev.set_adjoint_energy(np.ones(n))
        # a linearised handle without a covering tape: none, not begun, another length
        refused(dev.run_adjoint, s1, n, w, code=FC_ERR_INVALID, match="the state tape does not hold this run: no tape is reserved")
        dev.adjoint_tape_reserve(n)
        refused(dev.run_adjoint, s1, n, w, code=FC_ERR_INVALID, match="the tape is not begun")
        dev.set_state(*sc.initial_state(h.th, 1))
        dev.adjoint_tape_begin()
        dev.run(s1, n - 1, np.zeros((n - 1, N_ACT)), compute_energy=False)
        refused(dev.run_adjoint, s1, n, w, code=FC_ERR_INVALID, match=f"the tape holds {n - 1} steps, the run has {n}")
        # rows with another n_steps or k
        refused(dev.run_adjoint, s1, n - 1, w[: n - 1], code=FC_ERR_INVALID, match=f"they have n_steps = {n} rows, the march has n_steps = {n - 1}")
        lc.put_bank(dev, lm.random_bank(3, 2, 2, len(m.rows), N_ACT))
        dev.adjoint_loop_reserve(n)
        dev.set_state(*sc.initial_state(h.th, 1))
        dev.adjoint_tape_begin()
        dev.adjoint_loop_begin()
        dev.run_closed_loop(s1, n - 1, np.zeros(len(m.rows)), compute_energy=False)
        refused(dev.run_adjoint_closed_loop, s1, n - 1, w[: n - 1], code=FC_ERR_INVALID, match=f"they have n_steps = {n} rows")
        dev.set_controllers(None, mc.DT)
        refused(dev.set_adjoint_energy, np.ones((n, k)), code=FC_ERR_NOT_READY, match="fc_set_batch not called")  # rows of k columns, no batch
        assert dev.adjoint_energy_info()["n_steps"] == n  # (a refused call leaves the held rows alone)
        # fc_step_adjoint with rows held
        dev.adjoint_reset(None)
        refused(dev.step_adjoint, s1, 0.0, 0.0, None, code=FC_ERR_INVALID, match="a single backward step carries no state")
        dev.set_adjoint_energy(None)
        dev.step_adjoint(s1, 0.0, 0.0, None)  # (cleared: the step runs)
        refused(dev.set_adjoint_energy, np.array([1.0, np.nan]), code=FC_ERR_INVALID, match="non-finite weight")
    finally:
        h.close()
    hb = handle("5x3", "default", False, k)
    try:
        dev = hb.dev
        s1 = hb.slot_of[1]
        wb = np.ones((n, k, len(hb.model.rows)))
        refused(dev.set_adjoint_energy, np.ones((n, k + 1)), code=FC_ERR_INVALID, match="k differs from fc_set_batch")
        dev.set_adjoint_energy(np.ones(n))  # rows of a single march on a handle with a batch: the batched march refuses them
        refused(dev.run_adjoint_batch, s1, n, wb, code=FC_ERR_INVALID, match="rows of a single march (k = 0), this march is batched")
        dev.set_adjoint_energy(np.ones((n, k)))
        refused(dev.run_adjoint_batch, s1, n, wb, code=FC_ERR_INVALID, match="the batched state tape does not hold this run: no tape is reserved")
        refused(dev.run_adjoint_batch, s1, n - 1, wb[: n - 1], code=FC_ERR_INVALID, match=f"they have n_steps = {n} rows, the march has n_steps = {n - 1}")
        dev.set_adjoint_energy(None)
        dev.run_adjoint_batch(s1, n, wb, None, False)  # (cleared: the linearised march needs no tape again)
    finally:
        hb.close()
    print("refusals: every message as stated", flush=True)


def run_partitioned():
    """A partitioned handle refuses the rows (one rank of a world of two, host exchange: no second process is needed to ask)."""
    from flowcontrol_amd import _lib
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    dev = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
    try:
        fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
        _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
        refused(dev.set_adjoint_energy, np.ones(3), code=_lib.FC_ERR_INVALID, match="partitioned handles are not supported")
        assert dev.adjoint_energy_info()["bytes"] == 0
    finally:
        dev.close()


# ── 5. the cost helper ─────────────────────────────────────────────────────────────────────────────────────────────────────────────
def square_flowsolver(nx=9, ny=9, nonlinear=False):
    """A FlowSolver on the nx x ny unit square: the lid-driven cavity's boundaries, sensors and lid actuator on a mesh written for
    this run, linearised about the fluid at rest (a base flow the test needs no Newton solve for)."""
    import tempfile
    from pathlib import Path

    from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    tmp = Path(tempfile.mkdtemp())
    mesh = Mesh.unit_square(nx, ny)
    np.savez(tmp / "square.npz", coords=mesh.coords, cells=mesh.cells)
    fs = LidCavityFlowSolver.make_default(Re=100, path_out=tmp, num_steps=20, meshpath=tmp / "square.npz")
    fs.params_solver.is_eq_nonlinear = bool(nonlinear)
    fs.params_ic = ParamIC(xloc=0.5, yloc=0.5, radius=0.2, amplitude=1.0)
    U0, P0 = Function(fs.W, np.zeros(fs.th.N)).split()
    fs._assign_steady_state(U0, P0)
    return fs


def run_cost():
    """optim.closed_loop_cost_gradients(signal="dE") on the 9x9 square with two candidates against closed_loop_costs(on_device=True):
    both are sums of the same device series, so 1e-12 relative."""
    from flowcontrol_amd import optim

    fs = square_flowsolver(9, 9)
    try:
        assert fs.th.mesh.cells.shape[0] == 162
        candidates = lambda: small_controllers(2)  # noqa: E731

        n = 6
        for criterion in ("integral", "terminal"):
            Jc, series = optim.closed_loop_costs(fs, candidates(), n, u_penalty=0.3, signal="dE", criterion=criterion, on_device=True)
            J, grads = optim.closed_loop_cost_gradients(fs, candidates(), n, signal="dE", criterion=criterion, u_penalty=0.3)
            assert np.all(np.isfinite(Jc)) and np.all(Jc > 0) and series[0]["dE"].iloc[0] > 0
            d = np.abs(J - Jc) / np.abs(Jc)
            print(f"cost helper, {criterion}: J {J.tolist()} against closed_loop_costs {Jc.tolist()}: {d.max():.2e}", flush=True)
            assert np.all(d <= 1e-12), d
            assert len(grads) == 2 and all(np.any(g["C"]) and np.any(g["A"]) for g in grads)
    finally:
        fs.th.release_device()


# ── 6. the solver level: energy= on FlowSolver / BatchedFlowSolver and the flu functions ────────────────────────────────────────────────
def small_controllers(count, seed=8):
    from flowcontrol_amd.controller import Controller

    r = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        A = r.standard_normal((3, 3))
        A = A - (np.abs(np.linalg.eigvals(A).real).max() + 1.0) * np.eye(3)
        out.append(Controller(A, r.standard_normal((3, 1)), 0.3 * r.standard_normal((1, 3)), 0.1 * r.standard_normal((1, 1)), x0=0.2 * r.standard_normal(3)))
    return out


def copies(arrays):
    return [np.array(a, copy=True) for a in arrays]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, (list, tuple)) else np.array_equal(a, b)


def same_grads(g, h):
    return set(g) == set(h) and all(np.array_equal(g[q], h[q]) for q in g)


def cut_like(full, part):
    """The leading block of a bank-sized device array that a gradient cut to its controller's own size covers."""
    return full[tuple(slice(0, s) for s in part.shape)]


# Bounds of this section.  J against the device's own forward cost: the sibling tests' 1e-12 (the same device series, summed twice on
# the host).  The gradients against the device-level march: the solver-level functions make the same launches on the same inputs as the
# device-level calls the test makes itself, and two identical marches are bit-identical (section 2), so they are compared bit for bit;
# the device-level marches are the ones section 2 holds against central differences of the device's cost.
TOL_J = 1e-12


def run_solver_single(kind):
    """FlowSolver.cost_gradient / closed_loop_gradient, flu.quadratic_cost_gradient / closed_loop_gradient, AdjointRun.run /
    run_closed_loop_adjoint with energy=, on the 9 x 9 cavity after two steps of its own (a counter and a log to leave alone)."""
    import flowcontrol_amd.utils as flu
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
    from flowcontrol_amd.examples.cylinder.optimize_controller_gradient import descend

    nl = kind == "nl"
    fs = square_flowsolver(9, 9, nonlinear=nl)
    try:
        fs.initialize_time_stepping(ic=None)
        na = fs.params_control.actuator_number
        for j in range(2):
            fs.step(0.05 * (j + 1) * np.ones(na))
        fs._begin_stepping()
        dev = fs.th.device()
        assert bool(fs.params_solver.is_eq_nonlinear) == nl and fs.iter == 2 and fs.order == 2
        n, ns, dt = N_E2E, dev.n_sens, fs.params_time.dt
        slot, order = (SLOT_BDF1, 1) if fs.order == 1 else (SLOT_BDF2, 2)
        rng = np.random.default_rng(5)
        u = 0.1 * rng.standard_normal((n, na))
        Q, R = np.diag(1.0 + np.arange(ns)), 0.1 * np.eye(na)
        e = ec.weights(n)
        K = small_controllers(1)[0]
        xc0 = K.x.copy()

        def snapshot():
            return {"state": copies(dev.get_state()), "iter": fs.iter, "t": fs.t, "order": fs.order, "log": fs.timeseries.copy(), "y": np.array(fs.y_meas, copy=True)}

        def untouched(s0, what):
            s1 = snapshot()
            assert same(s0["state"], s1["state"]), f"{what}: the state moved"
            assert (s0["iter"], s0["t"], s0["order"]) == (s1["iter"], s1["t"], s1["order"]) and np.array_equal(s0["y"], s1["y"]), f"{what}: the counters moved"
            assert len(s1["log"]) == 3 and s0["log"].equals(s1["log"]), f"{what}: the log was written to"
            assert np.array_equal(K.x, xc0), f"{what}: the controller's state moved"
            assert dev.adjoint_energy_info()["bytes"] == 0 and dev.adjoint_energy_info()["n_steps"] == 0, f"{what}: weights are still held"
            assert dev.adjoint_tape_info()["bytes"] == 0 and dev.adjoint_loop_info()["bytes"] == 0, f"{what}: a tape is still reserved"

        s0 = snapshot()
        # energy=None is the call without the keyword, bit for bit
        J0, g0 = fs.cost_gradient(u, Q, R)
        Jn, gn = fs.cost_gradient(u, Q, R, energy=None)
        assert J0 == Jn and np.array_equal(g0, gn)
        Jc0, gc0 = fs.closed_loop_gradient(K, n, Q, R)
        Jcn, gcn = fs.closed_loop_gradient(K, n, Q, R, energy=None)
        assert Jc0 == Jcn and same_grads(gc0, gcn)
        untouched(s0, "energy=None")
        # open loop with weights: the method, the function, a scalar
        Je, ge = fs.cost_gradient(u, Q, R, energy=e)
        untouched(s0, "FlowSolver.cost_gradient(energy=)")
        Jf, gf = flu.quadratic_cost_gradient(fs, u, Q, R, energy=e)
        untouched(s0, "quadratic_cost_gradient(energy=)")
        assert Je == Jf and np.array_equal(ge, gf)
        Js, gs = fs.cost_gradient(u, Q, R, energy=2.5)
        Jv, gv = fs.cost_gradient(u, Q, R, energy=np.full(n, 2.5))
        assert Js == Jv and np.array_equal(gs, gv) and not np.array_equal(gs, ge)
        with flu.AdjointRun(fs, tape=n) as run:
            y, dE = run.forward(u, compute_energy=True)
            Jref = 0.5 * (np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", u, R, u)) + float(e @ dE)
            dev.set_adjoint_energy(e)
            try:
                gdev = dev.run_adjoint(slot, n, y @ Q, None, False)[0] + u @ R
                assert int(dev.adjoint_route()[0]) in (ec.ELEM_NL_EN if nl else ec.ELEM_EN, ec.ELEM_NL_REG_EN if nl else ec.ELEM_EN_REG)
            finally:
                dev.set_adjoint_energy(None)
            grun = run.run(n, w=y @ Q, first_order=order, state_gradients=False, energy=e)[0] + u @ R
            assert dev.adjoint_energy_info()["bytes"] == 0 and dev.adjoint_energy_info()["steps"] == n
            dev.set_state(*s0["state"])
        dJ = abs(Je - Jref) / abs(Jref)
        print(f"{kind} FlowSolver open loop: J {Je:.6e} against the device's forward cost {dJ:.2e} of {TOL_J:.0e}; energy share {abs(float(e @ dE)) / abs(Jref):.2e}; "
              f"gradient against the device-level march {lm.rel(ge, gdev):.2e}, against the march without weights {lm.rel(ge, g0):.2e}", flush=True)
        assert dJ <= TOL_J
        assert np.array_equal(grun, gdev), "AdjointRun.run(energy=) is not the march with the rows held"
        assert np.array_equal(ge, gdev), "FlowSolver.cost_gradient(energy=) is not the device-level march"
        assert lm.rel(ge, g0) > 100 * ec.FD_TOL and abs(Je - J0) > 100 * TOL_J * abs(J0), "the weights do not show"
        untouched(s0, "the device-level march")
        # closed loop with weights
        Jce, gce = fs.closed_loop_gradient(K, n, Q, R, energy=e)
        untouched(s0, "FlowSolver.closed_loop_gradient(energy=)")
        Jcf, gcf = flu.closed_loop_gradient(fs, K, n, Q, R, energy=e)
        untouched(s0, "closed_loop_gradient(energy=)")
        assert Jce == Jcf and same_grads(gce, gcf)
        with flu.AdjointRun(fs, tape=n, loop=n) as run:
            dev.set_controllers([K], dt)
            try:
                y, uc, dE = run.forward_closed_loop(n, np.array(fs.y_meas, dtype=float), compute_energy=True)
                Jref = 0.5 * (np.einsum("mi,ij,mj->", y, Q, y) + np.einsum("mi,ij,mj->", uc, R, uc)) + float(e @ dE)
                dev.set_adjoint_energy(e)
                try:
                    gdev = dev.run_adjoint_closed_loop(slot, n, y @ Q, uc @ R, None, False)
                finally:
                    dev.set_adjoint_energy(None)
                grun = run.run_closed_loop_adjoint(n, w=y @ Q, r=uc @ R, first_order=order, state_gradients=False, energy=e)
                assert dev.adjoint_energy_info()["bytes"] == 0
            finally:
                dev.set_state(*s0["state"])
                dev.set_controllers(None, dt)
        dJ = abs(Jce - Jref) / abs(Jref)
        print(f"{kind} FlowSolver closed loop: J {Jce:.6e} against the device's forward cost {dJ:.2e} of {TOL_J:.0e}; dJ/dC against the march without weights "
              f"{lm.rel(gce['C'], gc0['C']):.2e}", flush=True)
        assert dJ <= TOL_J
        for q in ("Ad", "Bd", "C", "D", "x0", "G", "g0", "y0"):
            assert np.array_equal(grun[q], gdev[q]), f"AdjointRun.run_closed_loop_adjoint(energy=): {q} is not the march with the rows held"
            assert np.array_equal(gce[q], cut_like(gdev[q], gce[q])), f"FlowSolver.closed_loop_gradient(energy=): {q} is not the device-level march"
        assert lm.rel(gce["C"], gc0["C"]) > 100 * ec.FD_TOL and abs(Jce - Jc0) > 100 * TOL_J * abs(Jc0), "the weights do not show"
        untouched(s0, "the device-level closed-loop march")
        # the descent example on the reference's J: the cost goes down and the solver is left as it was
        res = descend(fs, K, n_steps=n, n_iter=2, cost="energy")
        assert np.all(np.isfinite(res["J"])) and np.all(np.diff(res["J"]) <= 0) and res["J"][-1] < res["J"][0], res["J"]
        untouched(s0, "descend(cost='energy')")
    finally:
        fs.th.release_device()


def run_solver_batched(kind):
    """BatchedFlowSolver.cost_gradient / closed_loop_gradient, flu.batched_cost_gradient / batched_closed_loop_gradient, AdjointRun.run_batch
    / run_closed_loop_adjoint_batch with energy=, k = 3 runs of the 9 x 9 cavity after one batched step of their own."""
    import flowcontrol_amd.utils as flu
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
    from flowcontrol_amd.batch import BatchedFlowSolver
    from flowcontrol_amd.flowsolverparameters import ParamIC

    nl = kind == "nl"
    k = K_E2E
    fs = square_flowsolver(9, 9, nonlinear=nl)
    try:
        bfs = BatchedFlowSolver(fs, k)
        bfs.initialize_time_stepping(ics=[ParamIC(xloc=0.4 + 0.1 * s, yloc=0.5, radius=0.2, amplitude=1.0 - 0.1 * s) for s in range(k)])
        na = fs.params_control.actuator_number
        bfs.step(0.05 * np.ones((k, na)))
        dev = bfs.dev
        assert bool(fs.params_solver.is_eq_nonlinear) == nl and bfs.iter == 1 and bfs.order == 2
        n, ns, dt = N_E2E, dev.n_sens, fs.params_time.dt
        slot, order = (SLOT_BDF1, 1) if bfs.order == 1 else (SLOT_BDF2, 2)
        rng = np.random.default_rng(6)
        u = 0.1 * rng.standard_normal((n, k, na))
        Q, R = np.diag(1.0 + np.arange(ns)), 0.1 * np.eye(na)
        e = ec.weights(n, k)
        Ks = small_controllers(k)
        xc0 = [K.x.copy() for K in Ks]
        quad_k = lambda y, uu: 0.5 * (np.einsum("mki,ij,mkj->k", y, Q, y) + np.einsum("mki,ij,mkj->k", uu, R, uu))  # noqa: E731

        def snapshot():
            return {"state": copies(dev.get_state_batch()), "iter": bfs.iter, "t": bfs.t, "order": bfs.order, "log": [bfs.timeseries(i).copy() for i in range(k)],
                    "y": np.array(bfs.y_meas, copy=True), "bad": bfs.diverged.copy(), "dE0": bfs.initial_energy}

        def untouched(s0, what):
            s1 = snapshot()
            assert same(s0["state"], s1["state"]), f"{what}: the batched state moved"
            assert (s0["iter"], s0["t"], s0["order"]) == (s1["iter"], s1["t"], s1["order"]) and np.array_equal(s0["y"], s1["y"]), f"{what}: the counters moved"
            assert np.array_equal(s0["bad"], s1["bad"]) and np.array_equal(s0["dE0"], s1["dE0"])
            assert all(len(b) == 2 and a.equals(b) for a, b in zip(s0["log"], s1["log"])), f"{what}: the log was written to"
            assert all(np.array_equal(K.x, x) for K, x in zip(Ks, xc0)), f"{what}: a controller's state moved"
            assert dev.adjoint_energy_info()["bytes"] == 0 and dev.adjoint_energy_info()["n_steps"] == 0, f"{what}: weights are still held"
            assert dev.adjoint_tape_info_batch()["bytes"] == 0 and dev.adjoint_loop_info_batch()["bytes"] == 0, f"{what}: a tape is still reserved"

        s0 = snapshot()
        assert np.all(s0["dE0"] > 0) and np.array_equal(s0["dE0"], [bfs.timeseries(i)["dE"].iloc[0] for i in range(k)])
        J0, g0 = bfs.cost_gradient(u, Q, R)
        Jn, gn = bfs.cost_gradient(u, Q, R, energy=None)
        assert np.array_equal(J0, Jn) and np.array_equal(g0, gn)
        Jc0, gc0 = bfs.closed_loop_gradient(Ks, n, Q, R)
        Jcn, gcn = bfs.closed_loop_gradient(Ks, n, Q, R, energy=None)
        assert np.array_equal(Jc0, Jcn) and all(same_grads(a, b) for a, b in zip(gc0, gcn))
        untouched(s0, "energy=None")
        # open loop with weights: the method, the function, one row set for all columns
        Je, ge, dxe = bfs.cost_gradient(u, Q, R, state_gradient=True, energy=e)
        untouched(s0, "BatchedFlowSolver.cost_gradient(energy=)")
        Jf, gf, dxf = flu.batched_cost_gradient(bfs, u, Q, R, state_gradient=True, energy=e)
        untouched(s0, "batched_cost_gradient(energy=)")
        assert np.array_equal(Je, Jf) and np.array_equal(ge, gf) and np.array_equal(dxe, dxf)
        Js, gs = bfs.cost_gradient(u, Q, R, energy=e[:, 0])
        Jv, gv = bfs.cost_gradient(u, Q, R, energy=np.repeat(e[:, :1], k, axis=1))
        assert np.array_equal(Js, Jv) and np.array_equal(gs, gv) and np.array_equal(gs[:, 0], ge[:, 0]) and not np.array_equal(gs[:, 1], ge[:, 1])
        with flu.AdjointRun(bfs, tape=n) as run:
            y, dE = run.forward_batch(u, first_order=order, compute_energy=True)
            Jref = quad_k(y, u) + np.einsum("mk,mk->k", e, dE)
            dev.set_adjoint_energy(e)
            try:
                graw, dxdev, _ = dev.run_adjoint_batch(slot, n, y @ Q, None, True)
                assert int(dev.adjoint_route()[0]) == (ec.ELEM_NL_B_EN if nl else ec.ELEM_EN_B)
            finally:
                dev.set_adjoint_energy(None)
            grun, dxrun, _ = run.run_batch(n, w=y @ Q, first_order=order, state_gradients=True, energy=e)
            assert dev.adjoint_energy_info()["bytes"] == 0 and dev.adjoint_energy_info()["steps"] == n
            dev.set_state_batch(*s0["state"])
        gdev = graw + u @ R
        dJ = np.abs(Je - Jref) / np.abs(Jref)
        print(f"{kind} BatchedFlowSolver open loop: J {Je.tolist()} against the device's forward cost {dJ.max():.2e} of {TOL_J:.0e}; gradient against the "
              f"device-level march {lm.rel(ge, gdev):.2e}, against the march without weights {lm.rel(ge, g0):.2e}", flush=True)
        assert np.all(dJ <= TOL_J)
        assert np.array_equal(grun, graw) and np.array_equal(dxrun, dxdev), "AdjointRun.run_batch(energy=) is not the march with the rows held"
        assert np.array_equal(ge, gdev) and np.array_equal(dxe, dxdev), "BatchedFlowSolver.cost_gradient(energy=) is not the device-level march"
        assert lm.rel(ge, g0) > 100 * ec.FD_TOL and np.all(np.abs(Je - J0) > 100 * TOL_J * np.abs(J0)), "the weights do not show"
        untouched(s0, "the device-level batched march")
        # closed loops with weights
        Jce, gce = bfs.closed_loop_gradient(Ks, n, Q, R, energy=e)
        untouched(s0, "BatchedFlowSolver.closed_loop_gradient(energy=)")
        Jcf, gcf = flu.batched_closed_loop_gradient(bfs, Ks, n, Q, R, energy=e)
        untouched(s0, "batched_closed_loop_gradient(energy=)")
        assert np.array_equal(Jce, Jcf) and all(same_grads(a, b) for a, b in zip(gce, gcf))
        with flu.AdjointRun(bfs, tape=n, loop=n) as run:
            dev.set_controllers(Ks, dt)
            try:
                y, uc, dE, bad = run.forward_closed_loop_batch(n, np.array(bfs.y_meas, dtype=float), first_order=order, compute_energy=True)
                assert np.all(bad < 0)
                Jref = quad_k(y, uc) + np.einsum("mk,mk->k", e, dE)
                dev.set_adjoint_energy(e)
                try:
                    gdev = dev.run_adjoint_closed_loop_batch(slot, n, y @ Q, uc @ R, None, False)
                finally:
                    dev.set_adjoint_energy(None)
                grun = run.run_closed_loop_adjoint_batch(n, w=y @ Q, r=uc @ R, first_order=order, state_gradients=False, energy=e)
                assert dev.adjoint_energy_info()["bytes"] == 0
            finally:
                dev.set_state_batch(*s0["state"])
                dev.set_controllers(None, dt)
        dJ = np.abs(Jce - Jref) / np.abs(Jref)
        share = min(lm.rel(gce[s]["C"], gc0[s]["C"]) for s in range(k))
        print(f"{kind} BatchedFlowSolver closed loop: J {Jce.tolist()} against the device's forward cost {dJ.max():.2e} of {TOL_J:.0e}; dJ/dC against the march "
              f"without weights {share:.2e}", flush=True)
        assert np.all(dJ <= TOL_J)
        for q in ("Ad", "Bd", "C", "D", "x0", "G", "g0", "y0"):
            assert np.array_equal(grun[q], gdev[q]), f"AdjointRun.run_closed_loop_adjoint_batch(energy=): {q} is not the march with the rows held"
            for s in range(k):
                assert np.array_equal(gce[s][q], cut_like(gdev[q][s], gce[s][q])), f"BatchedFlowSolver.closed_loop_gradient(energy=): {q} of loop {s} is not the device-level march"
        assert share > 100 * ec.FD_TOL and np.all(np.abs(Jce - Jc0) > 100 * TOL_J * np.abs(Jc0)), "the weights do not show"
        untouched(s0, "the device-level batched closed-loop march")
        bfs.close()
    finally:
        fs.th.release_device()


def main(argv):
    mode = argv[0]
    if mode == "step":
        run_step(argv[1], argv[2])
    elif mode == "e2e":
        run_e2e(argv[1], argv[2])
    elif mode == "optin":
        run_optin()
    elif mode == "refusals":
        run_refusals()
    elif mode == "partitioned":
        run_partitioned()
    elif mode == "cost":
        run_cost()
    elif mode == "solver":
        (run_solver_single if argv[1] == "single" else run_solver_batched)(argv[2])
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    print("CHILD OK", " ".join(argv), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
