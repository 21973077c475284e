"""Host models of the device Krylov drivers, in float64 / complex128 numpy, written from the drivers' control flow:

    gmres_real      gmres_permuted      (fc_hip.hip; fc_multidot, fc_gmres_project, fc_gmres_givens, fc_gmres_combine, fc_gmres_begin)
    bicgstab_real   bicgstab_permuted   (fc_hip.hip; fc_dots2, fc_bicg_phase, fc_lin3_dev)
    gmres_complex   shifted_gmres       (fc_shifted_solver.hpp; fc_cmultidot, fc_cgs_update, fc_cgmres_givens via fc_cgivens.hpp)
    gmres_block     shifted_gmres_block (k runs of gmres_complex coupled by the lock-step budget alone)

A Krylov method with a slightly wrong projection, rotation or reduction still converges, only later; the models say WHEN the device
must stop and WHAT the iterate is at that moment.  The drivers solve the symmetrically permuted system, and a permutation changes no
inner product, so the models work in the caller's numbering.

Every model runs in two VARIANTS (``variants``) that differ only in what rounding may change: the order in which the inner products
are summed, and the column ordering of the preconditioner's LU.  The spread between the two is the model's own sensitivity to
rounding; a case is usable when that spread is far below the distance between the n-th iterate and the solution (the case tables
below and tests/test_krylov_model_host.py)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

#: the host looks at the device's state word every KRYLOV_CHECK iterations (kKrylovCheck, fc_hip.hip; kShiftedKrylovCheck,
#: fc_shifted_solver.hpp); tests/test_krylov_model_host.py reads both constants from the sources and compares
KRYLOV_CHECK = 4
#: restart length of gmres_permuted on a factor slot (fc_ctx::gmres_m)
GMRES_M = 30
#: restarts after a BiCGStab breakdown (kBicgRestarts)
BICG_RESTARTS = 8

OK, NOT_CONVERGED = 0, "not converged"


@dataclass
class Result:
    iters: int  # what the device reports (KS_ITERS; the sum of CG_USED)
    x: np.ndarray  # final iterate
    relres: float  # |b - A x| / |b| of that iterate
    code: object  # OK or NOT_CONVERGED
    history: list = field(default_factory=list)  # every residual norm the driver compared with rtol |b|, in the order of the tests (absolute)
    where: str = ""  # BiCGStab: "half" or "full"
    xmax: float = 0.0  # largest |x|_2 of the run
    iterates: list = field(default_factory=list)  # (x, recurrence residual) after every step, when asked for
    cycles: int = 0


class _Dots:
    """Inner products conj(a) . b, summed forwards or backwards."""

    def __init__(self, reverse):
        self.reverse = reverse

    def __call__(self, a, b):
        if self.reverse:
            return np.vdot(np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1]))
        return np.vdot(a, b)

    def multi(self, V, nv, w):
        return np.array([self(V[i], w) for i in range(nv)])


def variants(factored, trans="N", perm=None):
    """The two variants of a model run as keyword sets: (reverse, precond).  ``factored``: the matrix the device holds factors of;
    trans "H": the preconditioner is the inverse of its conjugate transpose (the shifted solver's adjoint mode)."""
    if perm is not None:
        # a mesh too large for SuperLU's own orderings: ONE LU of P A P^T in the caller's fill-reducing ordering serves both variants,
        # which then differ in the summation order alone
        perm = np.asarray(perm)
        lu = spla.splu(sp.csr_matrix(factored)[perm][:, perm].tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.01)

        def precond(v):
            x = np.empty_like(v)
            x[perm] = lu.solve(v[perm], trans)
            return x

        return [{"reverse": False, "precond": precond}, {"reverse": True, "precond": precond}]
    out = []
    for reverse, spec in ((False, "COLAMD"), (True, "MMD_AT_PLUS_A")):
        lu = spla.splu(sp.csc_matrix(factored), permc_spec=spec)
        out.append({"reverse": reverse, "precond": (lambda v, lu=lu: lu.solve(v, trans))})
    return out


# ── real GMRES ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def gmres_real(A, precond, b, rtol, max_iter, restart=GMRES_M, reverse=False):
    """gmres_permuted: right preconditioning, classical Gram-Schmidt twice (column h + h2), real Givens rotations, back substitution at
    convergence (state 3) or at the end of a cycle (state 4), x += M^-1 (V y); a cycle that converged by the estimate recomputes the
    true residual and begin_cycle(0) decides, with the stagnation rule; the result is accepted at relres <= 10 rtol."""
    dot = _Dots(reverse)
    N = b.size
    m = max(1, min(restart, max_iter))
    x = np.zeros(N)
    r = b.astype(float).copy()
    V = np.zeros((m + 1, N))
    H = np.zeros((m + 1, m))  # column j: H[:, j]
    cs, sn, g, y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
    res = Result(0, x, 0.0, OK)
    st = {"state": 0.0, "iters": 0, "bnorm2": 0.0, "rnorm2": 0.0, "used": 0}

    def begin_cycle(first):
        r2 = float(dot(r, r))
        if first:
            st["bnorm2"] = float(dot(b, b))
            st["iters"] = 0
        st["rnorm2"] = r2
        g[:] = 0.0
        g[0] = np.sqrt(r2)
        st["state"] = 1.0 if (np.sqrt(r2) <= rtol * np.sqrt(st["bnorm2"]) or not st["bnorm2"] > 0.0) else 0.0
        if st["state"] == 0.0:
            V[0] = r / np.sqrt(r2)

    def arnoldi(j):
        w = A @ precond(V[j])
        h1 = dot.multi(V, j + 1, w)
        for i in range(j + 1):
            w = w - h1[i] * V[i]
        h2 = dot.multi(V, j + 1, w)
        for i in range(j + 1):
            w = w - h2[i] * V[i]
        norm2 = float(dot(w, w))
        Hj = H[:, j]
        Hj[: j + 1] = h1 + h2
        Hj[j + 1] = np.sqrt(norm2)
        for i in range(j):
            a_, b_ = cs[i] * Hj[i] + sn[i] * Hj[i + 1], -sn[i] * Hj[i] + cs[i] * Hj[i + 1]
            Hj[i], Hj[i + 1] = a_, b_
        a_, b_ = Hj[j], Hj[j + 1]
        rr = np.hypot(a_, b_)
        if not rr > 0.0 or not np.isfinite(rr):
            st["state"] = -4.0
            return
        cs[j], sn[j] = a_ / rr, b_ / rr
        Hj[j], Hj[j + 1] = rr, 0.0
        g[j + 1] = -sn[j] * g[j]
        g[j] = cs[j] * g[j]
        st["iters"] += 1
        st["rnorm2"] = g[j + 1] * g[j + 1]
        st["used"] = j + 1
        res.history.append(abs(g[j + 1]))
        conv = abs(g[j + 1]) <= rtol * np.sqrt(st["bnorm2"])
        if conv or j + 1 == m:
            for i in range(j, -1, -1):
                s = g[i]
                for k in range(i + 1, j + 1):
                    s -= H[i, k] * y[k]
                y[i] = s / H[i, i]
            st["state"] = 3.0 if conv else 4.0
        else:
            V[j + 1] = w / np.sqrt(norm2)

    begin_cycle(1)
    res.history.append(float(np.sqrt(st["bnorm2"])))  # history[j]: the estimate after j rotation steps, whatever the cycle
    total, done, last_true = 0, False, -1.0
    failed_inside = False
    while not done:
        j = 0
        while j < m and total < max_iter:
            if st["state"] == 0.0:
                arnoldi(j)
            j += 1
            total += 1
            if (j % KRYLOV_CHECK == 0 or j == m or total == max_iter) and st["state"] != 0.0:
                break
        state = st["state"]
        if state < 0.0:
            return _finish_real(res, A, b, x, st["iters"], NOT_CONVERGED, dot)
        if state == 1.0:
            break
        if state == 0.0:  # iteration cap inside a cycle: the driver returns before it reads the count
            failed_inside = True
            break
        res.cycles += 1
        used = st["used"]
        x = x + precond(y[:used] @ V[:used])
        res.xmax = max(res.xmax, float(np.linalg.norm(x)))
        r = b - A @ x
        if state == 3.0 and total < max_iter:
            begin_cycle(0)
            if st["state"] == 1.0:
                done = True
            else:
                if last_true >= 0.0 and not st["rnorm2"] < 0.25 * last_true:
                    done = True
                last_true = st["rnorm2"]
        elif state == 3.0:
            done = True
        elif total >= max_iter:
            done = True
        else:
            begin_cycle(0)
    if failed_inside:
        return _finish_real(res, A, b, x, 0, NOT_CONVERGED, dot)
    out = _finish_real(res, A, b, x, st["iters"], OK, dot)
    if st["bnorm2"] > 0.0 and not out.relres <= 10.0 * rtol:
        out.code = NOT_CONVERGED
    return out


def _finish_real(res, A, b, x, iters, code, dot):
    bn = np.sqrt(float(dot(b, b)))
    r = b - A @ x
    res.iters, res.x, res.code = int(iters), x, code
    res.relres = float(np.sqrt(float(dot(r, r))) / bn) if bn > 0.0 else 0.0
    res.xmax = max(res.xmax, float(np.linalg.norm(x)))
    return res


# ── real BiCGStab ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def bicgstab_real(A, precond, b, rtol, max_iter, restart=None, reverse=False, keep_iterates=False):
    """bicgstab_permuted: the five phases of fc_bicg_phase between the vector updates of fc_lin3_dev (no-ops once the state is 1 or
    negative), convergence at the half step (state 2: the iteration is finished with omega = 0), the breakdown tests, and the restart
    from the true residual that the host starts when it meets a negative state at its check cadence."""
    dot = _Dots(reverse)
    N = b.size
    b = b.astype(float)
    x, p, v, s, t = (np.zeros(N) for _ in range(5))
    r, rh = b.copy(), b.copy()
    k = {"state": 0.0, "iters": 0, "bnorm2": 0.0, "rnorm2": 0.0, "rho": 0.0, "rho_old": 1.0, "alpha": 1.0, "omega": 1.0}
    cS, cX, cR, cP = [0.0] * 3, [0.0] * 3, [0.0] * 3, [1.0, 0.0, 0.0]
    res = Result(0, x, 0.0, OK)
    where = [""]

    def live():
        return not (k["state"] == 1.0 or k["state"] < 0.0)

    def lin3(c, v0, v1, v2, out):
        if not live():
            return out
        o = c[0] * v0 + c[1] * v1
        if v2 is not None:
            o = o + c[2] * v2
        return o

    def conv(d0):
        return np.sqrt(d0) <= rtol * np.sqrt(k["bnorm2"])

    # phase 0
    d0, d1 = float(dot(r, r)), float(dot(rh, r))
    k.update(bnorm2=d0, rnorm2=d0, rho=d1, state=0.0 if d0 > 0.0 else 1.0)
    res.history.append(np.sqrt(d0))
    restarts = 0
    for it in range(1, max_iter + 1):
        p = lin3(cP, r, p, v, p)
        ph = precond(p)
        v = A @ ph
        if live():  # phase 1
            d0 = float(dot(rh, v))
            if not np.isfinite(d0) or d0 == 0.0 or not np.isfinite(k["rho"]) or abs(k["rho"]) < 1e-300 * k["bnorm2"]:
                k["state"] = -1.0
            else:
                k["alpha"] = k["rho"] / d0
                cS[:] = [1.0, -k["alpha"], 0.0]
        s = lin3(cS, r, v, None, s)
        if live():  # phase 2
            d0 = float(dot(s, s))
            k["iters"] += 1
            res.history.append(np.sqrt(d0))
            if conv(d0):
                k["state"] = 2.0
        sh = precond(s)
        t = A @ sh
        if live():  # phase 3
            omega = 0.0
            if k["state"] != 2.0:
                d0, d1 = float(dot(t, s)), float(dot(t, t))
                if not np.isfinite(d1) or d1 == 0.0:
                    k["state"] = -2.0
                else:
                    omega = d0 / d1
            if live():
                k["omega"] = omega
                cX[:] = [1.0, k["alpha"], omega]
                cR[:] = [1.0, -omega, 0.0]
        x = lin3(cX, x, ph, sh, x)
        r = lin3(cR, s, t, None, r)
        if live():  # phase 4
            d0, d1 = float(dot(r, r)), float(dot(rh, r))
            k["rnorm2"] = d0
            if k["state"] == 2.0:
                k["state"], where[0] = 1.0, "half"
            else:
                res.history.append(np.sqrt(d0))
                if conv(d0):
                    k["state"], where[0] = 1.0, "full"
                elif k["omega"] == 0.0:
                    k["state"] = -3.0
                else:
                    k["rho_old"], k["rho"] = k["rho"], d1
                    beta = (d1 / k["rho_old"]) * (k["alpha"] / k["omega"])
                    cP[:] = [1.0, beta, -beta * k["omega"]]
            if keep_iterates:
                res.iterates.append((x.copy(), r.copy()))
            res.xmax = max(res.xmax, float(np.linalg.norm(x)))
        if it % KRYLOV_CHECK == 0 or it == max_iter:
            if k["state"] < 0.0 and restarts < BICG_RESTARTS and it < max_iter:
                restarts += 1
                r = b - A @ x
                rh = r.copy()
                d0, d1 = float(dot(r, r)), float(dot(rh, r))  # phase 5
                k.update(rnorm2=d0, rho=d1, rho_old=1.0, alpha=1.0, omega=1.0, state=1.0 if conv(d0) else 0.0)
                cP[:] = [1.0, 0.0, 0.0]
                continue
            if k["state"] != 0.0:
                break
    res.iters, res.x, res.where = k["iters"], x, where[0]
    bn = np.sqrt(k["bnorm2"])
    if k["state"] < 0.0:
        res.code = NOT_CONVERGED
    elif not bn > 0.0:
        res.relres = 0.0
    elif k["state"] != 1.0:
        res.relres, res.code = float(np.sqrt(k["rnorm2"]) / bn), NOT_CONVERGED
    else:
        tr = b - A @ x
        res.relres = float(np.sqrt(float(dot(tr, tr))) / bn)
    return res


# ── complex GMRES ────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _cgivens_column(j, col, cs, sn, g):
    """fc_cgivens_column: G_i = [[cs_i, sn_i], [-conj(sn_i), cs_i]]; returns |g[j + 1]| or -1."""
    for i in range(j):
        xx, yy, s, c = col[i], col[i + 1], sn[i], cs[i]
        col[i] = c * xx + s * yy
        col[i + 1] = c * yy - np.conj(s) * xx
    a, b = col[j], col[j + 1]
    na, nb = abs(a), abs(b)
    rr = np.hypot(na, nb)
    if not rr > 0.0 or not np.isfinite(rr):
        return -1.0
    ph = a / na if na > 0.0 else 1.0 + 0.0j
    cs[j] = na / rr
    sn[j] = ph * np.conj(b / rr) if na > 0.0 else 1.0 + 0.0j
    col[j] = ph * rr if na > 0.0 else b
    col[j + 1] = 0.0
    gj = g[j]
    g[j + 1] = -(gj * np.conj(sn[j]))
    g[j] = cs[j] * gj
    return abs(g[j + 1])


class _ComplexColumn:
    """One column of shifted_gmres / shifted_gmres_block, advanced cycle by cycle so that a block can cut the cycles of all its
    columns at the common budget."""

    def __init__(self, Mop, precond, b, rtol, m, reverse):
        self.M, self.P, self.b, self.rtol, self.m = Mop, precond, np.asarray(b, dtype=complex), rtol, m
        self.dot = _Dots(reverse)
        n = self.b.size
        self.x = np.zeros(n, dtype=complex)
        self.r = self.b.copy()
        self.r2 = float(self.dot(self.r, self.r).real)
        self.b2 = self.r2
        self.iters, self.state, self.history, self.xmax, self.cycles = 0, 0.0, [np.sqrt(self.b2)], 0.0, 0

    def begin(self):
        """fc_cgmres_begin: True when the column still runs"""
        self.state = 1.0 if (np.sqrt(self.r2) <= self.rtol * np.sqrt(self.b2) or not self.b2 > 0.0) else 0.0
        return self.state == 0.0

    def cycle(self, jend):
        """one cycle of at most jend columns (closed at jend); returns the columns used"""
        m, dot = self.m, self.dot
        n = self.b.size
        V = np.zeros((jend + 1, n), dtype=complex)
        R = np.zeros((m + 1, m), dtype=complex)
        cs, sn, g = np.zeros(m), np.zeros(m, dtype=complex), np.zeros(m + 1, dtype=complex)
        g[0] = np.sqrt(self.r2)
        V[0] = (1.0 / np.sqrt(self.r2)) * self.r
        used = 0
        for j in range(jend):
            w = self.M @ self.P(V[j])
            h1 = dot.multi(V, j + 1, w)
            for i in range(j + 1):
                w = w - h1[i] * V[i]
            h2 = dot.multi(V, j + 1, w)
            for i in range(j + 1):
                w = w - h2[i] * V[i]
            nsum = float(dot(w, w).real)
            col = np.zeros(j + 2, dtype=complex)
            col[: j + 1] = h1 + h2
            col[j + 1] = np.sqrt(max(nsum, 0.0))
            beta = col[j + 1].real
            est = _cgivens_column(j, col, cs, sn, g)
            if est < 0.0:
                self.state = -4.0
                return used
            conv = est <= self.rtol * np.sqrt(self.b2)
            used = j + 1
            self.history.append(est)
            R[: j + 1, j] = col[: j + 1]
            if conv or j + 1 == jend:
                self.state = 3.0 if conv else 4.0
                break
            V[j + 1] = (1.0 / beta) * w
        gg = g[:used].copy()
        y = np.zeros(used, dtype=complex)
        for i in range(used - 1, -1, -1):  # fc_cgivens_backsolve: column by column
            y[i] = gg[i] / R[i, i]
            gg[:i] -= R[:i, i] * y[i]
        self.x = self.x + self.P(y @ V[:used])
        self.xmax = max(self.xmax, float(np.linalg.norm(self.x)))
        self.r = self.b - self.M @ self.x
        self.r2 = float(self.dot(self.r, self.r).real)
        self.iters += used
        self.cycles += 1
        return used

    def result(self, code):
        rel = float(np.sqrt(self.r2 / self.b2)) if self.b2 > 0.0 else float(np.sqrt(self.r2))
        return Result(self.iters, self.x, rel, code, self.history, xmax=self.xmax, cycles=self.cycles)


def gmres_complex(Mop, precond, b, rtol, max_iter, restart, reverse=False):
    """shifted_gmres from a zero start: every cycle starts from the true residual, jend = min(restart, max_iter - iters), the last
    column of a cycle closes it, the count is the sum of the columns used.  ``Mop``: sigma E - A, or its conjugate transpose in the
    adjoint mode (with the preconditioner of ``variants(..., trans="H")``)."""
    c = _ComplexColumn(Mop, precond, b, rtol, restart, reverse)
    while True:
        if not c.begin():
            return c.result(OK)
        jend = min(restart, max_iter - c.iters)
        if jend <= 0:
            return c.result(NOT_CONVERGED)
        c.cycle(jend)
        if c.state <= 0.0:
            return c.result(NOT_CONVERGED)


def gmres_block(Mops, precond, B, rtol, max_iter, restart, reverse=False):
    """shifted_gmres_block: column c is gmres_complex on Mops[c], B[c]; the cycles of all columns are cut at
    jend = min(restart, max_iter - total), where total adds the LONGEST column of every cycle.  Returns (results, cycles, launched):
    launched counts the lock-step iterations the host enqueued -- it leaves a cycle early only at its check cadence."""
    cols = [_ComplexColumn(M, precond, b, rtol, restart, reverse) for M, b in zip(Mops, B)]
    total = cycles = launched = 0
    while True:
        running = [c for c in cols if c.state in (0.0, 3.0, 4.0) and c.begin()]
        jend = min(restart, max_iter - total)
        if not running or jend <= 0:
            break
        cycles += 1
        longest = max(c.cycle(jend) for c in running)
        if all(c.state < 0.0 for c in running):
            break
        stop = -(-longest // KRYLOV_CHECK) * KRYLOV_CHECK  # the first check at or after the last column stopped
        launched += stop if stop < jend else jend
        total += longest
    out = []
    for c in cols:
        r = c.result(OK)
        if r.relres > rtol:
            r.code = NOT_CONVERGED
        out.append(r)
    return out, cycles, launched


# ── cases ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
GAP = 1.4  # least ratio between the last residual norm that misses rtol |b| and the one that meets it
MARGIN = 100.0  # device iterate against the model's: this many spreads (the device sums in a third order, its factors are not splu's)
FLOOR = 1e-13  # ... and never less than this, relative


def rtol_for(history, k):
    """(rtol |b|, gap) that make the k-th test of a run the deciding one: the geometric mean of history[k] and the smallest norm any
    earlier test saw; gap = their ratio (a sharp prediction needs GAP)."""
    before = min(history[:k])
    return float(np.sqrt(before * history[k])), float(before / history[k])


def predicted_count(model, A, precond, b, rtol, max_iter):
    """(count, sharp) of ``model`` at a tolerance the caller fixed: sharp when the deciding residual norm lies at least sqrt(GAP)
    below rtol |b| and every earlier one at least sqrt(GAP) above -- the gap condition of the cases, seen from a given rtol.  Where it
    does not hold, rounding may decide the last iteration and a test can ask for the count to +-1 only."""
    r = model(A, precond, b, rtol, max_iter)
    h = np.asarray(r.history)
    tol = rtol * h[0]
    sharp = len(h) >= 2 and r.code == OK and tol / h[-1] >= np.sqrt(GAP) and h[:-1].min() / tol >= np.sqrt(GAP)
    return r.iters, bool(sharp)


def bicg_count_envelope(A, solve, b, rtols, max_iter, eps=1e-13):
    """BiCGStab on a pair where rounding decides the late iterations: the counts of a FAMILY of model runs -- sums forwards and
    backwards, the preconditioner exact and perturbed by ``eps`` relative (the accuracy class of the device's factor apply) -- at every
    tolerance of ``rtols``.  Returns [(lo, hi, sharp)]: the least and the largest count of the family, and whether every member puts
    the tolerance into a gap of sqrt(GAP) either side of its deciding test.  A count is the iteration of the first test, half step or
    full, that meets the tolerance (no breakdown on the way: asserted)."""
    hist = []
    for reverse in (False, True):
        for e in (0.0, eps):
            rng = np.random.default_rng(1)
            pre = (lambda v, e=e, rng=rng: solve(v) * (1.0 + e * rng.standard_normal(v.size))) if e else solve
            r = bicgstab_real(A, pre, b, 1e-300, max_iter, reverse=reverse)
            assert len(r.history) == 2 * max_iter + 1, "a breakdown: the history is no longer two tests per iteration"
            hist.append(np.asarray(r.history) / r.history[0])
    out = []
    for rtol in rtols:
        counts, sharp = [], True
        for h in hist:
            k = int(np.argmax(h[1:] <= rtol)) + 1
            assert h[k] <= rtol, "the family's free runs are too short for this tolerance"
            counts.append((k + 1) // 2)
            sharp = sharp and rtol / h[k] >= np.sqrt(GAP) and h[:k].min() / rtol >= np.sqrt(GAP)
        out.append((min(counts), max(counts), bool(sharp and min(counts) == max(counts))))
    return out


def spread(xa, xb):
    return float(np.linalg.norm(xa - xb) / np.linalg.norm(xa))


def bound(xa, xb):
    """what the device's iterate may differ from the model's by, relative"""
    return max(MARGIN * spread(xa, xb), FLOOR)


def history_run(model, A, b, max_iter, restart, var):
    """the residual norms of a run that never meets its tolerance before max_iter (rtol far below round-off)"""
    return model(A, var["precond"], b, 1e-300, max_iter, restart, reverse=var["reverse"]).history


#: Real drivers.  Factored: BDF2 at dt = 0.005, Re = 100 around a smooth velocity.  Current operator of a pair: the advection changed
#: by ADVECTION[pair] -- A M^-1 = I + dC A0^-1 has its spectrum in a disc around 1, so the estimate falls at an even rate from the first
#: step of every cycle on, and the run is well conditioned: the two variants of the model agree to some 1e-15 at every n below.
#:   "fast" (the pair of tests/test_krylov_gpu.py) some 20 per step, "mid" 3 to 5, "restart" 1.5 to 2, "crawl" 1.4 to 1.5.
#: "slow" is the same advection at mass = 30 (dt ten times larger): 59 GMRES(30) iterations to 1e-13 at 1.65 per step, but NOT a pair
#: for long runs: a perturbation of one rounding error grows about fourfold per step (an Arnoldi process with three full
#: re-orthogonalisations shows the same), so that the variants' iterates part by 1e-15 * 4^n while the error falls by 1.65^n only --
#: beyond n = 14 the n-th iterate is no sharper than the error itself, at n = 40 not even the count is.  It serves one short case.  The
#: first step after a restart gains a mere 1.1 on it, too.
ADVECTION = {"fast": 0.4, "mid": 2.0, "restart": 7.0, "crawl": 10.0}
#: GMRES on Mesh.unit_square(16, 16): (pair, n).  30 / 31: the last column of the first cycle, the first after the restart
GMRES_CASES = [("fast", 3), ("mid", 12), ("slow", 12), ("restart", 20), ("restart", 30), ("restart", 31), ("restart", 40), ("crawl", 45)]
#: BiCGStab: (pair, deciding iteration, ending)
BICG_CASES = [("fast", 3, "half"), ("fast", 3, "full"), ("mid", 8, "half"), ("mid", 8, "full"), ("restart", 11, "half")]
#: the second trip of fc_multidot's grid-stride loop (N > 65 536): Mesh.unit_square(96, 96), N = 83 907 -- 72 of the 256 workgroups go
#: round again.  fc_dots2 would need N > 131 072, unit_square(128, 128); tests/test_krylov_counts_gpu.py says what that costs.
LARGE_MESH = 96
LARGE_GMRES = ("mid", 8)
LARGE_BICG = ("mid", 6, "full")

DT, RE = 0.005, 100.0
REAL_MAX_ITER = 60


def smooth_velocity(xy):
    return np.r_[1.0 + 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]), 0.2 * np.cos(0.5 * xy[:, 0] + 0.1) * np.sin(xy[:, 1])]


def real_operators(pair, xy):
    """(factored, current) as keyword sets of assemble_matrix (the oracle's and the device's take the same)"""
    U0 = smooth_velocity(xy)
    f = dict(mass=1.5 / DT, nu=1.0 / RE, adv=U0, lin=U0)
    if pair == "slow":
        return f, dict(mass=30.0, nu=1.0 / RE, adv=U0, lin=U0)
    U1 = U0 + ADVECTION[pair] * np.r_[np.cos(2.0 * xy[:, 1]), np.sin(1.5 * xy[:, 0])]
    return f, dict(mass=1.5 / DT, nu=1.0 / RE, adv=U1, lin=U1)


def wall_dofs(th):
    """both velocity components on every boundary edge but the right-hand side's (the outflow)"""
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    return np.sort(np.r_[nodes, nodes + th.nn])


def real_rhs(N, dofs, seed=3):
    b = np.random.default_rng(seed).standard_normal(N)
    b[dofs] = 0.0
    return b


def bicg_index(iteration, ending):
    """where the test of (iteration, "half" | "full") stands in the history of a free BiCGStab run (history[0] = |b|)"""
    return 2 * iteration - (1 if ending == "half" else 0)


def real_case(model, A1, var, b, k):
    """(rtol, gap) that make the k-th test of ``model`` on (A1, var, b) the deciding one"""
    if model is gmres_real:  # (a cap below the restart length would shorten the cycle: the estimates up to k are the same)
        cap = k + 1 if k + 1 < GMRES_M else REAL_MAX_ITER
    else:
        cap = (k + 1) // 2 + 1
    h = history_run(model, A1, b, cap, GMRES_M, var)
    tol, gap = rtol_for(h, k)
    return tol / h[0], gap


#: Complex GMRES on the open problem: factors of SIGMA_F, solves at another shift.  At SIGMA_FAR the estimate falls by 7 to 25 per
#: step, at SIGMA_NEAR by some 150.
SIGMA_F = 0.3 + 0.7j
SIGMA_FAR = 0.3 + 1.5j
SIGMA_NEAR = 0.3 + 0.75j
#: single column: (shift, restart, n).  Restart 3: inside the first cycle, at its end, the first column after it, the end of the
#: second, the first of the third; restart 7: before, at, after; restart 60: no restart in reach.
COMPLEX_CASES = [
    (SIGMA_FAR, 3, 2), (SIGMA_FAR, 3, 3), (SIGMA_FAR, 3, 4), (SIGMA_FAR, 3, 6), (SIGMA_FAR, 3, 7),
    (SIGMA_FAR, 7, 6), (SIGMA_FAR, 7, 7), (SIGMA_FAR, 7, 8),
    (SIGMA_FAR, 60, 4), (SIGMA_FAR, 60, 8), (SIGMA_NEAR, 60, 2),
]
ADJOINT_CASES = [(SIGMA_FAR, 3, 3), (SIGMA_FAR, 3, 4), (SIGMA_FAR, 7, 7), (SIGMA_FAR, 7, 8), (SIGMA_FAR, 60, 5)]
COMPLEX_MAX_ITER = 200
#: max_iter ends inside a cycle on purpose: (shift, restart, max_iter, rtol): cycles of 7 and 3 columns, then nothing is left
CAPPED_CASE = (SIGMA_FAR, 7, 10, 1e-13)
#: the second trip of fc_cmultidot's grid-stride loop (n > 16 384): the open problem on square_mesh(48), N = 21 219
LARGE_COMPLEX = (48, SIGMA_FAR, 3, 7)
#: Block solves.  k columns padded to the widths 4, 8, 16, 32 (batch_width in fc_hip.hip, BatchWidths in fc_dispatch.hpp).  The columns
#: cycle through four shifts and two right-hand sides -- one tolerance serves all columns of a block, and it can sit in the gap of
#: EVERY column only when the distinct histories are few (32 unrelated columns leave no tolerance a gap of 1.4 all round).
BLOCK_KS = (3, 5, 12, 32)
BLOCK_BASE = 0.3 + 1j * np.array([0.72, 0.9, 1.2, 1.5])
BLOCK_RESTART = 3
BLOCK_MAX_ITER = 200
BLOCK_RTOLS = np.logspace(-9, -6, 301)  # the candidates of block_rtol
#: width 4 on square_mesh(32) (N = 9 539 > 64 * 256 / 4): the block multidot's loop makes a second trip at that width too
LARGE_BLOCK = (32, 3)


def block_columns(k, N):
    """(shifts [k], right-hand sides [k, N]): column c takes shift 3 c mod 4 and right-hand side (c div 4) mod 2"""
    c = np.arange(k)
    return BLOCK_BASE[(3 * c) % 4], complex_rhs(2, N)[(c // 4) % 2]


def block_rtol(histories, restart=BLOCK_RESTART):
    """the candidate tolerance with the widest gap over ALL columns among those at which one column is done in the first cycle and
    another needs a third; (rtol, gap, counts).  histories: per column, the estimates of a free run (absolute, [0] = |b|)"""
    best = None
    for tol in BLOCK_RTOLS:
        gaps, counts = [], []
        for h in histories:
            h = np.asarray(h) / h[0]
            n = int(np.argmax(h <= tol))
            gaps.append(min(h[:n].min() / tol, tol / h[n]) if n > 0 else 0.0)
            counts.append(n)
        if not (min(counts) <= restart and max(counts) > 2 * restart):
            continue
        if best is None or min(gaps) > best[1]:
            best = (float(tol), float(min(gaps)), counts)
    return best


def complex_case(Mop, var, b, restart, n):
    """(rtol, gap) that make step n of gmres_complex on (Mop, var, b) the deciding one"""
    h = gmres_complex(Mop, var["precond"], b, 1e-300, n + 1, restart, reverse=var["reverse"]).history
    tol, gap = rtol_for(h, n)
    return tol / h[0], gap


def complex_rhs(k, N, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, N)) + 1j * rng.standard_normal((k, N))


def shifted_op(A, E, sigma, adjoint=False):
    M = (sigma * E - A).astype(complex)
    return (M.conj().T if adjoint else M).tocsr()


def oracle_open_problem(n=10):
    """The open n x n problem of tests/support/shifted_open.py assembled by the oracle in ITS numbering: (A, E), identity rows on the
    left / bottom velocity dofs."""
    from oracle import ns_oracle as O
    from tests.support.shifted_open import square_mesh

    coords, cells, _, _ = square_mesh(n)
    d = O.Disc.from_mesh_arrays(coords, cells)
    xy = d.node_coords()
    adv = np.r_[1.0 + 0.2 * np.sin(3 * xy[:, 1]), 0.3 * np.cos(2 * xy[:, 0])]
    A = O.assemble_matrix(d, mass=0.0, nu=-0.02, adv=adv, adv_scale=-1.0, pressure=1.0, divergence=1.0)
    E = O.assemble_matrix(d, mass=1.0, pressure=0.0, divergence=0.0)
    wall = np.flatnonzero((xy[:, 0] < 1e-12) | (xy[:, 1] < 1e-12))
    A, _ = O.apply_bc_rows(A, None, np.r_[wall, d.nn + wall], None)
    return A.tocsr(), E.tocsr()
