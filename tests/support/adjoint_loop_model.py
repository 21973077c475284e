"""numpy / scipy model of a closed loop and of its exact discrete adjoint (``fc_run_closed_loop`` / ``fc_run_adjoint_closed_loop``) --
TEST INFRASTRUCTURE.  The plant is a ``StepModel`` (linearised) or a ``NonlinearStepModel``; the controller is a bank of one
(``flowcontrol_amd.controller.pack_controllers`` layout) advanced by ``controller.bank_step``.

Forward, m = 1 .. n (xi = controller state, y_0 given):

    yc_m = G y_{m-1} + g0 + w_y[m]      uc_m = C xi_{m-1} + D yc_m      xi_m = Ad xi_{m-1} + Bd yc_m
    v_m  = S uc_m + w_u[m]              u_m  = min(max(v_m, lo), hi)    x_m = plant step m with u_m,   y_m = C_s x_m

Cost ``J = sum_m (w_m . y_m + r_m . u_m) + z . x_n``.  Backward, written out on its own, m = n .. 1 from lambda_n = 0, eta_{n+1} = 0:

    mu_m  = A_s^-T [C_s^T (w_m + G^T eta_{m+1}) (+ z at m = n) + M Z (..) + J(x_m)^T Z (..)]
    ub_m  = B_s^T mu_m + r_m     vb_m = sigma_m o ub_m     ucb_m = S^T vb_m
    eta_m = D^T ucb_m + Bd^T lambda_m                      lambda_{m-1} = Ad^T lambda_m + C^T ucb_m

``wrong=`` switches one mistake on (the tests show that the inputs tell them apart): ``"xi_after"`` takes the controller state AFTER the
update in the outer products, ``"no_mask"`` ignores the clamp, ``"G_late"`` lets ``G^T eta`` enter the sensor weights one step late.
"""
from __future__ import annotations

import numpy as np

from flowcontrol_amd.controller import bank_step
from tests.support import adjoint_step_model as am

#: gradient groups of the bank and of the loop's inputs
PARAMS = ("Ad", "Bd", "C", "D", "G", "g0", "S")
GROUPS = PARAMS + ("x0", "y0", "w_y", "w_u", "dx0", "dxm1")


def _nonlinear(plant) -> bool:
    return hasattr(plant, "conv")


def _coeffs(plant, order):
    if _nonlinear(plant):
        from tests.support import adjoint_nl_model as nlm

        return nlm.coeffs(order, plant.dt)
    return (*am.coeffs(order, plant.dt), 0.0, 0.0)


def random_bank(nx, nyc, nuc, n_sens, n_act, seed=0, gain=1.0, radius=0.9):
    """A bank of one controller with a stable random ``Ad`` (spectral radius ``radius``) and generic matrices; ``nuc = 1`` is fanned out
    to every actuator by a column of ones, as ``pack_controllers`` does."""
    rng = np.random.default_rng(seed)
    Ad = rng.standard_normal((nx, nx))
    if nx:
        Ad *= radius / max(abs(np.linalg.eigvals(Ad)))
    S = np.ones((n_act, 1)) if nuc == 1 else np.eye(n_act, nuc) + 0.1 * rng.standard_normal((n_act, nuc))
    bank = {"k": 1, "nx": nx, "nyc": nyc, "nuc": nuc, "Ad": Ad[None], "Bd": rng.standard_normal((1, nx, nyc)) / np.sqrt(max(nx, 1)),
            "C": gain * rng.standard_normal((1, nuc, nx)) / np.sqrt(max(nx, 1)), "D": gain * rng.standard_normal((1, nuc, nyc)),
            "x0": 0.3 * rng.standard_normal((1, nx)), "G": rng.standard_normal((1, nyc, n_sens)), "g0": 0.1 * rng.standard_normal((1, nyc)),
            "S": S[None], "sizes": [(nx, nuc)]}
    return bank


def copy_bank(bank):
    return {k: (v.copy() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, list) else v)) for k, v in bank.items()}


class Loop:
    """One closed-loop problem: plant, bank, first step's order, the two initial time levels, ``y0``, signals ``w_y`` (n, nyc) /
    ``w_u`` (n, n_act) and limits ``lo`` / ``hi`` (n_act,), each optional."""

    def __init__(self, plant, bank, first_order, n, x0, xm1, y0, w_y=None, w_u=None, lo=None, hi=None):
        self.plant, self.bank, self.first_order, self.n = plant, bank, int(first_order), int(n)
        self.x0, self.xm1, self.y0 = (np.asarray(a, dtype=float).copy() for a in (x0, xm1, y0))
        self.w_y = None if w_y is None else np.asarray(w_y, dtype=float).reshape(n, bank["nyc"]).copy()
        self.w_u = None if w_u is None else np.asarray(w_u, dtype=float).reshape(n, plant.n_act).copy()
        self.lo = None if lo is None else np.broadcast_to(np.asarray(lo, dtype=float), (plant.n_act,)).copy()
        self.hi = None if hi is None else np.broadcast_to(np.asarray(hi, dtype=float), (plant.n_act,)).copy()

    def clone(self):
        return Loop(self.plant, copy_bank(self.bank), self.first_order, self.n, self.x0, self.xm1, self.y0, self.w_y, self.w_u, self.lo, self.hi)

    # ── forward ──────────────────────────────────────────────────────────────
    def plant_step(self, order, x1, x2, u):
        p = self.plant
        cn, cnn, ccn, ccnn = _coeffs(p, order)
        inner = p.M @ (cn * x1 + cnn * x2)
        if _nonlinear(p):
            inner = inner + ccn * p.conv(x1)
            if ccnn != 0.0:
                inner = inner + ccnn * p.conv(x2)
        return p.lu[order].solve(p.free * inner + p.B[order] @ u)

    def forward(self):
        """dict: X [n + 2, N], y [n + 1, n_sens] (row 0 = y0), u, v [n, n_act], xi [n + 1, nx], yc [n, nyc], uc [n, nuc]."""
        p, b, n = self.plant, self.bank, self.n
        X = [self.xm1, self.x0]
        y, xi = [self.y0], [b["x0"][0].copy()]
        u, v, yc, uc = [], [], [], []
        for m in range(1, n + 1):
            kw = {}
            if self.w_y is not None:
                kw["w_y"] = self.w_y[m - 1][None]
            if self.w_u is not None:
                kw["w_u"] = self.w_u[m - 1][None]
            if self.lo is not None:
                kw["u_lo"], kw["u_hi"] = self.lo[None], self.hi[None]
            um, xn = bank_step(b, xi[-1][None], y[-1][None], **kw)
            ycm = b["G"][0] @ y[-1] + b["g0"][0] + (0.0 if self.w_y is None else self.w_y[m - 1])
            ucm = b["C"][0] @ xi[-1] + b["D"][0] @ ycm
            vm = b["S"][0] @ ucm + (0.0 if self.w_u is None else self.w_u[m - 1])
            X.append(self.plant_step(p.order_of(m, self.first_order), X[-1], X[-2], um[0]))
            y.append(p.C @ X[-1])
            xi.append(xn[0]), u.append(um[0]), v.append(vm), yc.append(ycm), uc.append(ucm)
        return {"X": np.array(X), "y": np.array(y), "u": np.array(u), "v": np.array(v), "xi": np.array(xi).reshape(n + 1, b["nx"]),
                "yc": np.array(yc), "uc": np.array(uc)}

    def cost(self, w, r, z=None):
        f = self.forward()
        return float(np.sum(np.asarray(w) * f["y"][1:]) + np.sum(np.asarray(r) * f["u"]) + (0.0 if z is None else np.dot(z, f["X"][-1])))

    def mask(self, v):
        """sigma: 1 where the control is free, 0 where a limit holds it."""
        if self.lo is None:
            return np.ones_like(v)
        return ((self.lo < v) & (v < self.hi)).astype(float)

    # ── backward ─────────────────────────────────────────────────────────────
    def _products(self, X, col, a_m, a_c):
        p = self.plant
        out = p.M.T @ (p.free * a_m)
        if _nonlinear(p):
            out = out + p.jac(X[col]).T @ (p.free * a_c)
        return out

    def adjoint(self, f, w, r, z=None, wrong=None):
        """Gradients of ``cost(w, r, z)`` for the forward run ``f``: dict over ``GROUPS`` plus ``ubar`` (n, n_act) and ``mask``."""
        p, b, n = self.plant, self.bank, self.n
        Ad, Bd, C, D, G, S = (b[k][0] for k in ("Ad", "Bd", "C", "D", "G", "S"))
        X, y, v, xi, yc, uc = f["X"], f["y"], f["v"], f["xi"], f["yc"], f["uc"]
        w = np.asarray(w, dtype=float).reshape(n, -1)
        r = np.asarray(r, dtype=float).reshape(n, p.n_act)
        Ct = p.C.T.tocsr()
        cf = lambda j: _coeffs(p, p.order_of(j, self.first_order))  # noqa: E731
        zero = np.zeros(p.N)
        mu = {n + 1: zero, n + 2: zero}
        eta = {n + 1: np.zeros(b["nyc"]), n + 2: np.zeros(b["nyc"])}
        lam = np.zeros(b["nx"])
        g = {k: np.zeros_like(b[k][0]) for k in PARAMS}
        g["w_y"], g["w_u"], ubar = np.zeros((n, b["nyc"])), np.zeros((n, p.n_act)), np.zeros((n, p.n_act))
        sig = np.ones_like(v) if wrong == "no_mask" else self.mask(v)

        def combined(m):  # what the forward steps m + 1 and m + 2 did with x_m, gated by the horizon
            a_m, a_c = zero.copy(), zero.copy()
            if m + 1 <= n:
                c = cf(m + 1)
                a_m += c[0] * mu[m + 1]
                a_c += c[2] * mu[m + 1]
            if m + 2 <= n:
                c = cf(m + 2)
                a_m += c[1] * mu[m + 2]
                a_c += c[3] * mu[m + 2]
            return a_m, a_c

        for m in range(n, 0, -1):
            rhs = Ct @ (w[m - 1] + G.T @ eta[m + 2 if wrong == "G_late" else m + 1])
            if m == n and z is not None:
                rhs = rhs + np.asarray(z, dtype=float)
            if m < n:
                rhs = rhs + self._products(X, m + 1, *combined(m))
            s = p.order_of(m, self.first_order)
            mu[m] = p.lu[s].solve(rhs, trans="T")
            ubar[m - 1] = p.B[s].T @ mu[m] + r[m - 1]
            vb = sig[m - 1] * ubar[m - 1]
            ucb = S.T @ vb
            eta[m] = D.T @ ucb + Bd.T @ lam
            xi_used = xi[m] if wrong == "xi_after" else xi[m - 1]
            g["Ad"] += np.outer(lam, xi_used)
            g["Bd"] += np.outer(lam, yc[m - 1])
            g["C"] += np.outer(ucb, xi_used)
            g["D"] += np.outer(ucb, yc[m - 1])
            g["G"] += np.outer(eta[m], y[m - 1])
            g["g0"] += eta[m]
            g["S"] += np.outer(vb, uc[m - 1])
            g["w_y"][m - 1], g["w_u"][m - 1] = eta[m], vb
            lam = Ad.T @ lam + C.T @ ucb
        g["x0"] = lam
        g["y0"] = G.T @ eta[2 if wrong == "G_late" else 1]
        g["dx0"] = self._products(X, 1, *combined(0))
        c1 = cf(1)
        g["dxm1"] = self._products(X, 0, c1[1] * mu[1], c1[3] * mu[1])
        g["ubar"], g["mask"] = ubar, sig
        return g

    # ── finite differences of the model's own forward run ────────────────────
    def perturbed(self, group, direction, h):
        """A copy with ``group`` moved by ``h * direction``."""
        q = self.clone()
        d = np.asarray(direction, dtype=float)
        if group in PARAMS:
            q.bank[group][0] += h * d
        elif group == "x0":
            q.bank["x0"][0] += h * d
        elif group == "y0":
            q.y0 += h * d
        elif group == "w_y":
            q.w_y = (np.zeros((self.n, self.bank["nyc"])) if q.w_y is None else q.w_y) + h * d
        elif group == "w_u":
            q.w_u = (np.zeros((self.n, self.plant.n_act)) if q.w_u is None else q.w_u) + h * d
        elif group == "dx0":
            q.x0 += h * d
        elif group == "dxm1":
            q.xm1 += h * d
        else:
            raise KeyError(group)
        return q

    def fd_directional(self, group, direction, h, w, r, z=None):
        return (self.perturbed(group, direction, h).cost(w, r, z) - self.perturbed(group, direction, -h).cost(w, r, z)) / (2.0 * h)

    def fd_gradient(self, group, shape, h, w, r, z=None):
        """Central differences entry by entry."""
        out = np.zeros(shape)
        for idx in np.ndindex(*shape):
            d = np.zeros(shape)
            d[idx] = 1.0
            out[idx] = self.fd_directional(group, d, h, w, r, z)
        return out


def limits_report(v, lo, hi):
    """(clamped count, free count, smallest distance of a free value to a limit relative to that limit's magnitude)."""
    v = np.asarray(v, dtype=float)
    lo, hi = np.broadcast_to(lo, v.shape), np.broadcast_to(hi, v.shape)
    free = (lo < v) & (v < hi)
    dist = np.minimum(np.abs(v - lo) / np.abs(lo), np.abs(hi - v) / np.abs(hi))
    return int(np.sum(~free)), int(np.sum(free)), float(np.min(dist[free])) if np.any(free) else np.inf


def assert_limits_tell(v, lo, hi):
    """The conditions a clamped test case must meet: at least two control values clamped, at least two free, and no free value closer
    to a limit than 1e-3 of the limit's magnitude (no finite-difference step crosses a kink)."""
    clamped, free, dist = limits_report(v, lo, hi)
    assert clamped >= 2 and free >= 2, (clamped, free)
    assert dist >= 1e-3, dist


def rel(a, ref):
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    nr = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / nr) if nr > 0 else float(np.linalg.norm(a))
