"""numpy / scipy model of the TANGENT of a closed loop (``fc_run_tangent_closed_loop`` / ``_batch``) -- TEST INFRASTRUCTURE.  It
linearises ``tests/support/adjoint_loop_model.Loop`` about its own forward run: the arrays of ``Loop.forward()``, the bank's matrices
and, for a nonlinear plant, ``plant.jac`` at the states every step read.

Tangent step m = 1 .. n along ``d`` (a dict over ``adjoint_loop_model.GROUPS``; an absent group is zero):

    dyc_m = G dy_{m-1} + dG y_{m-1} + dg0 + dw_y[m]
    duc_m = C dxi_{m-1} + dC xi_{m-1} + D dyc_m + dD yc_m
    dxi_m = Ad dxi_{m-1} + dAd xi_{m-1} + Bd dyc_m + dBd yc_m
    dv_m  = S duc_m + dS uc_m + dw_u[m]        du_m = sigma_m o dv_m
    A_s dx_m = Z [M (cm_n dx_{m-1} + cm_nn dx_{m-2}) + cc_n J(x_{m-1}) dx_{m-1} + cc_nn J(x_{m-2}) dx_{m-2}] + B_s du_m,   dy_m = C_s dx_m

``wrong=`` switches one mistake on (tests/test_tangent_loop_host.py shows that the inputs tell them apart): ``"no_mask"`` ignores the
clamp, ``"xi_after"`` takes the controller state and its tangent AFTER the update in ``duc_m``, ``"dy_late"`` feeds ``dy_{m-2}`` to
step m.
"""
from __future__ import annotations

import numpy as np

from tests.support import adjoint_loop_model as lm


def tangent(loop, f, d, wrong=None):
    """dict: dy (n, n_sens), du (n, n_act), xi (nx,) = dxi_n, dxn, dxnm1 (N,), dX (n + 2, N)."""
    p, b, n = loop.plant, loop.bank, loop.n
    Ad, Bd, C, D, G, S = (b[k][0] for k in ("Ad", "Bd", "C", "D", "G", "S"))
    X, y, v, xi, yc, uc = f["X"], f["y"], f["v"], f["xi"], f["yc"], f["uc"]
    get = lambda k, shape: np.zeros(shape) if d.get(k) is None else np.asarray(d[k], dtype=float).reshape(shape)  # noqa: E731
    dAd, dBd, dC, dD, dG, dS = (get(k, b[k][0].shape) for k in ("Ad", "Bd", "C", "D", "G", "S"))
    dg0 = get("g0", (b["nyc"],))
    dw_y, dw_u = get("w_y", (n, b["nyc"])), get("w_u", (n, p.n_act))
    dxi = get("x0", (b["nx"],))
    dys = [get("y0", y[0].shape)]
    dX = [get("dxm1", (p.N,)), get("dx0", (p.N,))]
    sig = np.ones_like(v) if wrong == "no_mask" else loop.mask(v)
    du = np.zeros((n, p.n_act))
    for m in range(1, n + 1):
        dy_in = dys[max(m - 2, 0)] if wrong == "dy_late" else dys[m - 1]
        dyc = G @ dy_in + dG @ y[m - 1] + dg0 + dw_y[m - 1]
        dxi_new = Ad @ dxi + dAd @ xi[m - 1] + Bd @ dyc + dBd @ yc[m - 1]
        if wrong == "xi_after":
            duc = C @ dxi_new + dC @ xi[m] + D @ dyc + dD @ yc[m - 1]
        else:
            duc = C @ dxi + dC @ xi[m - 1] + D @ dyc + dD @ yc[m - 1]
        dxi = dxi_new
        du[m - 1] = sig[m - 1] * (S @ duc + dS @ uc[m - 1] + dw_u[m - 1])
        order = p.order_of(m, loop.first_order)
        cn, cnn, ccn, ccnn = lm._coeffs(p, order)
        d1, d2 = dX[-1], dX[-2]  # dx_{m-1}, dx_{m-2}; X[m] = x_{m-1}, X[m - 1] = x_{m-2}
        inner = p.M @ (cn * d1 + cnn * d2)
        if lm._nonlinear(p):
            inner = inner + ccn * (p.jac(X[m]) @ d1)
            if ccnn != 0.0:
                inner = inner + ccnn * (p.jac(X[m - 1]) @ d2)
        dX.append(p.lu[order].solve(p.free * inner + p.B[order] @ du[m - 1]))
        dys.append(np.asarray(p.C @ dX[-1]).reshape(-1))
    return {"dy": np.array(dys[1:]), "du": du, "xi": dxi, "dxn": dX[-1], "dxnm1": dX[-2], "dX": np.array(dX)}


def directions(g, seed=5, nn2=None, groups=lm.GROUPS):
    """One random direction per gradient group of ``g`` (``adjoint_loop_cases.fd_direction``), in the group's shape."""
    from tests.support import adjoint_loop_cases as lc

    return {grp: lc.fd_direction(grp, np.shape(g[grp]), seed=seed, nn2=nn2) for grp in groups}


def perturbed(loop, d, h):
    """A copy of ``loop`` with every group of ``d`` moved by ``h`` times its direction."""
    q = loop
    for grp, a in d.items():
        if a is not None:
            q = q.perturbed(grp, a, h)
    return q


def identity_terms(t, g, d, w, r, z=None):
    """(lhs, rhs, scale) of ``sum w . dy + sum r . du + z . dx_n = sum_groups <g, d>``; scale: the summed absolute terms."""
    left = [np.sum(np.asarray(w) * t["dy"]), np.sum(np.asarray(r) * t["du"])] + ([] if z is None else [np.dot(z, t["dxn"])])
    right = [np.sum(g[grp] * a) for grp, a in d.items() if a is not None]
    return float(sum(left)), float(sum(right)), float(sum(abs(x) for x in left) + sum(abs(x) for x in right))
