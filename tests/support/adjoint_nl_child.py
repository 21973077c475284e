"""The stepping problem of tests/test_adjoint_nl_gpu.py (the NONLINEAR 7 x 5 square: 70 cells, so the last workgroup of the
eight-lane element kernel is partial; both order slots set up with ``set_time_scheme(dt, True)``), the comparison of a taped device
run and its adjoint with the scipy model of tests/support/adjoint_nl_model.py, and the child process of that test:

    python adjoint_nl_child.py reg    the comparison in this process's environment (FC_ELEM_REG_MIN=1: the thread-per-cell kernel)

Prints CHILD OK <mode> at the end; exits non-zero with the failed assertion."""
import sys

import numpy as np

from tests.support import adjoint_nl_model as nm

#: the project's series tolerance against its oracle
TOL = 1e-8
#: central differences of the device forward run at EPS (J is not quadratic: truncation error remains)
EPS, TOL_FD = 1e-4, 1e-6
#: (first order, n)
CASES = [(1, 6), (2, 3)]


class NlSquare:
    """Device handle, scipy model and fixed inputs of the nonlinear square."""

    def __init__(self, nx=7, ny=5, refine=1):
        from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood

        th = self.th = TaylorHood(Mesh.unit_square(nx, ny))
        dev = self.dev = DeviceSolver(th)
        self.dt = nm.DT
        U0, dofs, prof, row, self.u_n, self.u_nn, self.p = nm.square_inputs(th)
        dev.set_bc(dofs, prof)
        dev.set_time_scheme(self.dt, True)
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        M = dev.matrix(SLOT_MASS)
        raw, A = {}, {}
        for order, slot, c in ((1, SLOT_BDF1, 1.0 / self.dt), (2, SLOT_BDF2, 1.5 / self.dt)):
            dev.assemble_matrix(slot, mass=c, nu=1.0 / nm.RE, adv=U0, lin=U0)
            raw[order] = dev.matrix(slot)
            dev.apply_bc(slot)
            A[order] = dev.matrix(slot)
            dev.setup_solver(slot, refine=refine)
            assert not dev.factors_inexact[slot]
        dev.set_sensors([row])
        self.model = nm.model_from(th, raw, A, M, dofs, prof, row, self.dt)
        self.x0, self.xm1 = np.r_[self.u_n, self.p], np.r_[self.u_nn, self.p]
        self.restart()

    def restart(self):
        self.dev.set_state(self.u_n, self.u_nn, self.p)

    def close(self):
        self.dev.close()


def compare_run(sq, first_order, n, seed=5, label=""):
    """A taped device run and its adjoint (transposed factors and a tape of at least n steps must be set) against the model, and the
    directional derivative of the device's own forward run; returns the figures.  Asserts TOL / TOL_FD and bit-identical repeats."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    dev, model = sq.dev, sq.model
    nn2 = 2 * sq.th.nn
    slot = SLOT_BDF1 if first_order == 1 else SLOT_BDF2
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, dev.n_act))
    w = rng.standard_normal((n, dev.n_sens))
    z = rng.standard_normal(dev.N)
    sq.restart()
    dev.adjoint_tape_begin()
    y, _ = dev.run(slot, n, u, compute_energy=False)
    info = dev.adjoint_tape_info()
    assert info["count"] == n and info["begun"] and not info["overflowed"], info
    X = dev.adjoint_tape_states()
    Xm, ym = model.forward(first_order, u, sq.x0, sq.xm1)
    assert np.array_equal(X[0], sq.xm1) and np.array_equal(X[1], sq.x0) and np.array_equal(X[-1], dev.get_solution())
    out = {"forward_X": nm.rel(X, Xm), "forward_y": nm.rel(y, ym)}
    g, dx0, dxm1 = dev.run_adjoint(slot, n, w, z)
    g2, dx02, dxm12 = dev.run_adjoint(slot, n, w, z)
    assert np.array_equal(g, g2) and np.array_equal(dx0, dx02) and np.array_equal(dxm1, dxm12), "two identical adjoint runs differ"
    gm, dx0m, dxm1m, _ = model.adjoint(first_order, Xm, w, z)
    out["g"], out["dx0"] = nm.rel(g, gm), nm.rel(dx0, dx0m)
    if np.any(dxm1m):
        out["dxm1"] = nm.rel(dxm1, dxm1m)
    else:  # a BDF1 first step never reads x_{-1}
        assert not np.any(dxm1)
        out["dxm1"] = 0.0
    # ... and they differ from the linear adjoint by far more than the tolerance (the convective term acts)
    assert nm.rel(model.adjoint(first_order, Xm, w, z, wrong="linear")[0], gm) > 1e-4
    # the derivative of the DEVICE forward run in one direction (controls and both velocity levels)
    du, d0, dm1 = rng.standard_normal(u.shape), rng.standard_normal(nn2), rng.standard_normal(nn2)

    def cost(sign):
        dev.set_state(sq.u_n + sign * EPS * d0, sq.u_nn + sign * EPS * dm1, sq.p)
        yy, _ = dev.run(slot, n, u + sign * EPS * du, compute_energy=False)
        return float(np.sum(w * yy) + z @ dev.get_solution())

    fd = (cost(1.0) - cost(-1.0)) / (2 * EPS)
    ad = float(np.sum(g * du) + dx0[:nn2] @ d0 + dxm1[:nn2] @ dm1)
    fd_err = abs(fd - ad) / abs(fd)
    sq.restart()
    print(f"nonlinear adjoint run {label}first order {first_order}, n = {n}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()) +
          f", device central difference {fd_err:.3e}", flush=True)
    for k, v in out.items():
        assert v <= TOL, f"{k}: {v:.3e} > {TOL:.1e}"
    assert fd_err <= TOL_FD, f"central difference of the device run: {fd_err:.3e} > {TOL_FD:.1e}"
    out["fd"] = fd_err
    return out


def main(mode: str) -> None:
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    if mode == "reg":
        import os

        assert os.environ.get("FC_ELEM_REG_MIN") == "1"
        sq = NlSquare()
        try:
            for s in (SLOT_BDF1, SLOT_BDF2):
                sq.dev.set_adjoint_factors(s, 1)
            sq.dev.adjoint_tape_reserve(6)
            for first_order, n in CASES:
                compare_run(sq, first_order, n, label="(thread per cell) ")
        finally:
            sq.close()
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    print("CHILD OK", mode, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
