"""The stepping problem of tests/test_adjoint_step_gpu.py (the linearised 8 x 8 square of tests/test_modal_gpu.py::square with both
order slots set up), the comparison of a device adjoint run with the scipy model, and the child processes of that test:

    python adjoint_step_child.py run          the comparison of test 3 in this process's environment (FC_UP_FORM=column)
    python adjoint_step_child.py partitioned  a thread-rank handle refuses the transposed factors

Prints CHILD OK <mode> at the end; exits non-zero with the failed assertion."""
import sys

import numpy as np
import scipy.sparse as sp

#: the project's series tolerance against its oracle
TOL = 1e-8


def smooth_velocity(th, k=1.0):
    x = th.node_coords
    return np.r_[1.0 + 0.3 * np.sin(k * x[:, 0]) * np.cos(0.7 * k * x[:, 1]), 0.2 * np.cos(0.5 * k * x[:, 0] + 0.1) * np.sin(k * x[:, 1])]


def bc_setup(th):
    """Dirichlet everywhere but on the x = xmax side, two actuators with smooth profiles (as tests/test_modal_gpu.py)."""
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    dofs = np.r_[nodes, nodes + th.nn]
    x = th.node_coords[nodes]
    p0 = np.r_[np.sin(x[:, 0] + 2 * x[:, 1]), 0 * x[:, 0]]
    p1 = np.r_[0 * x[:, 0], np.cos(3 * x[:, 0] - x[:, 1])]
    order = np.argsort(dofs)
    return dofs[order], np.stack([p0, p1], axis=1)[order]


class Square:
    """Device handle, scipy model and fixed inputs of the linearised square."""

    def __init__(self, nx=8, refine=1):
        from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood
        from tests.support import adjoint_step_model as am

        th = self.th = TaylorHood(Mesh.unit_square(nx, nx))
        dev = self.dev = DeviceSolver(th)
        self.dt, Re = 0.005, 100.0
        U0 = smooth_velocity(th)
        dofs, prof = bc_setup(th)
        self.dofs, self.prof = dofs, prof
        dev.set_bc(dofs, prof)
        dev.set_time_scheme(self.dt, False)
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        self.M = dev.matrix(SLOT_MASS)
        raw, A = {}, {}
        for order, slot, c in ((1, SLOT_BDF1, 1.0 / self.dt), (2, SLOT_BDF2, 1.5 / self.dt)):
            dev.assemble_matrix(slot, mass=c, nu=1.0 / Re, adv=U0, lin=U0)
            raw[order] = dev.matrix(slot)
            dev.apply_bc(slot)
            A[order] = dev.matrix(slot)
            dev.setup_solver(slot, refine=refine)
            assert not dev.factors_inexact[slot]
        self.A, self.U0, self.Re = A, U0, Re
        row = th.point_eval_row((0.31, 0.42), 1)
        dev.set_sensors([row])
        G = np.zeros((dev.N, 2))
        G[dofs] = prof
        C = sp.csr_matrix((row[1], (np.zeros(len(row[0]), dtype=int), row[0])), shape=(1, dev.N))
        self.model = am.StepModel(A[1], A[2], self.M, dofs, prof, raw[1] @ G, raw[2] @ G, C, self.dt)
        rng = np.random.default_rng(2)
        self.u_n = 0.1 * smooth_velocity(th, 2.0) + 0.01 * rng.standard_normal(2 * th.nn)
        self.u_nn = 0.1 * smooth_velocity(th, 1.5)
        self.p = 0.01 * rng.standard_normal(th.nv)

    def restart(self):
        self.dev.set_state(self.u_n, self.u_nn, self.p)

    def close(self):
        self.dev.close()


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(ref)) / np.linalg.norm(ref))


def compare_run(sq, first_order, n, seed=5, label=""):
    """Device adjoint run (transposed factors must be set) against the model, and the dot-product identity of the device's own forward
    run with it; returns the figures.  Asserts TOL on all of them and bit-identical repeats."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
    from tests.support import adjoint_step_model as am

    dev, model = sq.dev, sq.model
    slot = SLOT_BDF1 if first_order == 1 else SLOT_BDF2
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, dev.n_act))  # non-zero on both (Dirichlet) actuators
    w = rng.standard_normal((n, dev.n_sens))
    z = rng.standard_normal(dev.N)
    g, dx0, dxm1 = dev.run_adjoint(slot, n, w, z)
    g2, dx02, dxm12 = dev.run_adjoint(slot, n, w, z)
    # the last backward step took the route of a small linearised handle with two actuators: eight lanes per cell, one tail pass, the reduction
    route = dict(zip(dev.ADJ_ROUTE_COLS, (int(v) for v in dev.adjoint_route())))
    assert (route["elem"], route["KB"], route["passes"], route["reduced"], route["w"]) == (1, 0, 1, 1, 1), route
    assert route["g_tail"] == route["gx"] == route["g_gather"] == -(-dev.N // 256) and route["term"] == (1 if n == 1 else 0), route
    assert np.array_equal(g, g2) and np.array_equal(dx0, dx02) and np.array_equal(dxm1, dxm12), "two identical adjoint runs differ"
    gm, dx0m, dxm1m, _ = model.adjoint(first_order, n, w, z)
    out = {"g": rel(g, gm), "dx0": rel(dx0, dx0m)}
    if np.any(dxm1m):
        out["dxm1"] = rel(dxm1, dxm1m)
    else:  # a BDF1 first step never reads x_{-1}
        assert not np.any(dxm1)
        out["dxm1"] = 0.0
    # the identity with the DEVICE forward run
    sq.restart()
    y, _ = dev.run(slot, n, u, compute_energy=False)
    xn = dev.get_solution()
    x0, xm1 = np.r_[sq.u_n, sq.p], np.r_[sq.u_nn, sq.p]
    out["identity"] = model.dot_defect(*am.identity_terms(w, y, z, xn, u, g, x0, dx0, xm1, dxm1))
    # (and the forward run is the model's: the comparison above is about the same recurrence)
    X, ym = model.forward(first_order, u, x0, xm1)
    out["forward_y"] = rel(y, ym)
    sq.restart()
    print(f"adjoint run {label}first order {first_order}, n = {n}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()), flush=True)
    for k, v in out.items():
        assert v <= TOL, f"{k}: {v:.3e} > {TOL:.1e}"
    return out


def main(mode: str) -> None:
    from flowcontrol_amd import _lib
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    if mode == "run":
        import os

        assert os.environ.get("FC_UP_FORM") == "column"
        sq = Square()
        try:
            for s in (SLOT_BDF1, SLOT_BDF2):
                sq.dev.set_adjoint_factors(s, 1)
            compare_run(sq, 1, 12, label="(column-form up-sweep) ")
        finally:
            sq.close()
    elif mode == "partitioned":
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood

        dev = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
        try:
            fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
            _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
            try:
                dev.set_adjoint_factors(SLOT_BDF2, 1)
            except _lib.FcError as e:
                assert e.code == _lib.FC_ERR_INVALID and "partitioned" in str(e), str(e)
            else:
                raise AssertionError("a partitioned handle took transposed factors")
        finally:
            dev.close()
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    print("CHILD OK", mode, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
