"""The closed-loop problems of tests/test_adjoint_loop_host.py and tests/test_adjoint_loop_gpu.py -- TEST INFRASTRUCTURE: the linearised
8 x 8 square of tests/support/adjoint_step_child.py and the nonlinear 7 x 5 square of tests/support/adjoint_nl_child.py, each with TWO
sensors (so that the columns of G are distinguishable), once from the oracle's operators (no device) and once on a device handle, and
the fixed inputs of a case: bank, signals, limits and cost weights from one seed."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.support import adjoint_loop_model as lm

#: sensor points and velocity components
SENSORS = (((0.31, 0.42), 1), ((0.62, 0.55), 0))
#: step of the central differences of the DEVICE's closed-loop cost along a random direction of a group, and their bound
#: (tests/support/adjoint_nl_child.py's bound; its step of 1e-4 leaves 2e-7 of truncation error in dJ/dAd at n = 12, so the step is
#: smaller here).  The model alone must meet FD_MODEL_TOL with the same inputs, directions and step: tests/test_adjoint_loop_host.py.
FD_EPS, FD_TOL, FD_MODEL_TOL = 2e-5, 1e-6, 1e-7
#: (first order, n) of the comparisons with the model: linearised and nonlinear plant
MAIN_CASES = ((1, 12), (2, 3))
NL_CASES = ((1, 6), (2, 3))
#: shapes that take every branch of fc_ctrl_adj_step / fc_ctrl_adj_grads: a static gain, one state, the shipped controller's 13, a
#: partial second pass over the state rows (65), the largest bank (256); one or two controller inputs; one output fanned out to both
#: actuators or one per actuator; each with and without signals and limits.  n = 3 (six control values: limits can clamp two and leave
#: two free), first step alternating between BDF1 and BDF2.
SHAPE_CASES = tuple(dict(nx=nx, nyc=nyc, nuc=nuc, signals=full, limits=full, n=3, first_order=1 + (i + nyc + nuc) % 2, seed=20 + i)
                    for i, nx in enumerate((0, 1, 13, 65, 256)) for nyc in (1, 2) for nuc in (1, 2) for full in (False, True))
#: the shortest runs.  n = 1 has two control values in all, so no limits can clamp two and leave two free: it runs without limits.
SHORT_CASES = (dict(nx=13, nyc=2, nuc=2, signals=True, limits=False, n=1, first_order=1, seed=71),
               dict(nx=13, nyc=2, nuc=2, signals=True, limits=False, n=1, first_order=2, seed=72),
               dict(nx=13, nyc=2, nuc=2, signals=True, limits=True, n=2, first_order=1, seed=73),
               dict(nx=13, nyc=2, nuc=2, signals=True, limits=True, n=2, first_order=2, seed=76))


def case_id(c):
    return f"nx{c['nx']}-nyc{c['nyc']}-nuc{c['nuc']}-{'full' if c['signals'] else 'bare'}-n{c['n']}-bdf{c['first_order']}"


def fd_direction(group, shape, seed=0, nn2=None):
    """The random direction of the central differences along ``group`` (one per group, fixed by its name).  The two time levels of a
    device state share one pressure, which no step reads: with ``nn2`` a state direction moves the 2 nn velocity entries only."""
    d = np.random.default_rng(seed + sum(map(ord, group))).standard_normal(shape)
    if nn2 is not None and group in ("dx0", "dxm1"):
        d[nn2:] = 0.0
    return d


def sensor_rows(th):
    return [th.point_eval_row(pt, comp) for pt, comp in SENSORS]


def sensor_matrix(th, rows):
    r = np.concatenate([np.full(len(row[0]), i) for i, row in enumerate(rows)])
    return sp.csr_matrix((np.concatenate([row[1] for row in rows]), (r, np.concatenate([row[0] for row in rows]))), shape=(len(rows), th.N))


def host_plant(nonlinear: bool):
    """(model, x0, xm1) from the oracle's operators: the device problems below without a device."""
    from oracle import ns_oracle as O
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from tests.support import adjoint_nl_model as nm
    from tests.support import adjoint_step_model as am

    nx, ny, amplitude = (7, 5, 1.0) if nonlinear else (8, 8, 0.1)
    th = TaylorHood(Mesh.unit_square(nx, ny))
    d = O.Disc.from_taylor_hood(th)
    U0, dofs, prof, _, u_n, u_nn, p = nm.square_inputs(th, amplitude)
    free = np.ones(th.N)
    free[dofs] = 0.0
    Zf, Zd = sp.diags(free), sp.diags(1.0 - free)
    raw, A = {}, {}
    for order, c in ((1, 1.0 / nm.DT), (2, 1.5 / nm.DT)):
        raw[order] = O.assemble_matrix(d, mass=c, nu=1.0 / nm.RE, adv=U0, lin=U0)
        A[order] = (Zf @ raw[order] @ Zf + Zd).tocsr()
    M = sp.block_diag([O.velocity_mass(d), sp.csr_matrix((th.nv, th.nv))]).tocsr()
    G = np.zeros((th.N, prof.shape[1]))
    G[dofs] = prof
    C = sensor_matrix(th, sensor_rows(th))
    args = (A[1], A[2], M, dofs, prof, raw[1] @ G, raw[2] @ G, C, nm.DT)
    model = nm.NonlinearStepModel(d, *args) if nonlinear else am.StepModel(*args)
    return model, np.r_[u_n, p], np.r_[u_nn, p]


class DevicePlant:
    """The device handle of ``Square`` / ``NlSquare`` with the two sensors, its model, and the adjoint setup of both slots."""

    def __init__(self, nonlinear: bool):
        from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
        from tests.support.adjoint_nl_child import NlSquare
        from tests.support.adjoint_step_child import Square

        self.nonlinear = nonlinear
        self.sq = sq = NlSquare() if nonlinear else Square()
        self.dev, self.th = sq.dev, sq.th
        rows = sensor_rows(sq.th)
        self.dev.set_sensors(rows)
        self.model = sq.model
        self.model.C = sensor_matrix(sq.th, rows)
        self.x0, self.xm1 = np.r_[sq.u_n, sq.p], np.r_[sq.u_nn, sq.p]
        for s in (SLOT_BDF1, SLOT_BDF2):
            self.dev.set_adjoint_factors(s, 1)

    def restart(self):
        self.sq.restart()

    def close(self):
        self.sq.close()


def make_case(model, x0, xm1, first_order, n, nx=3, nyc=2, nuc=2, signals=True, limits=True, seed=11, gain=1.0):
    """(Loop, w, r, z): bank, signals, limits and cost weights of one case.  The limits are symmetric and chosen from the model's own
    controls so that part of the control values is clamped and part is free."""
    rng = np.random.default_rng(seed)
    ns, na = model.C.shape[0], model.n_act
    bank = lm.random_bank(nx, nyc, nuc, ns, na, seed=seed + 1, gain=gain)
    y0 = np.asarray(model.C @ x0).reshape(ns)
    w_y = 0.2 * rng.standard_normal((n, nyc)) if signals else None
    w_u = 0.2 * rng.standard_normal((n, na)) if signals else None
    loop = lm.Loop(model, bank, first_order, n, x0, xm1, y0, w_y, w_u)
    if limits:
        # candidates: the geometric means of neighbouring magnitudes of the unlimited run's controls, tried from the middle outwards (a
        # clamp changes the later controls, so the first candidate need not serve); taken is the first that clamps at least two values,
        # leaves at least two free and keeps every free value 1e-2 of the limit away from it -- ten times what the tests demand
        mag = np.sort(np.abs(loop.forward()["v"]).ravel())
        for i in sorted(range(1, mag.size), key=lambda i: abs(i - mag.size / 2)):
            c = float(np.sqrt(mag[i - 1] * mag[i]))
            loop.lo, loop.hi = np.full(na, -c), np.full(na, c)
            clamped, free, dist = lm.limits_report(loop.forward()["v"], loop.lo, loop.hi)
            if clamped >= 2 and free >= 2 and dist >= 1e-2:
                break
        else:
            raise AssertionError(f"no symmetric limit clamps two and frees two control values (seed {seed})")
    w, r, z = rng.standard_normal((n, ns)), rng.standard_normal((n, na)), rng.standard_normal(model.N)
    return loop, w, r, z


def put_bank(dev, bank):
    """The bank onto the device as it is (``DeviceSolver.set_controllers`` packs Controller objects; a test wants generic matrices)."""
    from flowcontrol_amd._lib import check, ptr

    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    keep = [f(bank[k]) for k in ("Ad", "Bd", "C", "D", "x0", "G", "g0", "S")]
    check(dev.lib.fc_set_controllers(dev._h, 1, bank["nx"], bank["nyc"], bank["nuc"], *(ptr(a) for a in keep)))
    dev._ctrl_bank = bank


def put_loop(dev, loop):
    """Bank, signals and limits of ``loop`` onto the device (a loop tape, if reserved, follows the bank and is not begun)."""
    put_bank(dev, loop.bank)
    if loop.w_y is not None or loop.w_u is not None:
        dev.set_loop_signals(loop.w_y, loop.w_u)
    if loop.lo is not None:
        dev.set_control_limits(loop.lo, loop.hi)
