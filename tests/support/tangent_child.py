"""The comparison of the device's single tangent march (``fc_run_tangent``) with the scipy model of tests/support/tangent_model.py on
the nonlinear 7 x 5 square of tests/support/adjoint_nl_child.py (``NlSquare``: 70 cells, so the last workgroup of the eight-lane
element kernel is partial), and the child process of tests/test_tangent_gpu.py:

    python tangent_child.py reg            the comparison in this process's environment (FC_ELEM_REG_MIN=1: the thread-per-cell kernel)
    python tangent_child.py partitioned    the refusals of a handle with an exchange (fc_set_host_exchange)

Prints CHILD OK <mode> at the end; exits non-zero with the failed assertion."""
import sys

import numpy as np

from tests.support import adjoint_nl_model as nm
from tests.support.adjoint_nl_child import EPS, TOL, TOL_FD, NlSquare
from tests.support.tangent_model import TangentModel

#: (first order, n): the short ones catch the horizon gating and the read of x_{-1}
CASES = [(1, 6), (2, 3), (1, 1), (2, 1), (1, 2), (2, 2)]
#: which of (du, dx0, dxm1) are given; the others are NULL
GIVEN = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]


def taped_run(sq, first_order, n, u):
    """The device forward run of n steps from the square's start, taped: (X [n + 2, N] from the tape, y)."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    sq.restart()
    sq.dev.adjoint_tape_begin()
    y, _ = sq.dev.run(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n, u, compute_energy=False)
    return sq.dev.adjoint_tape_states(), y


def compare_tangent(sq, first_order, n, route, seed=9, label=""):
    """A taped device run and its tangent (a tape of at least n steps and the tangent buffers must be reserved) against the model, each
    of du, dx0, dxm1 given and NULL in turn, and against central differences of the device's own forward run; returns the figures.
    Asserts TOL / TOL_FD, bit-identical repeats and the element-kernel route."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    dev, tm = sq.dev, TangentModel(sq.model)
    nn2 = 2 * sq.th.nn
    slot = SLOT_BDF1 if first_order == 1 else SLOT_BDF2
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, dev.n_act))
    du, d0, dm1 = rng.standard_normal((n, dev.n_act)), rng.standard_normal(dev.N), rng.standard_normal(dev.N)
    X, _ = taped_run(sq, first_order, n, u)
    marches0 = dev.tangent_info()["marches"]
    out = {}
    for gu, g0, gm in GIVEN:
        args = (du if gu else None, d0 if g0 else None, dm1 if gm else None)
        dy, dxn, dxnm1 = dev.run_tangent(slot, n, *args)
        again = dev.run_tangent(slot, n, *args)
        assert all(np.array_equal(a, b) for a, b in zip((dy, dxn, dxnm1), again)), "two identical tangent marches differ"
        D, dym = tm.tangent(first_order, X, *args)
        tag = "".join(c for c, g in zip("u01", (gu, g0, gm)) if g)
        if gm and not gu and not g0 and first_order == 1:  # a BDF1 first step never reads dx_{-1}, and no later step does: exact zeros
            assert not np.any(dy) and not np.any(dxn) and not np.any(dxnm1) and not np.any(D[2:])
            continue
        out[f"dy[{tag}]"], out[f"dxn[{tag}]"] = nm.rel(dy, dym), nm.rel(dxn, D[-1])
        if np.any(D[-2][:nn2]):
            out[f"dxnm1[{tag}]"] = nm.rel(dxnm1[:nn2], D[-2][:nn2])  # (n = 1: dx_0 itself, whose pressure rows are the caller's)
        else:
            assert not np.any(dxnm1[:nn2])
    info = dev.tangent_info()
    assert info["route"] == route and info["steps"] == n and info["marches"] == marches0 + 2 * len(GIVEN) and info["run_ms"] > 0.0, info
    # the derivative of the DEVICE forward run in the same direction (controls and both velocity levels)
    dy, dxn, _ = dev.run_tangent(slot, n, du, d0, dm1)

    def run(sign):
        dev.set_state(sq.u_n + sign * EPS * d0[:nn2], sq.u_nn + sign * EPS * dm1[:nn2], sq.p)
        yy, _ = dev.run(slot, n, u + sign * EPS * du, compute_energy=False)
        return yy, dev.get_solution()

    (yp, xp), (ym, xm) = run(1.0), run(-1.0)
    fd_y, fd_x = nm.rel(dy, (yp - ym) / (2 * EPS)), nm.rel(dxn, (xp - xm) / (2 * EPS))
    sq.restart()
    print(f"tangent run {label}first order {first_order}, n = {n}: " + ", ".join(f"{k} {v:.3e}" for k, v in out.items()) +
          f", device central difference y {fd_y:.3e}, x_n {fd_x:.3e}", flush=True)
    for k, v in out.items():
        assert v <= TOL, f"{k}: {v:.3e} > {TOL:.1e}"
    assert fd_y <= TOL_FD and fd_x <= TOL_FD, f"central difference of the device run: y {fd_y:.3e}, x_n {fd_x:.3e} > {TOL_FD:.1e}"
    out["fd_y"], out["fd_x"] = fd_y, fd_x
    return out


def main(mode: str) -> None:
    if mode == "reg":
        import os

        assert os.environ.get("FC_ELEM_REG_MIN") == "1"
        sq = NlSquare()
        try:
            sq.dev.adjoint_tape_reserve(6)
            sq.dev.tangent_reserve(1)
            for first_order, n in CASES:
                compare_tangent(sq, first_order, n, route=2, label="(thread per cell) ")
        finally:
            sq.close()
    elif mode == "partitioned":
        from flowcontrol_amd import _lib
        from flowcontrol_amd._lib import SLOT_BDF2
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood

        dev = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
        try:
            fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
            _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
            calls = {"fc_tangent_reserve": lambda: dev.lib.fc_tangent_reserve(dev._h, 1),
                     "fc_run_tangent": lambda: dev.lib.fc_run_tangent(dev._h, SLOT_BDF2, 2, None, None, None, None, None, None),
                     "fc_run_tangent_batch": lambda: dev.lib.fc_run_tangent_batch(dev._h, SLOT_BDF2, 4, 2, -1, None, None, None, None, None, None, None)}
            for name, call in calls.items():
                code, msg = call(), dev.lib.fc_last_error().decode()
                assert code == _lib.FC_ERR_INVALID and name in msg and "partitioned" in msg, (name, code, msg)
            assert not dev.tangent_info()["reserved"] and dev.tangent_info()["bytes"] == 0
        finally:
            dev.close()
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    print("CHILD OK", mode, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
