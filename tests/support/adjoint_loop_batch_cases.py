"""The batched closed-loop problems of tests/test_adjoint_loop_batch_host.py and tests/test_adjoint_loop_batch_gpu.py -- TEST
INFRASTRUCTURE.  One ``adjoint_loop_model.Loop`` per column of the batch: column s starts from the plant's state scaled by
1 + 0.5 s / k plus its own noise (``adjoint_batch_cases.column_states``) and gets its own bank, signals, limits and cost weights from
``adjoint_loop_cases.make_case(..., seed=11 + 100 s)`` (a shape case: its own seed + 100 s), so every column has its own clamp pattern
and a column that read a neighbour's bank, signals or weights would be found out (the host test shows that on the model)."""
from __future__ import annotations

import numpy as np

from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm

#: (k, first order, n) of the comparisons with the model: neither k is a padded width, so padding columns exist
MAIN_CASES = tuple((k, fo, n) for k in (3, 5) for fo, n in lc.MAIN_CASES)
NL_CASES = tuple((k, fo, n) for k in (3, 5) for fo, n in lc.NL_CASES)
#: the shapes of the single march's tests at k = 3
SHAPE_K = 3
SHAPE_CASES = lc.SHAPE_CASES + lc.SHORT_CASES
#: every free control value stays this far (relative to the limit) from its limit
FREE_DISTANCE = 1.3e-2
BANK_KEYS = ("Ad", "Bd", "C", "D", "x0", "G", "g0", "S")


def velocity_dofs(nonlinear: bool) -> int:
    """2 nn of the plant's mesh (the state is [u (2 nn) | p (nv)])."""
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    return 2 * TaylorHood(Mesh.unit_square(*((7, 5) if nonlinear else (8, 8)))).nn


def _limits_at_distance(loop):
    """``make_case``'s own search for a symmetric limit -- the geometric means of neighbouring control magnitudes, from the middle
    outwards -- with FREE_DISTANCE in place of its 1e-2: ``make_case`` promises 1e-2, these tests ask 1.3e-2 of every column, and two
    columns of the k = 5 cases land in between.  False if no candidate serves."""
    free = loop.clone()
    free.lo = free.hi = None
    mag = np.sort(np.abs(free.forward()["v"]).ravel())
    na = loop.plant.n_act
    for i in sorted(range(1, mag.size), key=lambda i: abs(i - mag.size / 2)):
        c = float(np.sqrt(mag[i - 1] * mag[i]))
        loop.lo, loop.hi = np.full(na, -c), np.full(na, c)
        clamped, freed, dist = lm.limits_report(loop.forward()["v"], loop.lo, loop.hi)
        if clamped >= 2 and freed >= 2 and dist >= FREE_DISTANCE:
            return True
    return False


def columns(model, x0, xm1, nn2, k, first_order, n, seed=11, **shape):
    """[(Loop, w, r, z)] for the k columns.  Column s takes seed + 100 s; where that seed admits no limit that clamps two and frees two
    control values at FREE_DISTANCE (n = 2 has four control values in all), the next of seed + 100 s + 1000 j that does."""
    un, unn, pp = bc.column_states(x0[:nn2], xm1[:nn2], x0[nn2:], k)
    out = []
    for s in range(k):
        for j in range(8):
            try:
                case = lc.make_case(model, np.r_[un[s], pp[s]], np.r_[unn[s], pp[s]], first_order, n, seed=seed + 100 * s + 1000 * j, **shape)
            except AssertionError:
                continue
            loop = case[0]
            if loop.lo is None or lm.limits_report(loop.forward()["v"], loop.lo, loop.hi)[2] >= FREE_DISTANCE or _limits_at_distance(loop):
                break
        else:
            raise AssertionError(f"column {s}: no seed of 8 admits limits that clamp two and free two control values (seed {seed})")
        out.append(case)
    return out


def shape_columns(model, x0, xm1, nn2, case, k=SHAPE_K):
    c = dict(case)
    return columns(model, x0, xm1, nn2, k, c.pop("first_order"), c.pop("n"), seed=c.pop("seed"), **c)


def stack_bank(loops):
    """The banks of the columns as one bank of k (the layout of ``pack_controllers``)."""
    b0 = loops[0].bank
    bank = {"k": len(loops), "nx": b0["nx"], "nyc": b0["nyc"], "nuc": b0["nuc"], "sizes": [q.bank["sizes"][0] for q in loops]}
    for key in BANK_KEYS:
        bank[key] = np.concatenate([q.bank[key] for q in loops])
    return bank


def stack_inputs(cols):
    """(w [n, k, n_sens], r [n, k, n_act], z [k, N])."""
    return np.stack([c[1] for c in cols], axis=1), np.stack([c[2] for c in cols], axis=1), np.array([c[3] for c in cols])


def put_bank(dev, bank):
    """A bank of k onto the device as it is."""
    from flowcontrol_amd._lib import check, ptr

    keep = [np.ascontiguousarray(bank[key], dtype=np.float64) for key in BANK_KEYS]
    check(dev.lib.fc_set_controllers(dev._h, bank["k"], bank["nx"], bank["nyc"], bank["nuc"], *(ptr(a) for a in keep)))
    dev._ctrl_bank = bank


def put_loops(dev, loops, nn2):
    """Initial states, bank, signals and limits of the columns onto the device's batch."""
    dev.set_state_batch(np.array([q.x0[:nn2] for q in loops]), np.array([q.xm1[:nn2] for q in loops]), np.array([q.x0[nn2:] for q in loops]))
    put_bank(dev, stack_bank(loops))
    if loops[0].w_y is not None or loops[0].w_u is not None:
        dev.set_loop_signals(None if loops[0].w_y is None else np.stack([q.w_y for q in loops], axis=1),
                             None if loops[0].w_u is None else np.stack([q.w_u for q in loops], axis=1))
    if loops[0].lo is not None:
        dev.set_control_limits(np.array([q.lo for q in loops]), np.array([q.hi for q in loops]))


def assert_limits_tell(loop):
    """At least two control values clamped, at least two free, every free one FREE_DISTANCE of the limit away from it."""
    clamped, free, dist = lm.limits_report(loop.forward()["v"], loop.lo, loop.hi)
    assert clamped >= 2 and free >= 2, (clamped, free)
    assert dist >= FREE_DISTANCE, dist
