"""The tangents of k lock-step closed loops on the MI355X (``fc_run_tangent_closed_loop_batch``; csrc/fc_tangent_loop.hip.h,
csrc/fc_tangent_loop_run.hpp) against the numpy model of tests/support/tangent_loop_model.py run once per column and against the
device's own single closed-loop tangent.  The columns are those of tests/test_adjoint_loop_batch_gpu.py
(tests/support/adjoint_loop_batch_cases.py): every column has its own initial state, bank, signals and limits; k = 3 and 5, so padding
columns exist at the padded widths 4 and 8."""
import numpy as np
import pytest

from flowcontrol_amd import _lib
from flowcontrol_amd._lib import SLOT_BDF1, FcDiverged
from tests.support import adjoint_loop_batch_cases as lbc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import tangent_loop_model as tm
from tests.test_adjoint_loop_batch_gpu import CAPACITY, TOL, forward, main_columns, refused, slot_of, use_batch

pytestmark = pytest.mark.gpu

INV = _lib.FC_ERR_INVALID
OUT = ("dy", "du", "xi", "dxn", "dxnm1")
BY_STEP = ("dy", "du", "w_y", "w_u")
LOOP_KEYS = ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u")


@pytest.fixture(scope="module")
def plant():
    p = lc.DevicePlant(False)
    yield p
    p.close()


@pytest.fixture(scope="module")
def nl_plant():
    p = lc.DevicePlant(True)
    yield p
    p.close()


def ready(p, k):
    """A batch of k on the plant's handle (0: the single mode) with the tangent buffers of that mode."""
    if k:
        use_batch(p, k)
    elif p.dev.batch_k:
        p.dev.adjoint_loop_reserve_batch(0)
        p.dev.set_controllers(None, p.sq.dt)
        p.dev.set_batch(0)
    if not p.dev.tangent_info()["reserved"]:
        p.dev.tangent_reserve(1)


def column_directions(p, cols):
    """[(model forward, directions)] per column: every group moved, column s with its own seed."""
    out = []
    for s, (loop, w, r, z) in enumerate(cols):
        f = loop.forward()
        out.append((f, tm.directions(loop.adjoint(f, w, r, z), seed=5 + s, nn2=2 * p.th.nn)))
    return out


def march(p, cols, ds, ref_col=None):
    direction = {key: np.stack([d[key] for d in ds], axis=1 if key in BY_STEP else 0) for key in LOOP_KEYS}
    loop = cols[0][0]
    return p.dev.run_tangent_closed_loop_batch(slot_of(loop.first_order), loop.n, direction, np.array([d["dx0"] for d in ds]), np.array([d["dxm1"] for d in ds]),
                                               ref_col=ref_col)


def column(t, key, s):
    return t[key][:, s] if key in BY_STEP else t[key][s]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in OUT)


def column_against(t, s, ref, label):
    errs = {k: lm.rel(column(t, k, s), ref[k]) for k in OUT}
    print(f"{label}, column {s}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    for k, v in errs.items():
        assert v <= TOL, f"{label}, column {s}: {k}: {v:.3e} > {TOL:.1e}"


def against_model(p, cols, label):
    fd = column_directions(p, cols)
    _, u, bad = forward(p, [c[0] for c in cols])
    assert np.all(bad == -1)
    t = march(p, cols, [d for _, d in fd])
    for s, ((loop, *_), (f, d)) in enumerate(zip(cols, fd)):
        column_against(t, s, tm.tangent(loop, f, d), label)
        if loop.lo is not None:
            at_limit = (u[:, s] == loop.lo) | (u[:, s] == loop.hi)
            assert np.array_equal(t["du"][:, s] == 0.0, at_limit), (s, t["du"][:, s], at_limit)
    return t, fd


@pytest.mark.parametrize("k,first_order,n", lbc.MAIN_CASES)
def test_columns_against_the_model(plant, k, first_order, n):
    """Every column within 1e-8 of that column's model on the linearised plant; du is exactly 0 where that column's control sits at a
    limit; two marches are bit-identical."""
    ready(plant, k)
    cols = main_columns(plant, k, first_order, n)
    t, fd = against_model(plant, cols, f"batched closed-loop tangent, k = {k}, first order {first_order}, n = {n}")
    assert same(t, march(plant, cols, [d for _, d in fd])), "two identical marches differ"


@pytest.mark.parametrize("k,first_order,n", lbc.NL_CASES)
def test_nonlinear_plant_against_the_model(nl_plant, k, first_order, n):
    """The nonlinear 7 x 5 square: the march reads the batched state tape the closed-loop run advanced."""
    ready(nl_plant, k)
    cols = main_columns(nl_plant, k, first_order, n)
    t, fd = against_model(nl_plant, cols, f"nonlinear plant, k = {k}, first order {first_order}, n = {n}")
    assert same(t, march(nl_plant, cols, [d for _, d in fd])), "two identical marches differ"


@pytest.mark.parametrize("case", lbc.SHAPE_CASES, ids=lc.case_id)
def test_shapes(plant, case):
    """Every branch of the kernel at k = 3: nx = 0, 1, 13, 65, 256; nyc 1, 2; nuc fanned out and per actuator; with and without signals
    and limits; n = 1, 2, 3."""
    ready(plant, lbc.SHAPE_K)
    against_model(plant, lbc.shape_columns(plant.model, plant.x0, plant.xm1, 2 * plant.th.nn, case), lc.case_id(case))


@pytest.mark.parametrize("nonlinear,k,first_order,n", [(False, *c) for c in lbc.MAIN_CASES] + [(True, *c) for c in lbc.NL_CASES])
def test_columns_against_the_single_march(plant, nl_plant, nonlinear, k, first_order, n):
    """Each column of every main case (linearised plant) and nonlinear case, k = 3 and 5, against the device's own single closed-loop
    tangent of that column's loop, and with ref_col = 1 column s against the single march of loop 1 along direction s: 1e-8 (the
    controller's sums are the same in both; the batched factor apply and the single refined solve are different sums)."""
    p = nl_plant if nonlinear else plant
    dev, nn2 = p.dev, 2 * p.th.nn
    ready(p, k)
    cols = main_columns(p, k, first_order, n)
    ds = [d for _, d in column_directions(p, cols)]
    forward(p, [c[0] for c in cols])
    t, t_ref = march(p, cols, ds), march(p, cols, ds, ref_col=1)
    assert not same(t, t_ref)
    ready(p, 0)
    if nonlinear:
        dev.adjoint_tape_reserve(CAPACITY)
    try:
        for s in range(k):
            for about, got, label in ((s, t, "against the single march"), (1, t_ref, "ref_col = 1 against the single march of loop 1")):
                loop = cols[about][0]
                dev.set_state(loop.x0[:nn2], loop.xm1[:nn2], loop.x0[nn2:])
                lc.put_loop(dev, loop)
                dev.adjoint_loop_reserve(CAPACITY)
                if nonlinear:
                    dev.adjoint_tape_begin()
                dev.adjoint_loop_begin()
                dev.run_closed_loop(slot_of(first_order), n, loop.y0, compute_energy=False)
                single = dev.run_tangent_closed_loop(slot_of(first_order), n, {key: ds[s][key] for key in LOOP_KEYS}, ds[s]["dx0"], ds[s]["dxm1"])
                column_against(got, s, single, label)
    finally:
        dev.adjoint_loop_reserve(0)
        dev.set_controllers(None, p.sq.dt)
        if nonlinear:
            dev.adjoint_tape_reserve(0)


def test_refusals_of_the_batched_march(plant):
    """ref_col outside [-1, k), a Krylov method on the slots (the batched marches go through batch_ready, not tan_slot_ready) and a
    bank whose k is not the call's: FC_ERR_INVALID with the reason, nothing enqueued; the march in between returns the same bits."""
    dev = plant.dev
    ready(plant, 3)
    cols = main_columns(plant, 3, 1, 6)
    ds = [d for _, d in column_directions(plant, cols)]
    forward(plant, [c[0] for c in cols])
    ref = march(plant, cols, ds)
    marches = dev.tangent_info()["marches"]
    refused(INV, dev.run_tangent_closed_loop_batch, SLOT_BDF1, 6, None, None, None, 3, match="ref_col")
    # what the batched steps refuse on the slots of the run (batch_ready): a Krylov method
    dev.set_solver_options(refine=30, method="gmres")
    try:
        refused(INV, dev.run_tangent_closed_loop_batch, SLOT_BDF1, 6, match="apply the factors directly")
    finally:
        dev.set_solver_options(refine=0, check_residual=1)  # (tests/support/adjoint_batch_cases.batch_on's options)
    assert dev.tangent_info()["marches"] == marches
    forward(plant, [c[0] for c in cols])
    assert same(ref, march(plant, cols, ds))
    marches += 1
    lbc.put_bank(dev, lbc.stack_bank([c[0] for c in cols[:2]]))
    refused(INV, dev.run_tangent_closed_loop_batch, SLOT_BDF1, 6, match="k differs")
    assert dev.tangent_info()["marches"] == marches


def test_a_non_finite_column_stays_alone(plant):
    """Column 1 starts from an inf in a free velocity dof: flags mark column 1 only, its outputs are NaN, columns 0 and 2 match their
    models; the next march of the three columns is clean again."""
    dev, nn2 = plant.dev, 2 * plant.th.nn
    ready(plant, 3)
    cols = main_columns(plant, 3, 1, 6)
    fd = column_directions(plant, cols)
    ds = [d for _, d in fd]
    loops = [c[0].clone() for c in cols]
    loops[1].x0[np.flatnonzero(plant.model.free[:nn2])[40]] = np.inf  # (a free velocity dof: the mass term carries it into the right-hand side)
    _, _, bad = forward(plant, loops)
    assert bad[1] >= 0 and bad[0] == -1 and bad[2] == -1, bad
    with pytest.raises(FcDiverged):
        march(plant, cols, ds)
    assert dev.tangent_batch_flags.tolist() == [0, 1, 0]
    t = dev.tangent_loop_batch_last
    for key in OUT:
        assert np.all(np.isnan(column(t, key, 1))), key
    for s in (0, 2):
        column_against(t, s, tm.tangent(cols[s][0], fd[s][0], ds[s]), "beside a non-finite column")
    forward(plant, [c[0] for c in cols])
    march(plant, cols, ds)
    assert not np.any(dev.tangent_batch_flags)
