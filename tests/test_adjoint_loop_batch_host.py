"""The inputs of tests/test_adjoint_loop_batch_gpu.py, checked without a GPU on the scipy model of tests/support/adjoint_loop_model.py:
every column of every case clamps part of its controls and keeps the free ones away from the limits, the model alone meets
``FD_MODEL_TOL`` against central differences of its own forward run with those inputs, and the columns tell mistakes apart -- a column
that read its neighbour's bank, signals or weights would move every gradient group by far more than the GPU tests' tolerance."""
import numpy as np
import pytest

from tests.support import adjoint_loop_batch_cases as lbc
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm


@pytest.fixture(scope="module")
def plants():
    return {nl: (*lc.host_plant(nl), lbc.velocity_dofs(nl)) for nl in (False, True)}


def main_columns(plants, nonlinear, k, first_order, n):
    model, x0, xm1, nn2 = plants[nonlinear]
    return lbc.columns(model, x0, xm1, nn2, k, first_order, n)


@pytest.mark.parametrize("nonlinear,k,first_order,n", [(False, *c) for c in lbc.MAIN_CASES] + [(True, *c) for c in lbc.NL_CASES])
def test_every_column_clamps_and_frees(plants, nonlinear, k, first_order, n):
    """Every column's limits clamp at least two and free at least two control values, and every free value stays 1.3e-2 of the limit
    away from it (make_case raises if it finds no such limit)."""
    for loop, _, _, _ in main_columns(plants, nonlinear, k, first_order, n):
        lbc.assert_limits_tell(loop)


@pytest.mark.parametrize("case", [c for c in lbc.SHAPE_CASES if c["limits"]], ids=lc.case_id)
def test_every_column_of_the_shape_cases_clamps_and_frees(plants, case):
    model, x0, xm1, nn2 = plants[False]
    for loop, _, _, _ in lbc.shape_columns(model, x0, xm1, nn2, case):
        lbc.assert_limits_tell(loop)


@pytest.mark.parametrize("nonlinear,k,first_order,n", [(False, 3, 1, 12), (False, 5, 2, 3), (True, 3, 1, 6), (True, 5, 2, 3)])
def test_model_gradients_meet_central_differences(plants, nonlinear, k, first_order, n):
    """The model's adjoint against central differences of the model's forward run, per column, along the direction and at the step the
    GPU test uses: FD_MODEL_TOL."""
    nn2 = plants[nonlinear][3]
    for s, (loop, w, r, z) in enumerate(main_columns(plants, nonlinear, k, first_order, n)):
        g = loop.adjoint(loop.forward(), w, r, z)
        for grp in lm.GROUPS:
            if not np.any(g[grp]):
                continue
            d = lc.fd_direction(grp, g[grp].shape, seed=s, nn2=nn2)
            fd = loop.fd_directional(grp, d, lc.FD_EPS, w, r, z)
            ad = float(np.sum(g[grp] * d))
            assert abs(fd - ad) <= lc.FD_MODEL_TOL * abs(fd), (s, grp, fd, ad)


@pytest.mark.parametrize("nonlinear,first_order,n", [(False, 1, 12), (True, 1, 6)])
def test_the_columns_tell_mistakes_apart(plants, nonlinear, first_order, n):
    """Column s with the bank, the signals or the weights of column s + 1 moves every gradient group by more than 1e-3 relative."""
    cols = main_columns(plants, nonlinear, 3, first_order, n)
    for s in range(3):
        loop, w, r, z = cols[s]
        other, w2, r2, z2 = cols[(s + 1) % 3]
        ref = loop.adjoint(loop.forward(), w, r, z)
        wrong_bank = loop.clone()
        wrong_bank.bank = lm.copy_bank(other.bank)
        wrong_signals = loop.clone()
        wrong_signals.w_y, wrong_signals.w_u = other.w_y.copy(), other.w_u.copy()
        for label, q, args in (("bank", wrong_bank, (w, r, z)), ("signals", wrong_signals, (w, r, z)), ("weights", loop, (w2, r2, z2))):
            g = q.adjoint(q.forward(), *args)
            for grp in lm.GROUPS:
                if not np.any(ref[grp]):
                    continue
                assert lm.rel(g[grp], ref[grp]) > 1e-3, (s, label, grp, lm.rel(g[grp], ref[grp]))
