"""The per-column inputs of the batched adjoint march tests (tests/support/adjoint_batch_cases.py), on the scipy models alone: they tell
the batch-specific mistakes apart --

    one column's trajectory used for all columns,
    the weights of column s applied to column s + 1,
    the mean over the columns taken BEFORE the march instead of after it,

each of which misses the correct gradient by more than 1e-3 relative, while the correct per-column form meets 1e-7 against central
differences of the model's own forward run.  The nonlinear 7 x 5 square (N = 378) of tests/test_adjoint_nl_host.py, k = 3 columns."""
import numpy as np
import pytest

from tests.support import adjoint_batch_cases as bc
from tests.support import adjoint_nl_model as nm

CASES = [(1, 6), (2, 3)]
K = 3


@pytest.fixture(scope="module")
def square():
    model, th, (u_n, u_nn, p) = nm.host_square(7, 5)
    un, unn, pp = bc.column_states(u_n, u_nn, p, K)
    x0, xm1 = np.hstack([un, pp]), np.hstack([unn, pp])
    return model, x0, xm1


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"order{c[0]}-n{c[1]}")
def run(square, request):
    """The correct per-column run and march, computed once per case and shared (never modified)."""
    model, x0, xm1 = square
    first_order, n = request.param
    u, w, z = bc.column_inputs(n, K, model.n_act, model.C.shape[0], model.N)
    X, y = bc.model_forward_nl(model, first_order, u, x0, xm1)
    g, dx0, dxm1 = bc.model_adjoint_nl(model, first_order, X, w, z)
    return dict(model=model, x0=x0, xm1=xm1, first_order=first_order, n=n, u=u, w=w, z=z, X=X, y=y, g=g, dx0=dx0, dxm1=dxm1)


def test_the_columns_differ(run):
    """Initial states, controls, weights and terminal vectors differ from column to column by far more than any tolerance."""
    for name in ("x0", "xm1", "z"):
        a = run[name]
        assert min(bc.rel(a[s], a[t]) for s in range(K) for t in range(s)) > 1e-2, name
    for name in ("u", "w"):
        a = run[name]
        assert min(bc.rel(a[:, s], a[:, t]) for s in range(K) for t in range(s)) > 1e-1, name


def test_correct_form_is_the_derivative_of_every_column(run):
    """Per column: g_s . du + dx0_s . d0 + dxm1_s . dm1 against central differences of the model's forward run of that column at
    eps = 1e-4: <= 1e-7 relative."""
    model, fo = run["model"], run["first_order"]
    rng = np.random.default_rng(17)
    worst = 0.0
    for s in range(K):
        du, d0, dm1 = rng.standard_normal(run["u"][:, s].shape), rng.standard_normal(model.N), rng.standard_normal(model.N)
        args = (run["u"][:, s], run["x0"][s], run["xm1"][s])
        Jp = model.cost(fo, args[0] + bc.EPS * du, args[1] + bc.EPS * d0, args[2] + bc.EPS * dm1, run["w"][:, s], run["z"][s])
        Jm = model.cost(fo, args[0] - bc.EPS * du, args[1] - bc.EPS * d0, args[2] - bc.EPS * dm1, run["w"][:, s], run["z"][s])
        fd = (Jp - Jm) / (2 * bc.EPS)
        ad = float(np.sum(run["g"][:, s] * du) + run["dx0"][s] @ d0 + run["dxm1"][s] @ dm1)
        err = abs(fd - ad) / abs(fd)
        worst = max(worst, err)
        print(f"first order {fo}, n = {run['n']}, column {s}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.3e}")
    assert worst <= 1e-7


def test_one_trajectory_for_all_columns_is_told_apart(run):
    """Column 0's trajectory under every column's weights misses the gradient of each other column by more than 1e-3."""
    model, fo = run["model"], run["first_order"]
    for s in range(1, K):
        g, dx0, _, _ = model.adjoint(fo, run["X"][0], run["w"][:, s], run["z"][s])
        miss = min(bc.rel(g, run["g"][:, s]), bc.rel(dx0, run["dx0"][s]))
        print(f"first order {fo}, n = {run['n']}: trajectory of column 0 in column {s} misses by {miss:.3e}")
        assert miss > 1e-3


def test_shifted_weights_are_told_apart(run):
    """The weights (and terminal vector) of column s applied to column s + 1 miss every column's gradient by more than 1e-3."""
    model, fo = run["model"], run["first_order"]
    for s in range(K):
        t = (s + 1) % K
        g, dx0, _, _ = model.adjoint(fo, run["X"][t], run["w"][:, s], run["z"][s])
        miss = min(bc.rel(g, run["g"][:, t]), bc.rel(dx0, run["dx0"][t]))
        print(f"first order {fo}, n = {run['n']}: weights of column {s} on column {t} miss by {miss:.3e}")
        assert miss > 1e-3


def test_mean_before_the_march_is_told_apart(run):
    """The ensemble gradient is the column mean of the marches; one march on the mean trajectory with the mean weights misses it by more
    than 1e-3."""
    model, fo = run["model"], run["first_order"]
    right_g, right_dx0 = run["g"].mean(axis=1), run["dx0"].mean(axis=0)
    g, dx0, _, _ = model.adjoint(fo, run["X"].mean(axis=0), run["w"].mean(axis=1), run["z"].mean(axis=0))
    miss = min(bc.rel(g, right_g), bc.rel(dx0, right_dx0))
    print(f"first order {fo}, n = {run['n']}: the mean taken before the march misses by {miss:.3e}")
    assert miss > 1e-3
