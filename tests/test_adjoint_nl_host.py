"""The exact discrete adjoint of the NONLINEAR stepper on the host (tests/support/adjoint_nl_model.py, the model the device's
``fc_run_adjoint`` on a taped run is compared with): the Jacobian of the convective term, the gradient as the derivative of the
forward run, and the three mistakes the inputs tell apart.

The 7 x 5 square (N = 378) with the BC set, sensor and smooth states of tests/support/adjoint_step_child.py at amplitude 1,
dt = 0.005, Re = 100."""
import numpy as np
import pytest

from tests.support import adjoint_nl_model as nm

#: (first order, n): a BDF1 start, and the shortest BDF2 run in which both coefficient pairs act on both state gradients
CASES = [(1, 6), (2, 3)]


@pytest.fixture(scope="module")
def square():
    model, th, (u_n, u_nn, p) = nm.host_square(7, 5)
    assert model.N == 378
    return model, np.r_[u_n, p], np.r_[u_nn, p]


def _inputs(model, n, seed=5):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, model.n_act))
    w = rng.standard_normal((n, model.C.shape[0]))
    z = rng.standard_normal(model.N)
    return u, w, z


def test_jacobian_is_the_derivative_of_the_convective_term(square):
    """J(x) d against central differences of N (N is quadratic: no truncation error, round-off only): <= 1e-9 relative."""
    model, x0, _ = square
    J = model.jac(x0)
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(3):
        d = rng.standard_normal(model.N)
        eps = 1e-4
        fd = (model.conv(x0 + eps * d) - model.conv(x0 - eps * d)) / (2 * eps)
        worst = max(worst, nm.rel(J @ d, fd))
    print(f"J d against central differences of N: {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("first_order,n", CASES)
def test_gradient_is_the_derivative_of_the_forward_run(square, first_order, n):
    """g . du + dx0 . d0 + dxm1 . dm1 against central differences of the model forward run at eps = 1e-4 in three random directions:
    <= 1e-8 relative."""
    model, x0, xm1 = square
    u, w, z = _inputs(model, n)
    X, _ = model.forward(first_order, u, x0, xm1)
    g, dx0, dxm1, _ = model.adjoint(first_order, X, w, z)
    if first_order == 1:
        assert not dxm1.any()  # a BDF1 first step never reads x_{-1}
    else:
        assert dxm1.any()
    rng = np.random.default_rng(9)
    eps, worst = 1e-4, 0.0
    for k in range(3):
        du, d0, dm1 = rng.standard_normal(u.shape), rng.standard_normal(model.N), rng.standard_normal(model.N)
        Jp = model.cost(first_order, u + eps * du, x0 + eps * d0, xm1 + eps * dm1, w, z)
        Jm = model.cost(first_order, u - eps * du, x0 - eps * d0, xm1 - eps * dm1, w, z)
        fd = (Jp - Jm) / (2 * eps)
        ad = float(np.sum(g * du) + dx0 @ d0 + dxm1 @ dm1)
        err = abs(fd - ad) / abs(fd)
        worst = max(worst, err)
        print(f"first order {first_order}, n = {n}, direction {k}: central difference {fd:.12e}, adjoint {ad:.12e}, relative {err:.3e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("first_order,n", CASES)
def test_the_inputs_tell_the_mistakes_apart(square, first_order, n):
    """The linear adjoint, J taken at x_{m+1}, and the Dirichlet mask on the output of J^T each miss g by more than 1e-4 relative."""
    model, x0, xm1 = square
    u, w, z = _inputs(model, n)
    X, _ = model.forward(first_order, u, x0, xm1)
    g = model.adjoint(first_order, X, w, z)[0]
    for wrong in ("linear", "J_next", "mask_out"):
        miss = nm.rel(model.adjoint(first_order, X, w, z, wrong=wrong)[0], g)
        print(f"first order {first_order}, n = {n}: {wrong} misses g by {miss:.3e}")
        assert miss > 1e-4
