"""The exact discrete adjoint of the linearised stepper on the host (tests/support/adjoint_step_model.py, the model the device's
``fc_run_adjoint`` is compared with): its dot-product identity, the two classic mistakes the identity catches, and the layout rule
that makes the stepping handle's sweeps solve with A^T."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import TaylorHood
from tests.support import adjoint_layout, nd_numeric, ndsolver
from tests.support import adjoint_step_model as am


def _inputs(model, n, seed=3):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, model.n_act))  # non-zero controls on the Dirichlet actuators
    x0, xm1 = rng.standard_normal(model.N), rng.standard_normal(model.N)
    w = rng.standard_normal((n, model.C.shape[0]))
    z = rng.standard_normal(model.N)
    return u, x0, xm1, w, z


def _defect(model, first_order, n, wrong=None):
    u, x0, xm1, w, z = _inputs(model, n)
    X, y = model.forward(first_order, u, x0, xm1)
    g, dx0, dxm1, _ = model.adjoint(first_order, n, w, z, wrong=wrong)
    return model.dot_defect(*am.identity_terms(w, y, z, X[-1], u, g, x0, dx0, xm1, dxm1))


@pytest.mark.parametrize("first_order,n", [(1, 12), (2, 3), (1, 1), (2, 1), (1, 2)])
def test_dot_product_identity_of_the_model(first_order, n):
    """sum w . y + z . x_n = sum u . g + x0 . dx0 + xm1 . dxm1 to round-off: 1e-12 of the sum of absolute terms (the solves are
    LU-accurate, cond ~ 1e2, a dozen steps)."""
    model, _ = am.random_problem()
    d = _defect(model, first_order, n)
    print(f"first order {first_order}, n = {n}: defect {d:.3e}")
    assert d <= 1e-12


def test_the_identity_tells_the_two_mistakes_apart():
    """Z M in place of M Z, or BDF2's coefficients on the BDF1 step: the same inputs miss the identity by many orders of magnitude."""
    model, _ = am.random_problem()
    ok = _defect(model, 1, 12)
    zm = _defect(model, 1, 12, wrong="ZM")
    cf = _defect(model, 1, 12, wrong="bdf2_on_first")
    print(f"defect: exact {ok:.3e}, Z M {zm:.3e}, BDF2 coefficients on the first step {cf:.3e}")
    assert ok <= 1e-12
    assert zm >= 1e-6 and cf >= 1e-6
    # ... and with a BDF2 start the coefficient mistake is no mistake: the check above is about the BDF1 step
    assert _defect(model, 2, 3, wrong="bdf2_on_first") <= 1e-12


def test_gradient_is_the_derivative_of_the_forward_run():
    """J is linear in (u, x0, xm1): one forward run per unit direction reproduces entries of g, dx0 and dxm1."""
    model, _ = am.random_problem()
    n = 4
    u, x0, xm1, w, z = _inputs(model, n)
    g, dx0, dxm1, _ = model.adjoint(1, n, w, z)

    def J(u_, x0_, xm1_):
        X, y = model.forward(1, u_, x0_, xm1_)
        return float(np.sum(w * y) + z @ X[-1])

    zero_u, zero_x = np.zeros_like(u), np.zeros(model.N)
    for (m, k) in [(0, 0), (1, 1), (3, 0)]:
        e = zero_u.copy()
        e[m, k] = 1.0
        assert abs(J(e, zero_x, zero_x) - g[m, k]) <= 1e-10 * max(1.0, abs(g[m, k]))
    for i in (0, model.N // 3, model.N - 1):
        e = zero_x.copy()
        e[i] = 1.0
        assert abs(J(zero_u, e, zero_x) - dx0[i]) <= 1e-10 * max(1.0, abs(dx0[i]))
        assert abs(J(zero_u, zero_x, e) - dxm1[i]) <= 1e-10 * max(1.0, abs(dxm1[i]))
    assert not dxm1.any()  # a BDF1 first step never reads x_{-1}


def test_transposed_values_solve_the_transposed_system_on_the_square_plan():
    """The real (non-doubled) plan of the 8 x 8 square, an unsymmetric matrix on the Taylor-Hood pattern: block_solve on
    transpose_values(numeric factor values) is scipy's solve with A^T to the specification's own accuracy (1e-12, as the direct solve),
    and not the direct solve."""
    th = TaylorHood(Mesh.unit_square(8, 8))
    N = th.N
    cd = np.asarray(th.cell_dofs)
    tree = ndsolver.build_tree(cd, th.mesh.cell_centroids(), N, 4)
    rows, cols = np.repeat(cd, cd.shape[1], axis=1).ravel(), np.tile(cd, (1, cd.shape[1])).ravel()
    P = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(N, N))
    P.sum_duplicates()
    rng = np.random.default_rng(8)
    A = P.copy()
    A.data = rng.standard_normal(A.nnz)
    A = (A + sp.diags(np.full(N, 40.0))).tocsr()
    fac = nd_numeric.factorize_blocks(A, tree)
    shapes = adjoint_layout.node_shapes(fac.nodes, "block")
    assert any(ni % 32 for ni, _, _ in shapes) and any(nb > 32 for _, nb, _ in shapes)
    b = rng.standard_normal(N)
    rel = lambda x, ref: np.linalg.norm(x - ref) / np.linalg.norm(ref)  # noqa: E731
    direct = fac.vals.copy()
    e_direct = rel(nd_numeric.block_solve(fac, b), spla.spsolve(A.tocsc(), b))
    fac.vals = adjoint_layout.transpose_values(direct, fac.nodes, "block")
    xt = nd_numeric.block_solve(fac, b)
    e_t = rel(xt, spla.spsolve(A.T.tocsc(), b))
    print(f"square 8 x 8: direct error {e_direct:.3e}, transposed error {e_t:.3e}")
    assert e_direct <= 1e-12 and e_t <= 1e-12
    assert rel(xt, spla.spsolve(A.tocsc(), b)) > 1e-3
    assert np.array_equal(adjoint_layout.transpose_values(fac.vals, fac.nodes, "block"), direct)
