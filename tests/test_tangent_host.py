"""The host model of the tangent-linear march (tests/support/tangent_model.py) and the block Arnoldi driver of
flowcontrol_amd/tangent.py -- no GPU.  The model is what the device tests compare ``fc_run_tangent`` with, so it is pinned here three
ways on the 7 x 5 square of ``host_square()`` (N = 378): against central differences of the nonlinear forward model, against the
existing adjoint model through the dot-product identity, and against three wrong forms the inputs must tell apart."""
import numpy as np
import pytest

from flowcontrol_amd.tangent import block_arnoldi, floquet_multipliers
from tests.support import adjoint_nl_model as nm
from tests.support.tangent_model import ModelTangentBlocks, TangentModel

#: (first order, n)
CASES = [(1, 6), (2, 3), (1, 1), (2, 2)]
EPS = 1e-5
#: measured with these seeds: central differences agree to 1.7e-9 or better, the identity to 9.4e-15 or better (worst case (2, 3))
TOL_FD, TOL_DOT = 1e-7, 1e-12
#: measured with these seeds: each wrong form misses x_n by >= 8.0e-4 and the identity by >= 2.7e-5 ("half" at (1, 1))
WRONG_MIN = 1e-5


@pytest.fixture(scope="module")
def square():
    model, th, (u_n, u_nn, p) = nm.host_square()
    return model, TangentModel(model), np.r_[u_n, p], np.r_[u_nn, p]


def _inputs(model, n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, model.n_act))
    du = rng.standard_normal((n, model.n_act))
    dx0, dxm1 = rng.standard_normal(model.N), rng.standard_normal(model.N)
    w = rng.standard_normal((n, model.C.shape[0]))
    z = rng.standard_normal(model.N)
    return u, du, dx0, dxm1, w, z


def _identity_defect(model, first_order, X, D, dy, du, dx0, dxm1, w, z):
    g, gx0, gxm1, _ = model.adjoint(first_order, X, w, z)
    terms = [np.sum(w * dy), z @ D[-1], -np.sum(g * du), -(gx0 @ dx0), -(gxm1 @ dxm1)]
    return abs(sum(terms)) / sum(abs(t) for t in terms)


@pytest.mark.parametrize("first_order,n", CASES)
def test_tangent_model_against_central_differences(square, first_order, n):
    model, tm, x0, xm1 = square
    u, du, dx0, dxm1, _, _ = _inputs(model, n, 11 + n)
    X, _ = model.forward(first_order, u, x0, xm1)
    D, dy = tm.tangent(first_order, X, du, dx0, dxm1)
    Xp, yp = model.forward(first_order, u + EPS * du, x0 + EPS * dx0, xm1 + EPS * dxm1)
    Xm, ym = model.forward(first_order, u - EPS * du, x0 - EPS * dx0, xm1 - EPS * dxm1)
    ex, ey = nm.rel(D[-1], (Xp[-1] - Xm[-1]) / (2 * EPS)), nm.rel(dy, (yp - ym) / (2 * EPS))
    print(f"tangent model vs central differences, first order {first_order}, n = {n}: x_n {ex:.3e}, y {ey:.3e}")
    assert ex <= TOL_FD and ey <= TOL_FD
    assert np.array_equal(D[0], dxm1) and np.array_equal(D[1], dx0)


@pytest.mark.parametrize("first_order,n", CASES)
def test_tangent_model_dot_product_identity_with_the_adjoint_model(square, first_order, n):
    """<w, Phi v> = <Phi^T w, v> with v = (du, dx0, dxm1) and the weights (w on y, z on x_n) of the existing ``model.adjoint``."""
    model, tm, x0, xm1 = square
    u, du, dx0, dxm1, w, z = _inputs(model, n, 23 + n)
    X, _ = model.forward(first_order, u, x0, xm1)
    D, dy = tm.tangent(first_order, X, du, dx0, dxm1)
    defect = _identity_defect(model, first_order, X, D, dy, du, dx0, dxm1, w, z)
    print(f"tangent model x adjoint model, first order {first_order}, n = {n}: identity defect {defect:.3e}")
    assert defect <= TOL_DOT


@pytest.mark.parametrize("wrong", ["linear", "J_next", "half"])
def test_the_inputs_tell_the_wrong_forms_apart(square, wrong):
    model, tm, x0, xm1 = square
    for first_order, n in CASES:
        u, du, dx0, dxm1, w, z = _inputs(model, n, 37 + n)
        X, _ = model.forward(first_order, u, x0, xm1)
        D, _ = tm.tangent(first_order, X, du, dx0, dxm1)
        Dw, dyw = tm.tangent(first_order, X, du, dx0, dxm1, wrong=wrong)
        miss = nm.rel(Dw[-1], D[-1])
        defect = _identity_defect(model, first_order, X, Dw, dyw, du, dx0, dxm1, w, z)
        print(f"wrong = {wrong}, first order {first_order}, n = {n}: x_n off by {miss:.3e}, identity defect {defect:.3e}")
        assert miss > WRONG_MIN and defect > WRONG_MIN


def test_null_inputs_are_zeros(square):
    model, tm, x0, xm1 = square
    u, du, dx0, dxm1, _, _ = _inputs(model, 3, 5)
    X, _ = model.forward(2, u, x0, xm1)
    full = tm.tangent(2, X, du, dx0, dxm1)[0][-1]
    parts = [tm.tangent(2, X, du)[0][-1], tm.tangent(2, X, None, dx0)[0][-1], tm.tangent(2, X, None, None, dxm1)[0][-1]]
    assert nm.rel(sum(parts), full) < 1e-12  # (the march is linear in its three inputs)
    assert not np.any(tm.tangent(2, X)[0])


# ── block Arnoldi driver ─────────────────────────────────────────────────────────────────────────────────────────────────────────
class _Dense:
    def __init__(self, A, k):
        self.A, self.k, self.size, self.calls = A, k, A.shape[0], 0

    def apply(self, V):
        self.calls += 1
        return self.A @ V


def _separated_matrix(m=60, seed=3):
    rng = np.random.default_rng(seed)
    lam = np.r_[2.0, -1.6, 1.3, 1.0, 0.8, 0.04 * rng.uniform(-1, 1, m - 5)]
    S = np.linalg.qr(rng.standard_normal((m, m)))[0] + 0.05 * rng.standard_normal((m, m))
    return S @ np.diag(lam) @ np.linalg.inv(S), lam


def test_block_arnoldi_on_a_dense_matrix_with_a_separated_spectrum():
    A, _ = _separated_matrix()
    back = _Dense(A, 4)
    ref = np.linalg.eigvals(A)
    ref = ref[np.argsort(-np.abs(ref))][:5]
    # (the unwanted eigenvalues are <= 0.04, the smallest wanted one 0.8: a block step gains a factor 0.05, ten of them ~ 2e-12)
    lam, V, res = floquet_multipliers(back, 0, 5, blocks=10, seed=1, vectors=True)
    assert back.calls == 10
    assert np.max(np.abs(np.sort_complex(lam) - np.sort_complex(ref)) / np.abs(np.sort_complex(ref))) < 1e-10
    assert np.all(np.abs(lam[:-1]) >= np.abs(lam[1:]))  # sorted by modulus
    true_res = np.linalg.norm(A @ V - V * lam, axis=0) / np.abs(lam)
    assert np.allclose(np.linalg.norm(V, axis=0), 1.0, atol=1e-12)
    assert np.max(true_res) < 1e-8 and np.max(np.abs(res - true_res)) < 1e-8  # (the residual from the Arnoldi relation is the true one)
    assert np.array_equal(floquet_multipliers(_Dense(A, 4), 0, 5, blocks=10, seed=1), lam)


def test_block_arnoldi_relation_and_orthogonality():
    A, _ = _separated_matrix(m=40, seed=8)
    V0 = np.random.default_rng(2).standard_normal((40, 3))
    Qb, H = block_arnoldi(lambda V: A @ V, V0, 4)
    Q = np.hstack(Qb)
    assert np.max(np.abs(Q.T @ Q - np.eye(15))) < 1e-13
    assert np.max(np.abs(A @ Q[:, :12] - Q @ H)) < 1e-12
    assert not np.any(np.tril(H, -4))  # block Hessenberg (the sub-diagonal blocks are upper triangular)
    with pytest.raises(ValueError):
        block_arnoldi(lambda V: A @ V, np.ones((40, 2)), 2)
    with pytest.raises(ValueError):
        floquet_multipliers(_Dense(A, 3), 0, 13, blocks=4)


def test_ritz_values_of_the_tangent_model_take_apply_noise(square):
    """The pair map of the tangent model (k = 4, 4 blocks, n = 6) with relative noise of 1e-13 on every apply -- an order of magnitude
    above fp64 round-off of one product, and what the device's applies differ from the model's by at best: the five leading Ritz
    values move by 2e-13 (measured with these inputs).  The bound asserted is 1e-11 = 100 x the noise: an eigenvalue of the projected matrix moves by at
    most its condition number times the perturbation, and a leading, separated Ritz value whose condition number exceeded 100 would
    make the device comparison at 1e-8 (tests/test_tangent_batch_gpu.py) meaningless.  Hessenberg entries are not compared: QR signs
    differ."""
    model, tm, x0, xm1 = square
    n, k, blocks = 6, 4, 4
    u = np.random.default_rng(41).standard_normal((n, model.n_act))
    X, _ = model.forward(2, u, x0, xm1)
    start = np.random.default_rng(43).standard_normal((2 * model.N, k))
    clean = floquet_multipliers(ModelTangentBlocks(tm, X, k), n, 5, blocks=blocks, start=start)
    noisy = floquet_multipliers(ModelTangentBlocks(tm, X, k, noise=1e-13, seed=7), n, 5, blocks=blocks, start=start)
    move = np.max(np.abs(noisy - clean) / np.abs(clean))
    print(f"five leading Ritz values {np.abs(clean)}; moved by {move:.3e} under 1e-13 apply noise")
    assert move <= 1e-11
