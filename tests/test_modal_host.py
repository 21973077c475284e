"""The numpy model of POD / DMD (tests/support/modal_model.py) that the device results are compared with, checked against
independent formulations; and the host-side pieces of flowcontrol_amd/modal.py that need no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from flowcontrol_amd import modal
from tests.support import modal_model as mm


def _spd(n, seed):
    """A sparse symmetric positive definite 'mass matrix' of order n (condition number ~ 10)."""
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=4.0 / n, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    return (B @ B.T + sp.identity(n) * (1.0 + abs(B).sum(axis=1).max() / 10.0)).tocsr()


def _weight(nvel, npres, seed=0):
    """diag(M_vv, 0): the energy weight acts on the velocity part of a W-layout vector only."""
    Mvv = _spd(nvel, seed)
    return Mvv, sp.block_diag([Mvv, sp.csr_matrix((npres, npres))]).tocsr()


@pytest.mark.parametrize("center", [False, True])
def test_pod_model_matches_the_svd_of_the_cholesky_scaled_snapshots(center):
    nvel, npres, m = 120, 30, 17
    rng = np.random.default_rng(3)
    Mvv, M = _weight(nvel, npres)
    X = rng.standard_normal((m, 5)) @ rng.standard_normal((5, nvel + npres)) + 1e-3 * rng.standard_normal((m, nvel + npres))
    Lc = np.linalg.cholesky(Mvv.toarray())
    Xc = X - X.mean(axis=0) if center else X
    s_ref = np.linalg.svd(Lc.T @ Xc[:, :nvel].T, compute_uv=False)
    r = m - 1 if center else m
    sigma, V, Phi, mean = mm.pod(X, M, r=r, center=center)
    # Weyl: the eigenvalues of the Gram matrix carry its rounding error, m N eps sigma_0^2 at most
    assert np.max(np.abs(sigma[:r] ** 2 - s_ref[:r] ** 2)) <= 4 * m * X.shape[1] * mm.EPS * s_ref[0] ** 2
    assert np.max(np.abs(Phi @ (M @ Phi.T) - np.eye(r))) <= 1e-8  # eps (sigma_0 / sigma_min)^2 with sigma_min / sigma_0 ~ 1e-3
    assert np.linalg.norm((V * sigma[:r]) @ Phi + mean - X) <= 1e-10 * np.linalg.norm(X)
    assert np.allclose(mean, X.mean(axis=0) if center else 0.0)


def test_dmd_model_returns_the_eigenvalues_of_a_synthetic_sequence():
    nvel, npres = 200, 50
    _, M = _weight(nvel, npres, seed=1)
    X, mus = mm.synthetic_sequence(nvel + npres, 40, seed=5, nvel=nvel)
    for weight in (None, M):
        mu, lam, lam2 = mm.dmd(X, weight, r=6, dt=0.01, every=4)
        assert mm.match(mu, mus) <= 1e-10
        assert np.allclose(np.exp(lam * 0.04), mu) and np.allclose(mm.bdf2_amplification(lam2, 0.01, 4), mu)


def test_bdf2_map_round_trips():
    """lam -> mu (one BDF2 step of x' = lam x, physical root) -> lam, for rates around the cylinder's (dt |lam| << 1) and beyond; and
    mu is what the recurrence 3 x2 - 4 x1 + x0 = 2 dt lam x2 actually multiplies by."""
    dt = 0.005
    lam = np.array([0.13 + 0.78j, 0.13 - 0.78j, -0.5, -3.0 + 10j, 0.0, -40.0])
    for every in (1, 20):
        mu = mm.bdf2_amplification(lam, dt, every)
        assert np.max(np.abs(mm.bdf2_rate(mu, dt, every) - lam)) <= 1e-9 * (1 + np.abs(lam).max())
        assert np.max(np.abs(modal.bdf2_rate(mu, dt, every) - lam)) <= 1e-9 * (1 + np.abs(lam).max())
        assert np.allclose(modal.bdf2_amplification(lam, dt, every), mu, rtol=1e-14, atol=0)
    mu1 = mm.bdf2_amplification(lam, dt)
    assert np.max(np.abs(3 * mu1 ** 2 - 4 * mu1 + 1 - 2 * dt * lam * mu1 ** 2)) <= 1e-14
    # second order: mu = exp(dt lam) (1 + O((dt lam)^3))
    assert abs(mu1[0] - np.exp(dt * lam[0])) <= abs(dt * lam[0]) ** 3


def test_product_helpers_agree_with_the_model():
    rng = np.random.default_rng(0)
    G = rng.standard_normal((9, 30))
    G = G @ G.T
    sigma, V = modal.gram_eig(G)
    w, Vm = mm.sorted_eig(G)
    assert np.allclose(sigma ** 2, w) and np.all(np.diff(sigma) <= 0)
    assert np.allclose(np.abs(V.T @ Vm), np.eye(9), atol=1e-8)
    assert modal.numerical_rank(np.array([1.0, 1e-3, 1e-9, 0.0])) == 2 and modal.numerical_rank(np.array([1.0, 1e-3, 1e-9]), tol=1e-10) == 3
    assert modal.numerical_rank(np.zeros(3)) == 0
    for bad in ("mass", 1.5, True):
        with pytest.raises(ValueError):
            modal._weight_slot(bad)
    assert modal._weight_slot("energy") == 2 and modal._weight_slot(None) == -1 and modal._weight_slot(3) == 3


def test_batched_solver_refuses_to_record():
    from flowcontrol_amd.batch import BatchedFlowSolver

    with pytest.raises(RuntimeError, match="batched steps are not captured"):
        BatchedFlowSolver.record_snapshots(object(), 8)


class _HostBank:
    """The SnapshotBank interface on numpy arrays (rows = columns of the bank): what pod() needs of it, without a device."""

    def __init__(self, X, M, capacity=None):
        self.sets = [np.array(X, dtype=float), np.zeros((0, X.shape[1]))]
        self.M, self.capacity, self.every, self.mean_removed = M, capacity or X.shape[0], 1, None

    count = property(lambda self: self.sets[0].shape[0])
    kept = property(lambda self: self.sets[1].shape[0])

    def mean(self, subtract=False, download=True, **kw):
        mu = self.sets[0].mean(axis=0)
        if subtract:
            self.sets[0] -= mu
        return mu if download else None

    def gram(self, a=None, b=None, weight="energy", lset=0, rset=0):
        L, R = self.sets[lset], self.sets[rset]
        L, R = (L if a is None else L[a[0]:a[1]]), (R if b is None else R[b[0]:b[1]])
        return L @ (R.T if weight is None else self.M @ R.T)

    def combine(self, Q, c0=None, c1=None, set=0, keep=False, download=True):  # noqa: A002
        out = np.asarray(Q).T @ self.sets[set][c0:c1]
        if keep:
            assert self.kept + out.shape[0] <= self.capacity
            self.sets[1] = np.vstack([self.sets[1], out])
        return out if download else None

    def clear(self, set=0):  # noqa: A002
        self.sets[set] = self.sets[set][:0]


def test_pod_second_pass_resolves_what_one_gram_matrix_cannot():
    """Snapshots whose singular values fall by a factor 4 per index down to 1e-14: one Gram matrix loses them below sqrt(eps) sigma_0
    (reconstruction error ~ 1e-8), the deflated second pass follows them to ~ 1e-12 and reconstructs to 1e-10 in the energy norm."""
    nvel, npres, m = 150, 40, 30
    rng = np.random.default_rng(11)
    _, M = _weight(nvel, npres, seed=2)
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    B = rng.standard_normal((m, nvel + npres))
    s_true = 4.0 ** -np.arange(m)
    X = (U * s_true) @ B + 0.3 * rng.standard_normal(nvel + npres)  # (a common mean on top)
    en = lambda Y: np.sqrt(np.sum(Y * (M @ Y.T).T))  # noqa: E731
    errs = {}
    for refine in (False, True):
        bank = _HostBank(X, M)
        res = modal.pod(bank, refine=refine)
        assert bank.kept == 0 and res.modes.shape == (res.r, X.shape[1])
        errs[refine] = en((res.V * res.sigma[: res.r]) @ res.modes + res.mean - X) / en(X)
        # V = [V_1, W]: orthonormal to rounding inside each block; across the blocks to m eps sigma_0 / sigma_i (margin 100), the
        # error the residual's entries carry relative to its i-th direction
        r1 = int(np.count_nonzero(res.sigma > modal.POD_SPLIT * res.sigma[0])) if refine else res.r
        VtV = res.V.T @ res.V - np.eye(res.r)
        assert max(np.max(np.abs(VtV[:r1, :r1])), np.max(np.abs(VtV[r1:, r1:]), initial=0.0)) <= 1e-12
        assert np.all(np.abs(VtV[:r1, r1:]) <= 100 * m * mm.EPS * res.sigma[0] / res.sigma[r1:res.r])
        big = res.sigma[: res.r] >= 1e-3 * res.sigma[0]
        P = res.modes[big]
        assert np.max(np.abs(P @ (M @ P.T) - np.eye(P.shape[0]))) <= 1e-8
        rank = res.r
        if refine:
            s_ref = np.linalg.svd(np.linalg.cholesky(M[:nvel, :nvel].toarray()).T @ (X - X.mean(axis=0))[:, :nvel].T, compute_uv=False)
            assert np.max(np.abs(res.sigma[:rank] - s_ref[:rank]) / s_ref[:rank]) <= 1e-3 and rank >= 17
    assert errs[True] <= 1e-10 < errs[False]
    with pytest.raises(ValueError, match="set 1"):
        bank = _HostBank(X, M)
        bank.sets[1] = X[:2].copy()
        modal.pod(bank, refine=True)
