"""Iteration counts and iterates of the shifted solver's complex GMRES -- single column (shifted_gmres), adjoint mode, and block
(shifted_gmres_block) -- against the host models of tests/support/krylov_model.py, on A, E and the shifts of the open problem
(tests/support/shifted_open.py).  Factors of SIGMA_F; every solve runs at another shift, so GMRES starts from zero on lagged factors.

Every case puts the tolerance into a gap of at least 1.4 between two consecutive residual estimates of the model
(tests/test_krylov_model_host.py holds the tables to that): the device must report exactly the model's count per column
(``fc_shifted_krylov_info``), return the model's iterate, its true residual, and the same bits when asked again.  The residual check
is that of tests/test_krylov_counts_gpu.py: within a factor 1.4 of the MODEL's true residual and on its side of rtol ("within 1.4 of
rtol" cannot hold at the gaps of 7 to 600 these cases have).

Sizes.  square_mesh(10), N = 1 003 (four workgroups, the last one partly filled): restart lengths 3, 7 and 60 with n before, at and
after a restart, direct and adjoint mode, the cap inside a cycle, the blocks of k = 3, 5, 12, 32 (widths 4, 8, 16, 32; at width 32 the
block multidot already loops: 1 003 > 64 * 256 / 32).  square_mesh(48), N = 21 219 > 64 * 256: the second trip of fc_cmultidot.
square_mesh(32), N = 9 539 > 64 * 256 / 4: the block multidot loops at width 4 too."""
import numpy as np
import pytest
import scipy.sparse as sp

from flowcontrol_amd import _lib
from tests.support import krylov_model as km
from tests.support.shifted_open import Open

pytestmark = pytest.mark.gpu


class _Problem:
    def __init__(self, n):
        self.p = p = Open(n)
        p.setup(km.SIGMA_F)
        self._vs = {}
        self.b = km.complex_rhs(1, p.N, 5)[0]
        self.adjoint = False

    def vs(self, adjoint):
        if adjoint not in self._vs:
            self._vs[adjoint] = km.variants(km.shifted_op(self.p.A, self.p.E, km.SIGMA_F), "H" if adjoint else "N")
        return self._vs[adjoint]

    def mode(self, adjoint):
        if adjoint != self.adjoint:
            self.p.ok(self.p.lib.fc_shifted_set_adjoint(self.p.h, 1 if adjoint else 0))
            self.adjoint = adjoint

    def krylov(self, sigma, max_iter, restart, rtol):
        p = self.p
        p.ok(p.lib.fc_shifted_set_krylov(p.h, max_iter, restart, rtol))
        p.ok(p.lib.fc_shifted_set_shift(p.h, complex(sigma).real, complex(sigma).imag))


@pytest.fixture(scope="module")
def open10():
    q = _Problem(10)
    yield q
    q.p.close()


def _norm1(M):
    return abs(sp.csr_matrix(M)).sum(axis=0).max()


def _compare(tag, x, res, runs, Mop, b, rtol):
    """iterate and residual of one column against the model's two variants"""
    ref = runs[0]
    bound = km.bound(runs[0].x, runs[1].x)
    diff = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res_bound = _norm1(Mop) * np.linalg.norm(x) / np.linalg.norm(b) * bound
    print(f"[{tag}] iterate differs by {diff:.2e}, spread {km.spread(runs[0].x, runs[1].x):.2e}, bound {bound:.2e}; residual {res:.6e}, "
          f"model {ref.relres:.6e}, bound {res_bound:.2e}")
    assert diff <= bound
    assert abs(res - ref.relres) <= res_bound
    assert (res <= rtol) == (ref.relres <= rtol) and ref.relres / 1.4 <= res <= 1.4 * ref.relres


def _single(q, adjoint, sigma, m, n):
    p = q.p
    q.mode(adjoint)
    Mop = km.shifted_op(p.A, p.E, sigma, adjoint)
    vs = q.vs(adjoint)
    rtol, gap = km.complex_case(Mop, vs[0], q.b, m, n)
    assert gap >= km.GAP, f"the case lost its gap on the device's numbers: {gap}"
    runs = [km.gmres_complex(Mop, v["precond"], q.b, rtol, km.COMPLEX_MAX_ITER, m, reverse=v["reverse"]) for v in vs]
    assert [r.iters for r in runs] == [n, n]
    q.krylov(sigma, km.COMPLEX_MAX_ITER, m, rtol)
    rc, x, info = p.solve_cols(q.b)
    p.ok(rc)
    it, _ = p.krylov_info(1)
    print(f"GMRES({m}) at {sigma}, adjoint {adjoint}, N = {p.N}: rtol {rtol:.3e} gap {gap:.2f}, model {n} iterations, device {int(it[0])}")
    assert int(it[0]) == n
    _compare(f"GMRES({m}) n = {n}", x[0], info[0], runs, Mop, q.b, rtol)
    rc, x2, info2 = p.solve_cols(q.b)
    p.ok(rc)
    assert np.array_equal(x2, x) and np.array_equal(info2, info) and int(p.krylov_info(1)[0][0]) == n


@pytest.mark.parametrize("sigma,m,n", km.COMPLEX_CASES)
def test_single_column_stops_where_the_model_stops(sigma, m, n, open10):
    """N = 1 003.  n < m: inside the first cycle; n == m: `close` and convergence on the same column; n == m + 1: the first column of a
    cycle that started from the true residual."""
    _single(open10, False, sigma, m, n)


@pytest.mark.parametrize("sigma,m,n", km.ADJOINT_CASES)
def test_adjoint_column_stops_where_the_model_stops(sigma, m, n, open10):
    """The operator conj(sigma) E^T - A^T on the transposed factors; the model's preconditioner is scipy's LU applied conjugate-transposed."""
    try:
        _single(open10, True, sigma, m, n)
    finally:
        open10.mode(False)


def test_second_trip_of_the_complex_multidot():
    """N = 21 219 > 64 * 256: every workgroup of fc_cmultidot walks its grid-stride loop twice."""
    n_mesh, sigma, m, n = km.LARGE_COMPLEX
    q = _Problem(n_mesh)
    try:
        _single(q, False, sigma, m, n)
    finally:
        q.p.close()


def test_cap_inside_a_cycle(open10):
    """max_iter = 10 at restart 7: cycles of 7 and 3 columns, then jend = 0: FC_ERR_NOT_CONVERGED after exactly 10 iterations."""
    q, p = open10, open10.p
    sigma, m, cap, rtol = km.CAPPED_CASE
    q.mode(False)
    q.krylov(sigma, km.COMPLEX_MAX_ITER, m, 1e-3)
    p.ok(p.solve_cols(q.b)[0])  # (a solve that ends well first: the per-column counts of a failed call are read under its column count)
    r = km.gmres_complex(km.shifted_op(p.A, p.E, sigma), q.vs(False)[0]["precond"], q.b, rtol, cap, m)
    assert r.code == km.NOT_CONVERGED and r.iters == cap
    q.krylov(sigma, cap, m, rtol)
    rc, _, _ = p.solve_cols(q.b)
    assert rc == _lib.FC_ERR_NOT_CONVERGED
    assert int(p.krylov_info(1)[0][0]) == r.iters


def test_zero_right_hand_side(open10):
    q, p = open10, open10.p
    q.mode(False)
    q.krylov(km.SIGMA_FAR, km.COMPLEX_MAX_ITER, 7, 1e-8)
    rc, x, info = p.solve_cols(np.zeros(p.N, dtype=complex))
    p.ok(rc)
    assert int(p.krylov_info(1)[0][0]) == 0 and not x.any() and info[0] == 0.0


def _block(q, k):
    """counts, lock-step figures, iterates and residuals of a block of k columns; the same columns one at a time; one zero column"""
    p = q.p
    q.mode(False)
    sig, B = km.block_columns(k, p.N)
    Mops = [km.shifted_op(p.A, p.E, s) for s in sig]
    vs = q.vs(False)
    memo = {}
    for s, M, b in zip(sig, Mops, B):  # (the columns cycle through a few shifts and right-hand sides)
        key = (complex(s), b.tobytes())
        if key not in memo:
            memo[key] = km.gmres_complex(M, vs[0]["precond"], b, 1e-300, 12, km.BLOCK_RESTART).history
    rtol, gap, counts = km.block_rtol([memo[(complex(s), b.tobytes())] for s, b in zip(sig, B)])
    assert gap >= km.GAP, f"the block lost its gap on the device's numbers: {gap}"
    runs = [km.gmres_block(Mops, v["precond"], B, rtol, km.BLOCK_MAX_ITER, km.BLOCK_RESTART, reverse=v["reverse"]) for v in vs]
    assert [r.iters for r in runs[0][0]] == counts == [r.iters for r in runs[1][0]] and runs[0][1:] == runs[1][1:]
    assert max(counts) - min(counts) >= 3 and min(counts) <= km.BLOCK_RESTART and max(counts) > 2 * km.BLOCK_RESTART
    _, cycles, launched = runs[0]
    p.ok(p.lib.fc_shifted_set_krylov(p.h, km.BLOCK_MAX_ITER, km.BLOCK_RESTART, rtol))
    p.ok(p.lib.fc_shifted_set_block(p.h, k))
    rc, X, info = p.solve_block(sig, B)
    p.ok(rc)
    it, bi = p.krylov_info(k)[0], p.block_info()
    print(f"block k = {k} (width {bi['KB']}), N = {p.N}: rtol {rtol:.3e} gap {gap:.2f}; model counts {counts}, device {it.tolist()}; cycles {bi['cycles']} / {cycles}, "
          f"lock-step iterations {bi['lockstep_iterations']} / {launched}")
    assert it.tolist() == counts
    assert bi["KB"] == min(w for w in (4, 8, 16, 32) if w >= k)  # (the instance of the `_b` kernels this block ran)
    assert bi["cycles"] == cycles and bi["lockstep_iterations"] == launched
    for c in range(k):
        _compare(f"block k = {k} column {c}", X[c], info[c], [runs[0][0][c], runs[1][0][c]], Mops[c], B[c], rtol)
    rc, X2, info2 = p.solve_block(sig, B)
    p.ok(rc)
    assert np.array_equal(X2, X) and np.array_equal(info2, info) and p.krylov_info(k)[0].tolist() == counts
    # one zero column among the others: 0 iterations, x = 0, the neighbours as before
    Bz = B.copy()
    Bz[1] = 0.0
    rc, Xz, _ = p.solve_block(sig, Bz)
    p.ok(rc)
    want = list(counts)
    want[1] = 0
    assert p.krylov_info(k)[0].tolist() == want and not Xz[1].any()
    assert all(np.array_equal(Xz[c], X[c]) for c in range(k) if c != 1)
    # the same columns one at a time
    for c in range(min(k, 8)):
        q.krylov(sig[c], km.BLOCK_MAX_ITER, km.BLOCK_RESTART, rtol)
        rc, _, _ = p.solve_cols(B[c])
        p.ok(rc)
        assert int(p.krylov_info(1)[0][0]) == counts[c]


@pytest.mark.parametrize("k", km.BLOCK_KS)
def test_block_columns_stop_where_the_model_stops(k, open10):
    """N = 1 003; k = 3, 5, 12, 32 pad to the widths 4, 8, 16, 32: every instance of the `_b` kernels.  One column is done in the first
    cycle of three iterations and stays frozen while another goes into a third."""
    try:
        _block(open10, k)
    finally:
        open10.p.ok(open10.p.lib.fc_shifted_set_block(open10.p.h, 0))


def test_block_multidot_loops_at_width_four():
    """N = 9 539 > 64 * 256 / 4: fc_cmultidot_b<4> makes a second trip."""
    n_mesh, k = km.LARGE_BLOCK
    q = _Problem(n_mesh)
    try:
        _block(q, k)
    finally:
        q.p.close()
