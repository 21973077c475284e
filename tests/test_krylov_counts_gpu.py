"""Iteration counts and iterates of the real Krylov drivers of ``fc_solve`` (gmres_permuted, bicgstab_permuted) against the host models
of tests/support/krylov_model.py.

A driver with a slightly wrong projection, rotation or reduction still converges -- later.  So every case puts the tolerance into a gap
of at least 1.4 between two consecutive residual norms of the model, and the device must stop at exactly the model's iteration, with
the model's iterate, the model's true residual, and the same bits when asked again.  The operators are read back from the device
(``dev.matrix``) before and after ``update_operator``, the preconditioner of the model is scipy's LU of the first: the model runs on the
device's own numbers.  The cases and the conditions that make them sharp: krylov_model.GMRES_CASES / BICG_CASES and
tests/test_krylov_model_host.py.

The reported residual.  "Within a factor 1.4 of rtol" cannot hold where the gap is wide (at a gap of 250 the n-th residual lies a factor
16 below the tolerance), so the check is the stricter one that does: the device's figure lies within a factor 1.4 of the MODEL's true
residual of its n-th iterate, on the same side of rtol as the model's, and agrees with it to |A|_1 |x| / |b| times the iterate's bound.

Sizes.  Mesh.unit_square(16, 16), N = 2 467 (no multiple of 256, ten workgroups): every case, among them n = 30 and n = 31 around the
restart of GMRES(30) and both endings of BiCGStab.  Mesh.unit_square(96, 96), N = 83 907: fc_multidot's grid-stride loop (256 workgroups
of 256 threads) makes a second trip in 72 workgroups.  fc_dots2 (512 workgroups) would need N > 131 072, unit_square(128, 128); the
large test prints what its parts take, and at (96, 96) it is the longest new test already, so the second trip of fc_dots2 stays
uncovered."""
import numpy as np
import pytest

from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import TaylorHood
from tests.support import krylov_model as km

pytestmark = pytest.mark.gpu

MODELS = {"gmres": km.gmres_real, "bicgstab": km.bicgstab_real}


class _Square:
    """One handle per mesh: the factored operator (the same for every pair) is set up once, the current one changes under the factors."""

    def __init__(self, n, own_ordering=False):
        from flowcontrol_amd.device import SLOT_BDF2, DeviceSolver

        self.slot = SLOT_BDF2
        self.th = th = TaylorHood(Mesh.unit_square(n, n))
        self.dev = dev = DeviceSolver(th)
        self.dofs = dofs = km.wall_dofs(th)
        dev.set_bc(dofs, np.zeros((dofs.size, 1)))
        f, _ = km.real_operators("fast", th.node_coords)
        dev.assemble_matrix(self.slot, **f)
        dev.apply_bc(self.slot)
        dev.setup_solver(self.slot)
        self.A0 = dev.matrix(self.slot).tocsr()
        self.vs = km.variants(self.A0, perm=dev.perm if own_ordering else None)
        self.b = km.real_rhs(dev.N, dofs)
        self._pair, self.A1 = None, None

    def current(self, pair):
        if pair != self._pair:
            _, c = km.real_operators(pair, self.th.node_coords)
            self.dev.assemble_matrix(self.slot, **c)
            self.dev.apply_bc(self.slot)
            self.dev.update_operator(self.slot)
            self.A1 = self.dev.matrix(self.slot).tocsr()
            self._pair = pair
        return self.A1

    def close(self):
        self.dev.set_solver_options(0, True)
        self.dev.close()


@pytest.fixture(scope="module")
def square16():
    s = _Square(16)
    yield s
    s.close()


def _check(s, method, pair, k, n, ending=None):
    """The k-th test of the model's run decides at iteration n: count, iterate, residual, repeatability."""
    model = MODELS[method]
    A1, b = s.current(pair), s.b
    rtol, gap = km.real_case(model, A1, s.vs[0], b, k)
    assert gap >= km.GAP, f"the case lost its gap on the device's numbers: {gap}"
    runs = [model(A1, v["precond"], b, rtol, km.REAL_MAX_ITER, reverse=v["reverse"]) for v in s.vs]
    assert [r.iters for r in runs] == [n, n] and all(r.code == km.OK for r in runs)
    s.dev.set_solver_options(refine=km.REAL_MAX_ITER, method=method, rtol=rtol)
    x, info = s.dev.solve(s.slot, b)
    ref = runs[0]
    bound = km.bound(runs[0].x, runs[1].x)
    diff = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    res_bound = abs(A1).sum(axis=0).max() * np.linalg.norm(x) / np.linalg.norm(b) * bound
    print(f"[{method} {pair} n = {n} {ending or ''}] N = {b.size} rtol {rtol:.3e} gap {gap:.2f}: device count {int(info[0])}; iterate differs by {diff:.2e}, "
          f"spread {km.spread(runs[0].x, runs[1].x):.2e}, bound {bound:.2e}; residual {info[1]:.6e}, model {ref.relres:.6e}, bound {res_bound:.2e}")
    assert int(info[0]) == n
    if ending:
        assert [r.where for r in runs] == [ending, ending]
    assert diff <= bound
    assert abs(info[1] - ref.relres) <= res_bound
    # on the model's side of the tolerance, and within a factor 1.4 of the model's figure
    assert (info[1] <= rtol) == (ref.relres <= rtol) and ref.relres / 1.4 <= info[1] <= 1.4 * ref.relres
    x2, info2 = s.dev.solve(s.slot, b)
    assert np.array_equal(x2, x) and np.array_equal(info2, info), "the same solve a second time gave other bits"


@pytest.mark.parametrize("pair,n", km.GMRES_CASES)
def test_gmres_stops_where_the_model_stops(pair, n, square16):
    """N = 2 467.  n = 30 closes the first cycle (state 4 and convergence fall on the same column), n = 31 is the first column after
    begin_cycle(0) took the true residual; n = 40 and 45 sit deep in the second cycle."""
    _check(square16, "gmres", pair, n, n)


@pytest.mark.parametrize("pair,it,ending", km.BICG_CASES)
def test_bicgstab_stops_where_the_model_stops(pair, it, ending, square16):
    """N = 2 467.  "half": |s| meets the tolerance, the iteration is finished with omega = 0 (state 2, then 1); "full": |r| does."""
    _check(square16, "bicgstab", pair, km.bicg_index(it, ending), it, ending)


@pytest.mark.parametrize("method", ["gmres", "bicgstab"])
def test_zero_right_hand_side(method, square16):
    s = square16
    s.current("fast")
    s.dev.set_solver_options(refine=km.REAL_MAX_ITER, method=method, rtol=1e-8)
    x, info = s.dev.solve(s.slot, np.zeros(s.dev.N))
    assert int(info[0]) == 0 and not x.any() and info[1] == 0.0


def test_gmres_cap_inside_a_cycle_is_refused(square16):
    """max_iter = 40 is no multiple of the restart length: the second cycle ends at the cap with nothing to close it, which the driver
    reports as a failure (the model: NOT_CONVERGED)."""
    from flowcontrol_amd._lib import FcError

    s = square16
    A1 = s.current("crawl")
    r = km.gmres_real(A1, s.vs[0]["precond"], s.b, 1e-13, 40)
    assert r.code == km.NOT_CONVERGED
    s.dev.set_solver_options(refine=40, method="gmres", rtol=1e-13)
    with pytest.raises(FcError, match="inside a cycle"):
        s.dev.solve(s.slot, s.b)


def test_second_trip_of_the_reduction_loops():
    """N = 83 907 > 256 * 256: 72 workgroups of fc_multidot walk their grid-stride loop twice (fc_dots2, 512 workgroups, once).  The
    model's preconditioner is ONE SuperLU of the factored operator in the device's own elimination ordering (SuperLU's orderings take
    minutes at this size), so the variants differ in the summation order alone."""
    import time

    t0 = time.time()
    s = _Square(km.LARGE_MESH, own_ordering=True)
    print(f"mesh, device factorisation and the model's one SuperLU at N = {s.dev.N}: {time.time() - t0:.1f} s")
    try:
        pair, n = km.LARGE_GMRES
        _check(s, "gmres", pair, n, n)
        pair, it, ending = km.LARGE_BICG
        _check(s, "bicgstab", pair, km.bicg_index(it, ending), it, ending)
    finally:
        s.close()
