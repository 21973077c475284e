"""The host models of the Krylov drivers (tests/support/krylov_model.py) and the cases the GPU tests take from them, on the CPU.

Model checks: the GMRES residual estimate is the minimum of |b - A M^-1 K c| over the Krylov space (computed independently from a dense
QR of the Krylov matrix), the true residual of every returned iterate equals the estimate, the BiCGStab recurrence residual is b - A x
at every step, b = 0 gives 0 iterations and x = 0.

Case conditions: an iteration count is a sharp prediction only when the tolerance sits in a gap of at least GAP = 1.4 between the last
residual norm that misses it and the first that meets it, when both variants of the model (inner products summed backwards, another
column ordering in the preconditioner's LU) give the same count, and when the n-th iterate is at least 1000 spreads away from the
solution, so that "the n-th iterate" is something a test can tell from "the solution".  Every case of the tables is held to these here;
tests/test_krylov_counts_gpu.py and tests/test_shifted_krylov_counts_gpu.py run the same tables on the device's own numbers."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import TaylorHood
from tests.support import krylov_model as km

CSRC = Path(__file__).resolve().parents[1] / "flowcontrol_amd" / "csrc"
EPS = np.finfo(float).eps


def _real_problem(n, pair):
    """(factored, current, b) on Mesh.unit_square(n, n), assembled by the oracle, identity rows on the Dirichlet dofs"""
    from oracle import ns_oracle as O

    th = TaylorHood(Mesh.unit_square(n, n))
    d = O.Disc.from_taylor_hood(th)
    dofs = km.wall_dofs(th)
    f, c = km.real_operators(pair, th.node_coords)
    A0, _ = O.apply_bc_rows(O.assemble_matrix(d, **f), None, dofs, None)
    A1, _ = O.apply_bc_rows(O.assemble_matrix(d, **c), None, dofs, None)
    return A0.tocsr(), A1.tocsr(), km.real_rhs(th.N, dofs)


@pytest.fixture(scope="module")
def real16():
    out = {}
    for pair in ("fast", "mid", "slow", "restart", "crawl"):
        A0, A1, b = _real_problem(16, pair)
        out[pair] = (A1, km.variants(A0), b, spla.splu(A1.tocsc()).solve(b))
    return out


@pytest.fixture(scope="module")
def open10():
    A, E = km.oracle_open_problem(10)
    return A, E, {adj: km.variants(km.shifted_op(A, E, km.SIGMA_F), "H" if adj else "N") for adj in (False, True)}


def test_the_constants_the_models_copy_are_the_sources():
    hip = (CSRC / "fc_hip.hip").read_text()
    shf = (CSRC / "fc_shifted_solver.hpp").read_text()
    dsp = (CSRC / "fc_dispatch.hpp").read_text()
    assert int(re.search(r"constexpr int kKrylovCheck = (\d+);", hip).group(1)) == km.KRYLOV_CHECK
    assert int(re.search(r"constexpr int kShiftedKrylovCheck = (\d+);", shf).group(1)) == km.KRYLOV_CHECK
    assert int(re.search(r"constexpr int kBicgRestarts = (\d+);", hip).group(1)) == km.BICG_RESTARTS
    assert int(re.search(r"int gmres_m = (\d+);", hip).group(1)) == km.GMRES_M
    widths = [int(w) for w in re.search(r"using BatchWidths = IntList<([\d, ]+)>;", dsp).group(1).split(",")]
    pad = lambda k: min(w for w in widths if w >= k)  # noqa: E731  (a block is padded to the narrowest instance that holds it)
    assert sorted({pad(k) for k in km.BLOCK_KS}) == sorted(widths), "a block width that pick_width instantiates is not run"


# ── the models ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _krylov_minimum(Mop, precond, b, j):
    """min over the j-dimensional Krylov space of |b - A M^-1 K c|, and the condition number of the (column-scaled) Krylov matrix"""
    B = lambda v: Mop @ precond(v)  # noqa: E731
    K = [b / np.linalg.norm(b)]
    for _ in range(j - 1):
        w = B(K[-1])
        K.append(w / np.linalg.norm(w))
    K = np.array(K).T
    Q, R = np.linalg.qr(K)
    W = np.array([B(Q[:, i]) for i in range(j)]).T
    c = np.linalg.lstsq(W, b, rcond=None)[0]
    return np.linalg.norm(b - W @ c), np.linalg.cond(R)


def _estimate_is_the_minimum(run, Mop, var, b, steps):
    h = run(1e-300).history
    checked = 0
    for j in range(1, steps + 1):
        best, cond = _krylov_minimum(Mop, var["precond"], b, j)
        if cond > 1e7:
            break
        # the estimate is the norm of a residual of size <= |b|; the dense computation loses cond(K) eps of |b|
        assert abs(h[j] - best) <= 100.0 * EPS * cond * h[0], (j, h[j], best, cond)
        checked += 1
    assert checked >= 3


def _norm1(A):
    return abs(A).sum(axis=0).max()


@pytest.mark.parametrize("problem", ["square8", "open10"])
def test_gmres_estimate_is_the_minimum_over_the_krylov_space_and_equals_the_true_residual(problem, open10):
    if problem == "square8":
        A0, A1, b = _real_problem(8, "slow")
        var = km.variants(A0)[0]
        run = lambda rtol, max_iter=12: km.gmres_real(A1, var["precond"], b, rtol, max_iter, reverse=var["reverse"])  # noqa: E731
        Mop = A1
    else:
        A, E, vs = open10
        var = vs[False][0]
        Mop = km.shifted_op(A, E, km.SIGMA_FAR)
        b = km.complex_rhs(1, A.shape[0], 5)[0]
        run = lambda rtol, max_iter=12: km.gmres_complex(Mop, var["precond"], b, rtol, max_iter, 60, reverse=var["reverse"])  # noqa: E731
    _estimate_is_the_minimum(run, Mop, var, b, 8)
    # every returned iterate: its true residual is the estimate it stopped on.  x = M^-1 (V y) and b - A x carry eps (|A| |x| + |b|)
    bn = np.linalg.norm(b)
    for rtol in (1e-2, 1e-4, 1e-6, 1e-8):
        r = run(rtol, 60)
        assert r.code == km.OK and 0 < r.iters < 60
        tol = 100.0 * EPS * (_norm1(Mop) * r.xmax + bn)
        assert abs(r.relres * bn - r.history[r.iters]) <= tol, (rtol, r.relres * bn, r.history[r.iters], tol)
        assert r.history[r.iters] <= rtol * bn < r.history[r.iters - 1]


def test_bicgstab_recurrence_residual_is_the_true_residual_at_every_step():
    for pair, n in (("fast", 8), ("slow", 8)):
        A0, A1, b = _real_problem(n, pair)
        var = km.variants(A0)[0]
        r = km.bicgstab_real(A1, var["precond"], b, 1e-300, 12, reverse=var["reverse"], keep_iterates=True)
        assert len(r.iterates) == 12
        bn = np.linalg.norm(b)
        for x, rec in r.iterates:
            # the recurrences accumulate eps (|A| |x| + |b|) per step at the largest iterate so far
            tol = 100.0 * 12 * EPS * (_norm1(A1) * r.xmax + bn)
            assert np.linalg.norm((b - A1 @ x) - rec) <= tol, (pair, np.linalg.norm((b - A1 @ x) - rec), tol)


def test_zero_right_hand_side_takes_no_iteration(open10):
    A0, A1, b = _real_problem(8, "fast")
    var = km.variants(A0)[0]
    for model in (km.gmres_real, km.bicgstab_real):
        r = model(A1, var["precond"], np.zeros_like(b), 1e-8, 60, reverse=var["reverse"])
        assert r.iters == 0 and not r.x.any() and r.code == km.OK and r.relres == 0.0
    A, E, vs = open10
    Mop = km.shifted_op(A, E, km.SIGMA_FAR)
    r = km.gmres_complex(Mop, vs[False][0]["precond"], np.zeros(A.shape[0], dtype=complex), 1e-8, 60, 7)
    assert r.iters == 0 and not r.x.any() and r.code == km.OK
    B = km.complex_rhs(3, A.shape[0])
    full, _, _ = km.gmres_block([Mop] * 3, vs[False][0]["precond"], B, 1e-6, 60, 3)
    B[1] = 0.0
    holed, _, _ = km.gmres_block([Mop] * 3, vs[False][0]["precond"], B, 1e-6, 60, 3)
    assert holed[1].iters == 0 and not holed[1].x.any()
    assert [r.iters for r in holed][::2] == [r.iters for r in full][::2]


def test_gmres_restart_takes_the_true_residual_and_the_cap_inside_a_cycle_fails(real16):
    """Control flow that no estimate shows: 31 iterations are 30 + 1 in two cycles; an iteration cap that is no multiple of the restart
    length ends the run inside a cycle, which the driver reports as a failure with no count."""
    A1, vs, b, _ = real16["restart"]
    h = km.history_run(km.gmres_real, A1, b, km.REAL_MAX_ITER, km.GMRES_M, vs[0])
    tol, _ = km.rtol_for(h, 31)
    r = km.gmres_real(A1, vs[0]["precond"], b, tol / h[0], km.REAL_MAX_ITER)
    assert r.iters == 31 and r.cycles == 2 and r.code == km.OK
    r = km.gmres_real(A1, vs[0]["precond"], b, 1e-14, 40)
    assert r.code == km.NOT_CONVERGED and r.iters == 0


# ── the cases ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _sharp(runs, n, x_exact, what):
    """both variants stop at n, and the n-th iterate is far from the solution on the scale of the variants' spread"""
    assert [r.iters for r in runs] == [n, n], (what, [r.iters for r in runs])
    assert all(r.code == km.OK for r in runs), what
    sprd = km.spread(runs[0].x, runs[1].x)
    dist = np.linalg.norm(runs[0].x - x_exact) / np.linalg.norm(x_exact)
    assert dist >= 1000.0 * sprd, (what, dist, sprd)
    return sprd


def test_the_tables_hold_what_the_issue_asks_for():
    ns = [n for _, n in km.GMRES_CASES]
    assert any(n < 5 for n in ns) and any(10 <= n <= 25 for n in ns) and {30, 31} <= set(ns) and any(40 <= n <= 55 for n in ns)
    assert {e for _, _, e in km.BICG_CASES} == {"half", "full"} and all(n <= 15 for _, n, _ in km.BICG_CASES)
    for m in (3, 7):
        got = {n for s, mm, n in km.COMPLEX_CASES if mm == m}
        assert {m - 1, m, m + 1} <= got, "n on both sides of a restart and exactly at one"
    assert {m for _, m, _ in km.COMPLEX_CASES} == {3, 7, 60}
    _, m, cap, _ = km.CAPPED_CASE
    assert cap % m != 0
    assert 5 <= km.LARGE_GMRES[1] <= 12 and 5 <= km.LARGE_BICG[1] <= 12


@pytest.mark.parametrize("pair,n", km.GMRES_CASES)
def test_real_gmres_cases_are_sharp(pair, n, real16):
    A1, vs, b, x_exact = real16[pair]
    rtol, gap = km.real_case(km.gmres_real, A1, vs[0], b, n)
    assert gap >= km.GAP, (pair, n, gap)
    runs = [km.gmres_real(A1, v["precond"], b, rtol, km.REAL_MAX_ITER, reverse=v["reverse"]) for v in vs]
    sprd = _sharp(runs, n, x_exact, (pair, n))
    assert runs[0].cycles == (1 if n <= 30 else 2)
    print(f"GMRES {pair} n = {n}: rtol {rtol:.3e} gap {gap:.2f} spread {sprd:.2e}")


@pytest.mark.parametrize("pair,it,ending", km.BICG_CASES)
def test_real_bicgstab_cases_are_sharp(pair, it, ending, real16):
    A1, vs, b, x_exact = real16[pair]
    rtol, gap = km.real_case(km.bicgstab_real, A1, vs[0], b, km.bicg_index(it, ending))
    assert gap >= km.GAP, (pair, it, ending, gap)  # the gap at BOTH tests of the deciding iteration: every earlier norm is above
    runs = [km.bicgstab_real(A1, v["precond"], b, rtol, km.REAL_MAX_ITER, reverse=v["reverse"]) for v in vs]
    sprd = _sharp(runs, it, x_exact, (pair, it, ending))
    assert [r.where for r in runs] == [ending, ending]
    print(f"BiCGStab {pair} iteration {it} ({ending} step): rtol {rtol:.3e} gap {gap:.2f} spread {sprd:.2e}")


@pytest.mark.parametrize("adjoint,case", [(False, c) for c in km.COMPLEX_CASES] + [(True, c) for c in km.ADJOINT_CASES])
def test_complex_gmres_cases_are_sharp(adjoint, case, open10):
    A, E, vs = open10
    sigma, m, n = case
    Mop = km.shifted_op(A, E, sigma, adjoint)
    b = km.complex_rhs(1, A.shape[0], 5)[0]
    rtol, gap = km.complex_case(Mop, vs[adjoint][0], b, m, n)
    assert gap >= km.GAP
    runs = [km.gmres_complex(Mop, v["precond"], b, rtol, km.COMPLEX_MAX_ITER, m, reverse=v["reverse"]) for v in vs[adjoint]]
    sprd = _sharp(runs, n, spla.splu(sp.csc_matrix(Mop)).solve(b), case)
    assert runs[0].cycles == -(-n // m)
    print(f"complex GMRES({m}) at {sigma} adjoint {adjoint} n = {n}: rtol {rtol:.3e} gap {gap:.2f} spread {sprd:.2e}")


def test_the_capped_case_ends_inside_a_cycle(open10):
    A, E, vs = open10
    sigma, m, cap, rtol = km.CAPPED_CASE
    b = km.complex_rhs(1, A.shape[0], 5)[0]
    runs = [km.gmres_complex(km.shifted_op(A, E, sigma), v["precond"], b, rtol, cap, m, reverse=v["reverse"]) for v in vs[False]]
    for r in runs:
        assert r.code == km.NOT_CONVERGED and r.iters == cap and r.cycles == 2
        assert r.history[-1] >= km.GAP * rtol * r.history[0]


@pytest.mark.parametrize("k", km.BLOCK_KS)
def test_block_cases_are_sharp(k, open10):
    A, E, vs = open10
    N = A.shape[0]
    sig, B = km.block_columns(k, N)
    Mops = [km.shifted_op(A, E, s) for s in sig]
    hist = [km.gmres_complex(M, vs[False][0]["precond"], b, 1e-300, 12, km.BLOCK_RESTART).history for M, b in zip(Mops, B)]
    rtol, gap, counts = km.block_rtol(hist)
    assert gap >= km.GAP, gap
    runs = [km.gmres_block(Mops, v["precond"], B, rtol, km.BLOCK_MAX_ITER, km.BLOCK_RESTART, reverse=v["reverse"]) for v in vs[False]]
    for res, cycles, launched in runs:
        assert [r.iters for r in res] == counts and all(r.code == km.OK for r in res)
    assert runs[0][1:] == runs[1][1:]
    assert max(counts) - min(counts) >= 3
    assert min(counts) <= km.BLOCK_RESTART and max(counts) > 2 * km.BLOCK_RESTART, "one column done in the first cycle, another in a third"
    assert runs[0][1] == -(-max(counts) // km.BLOCK_RESTART)
    for c in range(k):  # a column of a block is the single-column run: the budget is far away
        one = km.gmres_complex(Mops[c], vs[False][0]["precond"], B[c], rtol, km.BLOCK_MAX_ITER, km.BLOCK_RESTART)
        assert one.iters == counts[c] and np.array_equal(one.x, runs[0][0][c].x)
        x_exact = spla.splu(sp.csc_matrix(Mops[c])).solve(B[c]) if c < 8 else None
        if x_exact is not None:
            _sharp([runs[0][0][c], runs[1][0][c]], counts[c], x_exact, (k, c))
    print(f"block k = {k}: rtol {rtol:.3e} gap {gap:.2f} counts {counts} cycles {runs[0][1]} lock-step iterations {runs[0][2]}")


def test_the_lock_step_budget_cuts_the_cycles_of_every_column(open10):
    """max_iter counts lock-step iterations (the longest column of every cycle): with a budget of 5 and restart 3 the second cycle is
    cut to 2 columns for all, and the columns that would have needed more miss the tolerance."""
    A, E, vs = open10
    sig, B = km.block_columns(5, A.shape[0])
    Mops = [km.shifted_op(A, E, s) for s in sig]
    res, cycles, launched = km.gmres_block(Mops, vs[False][0]["precond"], B, 3.7e-8, 5, 3)
    assert cycles == 2 and launched == 5
    assert max(r.iters for r in res) == 5 and min(r.iters for r in res) == 3
    assert [r.code for r in res].count(km.NOT_CONVERGED) >= 1
