"""The optimal-perturbation iteration of ``flowcontrol_amd.transient`` on the numpy block backend of tests/support/optpert_model.py,
against a dense ``scipy.linalg.eigh(Phi^T M Phi, M_ff)`` (CPU only).  The figures in ``optpert_model.CASES`` are of that host model."""
import numpy as np
import pytest

from flowcontrol_amd import transient as tr
from tests.support import optpert_model as om


@pytest.fixture(scope="module")
def problems():
    return {(8, 8): om.host_problem(8, 8), (7, 5): om.host_problem(7, 5)}


def run_case(problems, name, x0=None):
    c = om.CASES[name]
    model, th = problems[(c["nx"], c["ny"])]
    be = om.ModelBlocks(model, c["k"], 2 * th.nn)
    tr.orthonormalise_start(be, tr.start_block(c["k"], be.N, x0, om.SEED, be.free))
    res = tr.subspace_iteration(be, c["n"], c["n_modes"], c["tol"], 60, om.FIRST_ORDER, 1e-13)
    return c, be, res


@pytest.fixture(scope="module")
def solved(problems):
    return {name: run_case(problems, name) for name in om.CASES}


@pytest.mark.parametrize("name", list(om.CASES))
def test_iteration_against_dense_eigh(solved, name):
    c, be, res = solved[name]
    w, _ = om.dense_reference(be, c["n"], om.FIRST_ORDER)
    m = c["n_modes"]
    gap = np.max(np.abs(res.gains - w[:m]))
    G = be.gram("U", "U", True)
    orth = np.max(np.abs(G - np.eye(c["k"])))
    print(f"{name}: iterations {res.iterations}, gains {res.gains}, |gain - dense| {gap:.2e}, |U^T M U - I| {orth:.2e}, residuals {res.residuals}")
    assert res.converged and np.all(res.residuals <= c["tol"])
    assert gap <= 1e-10 * w[0]
    assert orth <= 1e-12
    assert res.iterations <= c["iterations"]
    assert np.allclose(res.gains, c["gains"], rtol=2e-3)  # (the table's printed digits)
    # the modes are M-orthonormal, zero outside f, and the responses are their forward runs
    V = res.modes
    assert np.max(np.abs(V @ (be.M @ V.T) - np.eye(m))) <= 1e-12
    assert not np.any(V[:, be.fmask == 0.0])
    assert len(res.history) == res.iterations and res.n_steps == c["n"]


@pytest.mark.parametrize("name", list(om.CASES))
def test_rayleigh_property(solved, name):
    """theta_i is the energy ratio of a forward run from mode i."""
    c, be, res = solved[name]
    for i in range(c["n_modes"]):
        ratio = om.energy_ratio(be, res.modes[i], c["n"], om.FIRST_ORDER)
        assert abs(ratio - res.gains[i]) <= 1e-12 * res.gains[0], (i, ratio, res.gains[i])


def test_rayleigh_property_unconverged(problems):
    """... at every iteration, not only at convergence: two iterations of the first case."""
    c = om.CASES["8x8_n60"]
    model, th = problems[(8, 8)]
    be = om.ModelBlocks(model, c["k"], 2 * th.nn)
    tr.orthonormalise_start(be, tr.start_block(c["k"], be.N, None, om.SEED, be.free))
    res = tr.subspace_iteration(be, c["n"], 3, 1e-8, 2, om.FIRST_ORDER, 1e-13)
    assert not res.converged and res.iterations == 2
    for i in range(3):
        assert abs(om.energy_ratio(be, res.modes[i], c["n"], om.FIRST_ORDER) - res.gains[i]) <= 1e-12 * res.gains[0]


def test_warm_start_is_no_slower(problems, solved):
    """The n = 200 case from the n = 60 block (padded with the cold start's random columns) against its cold start."""
    c60, _, res60 = solved["8x8_n60"]
    c, _, cold = solved["8x8_n200"]
    x0 = tr.start_block(c["k"], res60.block.shape[1], None, om.SEED, solved["8x8_n200"][1].free)
    x0[: c60["k"]] = res60.block
    _, _, warm = run_case(problems, "8x8_n200", x0)
    print(f"n = 200: cold {cold.iterations} iterations, warm {warm.iterations}")
    assert warm.converged and warm.iterations <= cold.iterations
    assert np.max(np.abs(warm.gains - cold.gains)) <= 1e-10 * cold.gains[0]


def test_jacobi_cg_of_the_model(problems):
    model, th = problems[(8, 8)]
    be = om.ModelBlocks(model, 4, 2 * th.nn)
    A = be.Mff
    d = 1.0 / np.sqrt(A.diagonal())
    cond = np.linalg.cond((A.toarray() * d[:, None]) * d[None, :])
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    x, it, res = om.jacobi_cg(A, b, 1e-13)
    print(f"cond(D^-1/2 M_ff D^-1/2) = {cond:.3f}, CG iterations to 1e-13: {it}")
    assert cond < 6.0 and it <= 40 and res <= 1e-13
    assert np.linalg.norm(A @ x - b) <= 2e-13 * np.linalg.norm(b)
    x0, it0, res0 = om.jacobi_cg(A, np.zeros_like(b), 1e-13)
    assert it0 == 0 and res0 == 0.0 and not np.any(x0)


def test_defaults_and_argument_checks():
    assert [tr.default_width(m) for m in (1, 2, 3, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16, 32, 32]
    assert tr.check_arguments(10, 3, None, 1e-6, 50, None) == 8
    assert tr.check_arguments(10, 3, 17, 1e-6, 50, 1) == 17
    for bad in (dict(n_steps=0), dict(n_modes=0), dict(n_modes=17), dict(k=2, n_modes=3), dict(k=33), dict(tol=0.0), dict(max_iter=0), dict(first_order=3)):
        args = dict(n_steps=10, n_modes=1, k=None, tol=1e-6, max_iter=50, first_order=None)
        args.update(bad)
        with pytest.raises(ValueError):
            tr.check_arguments(**args)
    with pytest.raises(ValueError, match="x0 must be"):
        tr.start_block(4, 10, np.zeros((3, 10)), 0, np.arange(5))


def test_nonlinear_solver_is_refused():
    class Params:
        is_eq_nonlinear = True

    class Fs:
        params_solver = Params()

    with pytest.raises(ValueError, match="is_eq_nonlinear=False"):
        tr.optimal_perturbations(Fs(), 10)
    with pytest.raises(ValueError, match="is_eq_nonlinear=False"):
        tr.transient_growth(Fs(), [10, 20])


def test_rank_deficient_block_raises_with_the_iteration(problems):
    """Equal columns: the Cholesky of the start block fails and says so; nothing is repaired quietly."""
    model, th = problems[(7, 5)]
    be = om.ModelBlocks(model, 4, 2 * th.nn)
    x = np.random.default_rng(0).standard_normal((1, be.N))
    with pytest.raises(RuntimeError, match="start block"):
        tr.orthonormalise_start(be, np.repeat(x, 4, axis=0))


def test_flu_names():
    from flowcontrol_amd import utils as flu
    from flowcontrol_amd.flowsolver import FlowSolver

    assert flu.optimal_perturbations is tr.optimal_perturbations and flu.transient_growth is tr.transient_growth and flu.mass_solve is tr.mass_solve
    assert callable(FlowSolver.optimal_perturbations)


class _BrokenApply:
    """The model backend with an apply whose Rayleigh matrix is tampered with from iteration ``at`` on."""

    def __init__(self, be, at, how):
        self.be, self.at, self.how, self.calls = be, at, how, 0
        self.k, self.N, self.free = be.k, be.N, be.free

    def __getattr__(self, name):
        return getattr(self.be, name)

    def apply(self, n_steps, first_order):
        H, E = self.be.apply(n_steps, first_order)
        self.calls += 1
        if self.calls >= self.at and self.how == "indefinite":
            H = H - 2.0 * np.max(np.abs(H)) * np.eye(self.k)
        if self.calls >= self.at and self.how == "rank":  # the block collapses onto its first column: V S Theta^-1 has rank one
            self.be.blocks["G"] = np.repeat(self.be.blocks["G"][:1], self.k, axis=0)
        return H, E


@pytest.mark.parametrize("how, match", [("indefinite", "non-positive gain"), ("rank", "not positive definite")])
def test_failures_inside_the_iteration_name_the_iteration(problems, how, match):
    """A non-positive theta and a failed Cholesky of the block update raise with the number of the iteration they happened in."""
    model, th = problems[(7, 5)]
    be = om.ModelBlocks(model, 4, 2 * th.nn)
    tr.orthonormalise_start(be, tr.start_block(4, be.N, None, om.SEED, be.free))
    with pytest.raises(RuntimeError, match=match) as e:
        tr.subspace_iteration(_BrokenApply(be, 2, how), 10, 1, 1e-12, 6, 1, 1e-13)
    assert "iteration 2" in str(e.value), str(e.value)
