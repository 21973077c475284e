"""The pivot-stress matrices of tests/support/front_cases.py do what tests/test_front_elimination_gpu.py relies on (CPU only):
they are well conditioned, their elimination needs row exchanges inside the pivot blocks and nothing wider, and the exchanges
reach every path of the front kernels -- judged by the numpy model of the device's order of operations, never by the device."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import front_cases as fcs
from tests.support import nd_numeric

_cache: dict = {}


def _case(name):
    """Per case, computed once: tree, and per seed the matrix, the LAPACK-based host factors and the model at 32 / 64 / 128."""
    if name not in _cache:
        _, nx, ny, bits, _, _ = next(c for c in fcs.CASES if c[0] == name)
        th, dofs, tree = fcs.host_case(nx, ny, bits)
        rowptr, colidx = fcs.taylor_hood_pattern(th)
        per_seed = {}
        for seed in fcs.SEEDS:
            vals = fcs.pivot_stress_matrix(rowptr, colidx, tree, dofs, seed)
            A = sp.csr_matrix((vals, colidx, rowptr), shape=(th.N, th.N))
            host = nd_numeric.factorize_blocks(A, tree)
            per_seed[seed] = dict(A=A, host=host, model={kb: fcs.model_elimination(A, tree, kb) for kb in (32, 64, 128)})
        _cache[name] = dict(th=th, dofs=dofs, tree=tree, seeds=per_seed)
    return _cache[name]


NAMES = [c[0] for c in fcs.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_tree_shapes_are_the_documented_ones(name):
    """The geometry the cases were chosen for (front_cases.CASES)."""
    fronts = fcs.level_fronts(_case(name)["tree"])
    root, below = fronts[-1], fronts[-2]
    assert len(root) == 1 and root[0][0] == root[0][1]
    want = {"square8": (77, 33, 35), "wide16x9": (192, 73, 75), "huge20x9": (232, 380, 387), "huge16x16": (157, 576, 580)}[name]
    assert (root[0][0], min(ni for ni, _ in below), max(ni for ni, _ in below)) == want
    widths = {route: fcs.predicted_step_widths(_case(name)["tree"], route).tolist() for route in fcs.ROUTES}
    assert set(widths["default"]) == {32}
    if name == "square8":
        assert widths["wide"] == [32, 64, 64] and widths["huge"] == [32, 32, 32]  # leaves of order 57-59: no level qualifies for 128 columns
    elif name == "wide16x9":
        assert widths["wide"] == [64, 64, 64] and widths["huge"] == [32, 32, 32]
    else:
        assert widths["wide"] == [64, 64] and widths["huge"] == [128, 32]


@pytest.mark.parametrize("seed", fcs.SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_model_agrees_with_the_lapack_multifrontal_at_every_width(name, seed):
    """Block-local exchanges are SUFFICIENT: the model (pivot search confined to the 32 / 64-column block, to the 32-column
    sub-block at 128) reproduces the factors of nd_numeric.factorize_blocks, which inverts every pivot block with LAPACK.
    Both are numpy fp64 on a matrix of condition <= 1e3: 1e-12 of the largest value."""
    c = _case(name)["seeds"][seed]
    ref = c["host"].vals
    for kb in (32, 64, 128):
        got = c["model"][kb][0].vals
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), kb


@pytest.mark.parametrize("seed", fcs.SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_matrices_are_well_conditioned(name, seed):
    """A condition of the GPU test's 1e-10 / 1e-11 bounds, not a measurement (150 ... 200 on these cases)."""
    A = _case(name)["seeds"][seed]["A"]
    assert np.linalg.cond(A.toarray()) <= 1e3


@pytest.mark.parametrize("seed", fcs.SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_without_exchanges_the_elimination_fails(name, seed):
    """Block-local exchanges are NECESSARY: the same model with the diagonal always kept divides by zero or loses every digit."""
    c = _case(name)
    s = c["seeds"][seed]
    got = fcs.model_elimination(s["A"], c["tree"], 32, exchange=False)[0].vals
    ref = s["host"].vals
    with np.errstate(all="ignore"):
        err = np.abs(got - ref).max()
    assert not np.isfinite(got).all() or err > 1e-4 * np.abs(ref).max()


def test_forced_exchanges_reach_every_kernel_path():
    """The mandatory exchanges of the model (|diagonal| < 2**-10 |largest candidate|) and the trees, over all cases and seeds,
    counted only on the levels that take the width in question on the device (front_cases.census).
    At 64 columns a front of order < 64 cannot occur (such a level takes 32-column steps unless a wider front shares it); at 128
    columns the level's largest front has order >= 256, which on meshes of this size excludes root fronts and ni < 128."""
    exchanges = {"step 0", "step >= 1", "partial last block", "level with shorter fronts"}
    geometry = {"ni < KB", "ni multiple of KB, >= 2 steps", "nf not a multiple of 64", "root front"}
    required = {
        32: exchanges | geometry | {"nf < 64"},
        64: exchanges | geometry | {"k and p >= 32", "k < 16 <= p"},
        128: exchanges | {"sub-block c0 >= 32", "huge level with ni > 256", "ni multiple of KB, >= 2 steps", "nf not a multiple of 64"},
    }
    for kb, need in required.items():
        for seed in fcs.SEEDS:  # every seed on its own: the GPU test runs each seed through every route
            got = set()
            for name in NAMES:
                c = _case(name)
                got |= fcs.census(c["seeds"][seed]["model"][kb][1], c["tree"], kb)
            assert need <= got, (kb, seed, sorted(need - got))


def test_pairs_have_an_exactly_zero_diagonal_and_stay_inside_a_32_block():
    """What pivot_stress_matrix promises about its involution, checked on the matrix itself."""
    c = _case("wide16x9")
    A, tree = c["seeds"][0]["A"].tocsr(), c["tree"]
    N = A.shape[0]
    start = fcs._node_start(tree, N)
    is_bc = np.zeros(N, dtype=bool)
    is_bc[c["dofs"]] = True
    pairs = 0
    for r in np.nonzero(~is_bc)[0]:
        cols, v = A.indices[A.indptr[r] : A.indptr[r + 1]], A.data[A.indptr[r] : A.indptr[r + 1]]
        q = int(cols[np.argmax(np.abs(v))])
        if q == r or r >= 2 * c["th"].nn and tree.iperm[q] < start[tree.iperm[r]] + 32 * ((tree.iperm[r] - start[tree.iperm[r]]) // 32):
            continue  # dominant diagonal, or a pressure row anchored to an earlier column
        pairs += 1
        assert A[r, r] == 0.0
        ir, iq = int(tree.iperm[r]), int(tree.iperm[q])
        assert start[ir] == start[iq] and (ir - start[ir]) // 32 == (iq - start[iq]) // 32
    assert pairs >= 200
    assert np.array_equal(A[c["dofs"]].toarray(), np.eye(N)[c["dofs"]]) and A[:, c["dofs"]].count_nonzero() == c["dofs"].size
