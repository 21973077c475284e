"""The layout identity behind the adjoint mode of the shifted solver, on the host: the per-node transposition of the factor values
(tests/support/adjoint_layout.py, the model of ``fc_fe_export_t``) makes the project's own host multifrontal solve with M^H, and the
rule that gathers the values of A^T, E^T on the handle's pattern is an involutive permutation."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import TaylorHood
from tests.support import adjoint_layout, nd_numeric, ndsolver


def _doubled_problem(nx, ny, depth):
    """A random complex matrix M on the Taylor-Hood pattern of the nx x ny unit square, its real-equivalent form (dof i -> 2 i,
    2 i + 1; entry m -> [[mr, -mi], [mi, mr]]) and the block factors of the latter."""
    th = TaylorHood(Mesh.unit_square(nx, ny))
    N = th.N
    cd = np.asarray(th.cell_dofs)
    cd2 = np.stack([2 * cd, 2 * cd + 1], axis=-1).reshape(cd.shape[0], -1)
    tree = ndsolver.build_tree(cd2, th.mesh.cell_centroids(), 2 * N, depth)
    rows, cols = np.repeat(cd, cd.shape[1], axis=1).ravel(), np.tile(cd, (1, cd.shape[1])).ravel()
    P = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(N, N))
    rng = np.random.default_rng(nx)
    M = P.astype(complex).tocsr()
    M.data = rng.standard_normal(M.nnz) + 1j * rng.standard_normal(M.nnz)
    M = (M + sp.diags(np.full(N, 40.0 + 5j))).tocsr()
    Mc = M.tocoo()
    r2 = np.concatenate([2 * Mc.row, 2 * Mc.row, 2 * Mc.row + 1, 2 * Mc.row + 1])
    c2 = np.concatenate([2 * Mc.col, 2 * Mc.col + 1, 2 * Mc.col, 2 * Mc.col + 1])
    v2 = np.concatenate([Mc.data.real, -Mc.data.imag, Mc.data.imag, Mc.data.real])
    R = sp.csr_matrix((v2, (r2, c2)), shape=(2 * N, 2 * N))
    fac = nd_numeric.factorize_blocks(R, tree)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    return th, M, fac, b


def _solve(fac, b):
    bi = np.empty(2 * b.size)
    bi[0::2], bi[1::2] = b.real, b.imag
    x = nd_numeric.block_solve(fac, bi)
    return x[0::2] + 1j * x[1::2]


def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("nx,ny,depth", [(4, 4, 2), (6, 5, 3)])
def test_transposed_layout_solves_with_the_adjoint(nx, ny, depth):
    """block_solve on the model's output == scipy's solve with M^H to 1e-12 (5e-16 measured with OpenBLAS; the margin covers other
    BLAS builds), and it is NOT the solve with the plain transpose; the model is an involution."""
    _, M, fac, b = _doubled_problem(nx, ny, depth)
    direct = fac.vals.copy()
    assert _rel(_solve(fac, b), spla.spsolve(M.tocsc(), b)) <= 1e-12
    fac.vals = adjoint_layout.transpose_values(direct, fac.nodes, "block")
    assert not np.array_equal(fac.vals, direct)
    y = _solve(fac, b)
    refH = spla.spsolve(M.conj().T.tocsc(), b)
    print(nx, ny, "nodes", len(fac.nodes), "adjoint error", _rel(y, refH))
    assert _rel(y, refH) <= 1e-12
    assert _rel(y, spla.spsolve(M.T.tocsc(), b)) > 1e-3
    assert np.array_equal(adjoint_layout.transpose_values(fac.vals, fac.nodes, "block"), direct)


def test_both_node_tables_give_the_same_model():
    """plan_nodes ([g, 7]) and BlockFactors.nodes describe the same blocks."""
    _, _, fac, _ = _doubled_problem(4, 4, 2)
    plan = ndsolver.factor_plan(fac, np.zeros(fac.N + 1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    rng = np.random.default_rng(1)
    v = rng.standard_normal(fac.vals.size)
    assert np.array_equal(adjoint_layout.transpose_values(v, plan.nodes, "plan"), adjoint_layout.transpose_values(v, fac.nodes, "block"))


def test_transpose_positions_on_the_taylor_hood_pattern():
    """tpos is a permutation with tpos[tpos[k]] = k, and it turns the values of a matrix into those of its transpose."""
    th = TaylorHood(Mesh.unit_square(6, 5))
    cd = np.asarray(th.cell_dofs)
    rows, cols = np.repeat(cd, cd.shape[1], axis=1).ravel(), np.tile(cd, (1, cd.shape[1])).ravel()
    P = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(th.N, th.N))
    P.sum_duplicates()
    P.sort_indices()
    rp, col = P.indptr, P.indices
    tpos = adjoint_layout.transpose_positions(rp, col)
    assert np.array_equal(np.sort(tpos), np.arange(col.size))
    assert np.array_equal(tpos[tpos], np.arange(col.size))
    rng = np.random.default_rng(2)
    v = rng.standard_normal(col.size)
    At = sp.csr_matrix((v, col, rp), shape=P.shape).T.tocsr()
    At.sort_indices()
    assert np.array_equal(At.indices, col) and np.array_equal(At.data, v[tpos])
    # an entry without a partner is refused
    bad = sp.csr_matrix(np.array([[1.0, 1.0], [0.0, 1.0]]))
    with pytest.raises(ValueError, match="no partner"):
        adjoint_layout.transpose_positions(bad.indptr, bad.indices)
