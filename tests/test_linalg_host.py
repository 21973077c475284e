"""flowcontrol_amd.linalg without a GPU: the Krylov-Schur driver on a numpy backend, the frequency-response loop and its argument
checks on a scipy backend (the reference's tests/test_linalg.py cases), and the symbolic phase of the complex-shifted solver."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd import linalg


class NumpyKrylov:
    """The vector side of linalg.krylov_schur in numpy (what DeviceKrylov does on the device)."""

    def __init__(self, A, E, sigma):
        self.A, self.E, self.n = A.tocsc(), E.tocsc(), A.shape[0]
        self.lu = spla.splu((self.A - sigma * self.E).astype(complex).tocsc())

    def op(self, v):
        return self.lu.solve(self.E @ v)

    def start(self, m, v0):
        self.V = np.zeros((self.n, m + 1), dtype=complex)
        w = self.op(v0)
        self.V[:, 0] = w / np.linalg.norm(w)

    def step(self, j):
        w = self.op(self.V[:, j])
        h = np.zeros(j + 1, dtype=complex)
        for _ in range(2):
            c = self.V[:, : j + 1].conj().T @ w
            w = w - self.V[:, : j + 1] @ c
            h += c
        beta = np.linalg.norm(w)
        self.V[:, j + 1] = w / beta
        return h, beta

    def restart(self, Q):
        m, k = Q.shape
        self.V[:, :k] = self.V[:, :m] @ Q
        self.V[:, k] = self.V[:, m]

    def ritz(self, Y, lam, vectors):
        X = self.V[:, : Y.shape[0]] @ Y
        AX, EX = self.A @ X, self.E @ X
        res = np.stack([np.linalg.norm(AX - EX * lam, axis=0), np.linalg.norm(AX, axis=0), np.linalg.norm(EX, axis=0)], axis=1)
        return res, (X if vectors else None)


def _pencil(n=300, seed=3):
    """Random sparse pencil with a singular E: zero rows / columns on the last fifth (a pressure block's constraint rows)."""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.03, random_state=rng) + sp.diags(rng.uniform(-4.0, 1.0, n))
    d = rng.uniform(0.5, 2.0, n)
    d[4 * n // 5:] = 0.0
    E = sp.diags(d) + 0.0 * sp.random(n, n, density=0.01, random_state=rng)
    return sp.csr_matrix(A), sp.csr_matrix(E)


@pytest.mark.parametrize("sigma", [0.3 + 0.5j, -0.2 + 0.0j])
def test_krylov_schur_matches_eigs(sigma):
    A, E = _pencil()
    nev = 4
    lam, X, stats = linalg.krylov_schur(NumpyKrylov(A, E, sigma), nev, 20, sigma, tol=1e-12, maxit=200)
    ref = spla.eigs(A.astype(complex), k=nev, M=E.astype(complex), sigma=sigma, which="LM", return_eigenvectors=False, tol=1e-14)
    ref = ref[np.argsort(np.abs(ref - sigma))]
    assert lam.shape == (nev,) and X.shape == (A.shape[0], nev)
    # (a conjugate pair is equally near a real shift: compare as sets)
    assert max(np.min(np.abs(ref - v)) for v in lam) <= 1e-10
    assert max(np.min(np.abs(lam - v)) for v in ref) <= 1e-10
    # nearest sigma first, converged in the pencil's sense, unit vectors
    assert np.all(np.diff(np.abs(lam - sigma)) >= -1e-12)
    for i in range(nev):
        x = X[:, i]
        assert abs(np.linalg.norm(x) - 1.0) < 1e-12
        assert np.linalg.norm(A @ x - lam[i] * (E @ x)) <= 1e-10 * np.linalg.norm(A @ x)


def test_krylov_schur_argument_checks():
    A, E = _pencil(60)
    with pytest.raises(ValueError):
        linalg.krylov_schur(NumpyKrylov(A, E, 0.1), 20, 20, 0.1)


class ScipyShifted:
    """Host stand-in for linalg.ShiftedOperator (factor(sigma) / transfer(B, C)) in the frequency-response loop."""

    def __init__(self, A, Q):
        self.A, self.Q = sp.csc_matrix(A), sp.csc_matrix(Q)

    def factor(self, sigma):
        self.lu = spla.splu((sigma * self.Q - self.A).astype(complex).tocsc())

    def transfer(self, B, Cm):
        return Cm @ self.lu.solve(B.astype(complex))


def test_frequency_response_siso_analytic():
    """Reference tests/test_linalg.py: H(w) = 1/(jw+1) + 1/(jw+2) for A = diag(-1, -2), Q = I, B = [1, 1]^T, C = [1, 1]."""
    A = sp.diags([-1.0, -2.0], format="csc")
    Q = sp.eye(2, format="csc")
    B = np.array([[1.0], [1.0]])
    Cm = np.array([[1.0, 1.0]])
    ww = np.array([0.1, 1.0, 5.0, 20.0])
    H, ww_out = linalg.frequency_response(ScipyShifted(A, Q), B, Cm, ww, verbose=False)
    ref = (1.0 / (1j * ww + 1.0) + 1.0 / (1j * ww + 2.0)).reshape(1, 1, -1)
    assert H.shape == (1, 1, 4)
    np.testing.assert_allclose(H, ref, atol=1e-12)
    np.testing.assert_allclose(ww_out, ww)


def test_frequency_response_mimo_shape():
    n = 4
    A = sp.diags([-float(i + 1) for i in range(n)], format="csc")
    Q = sp.eye(n, format="csc")
    B = np.random.default_rng(0).standard_normal((n, 3))
    Cm = np.random.default_rng(1).standard_normal((2, n))
    ww = np.linspace(0.1, 10.0, 4)
    assert linalg._freqresp_sizes(A, B, Cm, ww) == (4, 3, 2, 4)
    H, _ = linalg.frequency_response(ScipyShifted(A, Q), B, Cm, ww, verbose=False)
    assert H.shape == (2, 3, 4) and np.all(np.isfinite(H))


def test_argument_checks():
    A = sp.diags([-1.0, -2.0], format="csr")
    Q = sp.eye(2, format="csr")
    with pytest.raises(ValueError, match="square"):
        linalg._freqresp_sizes(sp.csr_matrix(np.ones((2, 3))), np.ones((2, 1)), np.ones((1, 2)), [1.0])
    with pytest.raises(ValueError, match="non-empty"):
        linalg._freqresp_sizes(A, np.ones((2, 1)), np.ones((1, 2)), [])
    with pytest.raises(ValueError):
        linalg._freqresp_sizes(A, np.ones((3, 1)), np.ones((1, 2)), [1.0])
    for fn in (linalg.get_frequency_response_sequential, linalg.get_frequency_response_parallel, linalg.get_frequency_response_mpi):
        with pytest.raises(ValueError, match="flowsolver"):
            fn(A, np.ones((2, 1)), np.ones((1, 2)), Q, [1.0], verbose=False)
    with pytest.raises(ValueError, match="flowsolver"):
        linalg.get_field_response(A, np.ones((2, 1)), Q, [1.0])
    with pytest.raises(ValueError, match="flowsolver"):
        linalg.get_mat_vp(A, Q, n=1)
    assert linalg.get_mat_vp_slepc is linalg.get_mat_vp


def test_values_on_pattern():
    rowptr = np.array([0, 2, 3], dtype=np.int32)
    colidx = np.array([0, 1, 1], dtype=np.int32)
    M = sp.csr_matrix(np.array([[2.0, 3.0], [0.0, 4.0]]))
    np.testing.assert_array_equal(linalg.values_on_pattern(M, rowptr, colidx), [2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="outside"):
        linalg.values_on_pattern(sp.csr_matrix(np.array([[2.0, 0.0], [1.0, 4.0]])), rowptr, colidx)


def test_utils_reexports():
    from flowcontrol_amd import utils

    for name in ("get_frequency_response_sequential", "get_frequency_response_parallel", "get_frequency_response_mpi",
                 "get_field_response", "get_mat_vp", "get_mat_vp_slepc"):
        assert getattr(utils, name) is getattr(linalg, name)


def _sym_tables(fn, *args):
    from flowcontrol_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(fn(*args, C.byref(h)))
    try:
        out = {}
        for name in ("perm", "plan_nodes", "node_i0"):
            n = C.c_int64()
            if lib.fc_sym_size(h, name.encode(), C.byref(n)) != 0:
                continue
            v = np.empty(n.value, dtype=np.int64)
            _lib.check(lib.fc_sym_get(h, name.encode(), v))
            out[name] = v
        return out
    finally:
        lib.fc_sym_free(h)


def test_shifted_symbolic_phase_on_O1():
    """The doubled tree of fc_setup_shifted (fc_sym_build_shifted): the (re, im) pair of every dof lands in the same tree node, and
    every node is exactly twice the real tree's (same mesh, no skipped dofs)."""
    from flowcontrol_amd import _lib
    from flowcontrol_amd.examples.data import mesh_file
    from flowcontrol_amd.fem.mesh import read_xdmf_mesh

    lib = _lib.load()
    m = read_xdmf_mesh(mesh_file("O1"))
    args = (m.num_vertices, m.num_edges, m.num_cells, np.ascontiguousarray(m.coords, dtype=np.float64),
            np.ascontiguousarray(m.cells, dtype=np.int32), np.ascontiguousarray(m.cell_edges, dtype=np.int32))
    real = _sym_tables(lib.fc_sym_build, *args, 0, None, 0, 2, 1, 0, 0)
    dbl = _sym_tables(lib.fc_sym_build_shifted, *args, 0, 2)
    N = real["perm"].size
    assert dbl["perm"].size == 2 * N
    pn_r, pn_d = real["plan_nodes"].reshape(-1, 7), dbl["plan_nodes"].reshape(-1, 7)
    assert pn_r.shape == pn_d.shape
    np.testing.assert_array_equal(pn_d[:, 0], pn_r[:, 0])       # levels
    np.testing.assert_array_equal(pn_d[:, 2], 2 * pn_r[:, 2])   # front orders
    np.testing.assert_array_equal(pn_d[:, 3], 2 * pn_r[:, 3])   # pivot orders
    # node of every doubled dof
    iperm = np.empty(2 * N, dtype=np.int64)
    iperm[dbl["perm"]] = np.arange(2 * N)
    i0, ni = dbl["node_i0"], pn_d[:, 3]
    node = np.searchsorted(i0, iperm, side="right") - 1
    assert np.all(iperm < i0[node] + ni[node])
    np.testing.assert_array_equal(node[0::2], node[1::2])

