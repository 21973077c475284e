"""Adjoint solves of the shifted solver on the factors it holds (``fc_shifted_set_adjoint``): the transposed export against the numpy
model of its layout, adjoint solves / lagged factors / rescue / block solves against scipy's LU with trans="H", the direct side
untouched by switching, the refusals, resolvent gains against a dense SVD and the left eigenmodes of the cylinder.  The 10 x 10 open
square problem of test_shifted_block_gpu.py (N = 1003; the doubled system's tree has 21 nodes of uneven ni, nb on three levels:
partial tiles in both panels, fronts of several tiles, a root without a boundary)."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib, linalg
from tests.support import adjoint_layout

pytestmark = pytest.mark.gpu

S0 = 0.3 + 0.7j
MAX_ITER, RESTART, RTOL = 200, 60, 1e-12


def _square_mesh(n):
    xs = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    vid = lambda i, j: i * (n + 1) + j  # noqa: E731
    cells = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            cells += [(a, b, c), (a, c, d)]
    cells = np.array(cells, dtype=np.int32)
    edge_id, edges = {}, []
    cell_edges = np.empty_like(cells)
    for c, tri in enumerate(cells):
        for k in range(3):
            key = tuple(sorted((int(tri[(k + 1) % 3]), int(tri[(k + 2) % 3]))))
            if key not in edge_id:
                edge_id[key] = len(edges)
                edges.append(key)
            cell_edges[c, k] = edge_id[key]
    return coords, cells, cell_edges, np.array(edges, dtype=np.int32)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Open:
    """The open 10 x 10 problem of test_shifted_block_gpu.py on a handle of its own: an Oseen-type operator with identity rows on the
    left / bottom velocity dofs, scipy's LU per shift (shared by all instances: the matrices are the same)."""

    _LU: dict = {}

    def __init__(self):
        self.lib = lib = _lib.load()
        self.mesh = coords, cells, cell_edges, edges = _square_mesh(10)
        self.h = h = C.c_void_p()
        self.ok(lib.fc_create(C.byref(h), 0, len(coords), len(edges), len(cells), np.ascontiguousarray(coords), cells, cell_edges))
        N, nnz, nn = C.c_int64(), C.c_int64(), C.c_int64()
        self.ok(lib.fc_get_sizes(h, C.byref(N), C.byref(nnz), C.byref(nn)))
        self.N, nnz, self.nn = N.value, nnz.value, nn.value
        self.rowptr, self.col = np.empty(self.N + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        self.ok(lib.fc_get_pattern(h, self.rowptr, self.col))
        rowptr, col, nn = self.rowptr, self.col, self.nn
        node_xy = np.vstack([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])])
        adv = np.r_[1.0 + 0.2 * np.sin(3 * node_xy[:, 1]), 0.3 * np.cos(2 * node_xy[:, 0])]
        self.ok(lib.fc_assemble_matrix(h, _lib.SLOT_SCRATCH, 0.0, -0.02, _vp(adv), -1.0, None, 1.0, 1.0, 1.0))
        self.ok(lib.fc_assemble_matrix(h, _lib.SLOT_MASS, 1.0, 0.0, None, 1.0, None, 1.0, 0.0, 0.0))
        a, self.e = np.empty(nnz), np.empty(nnz)
        self.ok(lib.fc_get_matrix_values(h, _lib.SLOT_SCRATCH, a))
        self.ok(lib.fc_get_matrix_values(h, _lib.SLOT_MASS, self.e))
        wall = np.flatnonzero((node_xy[:, 0] < 1e-12) | (node_xy[:, 1] < 1e-12))
        keep = np.ones(self.N)
        keep[np.r_[wall, nn + wall]] = 0.0
        self.A = (sp.diags(keep) @ sp.csr_matrix((a, col, rowptr), shape=(self.N, self.N)) + sp.diags(1.0 - keep)).tocsr()
        self.E = sp.csr_matrix((self.e, col, rowptr), shape=(self.N, self.N))
        self.a_on = linalg.values_on_pattern(self.A, rowptr, col, "A")
        rng = np.random.default_rng(5)
        self.b = rng.standard_normal((2, self.N)) + 1j * rng.standard_normal((2, self.N))
        self.bre, self.bim = np.ascontiguousarray(self.b.real), np.ascontiguousarray(self.b.imag)

    def ok(self, rc):
        assert rc == 0, self.lib.fc_last_error().decode()

    def lu(self, sigma):
        sigma = complex(sigma)
        if sigma not in self._LU:
            self._LU[sigma] = spla.splu((sigma * self.E - self.A).astype(complex).tocsc())
        return self._LU[sigma]

    def setup(self, sigma, refine=2):
        self.ok(self.lib.fc_setup_shifted(self.h, _vp(self.a_on), _vp(self.e), sigma.real, sigma.imag, refine))

    def krylov(self, max_iter=MAX_ITER, restart=RESTART, rtol=RTOL):
        self.ok(self.lib.fc_shifted_set_krylov(self.h, max_iter, restart, rtol))

    def adjoint(self, on):
        return self.lib.fc_shifted_set_adjoint(self.h, on)

    def adjoint_info(self):
        iv, dv = np.zeros(4, dtype=np.int64), np.zeros(2)
        self.ok(self.lib.fc_shifted_adjoint_info(self.h, _vp(iv), _vp(dv)))
        return iv, dv

    def solve(self):
        """fc_solve_shifted of the two stock right-hand sides: (rc, x [2, N], info [2])"""
        xre, xim, info = np.empty((2, self.N)), np.empty((2, self.N)), np.full(2, np.nan)
        rc = self.lib.fc_solve_shifted(self.h, 2, self.bre, _vp(self.bim), _vp(xre), _vp(xim), _vp(info))
        return rc, xre + 1j * xim, info

    def solve_block(self, sig, b):
        """(rc, x [k, N], info [k]) of fc_solve_shifted_block for the shifts sig [k] and right-hand sides b [k, N] complex"""
        sig = np.asarray(sig, dtype=complex)
        sre, sim = np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag)
        bre, bim = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
        xre, xim, info = np.empty((sig.size, self.N)), np.empty((sig.size, self.N)), np.full(sig.size, np.nan)
        rc = self.lib.fc_solve_shifted_block(self.h, sig.size, sre, sim, bre, _vp(bim), _vp(xre), _vp(xim), _vp(info))
        return rc, xre + 1j * xim, info

    def krylov_info(self, k=2):
        it, cnt = np.zeros(k, dtype=np.int32), np.zeros(5, dtype=np.int64)
        self.ok(self.lib.fc_shifted_krylov_info(self.h, _vp(it), _vp(cnt)))
        return it, cnt

    def rel_err(self, x, sigma, trans="N", b=None):
        """per column, against scipy's LU of sigma E - A applied as is ("N"), transposed ("T") or conjugate-transposed ("H")"""
        b = self.b if b is None else b
        sig = np.broadcast_to(np.asarray(sigma, dtype=complex), (len(b),))
        ref = [self.lu(s).solve(bc, trans) for s, bc in zip(sig, b)]
        return np.array([np.linalg.norm(xc - r) / np.linalg.norm(r) for xc, r in zip(x, ref)])

    def factors(self, adjoint, n_val):
        out = np.empty(n_val)
        self.ok(self.lib.fc_debug_get_shifted_factors(self.h, adjoint, n_val, out))
        return out


@pytest.fixture()
def prob():
    p = _Open()
    yield p
    p.lib.fc_destroy(p.h)


def _plan_nodes(p):
    """plan_nodes [g, 7] and n_val of the doubled system's symbolic phase (fc_sym_build_shifted: what fc_setup_shifted builds)"""
    coords, cells, cell_edges, edges = p.mesh
    sy = C.c_void_p()
    p.ok(p.lib.fc_sym_build_shifted(len(coords), len(edges), len(cells), np.ascontiguousarray(coords), cells, cell_edges, 0, 2, C.byref(sy)))
    try:
        out = {}
        for name in ("plan_nodes", "n_val"):
            n = C.c_int64()
            p.ok(p.lib.fc_sym_size(sy, name.encode(), C.byref(n)))
            v = np.empty(n.value, dtype=np.int64)
            p.ok(p.lib.fc_sym_get(sy, name.encode(), v))
            out[name] = v
    finally:
        p.lib.fc_sym_free(sy)
    return out["plan_nodes"].reshape(-1, 7), int(out["n_val"][0])


def test_transposed_export_has_the_layout_of_the_model(prob):
    """1. The downloaded adjoint array == adjoint_layout applied to the downloaded direct array, bit for bit, after the first export
    (fc_shifted_set_adjoint) and after the one a second fc_setup_shifted at another sigma ends with; two exports counted."""
    p = prob
    nodes, n_val = _plan_nodes(p)
    shapes = adjoint_layout.node_shapes(nodes, "plan")
    assert len(shapes) >= 7 and np.unique(nodes[:, 0]).size >= 3 and any(nb == 0 for _, nb, _ in shapes)
    assert any(ni % 32 for ni, _, _ in shapes) and any(nb % 32 for _, nb, _ in shapes if nb) and any(ni + nb > 64 for ni, nb, _ in shapes)
    p.setup(S0)
    p.ok(p.adjoint(1))
    for sigma in (None, 0.1 - 1.3j):
        if sigma is not None:
            p.setup(sigma)
        d, t = p.factors(0, n_val), p.factors(1, n_val)
        model = adjoint_layout.transpose_values(d, nodes, "plan")
        assert np.any(d != 0.0) and not np.array_equal(d, t)
        assert d.tobytes() != model.tobytes() and t.tobytes() == model.tobytes()
    iv, dv = p.adjoint_info()
    print("adjoint info", list(iv), list(dv))
    assert iv[0] == 1 and iv[2] == 2 and iv[3] == 1 and dv[1] == 16.0 * n_val


def test_adjoint_solves_match_scipy_H(prob):
    """2. Two complex right-hand sides in the adjoint mode against lu.solve(b, "H"): error <= 1e-9, info <= 1e-8 (the tolerances of the
    direct-mode tests); each solution is more than 1e-3 away from lu.solve(b, "T"), so the plain transpose cannot pass for it."""
    p = prob
    p.setup(S0)
    p.ok(p.adjoint(1))
    rc, x, info = p.solve()
    p.ok(rc)
    err, err_t = p.rel_err(x, S0, "H"), p.rel_err(x, S0, "T")
    print("adjoint solve: error", err, "residual", info, "distance to the transposed solve", err_t)
    assert np.all(err <= 1e-9) and np.all(info <= 1e-8)
    assert np.all(err_t > 1e-3)
    # (s E^T - t A^T) x with s as given
    xs = np.random.default_rng(9).standard_normal(2 * p.N)
    y = np.empty(2 * p.N)
    p.ok(p.lib.fc_shifted_spmv(p.h, 0.4, -0.9, 1.0, xs, y))
    ref = ((0.4 - 0.9j) * p.E.T - p.A.T) @ xs.view(np.complex128)
    assert np.linalg.norm(y.view(np.complex128) - ref) <= 1e-13 * np.linalg.norm(ref)


def test_lagged_factors_and_rescue_in_the_adjoint_mode(prob):
    """3. Factors at 0.3 + 0.7i, operator moved to 0.3 + 0.75i, GMRES(60, 1e-12) in the adjoint mode: error <= 1e-9 against the "H"
    solve AT THE NEW SHIFT, iterations in [1, 200].  Rescue: refine = 0 and both factor arrays off by 1e-4
    (fc_debug_scale_shifted_factors): GMRES takes over, counted as a rescue."""
    p = prob
    S2 = 0.3 + 0.75j
    p.setup(S0)
    p.krylov()
    p.ok(p.adjoint(1))
    p.ok(p.lib.fc_shifted_set_shift(p.h, S2.real, S2.imag))
    rc, x, info = p.solve()
    p.ok(rc)
    it, cnt = p.krylov_info()
    err = p.rel_err(x, S2, "H")
    print("lagged, adjoint: error", err, "residual", info, "iterations", list(it))
    assert np.all(err <= 1e-9) and np.all((1 <= it) & (it <= 200)) and cnt[0] == 1
    assert np.all(p.rel_err(x, S0, "H") > 1e-3)
    p.setup(S0, refine=0)
    p.ok(p.lib.fc_debug_scale_shifted_factors(p.h, 1.0 + 1e-4))
    _, cnt0 = p.krylov_info()
    rc, x, info = p.solve()
    p.ok(rc)
    it, cnt = p.krylov_info()
    err = p.rel_err(x, S0, "H")
    print("rescue, adjoint: error", err, "residual", info, "iterations", list(it), "counters", list(cnt))
    assert np.all(info <= RTOL) and np.all(err <= 1e-9)
    assert np.all((1 <= it) & (it <= 200)) and cnt[4] - cnt0[4] == 2


@pytest.mark.parametrize("k", [4, 8])
def test_block_solves_in_the_adjoint_mode(prob, k):
    """4. k columns at their own shifts over 0.3 + [0.6, 0.8]i in the adjoint mode against the per-shift "H" solves: <= 1e-9; back in
    the direct mode the same call matches the direct references: the tiled copy of the factors was repacked."""
    p = prob
    sig = 0.3 + 1j * np.linspace(0.6, 0.8, k)
    sig[k // 2] = S0
    rng = np.random.default_rng(11)
    b = rng.standard_normal((k, p.N)) + 1j * rng.standard_normal((k, p.N))
    p.setup(S0)
    p.krylov()
    p.ok(p.lib.fc_shifted_set_block(p.h, k))
    p.ok(p.adjoint(1))
    rc, x, info = p.solve_block(sig, b)
    p.ok(rc)
    err = p.rel_err(x, sig, "H", b)
    print("block of", k, "adjoint: worst error", err.max(), "worst residual", info.max())
    assert np.all(err <= 1e-9) and np.all(info <= RTOL)
    assert np.all(p.rel_err(x, sig, "N", b) > 1e-3)
    p.ok(p.adjoint(0))
    rc, x, info = p.solve_block(sig, b)
    p.ok(rc)
    err = p.rel_err(x, sig, "N", b)
    print("block of", k, "direct again: worst error", err.max())
    assert np.all(err <= 1e-9) and np.all(info <= RTOL)


def test_switching_leaves_the_direct_side_alone(prob):
    """5. The two right-hand sides solved in the direct mode before the adjoint side ever existed, after on / off, and after
    fc_shifted_set_adjoint(-1): the same bits.  The adjoint side holds more than the factor size while it exists and nothing before
    and after; fc_shifted_info counts it."""
    p = prob
    _, n_val = _plan_nodes(p)

    def device_bytes():
        iv = np.zeros(4, dtype=np.int64)
        p.ok(p.lib.fc_shifted_info(p.h, _vp(iv), None, None))
        return int(iv[1])

    p.setup(S0)
    assert p.adjoint_info()[0][1] == 0
    rc, x0, _ = p.solve()
    p.ok(rc)
    base = device_bytes()  # (after the first solve: it allocates the solver's right-hand side and solution buffers)
    p.ok(p.adjoint(1))
    held = int(p.adjoint_info()[0][1])
    assert held > 8 * n_val and device_bytes() == base + held
    rc, xa, _ = p.solve()
    p.ok(rc)
    assert np.all(p.rel_err(xa, S0, "H") <= 1e-9)
    p.ok(p.adjoint(0))
    assert p.adjoint_info()[0][1] == held
    rc, x1, _ = p.solve()
    p.ok(rc)
    p.ok(p.adjoint(1))
    p.ok(p.adjoint(-1))
    iv, _ = p.adjoint_info()
    assert iv[0] == 0 and iv[1] == 0 and device_bytes() == base
    rc, x2, _ = p.solve()
    p.ok(rc)
    assert np.array_equal(x1, x0) and np.array_equal(x2, x0)
    assert np.all(p.rel_err(x0, S0) <= 1e-9)


def test_refusals(prob):
    """6. Before the first setup: FC_ERR_NOT_READY; on = 2: FC_ERR_INVALID; the resolvent operator without the adjoint array and an
    Arnoldi step after a switch: FC_ERR_NOT_READY; nothing was enqueued: the next direct solve passes."""
    p = prob
    assert p.adjoint(1) == _lib.FC_ERR_NOT_READY
    assert p.adjoint(0) == _lib.FC_ERR_NOT_READY
    p.setup(S0)
    assert p.adjoint(2) == _lib.FC_ERR_INVALID and p.adjoint(-2) == _lib.FC_ERR_INVALID
    assert p.lib.fc_shifted_arnoldi_set_op(p.h, 1) == _lib.FC_ERR_NOT_READY
    assert p.lib.fc_shifted_arnoldi_set_op(p.h, 2) == _lib.FC_ERR_INVALID
    out = np.empty(8)
    assert p.lib.fc_debug_get_shifted_factors(p.h, 1, 8, out) == _lib.FC_ERR_INVALID  # (wrong size)
    assert p.adjoint_info()[0][1] == 0
    rc, x, _ = p.solve()
    p.ok(rc)
    assert np.all(p.rel_err(x, S0) <= 1e-9)
    v0 = np.random.default_rng(3).standard_normal(2 * p.N)
    hcol, beta = np.empty(2 * 6), C.c_double()
    p.ok(p.lib.fc_shifted_arnoldi_start(p.h, 5, v0))
    p.ok(p.lib.fc_shifted_arnoldi_step(p.h, 0, hcol, C.byref(beta)))
    p.ok(p.adjoint(1))
    assert p.lib.fc_shifted_arnoldi_step(p.h, 1, hcol, C.byref(beta)) == _lib.FC_ERR_NOT_READY
    p.ok(p.lib.fc_shifted_arnoldi_start(p.h, 5, v0))
    p.ok(p.lib.fc_shifted_arnoldi_step(p.h, 0, hcol, C.byref(beta)))
    p.ok(p.adjoint(1))  # (no switch: the basis stays)
    p.ok(p.lib.fc_shifted_arnoldi_step(p.h, 1, hcol, C.byref(beta)))
    p.ok(p.adjoint(0))
    assert p.lib.fc_shifted_arnoldi_step(p.h, 2, hcol, C.byref(beta)) == _lib.FC_ERR_NOT_READY
    rc, x2, _ = p.solve()
    p.ok(rc)
    assert np.array_equal(x2, x)


class _HostedOperator:
    """What ShiftedOperator needs of a flowsolver, on the handle of an _Open problem."""

    def __init__(self, p):
        dev = types.SimpleNamespace(lib=p.lib, N=p.N, nn=p.nn, _h=p.h, rowptr=p.rowptr, colidx=p.col)
        self.th = types.SimpleNamespace(device=lambda: dev)


def test_resolvent_gains_match_the_dense_svd(prob):
    """7. resolvent_gains at w = 0.7 and 2.0 (sigma = i w), n = 3, ncv = 20 against the dense host computation: the singular values
    of L^T (M^-1)_vv L with E_vv = L L^T.  Bound: relative error of gamma <= 1e-8, the solver's own residual bound (kShiftedTol) --
    gamma^2 is an eigenvalue of an operator applied through solves of that accuracy.  Measured on the MI355X: at most 1.5e-15 at
    both frequencies (the printed lines; recorded in DESIGN §4.2).  With vectors: g^H E g = 1 and q^H E q = gamma^2 to 1e-8."""
    p = prob
    ww = np.array([0.7, 2.0])
    fs = _HostedOperator(p)
    gains, G, Q = linalg.resolvent_gains(p.A, p.E, ww, n=3, flowsolver=fs, ncv=20, vectors=True)
    assert gains.shape == (3, 2) and G.shape == (p.N, 3, 2) and Q.shape == (p.N, 3, 2)
    only = linalg.resolvent_gains(p.A, p.E, ww[:1], n=3, flowsolver=fs, ncv=20)
    assert only.shape == (3, 1) and np.allclose(only[:, 0], gains[:, 0], rtol=1e-12, atol=0.0)
    vel = np.arange(2 * p.nn)
    Ed = p.E.toarray()
    L = np.linalg.cholesky(Ed[np.ix_(vel, vel)])
    for i, w in enumerate(ww):
        Mi = np.linalg.inv((1j * w * p.E - p.A).toarray())
        ref = np.linalg.svd(L.T @ Mi[np.ix_(vel, vel)] @ L, compute_uv=False)[:3]
        err = np.abs(gains[:, i] - ref) / ref
        print("w =", w, "gains", gains[:, i], "dense", ref, "relative error", err)
        assert np.all(err <= 1e-8)
        for c in range(3):
            g, q = G[:, c, i], Q[:, c, i]
            gEg, qEq = np.vdot(g, Ed @ g), np.vdot(q, Ed @ q)
            assert abs(gEg - 1.0) <= 1e-8 and abs(qEq - gains[c, i] ** 2) <= 1e-8 * gains[c, i] ** 2
            assert np.linalg.norm(q - Mi @ (Ed @ g)) <= 1e-8 * np.linalg.norm(q)


_EIG_REF = 0.132643 + 0.770015j


def test_left_modes_of_the_cylinder(tmp_path, golden_dir):
    """8. get_mat_vp(left=True) on O1 (the set-up of test_linalg_gpu.py): the leading eigenvalue of the reference, host residuals of
    the LEFT pairs <= 1e-9, biorthonormality to 1e-8, and ONE numeric factorisation for both eigen solves."""
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.operatorgetter import OperatorGetter

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tmp_path)
    try:
        U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
        fs._assign_steady_state(U0, P0)
        A, E, _, _ = OperatorGetter(fs).get_all()
        A, E = A.tocsr(), E.tocsr()
        op = linalg.ShiftedOperator(fs, A, E)
        try:
            valp, vecp, vecl = linalg.get_mat_vp(A, E, n=2, target=0.1 + 0.8j, tol=1e-10, left=True, operator=op)
            info = op.krylov_info()
            ainfo = op.adjoint_info()
        finally:
            op.release()
        assert valp.shape == (2,) and vecp.shape == vecl.shape == (A.shape[0], 2)
        assert abs(valp[0] - _EIG_REF) <= 1e-6, valp
        AH, EH = A.T.conj().tocsr(), E.T.conj().tocsr()
        for i, lam in enumerate(valp):
            y = vecl[:, i]
            Ay, Ey = AH @ y, EH @ y
            res = np.linalg.norm(Ay - np.conj(lam) * Ey) / (abs(lam) * np.linalg.norm(Ey) + np.linalg.norm(Ay))
            print("left pair", i, "lambda", lam, "residual", res)
            assert res <= 1e-9
        G = vecl.conj().T @ (E @ vecp)
        print("biorthonormality: |Y^H E X - I|", np.abs(G - np.eye(2)).max(), "adjoint info", ainfo)
        assert np.all(np.abs(G - np.eye(2)) <= 1e-8)
        assert info["refactorisations"] == 1 and ainfo["exports"] == 1 and not ainfo["adjoint"]
        # the default return is unchanged
        out = linalg.get_mat_vp(A, E, n=1, target=0.1 + 0.8j, tol=1e-8, flowsolver=fs)
        assert len(out) == 2 and abs(out[0][0] - valp[0]) <= 1e-7
    finally:
        fs.th.release_device()
