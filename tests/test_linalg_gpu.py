"""flowcontrol_amd.linalg on the MI355X: frequency response, field response and shift-invert eigenvalues of the cylinder (O1 mesh,
golden base flow at Re = 100) against scipy on the same matrices and against the reference's own numbers; isolation of the handle's
time stepping from the shifted solver; the C ABI on its own; the refusals."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib, linalg
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.operatorgetter import OperatorGetter

pytestmark = pytest.mark.gpu

#: the reference's src/examples/operators/compute_eigenvalues.py: leading eigenvalue of the cylinder at Re = 100
_EIG_REF = 0.132643 + 0.770015j


def _cylinder(path, golden_dir, **kw):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=path, **kw)
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


@pytest.fixture(scope="module")
def cyl(tmp_path_factory, golden_dir):
    fs = _cylinder(tmp_path_factory.mktemp("linalg_cyl"), golden_dir)
    A, E, B, Cm = OperatorGetter(fs).get_all()
    lus = {}

    def lu(sigma):  # complex sparse LU of sigma E - A (the scipy reference), cached per sigma
        if sigma not in lus:
            lus[sigma] = spla.splu((sigma * E - A).astype(complex).tocsc())
        return lus[sigma]

    yield fs, A.tocsr(), E.tocsr(), B, Cm, lu
    fs.th.release_device()


def test_frequency_response_matches_scipy(cyl):
    fs, A, E, B, Cm, lu = cyl
    ww = np.array([0.01, 0.77, 3.0])
    H, ww_out = linalg.get_frequency_response_sequential(A, B, Cm, E, ww, verbose=False, flowsolver=fs)
    assert H.shape == (Cm.shape[0], B.shape[1], 3) and np.array_equal(ww_out, ww)
    for i, w in enumerate(ww):
        Href = Cm @ lu(1j * w).solve(B.astype(complex))
        assert np.max(np.abs(H[:, :, i] - Href)) <= 1e-9 * np.max(np.abs(Href)), f"w = {w}"
    # the reference's own formulation at w = 0.77: the real block system [[-A, -wE], [wE, -A]] [xr; xi] = [B; 0]
    w, n = 0.77, A.shape[0]
    Ablk = sp.bmat([[-A, -w * E], [w * E, -A]], format="csc")
    x = spla.splu(Ablk).solve(np.vstack([B, np.zeros_like(B)]))
    Hblk = Cm @ x[:n] + 1j * (Cm @ x[n:])
    assert np.max(np.abs(H[:, :, 1] - Hblk)) <= 1e-9 * np.max(np.abs(Hblk))
    # the parallel / mpi variants are the same computation
    Hp, _ = linalg.get_frequency_response_parallel(A, B, Cm, E, ww[1:2], verbose=False, n_jobs=4, flowsolver=fs)
    np.testing.assert_array_equal(Hp[:, :, 0], H[:, :, 1])


def test_field_response_matches_scipy(cyl):
    fs, A, E, B, Cm, lu = cyl
    X = linalg.get_field_response(A, B, E, 0.77, verbose=False, flowsolver=fs)
    assert X.shape == (A.shape[0], B.shape[1], 1)
    Xref = lu(0.77j).solve(B.astype(complex))
    for j in range(B.shape[1]):
        assert np.linalg.norm(X[:, j, 0] - Xref[:, j]) <= 1e-9 * np.linalg.norm(Xref[:, j])


def _check_pairs(A, E, valp, vecp, tol=1e-8):
    for i, lam in enumerate(valp):
        v = vecp[:, i]
        Av = A @ v
        assert np.linalg.norm(Av - lam * (E @ v)) <= tol * np.linalg.norm(Av), f"pair {i}: lambda = {lam}"


def test_eigenvalues_pinned_to_the_reference(cyl):
    fs, A, E, B, Cm, lu = cyl
    valp, vecp = linalg.get_mat_vp(A, E, n=2, target=0.1 + 0.8j, tol=1e-10, flowsolver=fs, eps_type="krylovschur", precond_type="lu")
    assert valp.shape == (2,) and vecp.shape == (A.shape[0], 2)
    assert abs(valp[0] - _EIG_REF) <= 1e-6, valp
    ref = spla.eigs(A.astype(complex), k=4, M=E.astype(complex), sigma=0.1 + 0.8j, return_eigenvectors=False, tol=1e-14)
    assert np.min(np.abs(ref - valp[0])) <= 1e-8
    _check_pairs(A, E, valp, vecp)
    assert linalg.get_mat_vp_slepc is linalg.get_mat_vp


def test_eigenvalues_near_zero(cyl):
    fs, A, E, B, Cm, lu = cyl
    valp, vecp = linalg.get_mat_vp(A, E, n=4, target=0.0, tol=1e-10, flowsolver=fs)
    ref = spla.eigs(A.astype(complex), k=8, M=E.astype(complex), sigma=0.0, return_eigenvectors=False, tol=1e-14)
    for lam in valp:
        assert np.min(np.abs(ref - lam)) <= 1e-8, (lam, ref)
    _check_pairs(A, E, valp, vecp)


def test_time_stepping_is_untouched_by_the_shifted_solver(cyl, tmp_path_factory, golden_dir):
    """10 steps with a frequency response and an eigen solve on the same handle between steps 5 and 6 == 10 steps of a fresh
    solver, bit for bit; after the release the shifted solver holds nothing, and a second setup gives the first H."""
    _, A, E, B, Cm, _ = cyl
    runs = []
    for host in (True, False):
        fs = _cylinder(tmp_path_factory.mktemp(f"iso{int(host)}"), golden_dir, num_steps=10)
        fs.initialize_time_stepping(ic=None)
        ys = []
        for k in range(10):
            if host and k == 5:
                H1, _ = linalg.get_frequency_response_sequential(A, B, Cm, E, [0.77], verbose=False, flowsolver=fs)
                linalg.get_mat_vp(A, E, n=2, target=0.1 + 0.8j, tol=1e-8, flowsolver=fs)
            ys.append(np.array(fs.step(u_ctrl=[0.05 * np.sin(0.7 * k), -0.02]), copy=True))
        dev = fs.th.device()
        state = [np.array(a, copy=True) for a in dev.get_state()]
        if host:
            iv, dv = np.zeros(4, dtype=np.int64), np.zeros(4)
            _lib.check(dev.lib.fc_shifted_info(dev._h, _lib.ptr(iv), _lib.ptr(dv), None))
            assert iv[0] == 0 and iv[1] == 0
            op = linalg.ShiftedOperator(fs, A, E)
            op.factor(0.3j)
            op.factor(0.77j)  # a second numeric phase at a new sigma on the same structure
            H2 = op.transfer(np.asarray(B, dtype=float), np.asarray(Cm, dtype=float))
            assert op.info()["device_bytes"] > 0
            op.release()
            np.testing.assert_allclose(H2, H1[:, :, 0], rtol=0, atol=1e-12 * np.max(np.abs(H1)))
        runs.append((ys, state))
        fs.th.release_device()
    (y1, s1), (y2, s2) = runs
    for a, b in zip(y1, y2):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(s1, s2):
        np.testing.assert_array_equal(a, b)


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


def test_shifted_solve_through_the_c_abi_only():
    """fc_setup_shifted -> fc_solve_shifted with ctypes and numpy alone (an Oseen-type operator on a 10 x 10 mesh, identity rows on
    the left / bottom velocity dofs), against scipy at sigma = 0.3 + 0.7i."""
    lib = _lib.load()
    coords, cells, cell_edges, edges = _square_mesh(10)
    nv, ne, nc = len(coords), len(edges), len(cells)
    h = C.c_void_p()

    def ok(rc):
        assert rc == 0, lib.fc_last_error().decode()

    ok(lib.fc_create(C.byref(h), 0, nv, ne, nc, np.ascontiguousarray(coords), cells, cell_edges))
    try:
        N, nnz, nn = C.c_int64(), C.c_int64(), C.c_int64()
        ok(lib.fc_get_sizes(h, C.byref(N), C.byref(nnz), C.byref(nn)))
        N, nnz, nn = N.value, nnz.value, nn.value
        rowptr, col = np.empty(N + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        ok(lib.fc_get_pattern(h, rowptr, col))
        node_xy = np.vstack([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])])
        adv = np.r_[1.0 + 0.2 * np.sin(3 * node_xy[:, 1]), 0.3 * np.cos(2 * node_xy[:, 0])]
        ok(lib.fc_assemble_matrix(h, _lib.SLOT_SCRATCH, 0.0, -0.02, adv.ctypes.data_as(C.c_void_p), -1.0, None, 1.0, 1.0, 1.0))
        ok(lib.fc_assemble_matrix(h, _lib.SLOT_MASS, 1.0, 0.0, None, 1.0, None, 1.0, 0.0, 0.0))
        a, e = np.empty(nnz), np.empty(nnz)
        ok(lib.fc_get_matrix_values(h, _lib.SLOT_SCRATCH, a))
        ok(lib.fc_get_matrix_values(h, _lib.SLOT_MASS, e))
        Araw = sp.csr_matrix((a, col, rowptr), shape=(N, N))
        wall = np.flatnonzero((node_xy[:, 0] < 1e-12) | (node_xy[:, 1] < 1e-12))
        keep = np.ones(N)
        keep[np.r_[wall, nn + wall]] = 0.0
        A = (sp.diags(keep) @ Araw + sp.diags(1.0 - keep)).tocsr()
        A_on = linalg.values_on_pattern(A, rowptr, col, "A")
        sigma = 0.3 + 0.7j
        ok(lib.fc_setup_shifted(h, A_on.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), sigma.real, sigma.imag, 2))
        rng = np.random.default_rng(5)
        b = rng.standard_normal((2, N)) + 1j * rng.standard_normal((2, N))
        bre, bim = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
        xre, xim, info = np.empty((2, N)), np.empty((2, N)), np.empty(2)
        ok(lib.fc_solve_shifted(h, 2, bre, bim.ctypes.data_as(C.c_void_p), xre.ctypes.data_as(C.c_void_p), xim.ctypes.data_as(C.c_void_p),
                                info.ctypes.data_as(C.c_void_p)))
        M = (sigma * sp.csr_matrix((e, col, rowptr), shape=(N, N)) - A).tocsc()
        lu = spla.splu(M)
        for c in range(2):
            xref = lu.solve(b[c])
            x = xre[c] + 1j * xim[c]
            assert np.linalg.norm(x - xref) <= 1e-10 * np.linalg.norm(xref)
            assert info[c] <= 1e-8
        iv, dv = np.zeros(4, dtype=np.int64), np.zeros(4)
        ok(lib.fc_shifted_info(h, iv.ctypes.data_as(C.c_void_p), dv.ctypes.data_as(C.c_void_p), None))
        assert iv[0] > 0 and iv[2] == 2 * N and iv[3] == 2 and dv[0] > 0.0 and dv[2] == sigma.real and dv[3] == sigma.imag
        ok(lib.fc_release_shifted(h))
        ok(lib.fc_shifted_info(h, iv.ctypes.data_as(C.c_void_p), dv.ctypes.data_as(C.c_void_p), None))
        assert iv[0] == 0 and iv[1] == 0
        assert lib.fc_solve_shifted(h, 1, bre, None, None, None, None) == _lib.FC_ERR_NOT_READY
    finally:
        lib.fc_destroy(h)


def test_refusals(cyl, tmp_path_factory):
    fs, A, E, B, Cm, _ = cyl
    dev = fs.th.device()
    # a matrix outside the handle's pattern
    bad = A.tolil()
    bad[0, A.shape[0] - 1] = 1.0
    with pytest.raises(ValueError, match="outside"):
        linalg.get_frequency_response_sequential(bad.tocsr(), B, Cm, E, [1.0], verbose=False, flowsolver=fs)
    with pytest.raises(ValueError, match="flowsolver"):
        linalg.get_mat_vp(A, E, n=2)
    # a partitioned handle (an exchange installed, as thread ranks do): FC_ERR_INVALID with a message
    from flowcontrol_amd.examples.lidcavity.lidcavityflowsolver import LidCavityFlowSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood
    from flowcontrol_amd.device import DeviceSolver

    part = DeviceSolver(TaylorHood(Mesh.unit_square(6, 6)), 0)
    try:
        cb = _lib.EXCHANGE_FN(lambda buf, n, user: None)
        _lib.check(part.lib.fc_set_host_exchange(part._h, 2, 0, cb, None))
        vals = np.zeros(part.nnz)
        rc = part.lib.fc_setup_shifted(part._h, vals.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), 0.0, 1.0, 2)
        assert rc == _lib.FC_ERR_INVALID and b"partitioned" in part.lib.fc_last_error()
    finally:
        part.close()
    # an enclosed flow (lid-driven cavity, pressure pin): ValueError from the package, FC_ERR_INVALID from the library
    lc = LidCavityFlowSolver.make_default(Re=100, path_out=tmp_path_factory.mktemp("linalg_lid"))
    try:
        Elc = OperatorGetter(lc).get_mass_matrix()
        with pytest.raises(ValueError, match="enclosed"):
            linalg.ShiftedOperator(lc, Elc, Elc)
        ldev = lc.th.device()
        ldev.set_pressure_pin(2 * ldev.nn)
        ev = linalg.values_on_pattern(Elc, ldev.rowptr, ldev.colidx)
        rc = ldev.lib.fc_setup_shifted(ldev._h, ev.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), 0.0, 1.0, 2)
        assert rc == _lib.FC_ERR_INVALID and b"pressure pin" in ldev.lib.fc_last_error()
    finally:
        lc.th.release_device()
    assert dev is fs.th.device()
