"""Snapshot sets of the shifted solver (``fc_shifted_snap_*``) and the balanced reduced models built on them (``flowcontrol_amd.rom``):
the Gram kernel on known data against a long-double product, pushes bit for bit, the combination, parity of ``balanced_rom`` with the
numpy / scipy model (tests/support/rom_model.py), the 2 * tail bound, the solver untouched by all of it, the refusals, and the
cylinder (O1) where many slices of N feed one Gram.  The 10 x 10 open-square problem of test_shifted_adjoint_gpu.py: N = 1003 is odd
and no multiple of a slice (4 slices of 256 rows, the last one 235)."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp

from flowcontrol_amd import _lib, linalg, rom
from tests.support import rom_model as M

pytestmark = pytest.mark.gpu

S0 = 0.3 + 0.7j
U = 2.0**-53


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
    """The open 10 x 10 problem, built exactly as ``_Open`` of test_shifted_adjoint_gpu.py builds it, with the inputs and outputs of
    the reduced-model fixture (tests/support/rom_model.py) and what ShiftedOperator needs of a flowsolver."""

    def __init__(self):
        self.lib = lib = _lib.load()
        coords, cells, cell_edges, edges = _square_mesh(10)
        self.h = h = C.c_void_p()
        self.ok(lib.fc_create(C.byref(h), 0, len(coords), len(edges), len(cells), np.ascontiguousarray(coords), cells, cell_edges))
        N, nnz, nn = C.c_int64(), C.c_int64(), C.c_int64()
        self.ok(lib.fc_get_sizes(h, C.byref(N), C.byref(nnz), C.byref(nn)))
        self.N, nnz, self.nn = N.value, nnz.value, nn.value
        self.rowptr, self.col = np.empty(self.N + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        self.ok(lib.fc_get_pattern(h, self.rowptr, self.col))
        node_xy = np.vstack([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])])
        adv = M.advection_field(node_xy)
        self.ok(lib.fc_assemble_matrix(h, _lib.SLOT_SCRATCH, 0.0, -0.02, _vp(adv), -1.0, None, 1.0, 1.0, 1.0))
        self.ok(lib.fc_assemble_matrix(h, _lib.SLOT_MASS, 1.0, 0.0, None, 1.0, None, 1.0, 0.0, 0.0))
        a, self.e = np.empty(nnz), np.empty(nnz)
        self.ok(lib.fc_get_matrix_values(h, _lib.SLOT_SCRATCH, a))
        self.ok(lib.fc_get_matrix_values(h, _lib.SLOT_MASS, self.e))
        self.A = M.with_wall_rows(sp.csr_matrix((a, self.col, self.rowptr), shape=(self.N, self.N)), node_xy, self.nn)
        self.E = sp.csr_matrix((self.e, self.col, self.rowptr), shape=(self.N, self.N))
        self.a_on = linalg.values_on_pattern(self.A, self.rowptr, self.col, "A")
        self.B, self.C = M.inputs_outputs(self.E, node_xy, self.nn)
        rng = np.random.default_rng(5)
        self.b = rng.standard_normal((2, self.N)) + 1j * rng.standard_normal((2, self.N))
        self.bre, self.bim = np.ascontiguousarray(self.b.real), np.ascontiguousarray(self.b.imag)
        dev = types.SimpleNamespace(lib=lib, N=self.N, nn=self.nn, _h=h, rowptr=self.rowptr, colidx=self.col)
        self.th = types.SimpleNamespace(device=lambda: dev)

    def ok(self, rc):
        assert rc == 0, self.lib.fc_last_error().decode()

    def setup(self, sigma=S0, refine=2):
        self.ok(self.lib.fc_setup_shifted(self.h, _vp(self.a_on), _vp(self.e), sigma.real, sigma.imag, refine))

    def solve(self):
        xre, xim, info = np.empty((2, self.N)), np.empty((2, self.N)), np.full(2, np.nan)
        self.ok(self.lib.fc_solve_shifted(self.h, 2, self.bre, _vp(self.bim), _vp(xre), _vp(xim), _vp(info)))
        return xre + 1j * xim

    def load(self, which, z, scale=1.0):
        re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        return self.lib.fc_shifted_snap_load(self.h, which, len(z), re, _vp(im), scale)

    def gram(self, left, right, kind):
        cnt = self.snap_info()
        out = np.full((2 * cnt[2 * left], 2 * cnt[2 * right]), np.nan)
        self.ok(self.lib.fc_shifted_snap_gram(self.h, left, right, kind, out))
        return out

    def snapshots(self, which, first, ncol):
        out = np.empty((ncol, self.N), dtype=complex)
        self.ok(self.lib.fc_debug_get_snapshots(self.h, which, first, ncol, out.view(np.float64)))
        return out

    def snap_info(self):
        iv = np.zeros(8, dtype=np.int64)
        self.ok(self.lib.fc_shifted_snap_info(self.h, iv))
        return iv

    def device_bytes(self):
        iv = np.zeros(4, dtype=np.int64)
        self.ok(self.lib.fc_shifted_info(self.h, _vp(iv), None, None))
        return int(iv[1])


@pytest.fixture()
def prob():
    p = _Open()
    yield p
    p.lib.fc_destroy(p.h)


_MODELS: dict = {}


def _model(p, nq):
    """The host model of the fixture for nq nodes, from the matrices the device holds (computed once, shared, never changed)."""
    if nq not in _MODELS:
        ww, weights = M.log_quadrature(*M.BAND, nq)
        _MODELS[nq] = M.Model(p.A, p.E, p.B, p.C, ww, weights)
    return _MODELS[nq]


def _parts(z):
    """complex columns [ncol, N] -> the real matrix [N, 2 ncol] of their parts (column 2 a + p), long double"""
    out = np.empty((z.shape[1], 2 * z.shape[0]), dtype=np.longdouble)
    out[:, 0::2], out[:, 1::2] = z.real.T, z.imag.T
    return out


def _csr_times(Mx, R):
    """Mx R for a CSR matrix and a long-double dense matrix, in long double (rows without entries give zeros)"""
    Mx = sp.csr_matrix(Mx)
    out = np.zeros((Mx.shape[0],) + R.shape[1:], dtype=np.longdouble)
    rows = np.flatnonzero(np.diff(Mx.indptr) > 0)
    prod = Mx.data.astype(np.longdouble).reshape((-1,) + (1,) * (R.ndim - 1)) * R[Mx.indices]
    out[rows] = np.add.reduceat(prod, Mx.indptr[rows], axis=0)
    return out


def _gram_ref(p, zl, zr, kind):
    """(G, bound): the long-double product and 2 (N + m) 2^-53 |L|^T |Op| |R|, m the longest pattern row: the dot-product rounding
    bound of the chain operator pass -> product, with a factor 2 for the two-stage sum (slices, then their partials)"""
    Op = (sp.identity(p.N, format="csr"), p.E, p.A)[kind]
    L, R = _parts(zl), _parts(zr)
    G = L.T @ _csr_times(Op, R)
    m = int(np.diff(p.rowptr).max())
    bound = 2.0 * (p.N + m) * U * (np.abs(L).T @ _csr_times(abs(Op), np.abs(R)))
    return G, bound


def _check_gram(p, got, zl, zr, kind, what):
    G, bound = _gram_ref(p, zl, zr, kind)
    err = np.abs(got.astype(np.longdouble) - G)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: {got.shape[0]} x {got.shape[1]}, max |G - G_ref| / bound = {ratio:.3e}")
    assert got.shape == G.shape and np.all(err <= bound)


def test_gram_kernel_on_known_data(prob):
    """1. 5 columns in set 1 (one 16-tile with bounds), 9 in set 0 (18 real columns: crosses a tile), 1 in set 2; Grams (1, 0, kind) for
    the three kinds and (1, 2, identity) against the long-double product, componentwise.  A zero column gives exact zeros, a set
    scaled by 2^40 the scaled result bit for bit, a repeated call the same bits; 17 against 33 columns runs the tile loops of both
    directions (33 columns: two operator chunks on the right, two 64-row tiles on the left)."""
    p = prob
    p.setup()
    rng = np.random.default_rng(11)
    z = {s: rng.standard_normal((k, p.N)) + 1j * rng.standard_normal((k, p.N)) for s, k in ((1, 5), (0, 9), (2, 1))}
    z[0][3] = 0.0
    z[1][2] = 0.0
    for s in (0, 1, 2):
        p.ok(p.lib.fc_shifted_snap_reserve(p.h, s, len(z[s])))
        p.ok(p.load(s, z[s]))
    assert list(p.snap_info()[:6]) == [9, 9, 5, 5, 1, 1]
    G = {}
    for kind in (0, 1, 2):
        G[kind] = p.gram(1, 0, kind)
        _check_gram(p, G[kind], z[1], z[0], kind, f"gram(1, 0, kind {kind})")
        assert not G[kind][4:6].any() and not G[kind][:, 6:8].any()  # (the zero columns: exact zeros)
        assert np.array_equal(p.gram(1, 0, kind), G[kind])  # (a repeated call: the same bits)
    _check_gram(p, p.gram(1, 2, 0), z[1], z[2], 0, "gram(1, 2, identity)")
    assert p.snap_info()[7] == 7
    p.ok(p.lib.fc_shifted_snap_clear(p.h, 0))
    p.ok(p.load(0, z[0], 2.0**40))
    for kind in (0, 1, 2):
        assert np.array_equal(p.gram(1, 0, kind), 2.0**40 * G[kind])
    big = {1: rng.standard_normal((17, p.N)) + 1j * rng.standard_normal((17, p.N)),
           0: rng.standard_normal((33, p.N)) + 1j * rng.standard_normal((33, p.N))}
    for s in (0, 1):
        p.ok(p.lib.fc_shifted_snap_reserve(p.h, s, len(big[s])))
        assert p.snap_info()[2 * s] == 0
        p.ok(p.load(s, big[s][:4]))
        p.ok(p.load(s, big[s][4:]))  # (appended)
        assert np.array_equal(p.snapshots(s, 0, len(big[s])), big[s])
    _check_gram(p, p.gram(1, 0, 1), big[1], big[0], 1, "gram(1, 0, E), 17 x 33 columns")
    _check_gram(p, p.gram(0, 1, 2), big[0], big[1], 2, "gram(0, 1, A), 33 x 17 columns")
    _check_gram(p, p.gram(0, 0, 0), big[0], big[0], 0, "gram(0, 0, identity), 33 x 33 columns")


def test_push_copies_the_solutions_bit_for_bit(prob):
    """2. After fc_solve_shifted, an adjoint solve and a block solve the pushed columns == scale * x bit for bit; a push past the
    capacity returns FC_ERR_INVALID and leaves the count unchanged."""
    p = prob
    p.setup()
    p.ok(p.lib.fc_shifted_snap_reserve(p.h, 0, 5))
    p.ok(p.lib.fc_shifted_snap_reserve(p.h, 1, 2))
    x = p.solve()
    p.ok(p.lib.fc_shifted_snap_push(p.h, 0, 2, 0.37))
    assert np.array_equal(p.snapshots(0, 0, 2), 0.37 * x.real + 1j * (0.37 * x.imag))
    p.ok(p.lib.fc_shifted_set_adjoint(p.h, 1))
    xa = p.solve()
    p.ok(p.lib.fc_shifted_snap_push(p.h, 1, 2, -1.5))
    p.ok(p.lib.fc_shifted_set_adjoint(p.h, 0))
    assert not np.array_equal(xa, x)
    assert np.array_equal(p.snapshots(1, 0, 2), -1.5 * xa.real + 1j * (-1.5 * xa.imag))
    p.ok(p.lib.fc_shifted_set_krylov(p.h, 200, 60, 1e-12))
    p.ok(p.lib.fc_shifted_set_block(p.h, 3))
    sig = np.array([0.3 + 0.7j, 0.3 + 0.75j, 0.28 + 0.7j])
    b3 = np.vstack([p.b, p.b[:1] * 1j])
    xre, xim, info = np.empty((3, p.N)), np.empty((3, p.N)), np.full(3, np.nan)
    p.ok(p.lib.fc_solve_shifted_block(p.h, 3, np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag), np.ascontiguousarray(b3.real),
                                      _vp(np.ascontiguousarray(b3.imag)), _vp(xre), _vp(xim), _vp(info)))
    p.ok(p.lib.fc_shifted_snap_push(p.h, 0, 3, 3.0))
    assert np.array_equal(p.snapshots(0, 2, 3), 3.0 * xre + 1j * (3.0 * xim))
    assert np.array_equal(p.snapshots(0, 0, 2), 0.37 * x.real + 1j * (0.37 * x.imag))  # (the earlier columns stay)
    before = p.snapshots(0, 0, 5)
    assert p.lib.fc_shifted_snap_push(p.h, 0, 1, 1.0) == _lib.FC_ERR_INVALID
    assert list(p.snap_info()[:4]) == [5, 5, 2, 2] and np.array_equal(p.snapshots(0, 0, 5), before)
    assert p.lib.fc_shifted_snap_push(p.h, 1, 1, 1.0) == _lib.FC_ERR_INVALID


def test_combine_against_numpy(prob):
    """3. out[c] = sum_J Q[J][c] part_J against the long-double product: |out - ref| <= 2 ncol 2^-53 |parts| |Q|, the dot-product
    bound for a sum of 2 ncol terms in one stage."""
    p = prob
    p.setup()
    rng = np.random.default_rng(3)
    for ncol, k in ((9, 4), (1, 1), (33, 7)):
        z = rng.standard_normal((ncol, p.N)) + 1j * rng.standard_normal((ncol, p.N))
        p.ok(p.lib.fc_shifted_snap_reserve(p.h, 1, ncol))
        p.ok(p.lib.fc_shifted_snap_clear(p.h, 1))
        p.ok(p.load(1, z))
        Q = np.ascontiguousarray(rng.standard_normal((2 * ncol, k)))
        out = np.full((k, p.N), np.nan)
        p.ok(p.lib.fc_shifted_snap_combine(p.h, 1, k, Q, out))
        S = _parts(z)
        ref = (S @ Q.astype(np.longdouble)).T
        bound = 2 * ncol * U * (np.abs(S) @ np.abs(Q).astype(np.longdouble)).T
        err = np.abs(out.astype(np.longdouble) - ref)
        print(f"combine {ncol} columns -> {k}: max err / bound = {float(np.max(err / bound)):.3e}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("nq", [6, 12])
def test_parity_with_the_model(prob, nq):
    """4. balanced_rom on the fixture (nq = 6: 24 and 36 real columns, partial tiles; nq = 12: 48 and 72): the first 12 Hankel singular
    values within 1e-10 relative of the model's, H_r for r = 4, 8, 12 within 1e-10 of the model's H_r relative to max |H_r|_2 (1e-10:
    the project's bound for device solves; the host model recomputed with another LU ordering moves by 6e-15 / 2e-14), and
    ReducedModel.H == linalg.frequency_response at the nodes, bit for bit."""
    p = prob
    m = _model(p, nq)
    reds = {r: rom.balanced_rom(p.A, p.B, p.C, p.E, band=M.BAND, nq=nq, r=r, flowsolver=p, modes=(r == 8), verbose=False) for r in (4, 8, 12)}
    red = reds[12]
    assert red.hsv.size == min(2 * nq * 2, 2 * nq * 3) and red.H.shape == (nq, 3, 2)
    np.testing.assert_allclose(red.ww, m.ww, rtol=1e-14)
    dh = np.max(np.abs(red.hsv[:12] - m.hsv[:12]) / m.hsv[:12])
    print(f"nq = {nq}: Hankel singular values, largest relative difference of the first 12: {dh:.3e}")
    assert dh <= 1e-10
    for r, rd in reds.items():
        Hm = M.response(*m.from_grams(r), M.CHECK_WW)
        scale = max(np.linalg.norm(h, 2) for h in Hm)
        d = M.worst_error(Hm, rd.frequency_response(M.CHECK_WW)) / scale
        print(f"nq = {nq}, r = {r}: max |H_r - H_r(model)|_2 / max |H_r|_2 = {d:.3e}")
        assert d <= 1e-10
        assert np.array_equal(rd.hsv, red.hsv) and np.array_equal(rd.H, red.H)  # (the sweep repeats bit for bit)
    Phi, Psi = reds[8].Phi, reds[8].Psi
    assert Phi.shape == Psi.shape == (p.N, 8) and reds[4].Phi is None
    assert np.max(np.abs(Psi.T @ (p.E @ Phi) - np.eye(8))) <= 1e-10
    op = linalg.ShiftedOperator(p, p.A, p.E)
    try:
        H, _ = linalg.frequency_response(op, p.B, p.C, red.ww, verbose=False)
    finally:
        op.release()
    assert np.array_equal(red.H, np.moveaxis(H, 2, 0))


def test_device_model_meets_the_truncation_bound(prob):
    """5. nq = 24, r = 4, 8, 12: max_w |H - H_r|_2 <= 2 * tail on 40 log-spaced frequencies in [0.1, 100], the full-order response from
    the device (the host reference stays at 0.29 / 0.39 / 0.52 of the bound)."""
    p = prob
    op = linalg.ShiftedOperator(p, p.A, p.E)
    try:
        H, _ = linalg.frequency_response(op, p.B, p.C, M.CHECK_WW, verbose=False)
        H = np.moveaxis(H, 2, 0)
        for r in (4, 8, 12):
            red = rom.balanced_rom(p.A, p.B, p.C, p.E, band=M.BAND, nq=24, r=r, operator=op, verbose=False)
            err = M.worst_error(H, red.frequency_response(M.CHECK_WW))
            print(f"r = {r}: max |H - H_r|_2 = {err:.4e} = {err / red.error_bound:.3f} x the bound {red.error_bound:.4e}")
            assert err <= red.error_bound and np.all(red.eigenvalues().real < 0)
    finally:
        op.release()


def test_solver_is_untouched(prob):
    """6. A direct solve before any snap_* call == the same solve in three later states, bit for bit: (a) after a full balanced_rom, which
    releases the shifted solver at its end, so this state is "released and set up again"; (b) on the live structure after sets were
    reserved, loaded, multiplied and freed again -- the handle that held snapshots; (c) on a fresh handle.  The device bytes of
    fc_shifted_info grow by exactly what fc_shifted_snap_info reports and return to their starting value once the sets are freed."""
    p = prob
    p.setup()
    x0 = p.solve()
    b0 = p.device_bytes()
    assert not p.snap_info().any()
    rom.balanced_rom(p.A, p.B, p.C, p.E, band=M.BAND, nq=6, r=4, flowsolver=p, verbose=False)
    p.setup()
    assert np.array_equal(p.solve(), x0) and p.device_bytes() == b0
    rng = np.random.default_rng(2)
    for s, k in ((0, 4), (1, 3), (2, 1)):
        p.ok(p.lib.fc_shifted_snap_reserve(p.h, s, k))
        p.ok(p.load(s, rng.standard_normal((k, p.N)) + 0j))
    p.gram(1, 0, 2)
    info = p.snap_info()
    assert info[6] > 16 * p.N * 8 and p.device_bytes() == b0 + info[6]
    for s in (0, 1, 2):
        p.ok(p.lib.fc_shifted_snap_reserve(p.h, s, 0))
    assert p.device_bytes() == b0 and not p.snap_info()[:7].any()
    assert np.array_equal(p.solve(), x0)
    q = _Open()
    try:
        q.setup()
        assert np.array_equal(q.solve(), x0)
    finally:
        q.lib.fc_destroy(q.h)


def test_refusals(prob):
    """7. reserve before fc_setup_shifted: FC_ERR_NOT_READY; a Gram with an empty set, an unknown kind or set, a push of more columns
    than the last solve had: FC_ERR_INVALID."""
    p = prob
    lib, h = p.lib, p.h
    INV, NR = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY
    out = np.zeros((64, 64))
    assert lib.fc_shifted_snap_reserve(h, 0, 4) == NR
    p.setup()
    assert lib.fc_shifted_snap_reserve(h, 3, 4) == INV and lib.fc_shifted_snap_reserve(h, -1, 4) == INV
    assert lib.fc_shifted_snap_reserve(h, 0, -1) == INV
    p.ok(lib.fc_shifted_snap_reserve(h, 0, 4))
    p.ok(lib.fc_shifted_snap_reserve(h, 1, 4))
    assert lib.fc_shifted_snap_gram(h, 1, 0, 1, out) == INV  # (both empty)
    assert lib.fc_shifted_snap_push(h, 0, 1, 1.0) == INV  # (no solve yet)
    p.solve()
    assert lib.fc_shifted_snap_push(h, 0, 3, 1.0) == INV  # (the solve had 2 columns)
    p.ok(lib.fc_shifted_snap_push(h, 0, 2, 1.0))
    assert lib.fc_shifted_snap_gram(h, 1, 0, 1, out) == INV  # (the left set is empty)
    assert lib.fc_shifted_snap_gram(h, 0, 2, 0, out) == INV  # (set 2 was never reserved)
    p.ok(lib.fc_shifted_snap_push(h, 1, 2, 1.0))
    for left, right, kind in ((1, 0, 3), (1, 0, -1), (3, 0, 1), (1, -1, 1)):
        assert lib.fc_shifted_snap_gram(h, left, right, kind, out) == INV
    assert lib.fc_shifted_snap_combine(h, 2, 1, out, out) == INV and lib.fc_shifted_snap_combine(h, 0, 0, out, out) == INV
    assert lib.fc_debug_get_snapshots(h, 0, 1, 2, out) == INV and lib.fc_shifted_snap_clear(h, 5) == INV
    assert list(p.snap_info()[:6]) == [2, 4, 2, 4, 0, 0]
    p.ok(lib.fc_shifted_snap_gram(h, 1, 0, 1, out))
    p.ok(lib.fc_release_shifted(h))
    assert not p.snap_info().any() and lib.fc_shifted_snap_push(h, 0, 1, 1.0) == NR


def test_cylinder_snapshots_and_modes(tmp_path, golden_dir):
    """8. O1 (the set-up of test_linalg_gpu.py), nq = 8 on [0.4, 1.5]: many slices of N feed one Gram.  The device Hankel singular values
    == the numpy SVD of the Gram formed on the host from the downloaded snapshots, within 1e-10 relative for those above 1e-8 hsv_0,
    and |Psi^T E Phi - I| <= 1e-10 with modes=True.  The quality of the reduced model is not asserted here (DESIGN §4.2 records it)."""
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.operatorgetter import OperatorGetter

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tmp_path)
    try:
        U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
        fs._assign_steady_state(U0, P0)
        A, E, B, Cm = OperatorGetter(fs).get_all()
        A, E = A.tocsr(), E.tocsr()
        B = np.asarray(B, dtype=float).reshape(A.shape[0], -1)
        nu, ny, nq, N = B.shape[1], Cm.shape[0], 8, A.shape[0]
        op = linalg.ShiftedOperator(fs, A, E)
        try:
            red = rom.balanced_rom(A, B, Cm, E, band=(0.4, 1.5), nq=nq, tol=1e-3, modes=True, operator=op, verbose=False)
            info = op.snap_info()
            assert info["columns"] == [nq * nu, nq * ny, nu]
            X = np.empty((nq * nu, N), dtype=complex)
            Z = np.empty((nq * ny, N), dtype=complex)
            check = _lib.check
            check(op.lib.fc_debug_get_snapshots(op._h, 0, 0, nq * nu, X.view(np.float64)))
            check(op.lib.fc_debug_get_snapshots(op._h, 1, 0, nq * ny, Z.view(np.float64)))
            timing = op.snap_gram_timing()
        finally:
            op.release()
        # the host Gram in long double, column by column, rounded once: the reference carries no summation error of its own (formed in
        # double by BLAS it differs from this one by as much as the device's does)
        Xs, Zs = _parts(X), _parts(Z)
        G = np.stack([Zs.T @ _csr_times(E, Xs[:, j]) for j in range(Xs.shape[1])], axis=1)
        hsv = np.linalg.svd(np.asarray(G, dtype=float), compute_uv=False)
        hsv_d = np.linalg.svd(np.asarray(Zs, dtype=float).T @ (E @ np.asarray(Xs, dtype=float)), compute_uv=False)
        big = hsv > 1e-8 * hsv[0]
        d = np.max(np.abs(red.hsv[big] - hsv[big]) / hsv[big])
        print(f"O1: host Gram in double against the long-double one: {np.max(np.abs(hsv_d[big] - hsv[big]) / hsv[big]):.3e}; device against "
              f"the double one: {np.max(np.abs(red.hsv[big] - hsv_d[big]) / hsv_d[big]):.3e}; per value {np.abs(red.hsv[big] - hsv[big]) / hsv[big]}")
        bi = np.max(np.abs(red.Psi.T @ (E @ red.Phi) - np.eye(red.r)))
        print(f"O1: hsv {red.hsv}, r = {red.r}, largest relative difference to the host Gram's {d:.3e}, |Psi^T E Phi - I| = {bi:.3e}, "
              f"last Gram {timing}")
        assert red.hsv.shape == hsv.shape and d <= 1e-10
        assert red.Phi.shape == red.Psi.shape == (N, red.r) and bi <= 1e-10
    finally:
        fs.th.release_device()


def test_three_grams_cost_less_than_one_factorisation(tmp_path, golden_dir):
    """9. The sizes of the 64-frequency model of O1 (128 direct and 192 adjoint columns, nu = 2: the Grams are 384 x 256, 384 x 256 and
    384 x 4) on loaded data: the three Gram calls of balanced_rom together take less device time (HIP events) than one numeric
    factorisation of the same operator (the time of a Gram does not depend on the values)."""
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.operatorgetter import OperatorGetter

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tmp_path)
    try:
        U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
        fs._assign_steady_state(U0, P0)
        og = OperatorGetter(fs)
        A, E = og.get_A().tocsr(), og.get_mass_matrix().tocsr()
        op = linalg.ShiftedOperator(fs, A, E)
        try:
            op.factor(0.77j)
            refactor_ms = op.info()["refactor_ms"]
            rng = np.random.default_rng(0)
            for which, ncol in ((0, 128), (1, 192), (2, 2)):
                op.snap_reserve(which, ncol)
                op.snap_load(which, rng.standard_normal((op.n, ncol)) + 1j * rng.standard_normal((op.n, ncol)))
            ms = {}
            for left, right, kind in ((1, 0, 1), (1, 0, 2), (1, 2, 0)):
                op.snap_gram(left, right, kind)  # (the work buffers are sized by the first call)
                G = op.snap_gram(left, right, kind)
                assert G.shape == (384, 2 * op.snap_info()["columns"][right]) and np.all(np.isfinite(G))
                ms[(left, right, kind)] = op.snap_gram_timing()["ms"]
            total = sum(ms.values())
            print(f"O1: three Grams {total:.3f} ms {ms} against one factorisation {refactor_ms:.3f} ms; sets hold {op.snap_info()['bytes']} bytes")
            assert total < refactor_ms
        finally:
            op.release()
    finally:
        fs.th.release_device()
