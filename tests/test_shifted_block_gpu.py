"""Block solves of the shifted solver (``fc_shifted_set_block`` / ``fc_solve_shifted_block``): k columns, each at a shift of its own,
on ONE set of factors, the factors read once per GMRES iteration for all of them.  The 10 x 10 open square problem of
test_shifted_krylov_gpu.py with scipy's LU per shift as the reference; factors at sigma_0 = 0.3 + 0.7i, columns over 0.3 + [0.6, 0.8]i."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib, linalg

pytestmark = pytest.mark.gpu

S0 = 0.3 + 0.7j
MAX_ITER, RESTART, RTOL = 200, 60, 1e-12
#: the lock-step loop reads the columns' records every CHECK iterations (kShiftedKrylovCheck): it may run CHECK - 1 iterations past
#: the one at which the last column stopped
CHECK = 4


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
    """The open 10 x 10 problem of test_shifted_krylov_gpu.py on a handle of its own: an Oseen-type operator with identity rows on the
    left / bottom velocity dofs, scipy's LU per shift (shared by all instances: the matrices are the same)."""

    _LU: dict = {}

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

    def set_block(self, k):
        return self.lib.fc_shifted_set_block(self.h, k)

    def solve(self):
        """fc_solve_shifted of the two stock right-hand sides: (rc, x [2, N], info [2])"""
        xre, xim, info = np.empty((2, self.N)), np.empty((2, self.N)), np.full(2, np.nan)
        rc = self.lib.fc_solve_shifted(self.h, 2, self.bre, _vp(self.bim), _vp(xre), _vp(xim), _vp(info))
        return rc, xre + 1j * xim, info

    def solve_block(self, sig, b, k=None):
        """(rc, x [k, N], info [k]) of fc_solve_shifted_block for the shifts sig [k] and right-hand sides b [k, N] complex"""
        sig = np.asarray(sig, dtype=complex)
        k = sig.size if k is None else k
        sre, sim = np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag)
        bre, bim = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
        xre, xim, info = np.empty((sig.size, self.N)), np.empty((sig.size, self.N)), np.full(sig.size, np.nan)
        rc = self.lib.fc_solve_shifted_block(self.h, k, sre, sim, bre, _vp(bim), _vp(xre), _vp(xim), _vp(info))
        return rc, xre + 1j * xim, info

    def krylov_info(self, k):
        it, cnt = np.zeros(k, dtype=np.int32), np.zeros(5, dtype=np.int64)
        self.ok(self.lib.fc_shifted_krylov_info(self.h, _vp(it), _vp(cnt)))
        return it, cnt

    def device_bytes(self):
        iv = np.zeros(4, dtype=np.int64)
        self.ok(self.lib.fc_shifted_info(self.h, _vp(iv), None, None))
        return int(iv[0]), int(iv[1])

    def rel_err(self, x, sig, b):
        ref = [self.lu(s).solve(bc) for s, bc in zip(sig, b)]
        return np.array([np.linalg.norm(xc - r) / np.linalg.norm(r) for xc, r in zip(x, ref)])


@pytest.fixture()
def prob():
    p = _Open()
    yield p
    p.lib.fc_destroy(p.h)


def _spread(k):
    """k shifts over 0.3 + [0.6, 0.8]i, the middle one exactly sigma_0"""
    sig = 0.3 + 1j * np.linspace(0.6, 0.8, k)
    sig[k // 2] = S0
    return sig


def _rhs(p, k, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((k, p.N)) + 1j * rng.standard_normal((k, p.N))


def _scipy_far_from_the_cap(p, sig, b, restart=RESTART, cycles=4):
    """scipy's gmres with the splu(sigma_0) preconditioner on the same shifts and right-hand sides: it must stay below a quarter of
    the device's cap of 200 iterations."""
    P = spla.LinearOperator((p.N, p.N), matvec=p.lu(S0).solve, dtype=complex)
    worst = 0
    for s, bc in zip(sig, b):
        if not np.any(bc):
            continue
        count = [0]
        M = (s * p.E - p.A).astype(complex).tocsc()
        _, flag = spla.gmres(M, bc, M=P, rtol=RTOL, restart=restart, maxiter=cycles, callback=lambda r: count.__setitem__(0, count[0] + 1),
                             callback_type="pr_norm")
        assert flag == 0 and count[0] <= MAX_ITER // 4, (s, count[0], flag)
        worst = max(worst, count[0])
    print("scipy gmres, splu(sigma_0) preconditioner: most iterations of a column", worst)
    return worst


@pytest.mark.parametrize("k", [3, 5, 32])
def test_parity_with_scipy_lu_per_shift(prob, k):
    """k = 3 (KB 4), 5 (KB 8), 32: distinct shifts, distinct complex right-hand sides; every column within 1e-9 of scipy's LU at ITS
    shift, true residual <= rtol, the column at sigma_0 done in at most 2 iterations, one numeric factorisation in all."""
    p = prob
    sig, b = _spread(k), _rhs(p, k)
    _scipy_far_from_the_cap(p, sig, b)
    p.setup(S0)
    p.krylov()
    p.ok(p.set_block(k))
    rc, x, info = p.solve_block(sig, b)
    p.ok(rc)
    it, cnt = p.krylov_info(k)
    err = p.rel_err(x, sig, b)
    print("block of", k, ": worst error", err.max(), "worst residual", info.max(), "iterations", list(it), "counters", list(cnt))
    assert np.all(err <= 1e-9)
    assert np.all(info <= RTOL)
    assert 1 <= it[k // 2] <= 2
    assert np.all((1 <= it) & (it <= MAX_ITER))
    assert cnt[0] == 1


def test_factors_are_read_once_per_iteration(prob):
    """32 columns: the `applies` counter grows by the LOCK-STEP iterations plus one update per cycle, not by the sum over the columns.
    The driver reports both (fc_shifted_block_info), so the count is exact: applies == lock-step iterations + cycles.  Its
    structure bounds the lock-step iterations: a cycle runs until its slowest column stopped and learns that at most CHECK - 1
    iterations late; the slowest column of the LAST cycle a column takes part in counts towards that column's own total, every
    earlier cycle is at most `restart` long.  Hence applies <= max_c(iterations_c) + (cycles - 1) restart + 2 cycles + the slack
    (CHECK - 1) cycles; with restart = 60 above every column's count (scipy: <= 50) one cycle is expected."""
    p = prob
    k = 32
    sig, b = _spread(k), _rhs(p, k)
    _scipy_far_from_the_cap(p, sig, b)
    p.setup(S0)
    p.krylov()
    p.ok(p.set_block(k))
    _, cnt0 = p.krylov_info(k)
    rc, _, _ = p.solve_block(sig, b)
    p.ok(rc)
    it, cnt1 = p.krylov_info(k)
    applies, matvecs = int(cnt1[1] - cnt0[1]), int(cnt1[2] - cnt0[2])
    bi = np.zeros(4, dtype=np.int64)
    p.ok(p.lib.fc_shifted_block_info(p.h, _vp(bi)))
    launched, cycles = int(bi[2]), int(bi[3])
    bound = int(it.max()) + (cycles - 1) * RESTART + 2 * cycles + (CHECK - 1) * cycles
    print("applies", applies, "matvecs", matvecs, "lock-step iterations", launched, "cycles", cycles, "iterations max", it.max(), "sum",
          it.sum(), "bound", bound)
    assert bi[0] == k and bi[1] == 32
    assert applies == launched + cycles and matvecs == launched + cycles + 1  # (+ the first true residual)
    assert 1 <= cycles <= 2 and it.max() + 1 <= applies <= bound
    assert bound < it.sum()  # (the check means something: a loop over the columns would need their sum)


def test_columns_are_independent_and_repeatable(prob):
    """The same (sigma, b) as column 0 of one block of 8 and as column 5 of another with other neighbours -- a zero right-hand side and
    a shift that needs more iterations among them: the same bits; a repeated call: the same bits."""
    p = prob
    k = 8
    sx, bx = 0.3 + 0.66j, _rhs(p, 1, seed=3)[0]
    sig1, b1 = _spread(k), _rhs(p, k, seed=21)
    sig1[0], b1[0] = sx, bx
    sig2, b2 = 0.3 + 1j * np.linspace(0.8, 0.6, k), _rhs(p, k, seed=22)
    sig2[5], b2[5] = sx, bx
    b2[2] = 0.0
    sig2[6] = 0.3 + 0.95j  # (further from sigma_0 than any other column)
    _scipy_far_from_the_cap(p, np.r_[sig1, sig2], np.vstack([b1, b2]))
    p.setup(S0)
    p.krylov()
    p.ok(p.set_block(k))
    rc, x1, _ = p.solve_block(sig1, b1)
    p.ok(rc)
    it1, _ = p.krylov_info(k)
    rc, x2, info2 = p.solve_block(sig2, b2)
    p.ok(rc)
    it2, _ = p.krylov_info(k)
    print("iterations", list(it1), list(it2))
    assert np.array_equal(x1[0], x2[5]) and it1[0] == it2[5]
    assert it2[6] > it2[5] and it2[2] == 0 and not np.any(x2[2]) and info2[2] == 0.0
    assert np.all(p.rel_err(np.delete(x2, 2, 0), np.delete(sig2, 2), np.delete(b2, 2, 0)) <= 1e-9)
    rc, x3, _ = p.solve_block(sig2, b2)
    p.ok(rc)
    assert np.array_equal(x3, x2)
    rc, x4, _ = p.solve_block(sig1, b1)
    p.ok(rc)
    assert np.array_equal(x4, x1)


def test_restart_crossing(prob):
    """restart = 5: the outer columns need several cycles, the one at sigma_0 a single iteration; all meet 1e-9."""
    p = prob
    k = 5
    sig, b = _spread(k), _rhs(p, k, seed=31)
    _scipy_far_from_the_cap(p, sig, b, restart=5, cycles=10)
    p.setup(S0)
    p.krylov(restart=5)
    p.ok(p.set_block(k))
    rc, x, info = p.solve_block(sig, b)
    p.ok(rc)
    it, _ = p.krylov_info(k)
    err = p.rel_err(x, sig, b)
    print("restart 5: iterations", list(it), "errors", err, "residuals", info)
    assert np.all(err <= 1e-9) and np.all(info <= RTOL)
    assert it.max() > 5 and len(set(it.tolist())) > 1


def test_a_failing_column_is_named(prob):
    """max_iter = 3 and one far-away shift among k = 4: FC_ERR_NOT_CONVERGED, that column's info above rtol, the others' at most rtol
    and their x the bits of a run in which every column converges.  (The near columns sit 1e-7 from sigma_0: the preconditioned
    operator is I + O(1e-7 |E M^-1|), three iterations reach 1e-10 with room.)"""
    p = prob
    k, rtol = 4, 1e-10
    b = _rhs(p, k, seed=41)
    near = np.array([S0, S0 + 1e-7j, S0 - 1e-7j, S0 + 1e-7])
    bad = near.copy()
    bad[2] = 0.3 + 3.0j
    p.setup(S0)
    p.krylov(max_iter=3, restart=3, rtol=rtol)
    p.ok(p.set_block(k))
    rc, xg, infog = p.solve_block(near, b)
    p.ok(rc)
    assert np.all(infog <= rtol)
    rc, xb, infob = p.solve_block(bad, b)
    print("failing column: rc", rc, "info", infob, p.lib.fc_last_error().decode())
    assert rc == _lib.FC_ERR_NOT_CONVERGED
    assert b"column 2" in p.lib.fc_last_error()
    assert infob[2] > rtol and np.all(np.delete(infob, 2) <= rtol)
    for c in (0, 1, 3):
        assert np.array_equal(xb[c], xg[c])
    it, _ = p.krylov_info(k)
    assert it[2] == 3
    # the handle goes on
    rc, x2, _ = p.solve_block(near, b)
    p.ok(rc)
    assert np.array_equal(x2, xg)


def test_refusals(prob):
    p = prob
    k = 4
    sig, b = _spread(k), _rhs(p, k)
    assert p.set_block(k) == _lib.FC_ERR_NOT_READY  # no structure yet
    assert p.set_block(33) == _lib.FC_ERR_INVALID
    p.setup(S0)
    p.ok(p.set_block(k))
    rc, _, _ = p.solve_block(sig, b)  # no fc_shifted_set_krylov
    assert rc == _lib.FC_ERR_INVALID and b"fc_shifted_set_krylov" in p.lib.fc_last_error()
    p.krylov()
    p.ok(p.set_block(0))
    rc, _, _ = p.solve_block(sig, b)  # no fc_shifted_set_block
    assert rc == _lib.FC_ERR_NOT_READY
    p.ok(p.set_block(k))
    rc, _, _ = p.solve_block(sig[:3], b[:3])  # k mismatch
    assert rc == _lib.FC_ERR_INVALID
    nan = sig.copy()
    nan[1] = complex(np.nan, 0.7)
    rc, _, _ = p.solve_block(nan, b)
    assert rc == _lib.FC_ERR_INVALID
    p.ok(p.set_block(0))
    rc, _, _ = p.solve_block(sig, b)  # after the release of the block
    assert rc == _lib.FC_ERR_NOT_READY
    # ... and the handle is as usable as ever
    p.ok(p.set_block(k))
    rc, x, _ = p.solve_block(sig, b)
    p.ok(rc)
    assert np.all(p.rel_err(x, sig, b) <= 1e-9)


def test_single_column_solves_are_untouched(prob):
    """fc_solve_shifted at the factored shift and on lagged factors (fc_shifted_set_shift), before and after a block solve and after
    a refactorisation with the block set: the bits of a handle that never had a block.  The block's memory -- at least the factor
    size more -- shows in fc_shifted_info and is gone after fc_shifted_set_block(0)."""
    p = prob
    S2 = 0.3 + 0.75j
    k = 4
    sig, b = _spread(k), _rhs(p, k)

    def run(q, block):
        out = []
        q.setup(S0)
        q.krylov()
        out.append(q.solve()[1])
        q.ok(q.lib.fc_shifted_set_shift(q.h, S2.real, S2.imag))
        out.append(q.solve()[1])
        if block:
            fb, before = q.device_bytes()
            q.ok(q.set_block(k))
            assert q.device_bytes()[1] >= before + fb
            rc, x, _ = q.solve_block(sig, b)
            q.ok(rc)
            assert np.all(q.rel_err(x, sig, b) <= 1e-9)
        out.append(q.solve()[1])  # (the operator's shift is still S2)
        q.setup(S0)  # (with a block set: the tiled copy is redone)
        out.append(q.solve()[1])
        if block:
            rc, x, _ = q.solve_block(sig, b)
            q.ok(rc)
            assert np.all(q.rel_err(x, sig, b) <= 1e-9)
            q.ok(q.set_block(0))
            assert q.device_bytes()[1] <= before + 8 * 2 * q.N * k  # (xz grew to the block's k columns; nothing else stays)
        out.append(q.solve()[1])
        return out

    with_block = run(p, True)
    q = _Open()
    try:
        without = run(q, False)
    finally:
        q.lib.fc_destroy(q.h)
    for a, c in zip(with_block, without):
        assert np.array_equal(a, c)
    assert np.array_equal(with_block[1], with_block[2])


def test_time_stepping_is_untouched_by_a_block_solve():
    """10 BDF2 steps on an 8 x 8 square with a shifted factorisation and a block solve on the same handle between steps 5 and 6 (the
    block stays set for the rest) == 10 plain steps, bit for bit."""
    from flowcontrol_amd._lib import SLOT_BDF2, SLOT_MASS
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    runs = []
    for with_block in (True, False):
        th = TaylorHood(Mesh.unit_square(8, 8))
        dev = DeviceSolver(th, 0)
        try:
            x = th.node_coords
            U0 = np.r_[1.0 + 0.3 * np.sin(x[:, 0]) * np.cos(0.7 * x[:, 1]), 0.2 * np.cos(0.5 * x[:, 0]) * np.sin(x[:, 1])]
            m = th.mesh
            be = m.boundary_edges()
            be = be[m.edge_midpoints()[be, 0] < 1.0 - 1e-9]
            nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
            dofs = np.sort(np.r_[nodes, nodes + th.nn])
            dev.set_bc(dofs, np.sin(3.0 * np.arange(dofs.size))[:, None])
            dev.set_time_scheme(0.005, True)
            dev.assemble_matrix(SLOT_BDF2, mass=1.5 / 0.005, nu=0.01, adv=U0, lin=U0)
            dev.apply_bc(SLOT_BDF2)
            dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
            dev.setup_solver(SLOT_BDF2, refine=1)
            dev.set_sensors([th.point_eval_row((0.31, 0.42), 1)])
            rng = np.random.default_rng(0)
            dev.set_state(0.1 * rng.standard_normal(2 * th.nn), 0.1 * rng.standard_normal(2 * th.nn), np.zeros(th.nv))
            ys = []
            for s in range(10):
                if with_block and s == 5:
                    lib, h = dev.lib, dev._h
                    nnz = dev.colidx.size
                    a, e = np.empty(nnz), np.empty(nnz)
                    _lib.check(lib.fc_get_matrix_values(h, SLOT_BDF2, a))
                    _lib.check(lib.fc_get_matrix_values(h, SLOT_MASS, e))
                    a = -a  # sigma E - A = sigma E + K with the (nonsingular) step operator K
                    _lib.check(lib.fc_setup_shifted(h, _vp(a), _vp(e), S0.real, S0.imag, 2))
                    _lib.check(lib.fc_shifted_set_krylov(h, MAX_ITER, RESTART, 1e-10))
                    _lib.check(lib.fc_shifted_set_block(h, 3))
                    sig = np.array([S0, S0 + 0.05j, S0 - 0.05j])
                    bb = rng.standard_normal((3, dev.N))
                    xre, xim, info = np.empty((3, dev.N)), np.empty((3, dev.N)), np.zeros(3)
                    _lib.check(lib.fc_solve_shifted_block(h, 3, np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag), bb, None,
                                                          _vp(xre), _vp(xim), _vp(info)))
                    assert np.all(info <= 1e-10)
                ys.append(np.array(dev.step(SLOT_BDF2, np.array([0.25 * np.sin(0.7 * s)]))[0], copy=True))
            runs.append((ys, [np.array(v, copy=True) for v in dev.get_state()]))
        finally:
            dev.close()
    (y1, s1), (y2, s2) = runs
    for a, c in zip(y1, y2):
        np.testing.assert_array_equal(a, c)
    for a, c in zip(s1, s2):
        np.testing.assert_array_equal(a, c)


class _HostedOperator:
    """What ShiftedOperator needs of a flowsolver, on the handle of an _Open problem."""

    def __init__(self, p):
        dev = types.SimpleNamespace(lib=p.lib, N=p.N, nn=p.nn, _h=p.h, rowptr=p.rowptr, colidx=p.col)
        self.th = types.SimpleNamespace(device=lambda: dev)


def test_frequency_sweep_in_blocks(prob, caplog):
    """8 frequencies, nu = 2, through linalg.frequency_response: refactor_every = 8 with block=True gives the H of refactor_every = 1
    to 1e-9 with ONE factorisation instead of 8 (16 columns in one block); with max_iter = 1 the block misses its tolerance, the
    group takes the logged per-frequency path and the result still agrees."""
    p = prob
    fs = _HostedOperator(p)
    ww = np.linspace(0.65, 0.75, 8)
    rng = np.random.default_rng(7)
    B = rng.standard_normal((p.N, 2))
    Cm = np.zeros((3, p.N))
    Cm[np.arange(3), [5, p.nn + 9, 2 * p.nn + 4]] = [1.0, -2.0, 0.5]
    Cm[0, 77] = 0.25
    op = linalg.ShiftedOperator(fs, p.A, p.E)
    Href, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False)
    assert op.krylov_info()["refactorisations"] == 8
    op.release()
    for i, w in enumerate(ww):  # (the reference path itself against scipy)
        Hs = Cm @ p.lu(1j * w).solve(B.astype(complex))
        assert np.max(np.abs(Href[:, :, i] - Hs)) <= 1e-9 * np.max(np.abs(Hs))
    scale = np.max(np.abs(Href))
    op = linalg.ShiftedOperator(fs, p.A, p.E, krylov={"max_iter": MAX_ITER, "restart": RESTART, "rtol": 1e-11})
    H, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=8, block=True)
    info = op.krylov_info()
    print("block sweep: |dH| / max|H|", np.max(np.abs(H - Href)) / scale, "iterations", list(info["iterations"]), info)
    assert np.max(np.abs(H - Href)) <= 1e-9 * scale
    assert info["refactorisations"] == 1 and info["iterations"].size == 16
    # two groups of four through the public keyword, one block solve each
    H4, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=4, block=True)
    assert np.max(np.abs(H4 - Href)) <= 1e-9 * scale and op.krylov_info()["refactorisations"] == 3
    op.release()
    op = linalg.ShiftedOperator(fs, p.A, p.E, krylov={"max_iter": 1, "restart": 1, "rtol": 1e-11})
    with caplog.at_level("WARNING", logger="flowcontrol_amd.linalg"):
        Hf, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=8, block=True)
    op.release()
    assert sum("solving them one by one" in r.getMessage() for r in caplog.records) == 1
    assert np.max(np.abs(Hf - Href)) <= 1e-9 * scale
    # the field response takes the same path
    op_kw = {"krylov": {"max_iter": MAX_ITER, "restart": RESTART, "rtol": 1e-11}}
    X = linalg.get_field_response(p.A, B, p.E, ww[:4], verbose=False, flowsolver=fs, refactor_every=4, block=True, **op_kw)
    for i, w in enumerate(ww[:4]):
        Xs = p.lu(1j * w).solve(B.astype(complex))
        assert np.linalg.norm(X[:, :, i] - Xs) <= 1e-9 * np.linalg.norm(Xs)
