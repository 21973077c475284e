"""The open n x n problem of the shifted solver's tests, through the C ABI alone: a structured mesh of the unit square and an
Oseen-type operator with identity rows on the left / bottom velocity dofs.  Shared by tests/test_shifted_krylov_gpu.py and
tests/test_shifted_krylov_counts_gpu.py; ``square_mesh`` needs no device (tests/support/krylov_model.py builds the oracle's form of the
same problem on it)."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def square_mesh(n):
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


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Open:
    """The open n x n problem (n = 10 unless told otherwise) on a handle of its own: an Oseen-type operator with identity rows on the
    left / bottom velocity dofs, two complex right-hand sides, scipy's LU per shift."""

    def __init__(self, n=10):
        from flowcontrol_amd import _lib, linalg

        self.lib = lib = _lib.load()
        coords, cells, cell_edges, edges = square_mesh(n)
        self.h = h = C.c_void_p()
        self.ok(lib.fc_create(C.byref(h), 0, len(coords), len(edges), len(cells), np.ascontiguousarray(coords), cells, cell_edges))
        N, nnz, nn = C.c_int64(), C.c_int64(), C.c_int64()
        self.ok(lib.fc_get_sizes(h, C.byref(N), C.byref(nnz), C.byref(nn)))
        self.N, nnz, nn = N.value, nnz.value, nn.value
        rowptr, col = np.empty(self.N + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        self.ok(lib.fc_get_pattern(h, rowptr, col))
        node_xy = np.vstack([coords, 0.5 * (coords[edges[:, 0]] + coords[edges[:, 1]])])
        adv = np.r_[1.0 + 0.2 * np.sin(3 * node_xy[:, 1]), 0.3 * np.cos(2 * node_xy[:, 0])]
        self.ok(lib.fc_assemble_matrix(h, _lib.SLOT_SCRATCH, 0.0, -0.02, vp(adv), -1.0, None, 1.0, 1.0, 1.0))
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
        self._lu = {}

    def close(self):
        if self.h:
            self.lib.fc_destroy(self.h)
            self.h = C.c_void_p()

    def ok(self, rc):
        assert rc == 0, self.lib.fc_last_error().decode()

    def lu(self, sigma):
        if sigma not in self._lu:
            self._lu[sigma] = spla.splu((sigma * self.E - self.A).astype(complex).tocsc())
        return self._lu[sigma]

    def setup(self, sigma, refine=2):
        self.ok(self.lib.fc_setup_shifted(self.h, vp(self.a_on), vp(self.e), sigma.real, sigma.imag, refine))

    def solve(self):
        """(rc, x [2, N], info [2]) for the two stock right-hand sides"""
        return self.solve_cols(self.b)

    def solve_cols(self, b):
        """fc_solve_shifted of the complex right-hand sides b [k, N]: (rc, x [k, N], info [k])"""
        b = np.atleast_2d(b)
        k = b.shape[0]
        bre, bim = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
        xre, xim, info = np.empty((k, self.N)), np.empty((k, self.N)), np.full(k, np.nan)
        rc = self.lib.fc_solve_shifted(self.h, k, bre, vp(bim), vp(xre), vp(xim), vp(info))
        return rc, xre + 1j * xim, info

    def solve_block(self, sig, b):
        """fc_solve_shifted_block for the shifts sig [k] and right-hand sides b [k, N]: (rc, x [k, N], info [k])"""
        sig = np.asarray(sig, dtype=complex)
        sre, sim = np.ascontiguousarray(sig.real), np.ascontiguousarray(sig.imag)
        bre, bim = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
        xre, xim, info = np.empty((sig.size, self.N)), np.empty((sig.size, self.N)), np.full(sig.size, np.nan)
        rc = self.lib.fc_solve_shifted_block(self.h, sig.size, sre, sim, bre, vp(bim), vp(xre), vp(xim), vp(info))
        return rc, xre + 1j * xim, info

    def block_info(self):
        iv = np.zeros(4, dtype=np.int64)
        self.ok(self.lib.fc_shifted_block_info(self.h, vp(iv)))
        return {"k": int(iv[0]), "KB": int(iv[1]), "lockstep_iterations": int(iv[2]), "cycles": int(iv[3])}

    def krylov_info(self, k=2):
        it, cnt = np.zeros(k, dtype=np.int32), np.zeros(5, dtype=np.int64)
        self.ok(self.lib.fc_shifted_krylov_info(self.h, vp(it), vp(cnt)))
        return it, cnt

    def rel_err(self, x, sigma):
        return max(np.linalg.norm(x[c] - self.lu(sigma).solve(self.b[c])) / np.linalg.norm(self.lu(sigma).solve(self.b[c])) for c in range(2))
