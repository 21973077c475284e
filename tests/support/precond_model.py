"""Host specification of the factorisation-free preconditioner (``fc_setup_krylov``; ``csrc/fc_precond.hpp`` builds it, ``apply_pc`` in
``csrc/fc_hip.hip`` runs it with the kernels of ``csrc/fc_precond.hip.h``) -- to ``fc_precond.hpp`` what ``ndsolver.py`` is to
``fc_symbolic.hpp``: scipy.sparse and numpy, written from the definition, sharing no code with the library.

    A = [ F  Bt ]      M^-1 r:   u  = k damped-Jacobi sweeps on F u = r_u from zero       (omega = min(1, 1.4 / rho(D^-1 F)); 1 for k = 1)
        [ B  0  ]                zp = one V(s,s)-cycle on S zp = B u - r_p               S = B diag(F)^-1 Bt (+ the pin's shift)
                                 zu = u - diag(F)^-1 Bt zp

:class:`Spec` rebuilds the setup in float64 (compact blocks in the order of the permuted positions, the Schur complement, the
three-pass greedy aggregation, smoothed prolongators, Galerkin products, the dense coarsest operator) and applies it in the UNFOLDED
textbook form in ``np.longdouble``: plain Jacobi sweeps, a recursive V-cycle with an exact solve on the coarsest level (not the stored
inverse).  ``reverse=True`` builds the second variant, which changes only what rounding may change (the sums of the power iteration and
the accumulation order of every sparse product reversed); :meth:`Spec.folded` gives the float64 folded operators of the device
(K_F, G, U, the dense inverse) and :func:`apply_folded` evaluates them with the kernels' formula -- together they measure the spread.

:meth:`Spec.route` is the launch list ``fc_get_pc_route`` must report, :func:`reach` what a launch list exercises in the kernels."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

L = np.longdouble
THETA, COARSE_MAX, MAX_LEVELS = 0.08, 256, 12
KERNELS = ("csr", "dense", "final", "bshare", "final_share", "fill")  # DeviceSolver.PC_KERNELS
CSR, DENSE, FINAL, BSHARE, FINAL_SHARE, FILL = range(6)

# ── measured host errors ──────────────────────────────────────────────────────────────────────────────────────────────────────────────
# The float64 folded apply (the C++ driver's matrices, the kernels' formula base + scale * dinv * (rhs - M x)) against the longdouble
# unfolded model, largest over CASES x SWEEPS x AMG_SWEEPS x both permutations x the three inputs, relative to the reference's norm of
# the same part: (2-norm, max-norm).  tests/test_precond_model_host.py re-measures them and fails when one is below the measurement or
# more than twice above it.  The device may miss the model by MARGIN times these: the project's margin for another fixed summation
# order (four partial sums per lane and a shuffle tree per row instead of one running sum).
# Measured: velocity 5.77e-15 / 9.27e-15, pressure 9.40e-15 / 6.13e-15 -- the velocity 2-norm on unit_square(48, 48) with the pressure-only
# input, the other three on the enclosed mesh, whose pinned Schur complement is the worst conditioned (coarsest operator: cond 1e4
# against 40 to 400 on the open meshes, which stay below 5.8e-15 / 6.5e-15 and 3.1e-15 / 2.5e-15).  What is measured is mostly the
# SETUP: the driver's hierarchy and the specification's part by rounding, and the V-cycle carries that to the result -- the
# specification's own two variants part by as much (1.4e-14 at most).
HOST_ERROR_VELOCITY = (6.6e-15, 1.07e-14)
HOST_ERROR_PRESSURE = (1.08e-14, 7.1e-15)
MARGIN = 16.0

# ── cases ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
#: Mesh.unit_square(n, n) -> (N, pressure dofs, sparse AMG levels, rows of the coarsest level), open flow (km.wall_dofs)
CASES = {6: (387, 49, 0, 49), 12: (1419, 169, 0, 169), 16: (2467, 289, 1, 46), 48: (21219, 2401, 2, 55)}
ENCLOSED = 16  # ... and this mesh once more with every wall Dirichlet and the pressure pinned
PIN_SHIFT = 1.0
SWEEPS = (1, 2, 3, 4)
AMG_SWEEPS = (1, 2)
#: the partitioned apply (world 2, thread ranks): meshes and sweeps
SHARE_CASES = (12, 16)
SHARE_SWEEPS = (1, 2)


def operator_args(xy, dt=0.005, Re=100.0):
    """keyword set of assemble_matrix (the oracle's and the device's take the same): the BDF2 operator of krylov_model's "fast" pair"""
    U0 = np.r_[1.0 + 0.3 * np.sin(xy[:, 0]) * np.cos(0.7 * xy[:, 1]), 0.2 * np.cos(0.5 * xy[:, 0] + 0.1) * np.sin(xy[:, 1])]
    return dict(mass=1.5 / dt, nu=1.0 / Re, adv=U0, lin=U0)


def pin_dof(th):
    """the pressure dof the enclosed case pins (W numbering): a vertex in the middle of the numbering"""
    return th.N - 1 - th.nv // 2


def all_wall_dofs(th):
    """both velocity components on every boundary edge: an enclosed flow"""
    m = th.mesh
    be = m.boundary_edges()
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    return np.sort(np.r_[nodes, nodes + th.nn])


def inputs(N, n_vel, perm, seed=11):
    """the three inputs of a case (W layout): random, random in the pressure part only, the unit vector of the last permuted row"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(N)
    b = rng.standard_normal(N)
    b[:n_vel] = 0.0
    c = np.zeros(N)
    c[int(perm[-1])] = 1.0
    return {"random": a, "pressure": b, "unit": c}


# ── sparse helpers that keep the STRUCTURAL pattern (scipy's products and sums drop entries that cancel to zero; the library keeps them,
#    and the lanes of a launch follow from the stored entries per row) ─────────────────────────────────────────────────────────────────
def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def _ones(M):
    return sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)


def _rows(M):
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))


def _on_pattern(num, pat):
    """the values of ``num`` on the (larger) sorted pattern ``pat``"""
    num, pat = _csr(num), _csr(pat)
    kp = _rows(pat).astype(np.int64) * pat.shape[1] + pat.indices
    kn = _rows(num).astype(np.int64) * num.shape[1] + num.indices
    at = np.searchsorted(kp, kn)
    assert np.array_equal(kp[at], kn)
    v = np.zeros(pat.nnz)
    v[at] = num.data
    return sp.csr_matrix((v, pat.indices.copy(), pat.indptr.copy()), shape=pat.shape)


def _reversed_rows(M):
    """the same matrix with every row stored back to front: scipy's products then accumulate in the reverse order"""
    M = _csr(M)
    idx = np.arange(M.nnz)
    start, stop = M.indptr[:-1], M.indptr[1:]
    r = _rows(M)
    back = start[r] + (stop[r] - 1 - idx)
    return sp.csr_matrix((M.data[back], M.indices[back], M.indptr), shape=M.shape)


def spgemm(A, B, reverse=False):
    A, B = _csr(A), _csr(B)
    num = (_reversed_rows(A) if reverse else A) @ B
    return _on_pattern(num, _ones(A) @ _ones(B))


def add(A, alpha, B, beta):
    return _on_pattern(alpha * _csr(A) + beta * _csr(B), _ones(A) + _ones(B))


def scale_rows(d, M):
    M = _csr(M).copy()
    M.data = M.data * np.asarray(d)[_rows(M)]
    return M


def scale_cols(M, d):
    M = _csr(M).copy()
    M.data = M.data * np.asarray(d)[M.indices]
    return M


def spmv_long(M, x):
    """M x with products and sums in np.longdouble"""
    M = _csr(M)
    out = np.zeros(M.shape[0], dtype=L)
    full = np.diff(M.indptr) > 0
    if M.nnz:
        out[full] = np.add.reduceat(M.data.astype(L) * np.asarray(x, dtype=L)[M.indices], M.indptr[:-1][full])
    return out


def solve_long(A, b):
    """A^-1 b of a small dense matrix to longdouble accuracy (numpy's solvers stop at float64: an LU in float64, refined with
    longdouble residuals until the correction is below the longdouble round-off)"""
    lu = sla.lu_factor(A)
    Al, b = A.astype(L), np.asarray(b, dtype=L)
    x = np.zeros(A.shape[0], dtype=L)
    for _ in range(8):
        dx = sla.lu_solve(lu, np.asarray(b - Al @ x, dtype=np.float64))
        x = x + dx
        if not np.any(dx) or np.abs(dx).max() <= 1e-22 * np.abs(x).max():
            break
    return x


# ── setup ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def lcg_start(n):
    """the start vector of the power iteration: a 64-bit linear congruential generator, 16 bits of every state"""
    s, x = 0x9E3779B97F4A7C15, np.empty(n)
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        x[i] = 0.5 + ((s >> 33) & 0xFFFF) / 65536.0
    return x


def rho_dinv(A, d, iters=40, reverse=False):
    """spectral radius of D^-1 A by 40 steps of the power iteration from lcg_start"""
    A = _csr(A)
    n = A.shape[0]
    if n == 0:
        return 1.0
    if reverse:
        A = _reversed_rows(A)
    x, rho = lcg_start(n), 1.0
    for _ in range(iters):
        y = (A @ x) / d
        # running sums, front to back as the library forms them (np.sum would add pairwise: sharper, and so further away) or back to front
        ny, nx = (np.cumsum((y * y)[::-1])[-1], np.cumsum((x * x)[::-1])[-1]) if reverse else (np.cumsum(y * y)[-1], np.cumsum(x * x)[-1])
        if not (ny > 0.0 and nx > 0.0):
            return rho
        rho = float(np.sqrt(ny / nx))
        x = y * (1.0 / np.sqrt(ny))
    return rho


def split_blocks(A, perm, n_vel):
    """(vpos, ppos, F, B, Bt, diag F): the blocks in compact numberings, velocity / pressure dofs each in the order of their permuted
    positions, exact zeros dropped"""
    perm = np.asarray(perm, dtype=np.int64)
    vel = perm < n_vel
    vpos, ppos = np.flatnonzero(vel), np.flatnonzero(~vel)
    vw, pw = perm[vpos], perm[ppos]
    A = _csr(A).copy()
    dF = A.diagonal()[vw]
    A.eliminate_zeros()
    rows_v, rows_p = A[vw], A[pw]
    F, Bt, B = _csr(rows_v[:, vw]), _csr(rows_v[:, pw]), _csr(rows_p[:, vw])
    assert rows_p[:, pw].nnz == 0, "pressure-pressure entries: not a Taylor-Hood saddle-point matrix"
    return vpos, ppos, F, B, Bt, dF


def strength_ratios(A, theta=THETA):
    """|a_ij| / (theta sqrt|a_ii a_jj|) of every stored off-diagonal entry: >= 1 is a strong connection"""
    A = _csr(A)
    d = A.diagonal()
    r, c = _rows(A), A.indices
    off = r != c
    return np.abs(A.data[off]) / (theta * np.sqrt(np.abs(d[r[off]] * d[c[off]])))


def aggregate(A, theta=THETA):
    """three-pass greedy aggregation on the strength graph: a free row whose strong neighbours are all free roots an aggregate of them
    all; a row left over joins the aggregate of its first strong neighbour that pass 1 placed; the rest become singletons"""
    A = _csr(A)
    n = A.shape[0]
    d = A.diagonal()
    strong = []
    for i in range(n):
        c, v = A.indices[A.indptr[i] : A.indptr[i + 1]], A.data[A.indptr[i] : A.indptr[i + 1]]
        keep = (c != i) & (np.abs(v) >= theta * np.sqrt(np.abs(d[i] * d[c])))
        strong.append(c[keep])
    agg, na = np.full(n, -1, dtype=np.int64), 0
    for i in range(n):
        if agg[i] < 0 and np.all(agg[strong[i]] < 0):
            agg[i] = na
            agg[strong[i]] = na
            na += 1
    pass1 = agg.copy()
    for i in range(n):
        if pass1[i] < 0:
            placed = strong[i][pass1[strong[i]] >= 0]
            if placed.size:
                agg[i] = pass1[placed[0]]
    for i in range(n):
        if agg[i] < 0:
            agg[i] = na
            na += 1
    return agg, na


def lanes_of(M):
    mean = M.nnz / M.shape[0] if M.shape[0] else 0.0
    return 4 if mean <= 6 else (8 if mean <= 40 else (16 if mean <= 96 else 32))


class Spec:
    """The preconditioner of one operator.  ``A``: the operator in W numbering (Dirichlet rows and columns eliminated symmetrically),
    ``perm``: permuted row -> W dof, ``n_vel`` = 2 nn, ``pin`` = (W dof, shift) or None."""

    def __init__(self, A, perm, n_vel, pin=None, reverse=False):
        self.N, self.n_vel, self.perm, self.reverse = A.shape[0], int(n_vel), np.asarray(perm, dtype=np.int64), reverse
        self.vpos, self.ppos, self.F, self.B, self.Bt, self.dF = split_blocks(A, perm, n_vel)
        assert np.all(np.abs(self.dF) > 0.0)
        self.nu, self.np = self.vpos.size, self.ppos.size
        self.dinv = 1.0 / self.dF
        self.rhoF = rho_dinv(self.F, self.dF, reverse=reverse)
        S = spgemm(scale_cols(self.B, self.dinv), self.Bt, reverse)
        if pin is not None:
            k = np.flatnonzero(self.perm[self.ppos] == int(pin[0]))
            if k.size:
                S = S + sp.csr_matrix(([float(pin[1])], ([k[0]], [k[0]])), shape=S.shape)
                S = _csr(S)
        self.S = S
        self.levels = []  # dicts: A, agg, na, rho, wdinv, P, R
        A = S
        while A.shape[0] > COARSE_MAX and len(self.levels) < MAX_LEVELS:
            n = A.shape[0]
            agg, na = aggregate(A)
            if na >= n:
                break
            T = sp.csr_matrix((1.0 / np.sqrt(np.bincount(agg, minlength=na)[agg].astype(float)), agg, np.arange(n + 1)), shape=(n, na))
            d = A.diagonal()
            assert np.all(np.abs(d) > 0.0)
            rho = rho_dinv(A, d, reverse=reverse)
            w = 4.0 / (3.0 * rho)
            AT = spgemm(A, T, reverse)
            P = AT.copy()
            r = _rows(P)
            P.data = (-w / d)[r] * P.data
            own = P.indices == agg[r]
            assert own.sum() == n  # the diagonal of A is stored: the pattern of A T holds the row's own aggregate
            P.data[own] += T.data[r[own]]
            R = _csr(P.T)
            Ac = spgemm(R, spgemm(A, P, reverse), reverse)
            self.levels.append(dict(A=A, agg=agg, na=na, rho=rho, wdinv=w / d, P=P, R=R))
            A = Ac
        assert A.shape[0] <= 4096
        self.Ac = A.toarray()
        self.level_rows = [V["A"].shape[0] for V in self.levels] + [A.shape[0]]
        self._folded = {}

    def omega(self, sweeps):
        return min(1.0, 1.4 / self.rhoF) if sweeps > 1 else 1.0

    # ── the apply, unfolded, in longdouble ──
    def _smooth(self, V, x, r, s):
        for _ in range(s):
            x = x + V["wdinv"].astype(L) * (r - spmv_long(V["A"], x))
        return x

    def vcycle(self, r, s, l=0):
        if l == len(self.levels):
            return solve_long(self.Ac, r)
        V = self.levels[l]
        x = self._smooth(V, np.zeros(r.size, dtype=L), r, s)
        x = x + spmv_long(V["P"], self.vcycle(spmv_long(V["R"], r - spmv_long(V["A"], x)), s, l + 1))
        return self._smooth(V, x, r, s)

    def apply(self, x, sweeps, amg_sweeps):
        """M^-1 x, W layout in and out, np.longdouble"""
        xp = np.asarray(x, dtype=L)[self.perm]
        ru, rp = xp[self.vpos], xp[self.ppos]
        wd = L(self.omega(sweeps)) * self.dinv.astype(L)
        u = np.zeros(self.nu, dtype=L)
        for _ in range(sweeps):
            u = u + wd * (ru - spmv_long(self.F, u))
        zp = self.vcycle(spmv_long(self.B, u) - rp, amg_sweeps)
        zu = u - self.dinv.astype(L) * spmv_long(self.Bt, zp)
        out_p = np.zeros(self.N, dtype=L)
        out_p[self.vpos], out_p[self.ppos] = zu, zp
        out = np.zeros(self.N, dtype=L)
        out[self.perm] = out_p
        return out

    # ── the device's operators: float64, folded ──
    def folded(self, sweeps, amg_sweeps):
        """dict of the matrices the device holds: vpos, ppos, perm, dinv, wdinv, KF (compact columns; None for one sweep), F, B, Bt,
        G[l], U[l] and the dense inverse cinv"""
        rev = self.reverse
        if amg_sweeps not in self._folded:
            G, U = [], []
            for V in self.levels:
                A, P, R, wd = V["A"], V["P"], V["R"], V["wdinv"]
                n = A.shape[0]
                I = sp.identity(n, format="csr")
                if amg_sweeps == 1:
                    G.append(spgemm(R, add(I, 1.0, scale_cols(A, wd), -1.0), rev))  # R (I - A Wd)
                    K = scale_rows(wd, add(I, 2.0, scale_cols(A, wd), -1.0))        # Wd (2 I - A Wd)
                    Q = add(P, 1.0, scale_rows(wd, spgemm(A, P, rev)), -1.0)        # (I - Wd A) P
                else:
                    E = add(I, 1.0, scale_rows(wd, A), -1.0)                        # I - Wd A
                    W2 = scale_cols(add(I, 1.0, E, 1.0), wd)                        # (I + E) Wd
                    G.append(spgemm(R, add(I, 1.0, spgemm(A, W2, rev), -1.0), rev))  # R (I - A W2)
                    E2 = spgemm(E, E, rev)
                    K = spgemm(add(I, 1.0, E2, 1.0), W2, rev)                       # (I + E^2) W2
                    Q = spgemm(E2, P, rev)                                          # E^2 P
                U.append(_csr(sp.hstack([K, Q], format="csr")))
            self._folded[amg_sweeps] = (G, U, np.linalg.inv(self.Ac))
        G, U, cinv = self._folded[amg_sweeps]
        wd = self.omega(sweeps) * self.dinv
        KF = scale_rows(wd, add(sp.identity(self.nu, format="csr"), 2.0, scale_cols(self.F, wd), -1.0)) if sweeps >= 2 else None
        if KF is not None:
            KF = _on_pattern(KF, self.F)  # the pattern of F: its diagonal is stored
        return dict(vpos=self.vpos, ppos=self.ppos, perm=self.perm, dinv=self.dinv, wdinv=wd, KF=KF, F=self.F, B=self.B, Bt=self.Bt, G=G, U=U, cinv=cinv)

    # ── what the apply launches ──
    def route(self, sweeps, amg_sweeps):
        """(rows of fc_get_pc_route, longest row of every launch's matrix or 0)"""
        m = self.folded(sweeps, amg_sweeps)
        longest = lambda M: int(np.diff(M.indptr).max()) if M.nnz else 0  # noqa: E731
        out, rows = [], []
        if sweeps >= 2:
            out.append((CSR, self.nu, lanes_of(m["KF"]), -1)), rows.append(longest(m["KF"]))
        else:
            out.append((CSR, self.nu, 1, -1)), rows.append(0)
        for _ in range(2, sweeps):
            out.append((CSR, self.nu, lanes_of(self.F), -1)), rows.append(longest(self.F))
        out.append((CSR, self.np, lanes_of(self.B), -1)), rows.append(longest(self.B))
        nl = len(self.levels)
        for l in range(nl):
            out.append((CSR, self.levels[l]["na"], lanes_of(m["G"][l]), l)), rows.append(longest(m["G"][l]))
        out.append((DENSE, self.Ac.shape[0], 64, nl)), rows.append(self.Ac.shape[0])
        for l in reversed(range(nl)):
            out.append((CSR, self.levels[l]["A"].shape[0], lanes_of(m["U"][l]), l)), rows.append(longest(m["U"][l]))
        out.append((FINAL, self.nu + self.np, 4, -1)), rows.append(longest(self.Bt))
        return np.array(out, dtype=np.int32), rows

    def launches(self, sweeps):
        return max(1, sweeps - 1) + 3 + 2 * len(self.levels)

    def share_route(self, rowkind, lead, sweeps, amg_sweeps):
        """the launch list of the partitioned apply on one rank: ``rowkind`` (W numbering: 0 another rank's dof, 1 owned, 2 the root's,
        replicated), ``lead``: this rank accounts for the root's rows.  Two fills (the output, the Schur right-hand side), K_F over the
        rank's velocity rows (own rows whole, the root's over the columns the rank accounts for; one sweep: D^-1, an entry per row),
        the rank's share of B, the replicated V-cycle, the final launch over the rows the rank computes and holds."""
        rowkind = np.asarray(rowkind)
        kv, kp = rowkind[self.perm[self.vpos]], rowkind[self.perm[self.ppos]]
        accounts = lambda k: (k == 1) | ((k == 2) & bool(lead))  # noqa: E731
        lv = np.r_[np.flatnonzero(kv == 1), np.flatnonzero(kv == 2)]
        nv = lv.size
        K = self.F if sweeps >= 2 else sp.identity(self.nu, format="csr")
        K = _csr(K)
        r, c = _rows(K), K.indices
        kept = ((kv[r] == 1) | ((kv[r] == 2) & accounts(kv[c])))
        assert not np.any((kv[r] == 1) & (kv[c] == 0)), "a velocity row of this rank couples to another rank's velocity column"
        k_nnz = int(np.count_nonzero(kept))
        local = kv != 0
        per_row = np.add.reduceat(local[self.B.indices].astype(np.int64), self.B.indptr[:-1])  # (every row of B holds an entry)
        assert np.all(np.diff(self.B.indptr) > 0)
        rows_b = accounts(kp) | (per_row > 0)
        nbs, b_nnz = int(np.count_nonzero(rows_b)), int(per_row[rows_b].sum())
        nph = int(np.count_nonzero(kp != 0))
        lanes = lambda nnz, n: 4 if nnz <= 6 * n else (8 if nnz <= 40 * n else (16 if nnz <= 96 * n else 32))  # noqa: E731
        single, _ = self.route(sweeps, amg_sweeps)
        cycle = single[max(1, sweeps - 1) + 1 : -1]
        head = [(FILL, self.N, 0, -1), (FILL, self.np, 0, -1), (CSR, nv, lanes(k_nnz, nv), -1), (BSHARE, nbs, 4 if lanes(b_nnz, nbs) == 4 else 8, -1)]
        return np.array(head + cycle.tolist() + [(FINAL_SHARE, nv + nph, 4, -1)], dtype=np.int32)


def apply_folded(m, x, sweeps):
    """the device's launch sequence in float64 on the matrices ``m`` (Spec.folded, or the C++ driver's), every launch in the kernels'
    form out = base + scale * dinv * (rhs - M x); W layout in and out"""
    xp = np.asarray(x, dtype=np.float64)[m["perm"]]
    ru, rp = xp[m["vpos"]], xp[m["ppos"]]
    if sweeps >= 2:
        u = 0.0 + -1.0 * (0.0 - m["KF"] @ ru)
    else:
        u = 0.0 + 1.0 * ((ru - 0.0) * m["dinv"])
    for _ in range(2, sweeps):
        u = u + 1.0 * ((ru - m["F"] @ u) * m["wdinv"])
    cat = [-1.0 * (rp - m["B"] @ u)]
    for G in m["G"]:
        cat.append(-1.0 * (0.0 - G @ cat[-1]))
    z = m["cinv"] @ cat[-1]
    for l in reversed(range(len(m["G"]))):
        z = -1.0 * (0.0 - m["U"][l] @ np.r_[cat[l], z])
    zu = u - m["dinv"] * (m["Bt"] @ z)
    out_p = np.zeros(xp.size)
    out_p[m["vpos"]], out_p[m["ppos"]] = zu, z
    out = np.zeros(xp.size)
    out[m["perm"]] = out_p
    return out


def part_errors(got, ref, n_vel):
    """((2-norm, max-norm) of the velocity part, the same of the pressure part), relative to the reference's norm of that part; a part
    the reference has zero in must be zero (error 0) or counts as infinitely wrong"""
    got, ref = np.asarray(got, dtype=L), np.asarray(ref, dtype=L)
    out = []
    for s in (slice(0, n_vel), slice(n_vel, None)):
        g, r = got[s], ref[s]
        if not np.any(r):
            out.append((0.0, 0.0) if not np.any(g) else (np.inf, np.inf))
        else:
            out.append((float(np.sqrt(np.sum((g - r) ** 2) / np.sum(r**2))), float(np.abs(g - r).max() / np.abs(r).max())))
    return tuple(out)


def tolerances():
    return tuple(tuple(MARGIN * e for e in part) for part in (HOST_ERROR_VELOCITY, HOST_ERROR_PRESSURE))


# ── reach: what a launch list exercises in the kernels ────────────────────────────────────────────────────────────────────────────────
#: everything the case table must reach between its cases
REACH = (
    "csr lanes 1", "csr lanes 8", "csr lanes 16", "csr lanes 32",
    "csr one trip", "csr two trips", "csr three trips", "csr last workgroup partial", "csr several workgroups",
    "csr rhs gather + dinv, no matrix", "csr matrix only", "csr matrix + base + dinv + rhs gather", "csr matrix + rhs gather",
    "dense n < 64, n % 4 != 0", "dense two column trips", "dense three column trips", "dense last workgroup partial",
    "final rows no multiple of 64", "final second trip of a Bt row",
    "sweeps 1", "sweeps 2", "sweeps 3: result in u1", "sweeps 4: result back in u0",
    "sparse levels 0", "sparse levels 1", "sparse levels 2", "V(1,1)", "V(2,2)", "pin",
)
#: what no case reaches, and why
UNREACHED = {
    "csr lanes 4": "no operator of the single-GPU apply has a mean of <= 6 entries per row (B, K_F and F hold 15 to 28, G and U more); the "
                   "partitioned apply with one sweep runs it (its K_F is D^-1, an entry per row): tests/test_krylov_partitioned_gpu.py",
    "csr scatter (opos)": "no call site passes a scatter list: every fc_pc_csr launch writes out[i]",
    "csr four trips and more": "a row of more than 12 * lanes entries needs a G / U row beyond 384 entries at 32 lanes: the level-1 rows "
                               "of unit_square(48, 48) stop at three trips",
    "more than 2 sparse levels": "needs more than ~16 000 pressure dofs (O1 refined: tests/test_krylov_free_gpu.py runs it, unpinned)",
}


def reach(route, rows, sweeps, amg_sweeps, levels, pinned=False):
    """the entries of REACH that one apply with this launch list exercises"""
    got = {f"sweeps {sweeps}" + {3: ": result in u1", 4: ": result back in u0"}.get(sweeps, ""), f"sparse levels {levels}",
           f"V({amg_sweeps},{amg_sweeps})"}
    if pinned:
        got.add("pin")
    for i, ((kernel, n, lanes, level), longest) in enumerate(zip(route.tolist(), rows)):
        if kernel == CSR:
            got.add(f"csr lanes {lanes}")
            rpb = 256 // lanes
            if n % rpb:
                got.add("csr last workgroup partial")
            if n > rpb:
                got.add("csr several workgroups")
            if lanes > 1:
                trips = -(-longest // (4 * lanes))
                got.add({1: "csr one trip", 2: "csr two trips", 3: "csr three trips"}.get(trips, "csr four trips and more"))
            if level >= 0 or (i == 0 and sweeps >= 2):  # G, U, K_F
                got.add("csr matrix only")
            elif i == 0:
                got.add("csr rhs gather + dinv, no matrix")
            elif i < max(1, sweeps - 1):  # a further sweep on F
                got.add("csr matrix + base + dinv + rhs gather")
            else:  # B u - in_p
                got.add("csr matrix + rhs gather")
        elif kernel == DENSE:
            if n < 64 and n % 4:
                got.add("dense n < 64, n % 4 != 0")
            if n > 64:
                got.add("dense two column trips")
            if n > 128:
                got.add("dense three column trips")
            if n % 4:
                got.add("dense last workgroup partial")
        elif kernel == FINAL:
            if n % 64:
                got.add("final rows no multiple of 64")
            if longest > 4:
                got.add("final second trip of a Bt row")
    return got
