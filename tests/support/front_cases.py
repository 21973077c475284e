"""Matrices that force row exchanges in every pivot block of the front elimination, and a numpy model of the device's
order of operations — TEST INFRASTRUCTURE (host only: nothing here imports the device package).

  pivot_stress_matrix   CSR values on a given pattern: a well-conditioned matrix whose elimination on a given tree needs
                        exchanges inside the 32-aligned pivot blocks, and only there
  model_elimination     blocked Gauss-Jordan of every front as csrc/fc_front.hip.h runs it (pivot search confined to the
                        block, the 8x threshold on the truncated key, ties to the smallest row), with a log of the
                        exchanges that no rounding could have avoided
  census                which kernel paths a log and a tree reach (the classes tests/test_front_cases_host.py requires)
  predicted_step_widths what fc_get_refactor_steps must report for a tree and a route
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.support import ndsolver
from tests.support.ndsolver import BlockFactors, NDTree

KEEP_LOG2 = 2  # FC_FE_PIVOT_KEEP_LOG2: the diagonal is kept while its binary exponent is within this many of the largest candidate's
MANDATORY = 2.0**-10  # an exchange is logged as mandatory when |diagonal| < this * |largest candidate|: far from the 8x rule
ROW_SUM_FLOOR = 8.0  # a row that keeps only a few free columns (next to a Dirichlet corner) is scaled as if its entries summed to this: rows of like size
HUGE_MIN_NF = 256  # FC_FE_HUGE_MIN_NF

ROUTES = {
    "default": {},
    "wide": {"FC_FE_WIDE_NF": "64", "FC_FE_HUGE_NF": "1000000", "FC_FE_HUGE_MB": "1e9"},
    "huge": {"FC_FE_HUGE_NF": "256"},
}


def _node_start(tree: NDTree, N: int) -> np.ndarray:
    """First row (new numbering) of the tree node that owns each row (new numbering)."""
    start = np.empty(N, dtype=np.int64)
    for ptr in tree.node_ptr:
        for a, b in zip(ptr[:-1], ptr[1:]):
            start[int(a) : int(b)] = int(a)
    return start


def pivot_stress_matrix(rowptr, colidx, tree: NDTree, bc_dofs, seed: int, frac: float = 0.5) -> np.ndarray:
    """CSR values on the pattern (rowptr, colidx): uniform(-1, 1) entries, made nonsingular by one dominant entry per row that
    sits OFF the diagonal for about ``frac`` of the rows.

    A random involution pairs row r with a column c != r of its pattern that the same tree node owns and that lies in the
    same 32-aligned pivot block of that node ((iperm[r] - i0) // 32 == (iperm[c] - i0) // 32; such a block is also inside one
    64-block and inside one 32-sub-block of a 128-block).  Paired rows get diagonal exactly 0.0 and the entry
    (r, c) = +-(2...3) * sum|row|, unpaired rows that entry on the diagonal: a row permutation of a strictly diagonally
    dominant matrix, for which exchanges inside the pivot blocks are both necessary and sufficient.

    Rows WITHOUT a diagonal in the pattern (the pressure rows of the device's pattern: no pressure-pressure coupling) cannot
    stay unpaired.  Each takes a partner in its own block when one is free (a forced exchange).  The others -- whole pivot
    blocks of pressure rows have no in-block partner at all -- are ANCHORED to a free, unpaired column c eliminated before
    their block starts: (r, c) = +-(6...8) * sum|row r| and (c, r) = +-8 * sum|row c| under c's dominant diagonal
    +-(2...3) * 9 * sum|row c| (row c is then divided by 9).  Eliminating c leaves -(r, c)(c, r) / (c, c), at least 0.3 |(r, c)|, on r's diagonal against
    at most 0.14 |(r, c)| elsewhere in the row (every pivot row is dominant by a factor >= 2): the block of such rows
    arrives diagonally dominant, as the pressure Schur complement of the real operators does.

    That bound is an estimate, not a proof: tests/test_front_cases_host.py asserts cond(A) <= 1e3 and the agreement of the
    block-local model with a LAPACK inverse for every case in use.  sum|row| is taken as at least ROW_SUM_FLOOR.

    Dirichlet rows are identity and Dirichlet columns zero elsewhere, as fc_apply_bc leaves them."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    N = rowptr.size - 1
    rng = np.random.default_rng(seed)
    is_bc = np.zeros(N, dtype=bool)
    is_bc[np.asarray(bc_dofs, dtype=np.int64)] = True
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    vals = rng.uniform(-1.0, 1.0, colidx.size)
    vals[is_bc[colidx] | is_bc[rows]] = 0.0
    iperm = np.asarray(tree.iperm, dtype=np.int64)
    start = _node_start(tree, N)
    block0 = start[iperm] + 32 * ((iperm - start[iperm]) // 32)  # first row (new numbering) of the 32-block of every dof (old numbering)
    slot = {}  # (row, col) -> position in vals, for the entries that may become dominant
    diag = np.full(N, -1, dtype=np.int64)
    diag[rows[rows == colidx]] = np.nonzero(rows == colidx)[0]
    has = sp.csr_matrix((np.ones(colidx.size, dtype=bool), colidx, rowptr), shape=(N, N))
    sym = has.multiply(has.T).tocsr()  # entries whose transpose is in the pattern too
    sym.sort_indices()

    def cols_of(r):
        c = sym.indices[sym.indptr[r] : sym.indptr[r + 1]]
        return c[(c != r) & ~is_bc[c]]

    def pos(r, c):
        key = (int(r), int(c))
        if key not in slot:
            seg = colidx[rowptr[r] : rowptr[r + 1]]
            slot[key] = int(rowptr[r] + np.nonzero(seg == c)[0][0])
        return slot[key]

    partner = np.full(N, -1, dtype=np.int64)  # the involution: partner[r] = c, partner[c] = r
    anchor = np.full(N, -1, dtype=np.int64)  # anchor[r] = c for the anchored rows, anchored_by[c] = r
    anchored_by = np.full(N, -1, dtype=np.int64)
    free = ~is_bc
    no_diag = np.nonzero((diag < 0) & ~is_bc)[0]
    # rows without a diagonal first: partner in the block, else an anchor eliminated before the block (the same node's columns first)
    for r in rng.permutation(no_diag):
        if not free[r]:
            continue  # already the partner of another row
        c = cols_of(r)
        c = c[free[c]]
        same = c[block0[c] == block0[r]]
        if same.size:
            q = int(rng.choice(same))
            partner[r], partner[q] = q, r
            free[r] = free[q] = False
            continue
        before = c[(iperm[c] < block0[r]) & (diag[c] >= 0)]
        own = before[start[iperm[before]] == start[iperm[r]]]
        pool = own if own.size else before
        if pool.size == 0:
            raise ValueError(f"row {int(r)} has no diagonal, no partner in its pivot block and no column eliminated before it")
        q = int(rng.choice(pool))
        anchor[r], anchored_by[q] = q, r
        free[r] = free[q] = False
    # ... then about frac of the others, in random order
    for r in rng.permutation(np.nonzero(free)[0]):
        if not free[r] or rng.random() >= frac:
            continue
        c = cols_of(r)
        c = c[free[c] & (block0[c] == block0[r])]
        if c.size:
            q = int(rng.choice(c))
            partner[r], partner[q] = q, r
            free[r] = free[q] = False
    # the dominant entries
    sign = lambda: rng.choice([-1.0, 1.0])  # noqa: E731
    rsum = lambda seg: max(np.abs(vals[seg]).sum(), ROW_SUM_FLOOR)  # noqa: E731
    for r in np.nonzero(~is_bc)[0]:
        seg = slice(int(rowptr[r]), int(rowptr[r + 1]))
        if diag[r] >= 0:
            vals[diag[r]] = 0.0
        if partner[r] >= 0:
            k = pos(r, partner[r])
            vals[k] = 0.0
            vals[k] = sign() * rng.uniform(2.0, 3.0) * rsum(seg)
        elif anchor[r] >= 0:
            k = pos(r, anchor[r])
            vals[k] = 0.0
            vals[k] = sign() * rng.uniform(6.0, 8.0) * rsum(seg)
        elif anchored_by[r] >= 0:
            k = pos(r, anchored_by[r])
            vals[k] = 0.0
            s = rsum(seg)
            vals[seg] /= 9.0  # (the whole row, so that its diagonal is the size of every other row's dominant entry)
            vals[k] = sign() * 8.0 * s / 9.0
            vals[diag[r]] = sign() * rng.uniform(2.0, 3.0) * s
        else:
            vals[diag[r]] = sign() * rng.uniform(2.0, 3.0) * rsum(seg)
    bc_rows = np.nonzero(is_bc)[0]
    if np.any(diag[bc_rows] < 0):
        raise ValueError("a Dirichlet row without a diagonal in the pattern")
    vals[diag[bc_rows]] = 1.0
    return vals


# ──────────────────────────────────────────────────────────────────────────────────────────
def _key(x: np.ndarray) -> np.ndarray:
    """The magnitude the device's pivot search compares: upper word of |x| (exponent + 20 mantissa bits) with the low six bits
    cleared (they carry the lane)."""
    hi = (np.abs(np.asarray(x, dtype=np.float64)).view(np.uint64) >> np.uint64(32)).astype(np.int64)
    return hi & ~np.int64(63)


def _gj_inverse(blk: np.ndarray, exchange: bool, on_swap) -> np.ndarray:
    """Inverse of ``blk`` by in-place Gauss-Jordan, one column at a time, as fc_fe_gj_block runs it: the pivot of column k is
    sought among the rows k.. of the block, the diagonal is kept while its exponent is within KEEP_LOG2 of the largest
    candidate's, ties go to the smallest row; the row exchanges are undone on the columns of the result.
    ``on_swap(k, p, mandatory)`` is called for every exchange."""
    a = np.array(blk, dtype=np.float64)
    n = a.shape[0]
    piv = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k
            if exchange and k + 1 < n:
                keys = _key(a[k:, k])
                m = int(np.argmax(keys))  # (first maximum: the smallest row)
                if (keys[m] >> 20) > (keys[0] >> 20) + KEEP_LOG2:
                    p = k + m
                    on_swap(k, p, abs(a[k, k]) < MANDATORY * np.abs(a[k:, k]).max())
                    a[[k, p]] = a[[p, k]]
            piv[k] = p
            d = 1.0 / a[k, k]
            g = a[:, k] * d
            g[k] = 0.0
            row = a[k].copy()
            a -= np.outer(g, row)
            a[:, k] = -g
            a[k] = row * d
            a[k, k] = d
    for k in range(n - 1, -1, -1):
        if piv[k] != k:
            a[:, [k, piv[k]]] = a[:, [piv[k], k]]
    return a


def _sweep(F: np.ndarray, ni: int, kb: int, invert) -> None:
    """Blocked Gauss-Jordan of the first ``ni`` pivot columns of the square ``F`` in place, ``kb`` at a time, in the order of
    fc_fe_pivot / fc_fe_panels / fc_fe_update: W = F[K, K]^-1 (``invert(block, step)``), the column panel saved, the pivot rows
    multiplied by W (their pivot columns become W), every other row updated with its pivot columns taken as zero."""
    with np.errstate(all="ignore"):
        for step, k0 in enumerate(range(0, ni, kb)):
            K = slice(k0, min(k0 + kb, ni))
            W = invert(F[K, K], step)
            Cs = F[:, K].copy()
            R = W @ F[K, :]
            R[:, K] = W
            F[:, K] = 0.0
            F -= Cs @ R
            F[K, :] = R


def model_elimination(A: sp.csr_matrix, tree: NDTree, kb: int, exchange: bool = True) -> tuple[BlockFactors, list[dict]]:
    """Numpy model of the device factorisation of ``A`` (original numbering) on ``tree`` with block steps of ``kb`` = 32, 64 or
    128 pivot columns: the swept fronts in the BlockFactors value layout, and the log of every mandatory exchange
    (|diagonal| < 2**-10 |largest candidate|: the truncation of the search key to 20 mantissa bits cannot flip it) as dicts
    level (plan level, deepest first), front (plan node), step, k, p (positions inside the kb-block), kbk (columns of that
    block step), ni, nf.  kb = 128 models fc_fe_pivot_huge: the 128-block is itself swept in sub-steps of 32 columns and the
    search stays inside the 32-sub-block.  ``exchange=False``: the same elimination with the diagonal always kept."""
    if kb not in (32, 64, 128):
        raise ValueError("kb must be 32, 64 or 128")
    fac = ndsolver.factorize_blocks(None, tree)
    A = sp.csr_matrix(A, copy=True)
    A.eliminate_zeros()
    A.sort_indices()
    plan = ndsolver.factor_plan(fac, A.indptr.astype(np.int64), A.indices.astype(np.int64))
    F = np.zeros(plan.front_size)
    np.add.at(F, plan.a_dst, np.asarray(A.data, dtype=np.float64)[plan.a_src])
    vals = np.zeros(fac.vals.size)
    nodes = plan.nodes
    log: list[dict] = []
    for li in range(plan.level_ptr.size - 1):
        g0, g1 = int(plan.level_ptr[li]), int(plan.level_ptr[li + 1])
        if li > 0:  # extend-add of the level below, children in slot order (as nd_numeric.factorize_with_plan)
            c0, c1 = int(plan.level_ptr[li - 1]), int(plan.level_ptr[li])
            for s in range(plan.max_slots):
                for gc in range(c0, c1):
                    if plan.ext_off[gc] < 0 or nodes[gc, 6] != s:
                        continue
                    _, fo, nf, ni, _, par, _ = nodes[gc]
                    S = F[fo : fo + nf * nf].reshape(nf, nf)[ni:, ni:]
                    pp = plan.ext_p[plan.ext_off[gc] : plan.ext_off[gc] + nf - ni]
                    pfo, pnf = nodes[par, 1], nodes[par, 2]
                    F[pfo : pfo + pnf * pnf].reshape(pnf, pnf)[np.ix_(pp, pp)] += S
        for g in range(g0, g1):
            _, fo, nf, ni, vo, _, _ = (int(v) for v in nodes[g])
            if ni == 0:
                continue
            Fm = F[fo : fo + nf * nf].reshape(nf, nf)

            def invert(blk, step, g=g, ni=ni, nf=nf):
                kbk = blk.shape[0]

                def note(c0):
                    def on_swap(k, p, mandatory):
                        if mandatory:
                            log.append(dict(level=li, front=g, step=step, k=c0 + k, p=c0 + p, kbk=kbk, ni=ni, nf=nf))
                    return on_swap

                if kb < 128:
                    return _gj_inverse(blk, exchange, note(0))
                a = np.array(blk)
                _sweep(a, kbk, 32, lambda sub, s: _gj_inverse(sub, exchange, note(32 * s)))
                return a

            _sweep(Fm, ni, kb, invert)
            nb = nf - ni
            vals[vo : vo + ni * nf] = np.hstack([Fm[:ni, :ni], -Fm[:ni, ni:]]).ravel()
            if nb:
                vals[vo + ni * nf : vo + ni * nf + nb * ni] = Fm[ni:, :ni].ravel()
    fac.vals = vals
    return fac, log


# ──────────────────────────────────────────────────────────────────────────────────────────
def level_fronts(tree: NDTree) -> list[list[tuple[int, int]]]:
    """(ni, nf) of the fronts with a pivot block, per plan level (deepest tree level first)."""
    out = []
    for k in range(tree.depth, -1, -1):
        ptr = tree.node_ptr[k]
        out.append([(int(ptr[n + 1] - ptr[n]), int(ptr[n + 1] - ptr[n]) + int(tree.bnd[k][n].size)) for n in range(tree.nnodes(k)) if ptr[n + 1] > ptr[n]])
    return out


def predicted_step_widths(tree: NDTree, route: str) -> np.ndarray:
    """Block-step width per plan level that csrc/fc_hip.hip::eliminate_fronts must choose under the knobs ROUTES[route]: 128
    exactly on the levels whose largest front has order >= 256 under "huge", 64 on the levels whose largest front has order
    >= 64 under "wide", 32 otherwise; 0 for a level without fronts."""
    out = []
    for fronts in level_fronts(tree):
        nfmax = max((nf for _, nf in fronts), default=0)
        if not fronts:
            out.append(0)
        elif route == "huge" and nfmax >= HUGE_MIN_NF:
            out.append(128)
        elif route == "wide" and nfmax >= 64:
            out.append(64)
        else:
            out.append(32)
    return np.array(out, dtype=np.int32)


def census(log: list[dict], tree: NDTree, kb: int) -> set[str]:
    """The classes of tests/test_front_cases_host.py that a model log (block steps of ``kb``) and the tree reach ON THE DEVICE:
    only the levels that take ``kb``-column steps under the route that selects this width (32: "default", 64: "wide", 128: "huge";
    predicted_step_widths) count, both for the exchanges and for the geometry."""
    fronts = level_fronts(tree)
    runs = predicted_step_widths(tree, {32: "default", 64: "wide", 128: "huge"}[kb]) == kb
    steps = lambda ni: -(-ni // kb)  # noqa: E731
    got = set()
    for e in log:
        if not runs[e["level"]]:
            continue
        got.add("step 0" if e["step"] == 0 else "step >= 1")
        if e["kbk"] < kb:
            got.add("partial last block")
        if any(steps(ni) < steps(e["ni"]) for ni, _ in fronts[e["level"]]):
            got.add("level with shorter fronts")
        if kb == 64:
            if e["k"] >= 32 and e["p"] >= 32:
                got.add("k and p >= 32")
            if e["k"] < 16 <= e["p"]:
                got.add("k < 16 <= p")
        if kb == 128 and e["k"] >= 32:
            got.add("sub-block c0 >= 32")
    for li, lv in enumerate(fronts):
        if not runs[li]:
            continue
        for ni, nf in lv:
            if ni < kb:
                got.add("ni < KB")
            if ni % kb == 0 and ni // kb >= 2:
                got.add("ni multiple of KB, >= 2 steps")
            if nf < 64:
                got.add("nf < 64")
            if nf % 64:
                got.add("nf not a multiple of 64")
            if nf == ni:
                got.add("root front")
        if kb == 128 and max(ni for ni, _ in lv) > 256:
            got.add("huge level with ni > 256")
    return got


# ──────────────────────────────────────────────────────────────────────────────────────────
# The cases of tests/test_front_cases_host.py and tests/test_front_elimination_gpu.py: (name, nx, ny, bisections fused per tree
# level root first, depth and merge arguments of setup_solver that ask for this shape).  Fronts (ni / nf, root first):
#   square8    659 rows   77/77; 33-35/72-76; 19-40/57-59       ni < 32, nf < 64, partial last blocks everywhere
#   wide16x9  1424 rows   192/192; 73-75/167-176; 39-80/117-129  root of 6 x 32 = 3 x 64 columns, leaves of 1 / 2 / 3 steps
#   huge20x9  1768 rows   232/232; 380-387/501-503               128-column level: ni = 384 = 3 x 128 beside 380 (3 steps) and 385, 387 (4 steps)
#   huge16x16 2467 rows   157/157; 576-580/657-659               128-column level of five steps, ni = 576 = 9 x 64 = 18 x 32 beside 578 and 580
CASES = [("square8", 8, 8, (2, 2), 4, 2), ("wide16x9", 16, 9, (2, 2), 4, 2), ("huge20x9", 20, 9, (2,), 2, 2), ("huge16x16", 16, 16, (2,), 2, 2)]
SEEDS = (0, 1)


def dirichlet_dofs(th) -> np.ndarray:
    """Velocity dofs on every boundary facet except the x = xmax side (as tests/test_hip_kernels.py::_bc_setup)."""
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    return np.sort(np.r_[nodes, nodes + th.nn])


def taylor_hood_pattern(th) -> tuple[np.ndarray, np.ndarray]:
    """(rowptr, colidx) of the device's CSR pattern: every pair of dofs of a cell except pressure-pressure, columns sorted."""
    cd = th.cell_dofs.astype(np.int64)
    i, j = np.meshgrid(np.arange(15), np.arange(15), indexing="ij")
    keep = ~((i >= 12) & (j >= 12))
    P = sp.csr_matrix((np.ones(cd.shape[0] * int(keep.sum())), (cd[:, i[keep]].ravel(), cd[:, j[keep]].ravel())), shape=(th.N, th.N))
    P.sum_duplicates()
    P.sort_indices()
    return P.indptr.astype(np.int32), P.indices.astype(np.int32)


def host_case(nx: int, ny: int, bits):
    """(TaylorHood space, Dirichlet dofs, tree) of a case, all on the host."""
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    th = TaylorHood(Mesh.unit_square(nx, ny))
    dofs = dirichlet_dofs(th)
    skip = np.zeros(th.N, dtype=bool)
    skip[dofs] = True
    tree = ndsolver.build_tree(th.cell_dofs, th.mesh.cell_centroids(), th.N, sum(bits), skip, bits=list(bits))
    return th, dofs, tree
