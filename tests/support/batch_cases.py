"""Host model of the batched factor apply's tables and launch choices, and a census of the kernel branches a tree, a knob set
and a batch width reach — TEST INFRASTRUCTURE (pure numpy: nothing here imports the device package).

  model(tree, knobs)         what csrc/fc_hip.hip::build_batch_tables lays out for the node layout of ndsolver.factorize_blocks(None, tree):
                             operand lists, fold lists, and per launch (up level, fold, down level, in launch order) the tasks
                             (rows, columns, operand offset, part / parts)
  launch_cg(launch, KB, ..)  the column-group wave count batch_launch_cg chooses for a block launch
  predicted_launches(...)    what fc_get_batch_launches must report (DeviceSolver.batch_launches)
  census(tree, knobs, KB)    labels of the branches of fc_nd_block_b / fc_nd_fold_b / build_batch_tables that run (LABELS)

The knobs are the environment variables the library reads once per process: FC_BATCH_CG, FC_BATCH_CPW, FC_BATCH_SPLIT, FC_BATCH_XCD,
FC_NT_BYTES (a dict of strings, as they would sit in os.environ).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests.support import ndsolver
from tests.support.ndsolver import NDTree

KBS = (4, 8, 16, 32)
NT_BYTES = 268435456.0  # FC_NT_BYTES of csrc/fc_hip.hip: factors beyond this are streamed with nontemporal loads
LAUNCH_COLS = ("kind", "count", "cg", "min", "max", "split", "parts", "nontemporal")  # DeviceSolver.BATCH_LAUNCH_COLS

# The branches, from the kernels' text (csrc/fc_batch.hip.h) and build_batch_tables:
LABELS = (
    # fc_nd_block_b: chunks of a wave (nw = 0: the wave only takes part in the LDS sum; 1, 2: the unpipelined forms at KB <= 16)
    "nw0", "nw1", "nw2", "nw_gt2",
    # ... nw rounded up to the pipeline's period (3 at KB <= 16, where only nw > 2 runs the pipeline; 2 at KB = 32): the extra chunks read
    # chunk 0 of the tile against the null group olist[0..8)
    "overrun1", "overrun2", "overrun1_kb32",
    "short_tile",  # nrows < 16: rows past the tile's last one are zeros in the tiled copy and are not stored
    "odd_cols", "cols_not_32",  # fc_b_repack's column guards (v.y of the last pair; zero columns up to the chunk's end)
    "up_list_separate",  # ooff_up: the -L block's operand list is a second copy of the node's own rows that ends with padding
    "node_without_boundary",  # nb == 0: no up tasks, no scratch rows, [D^-1] alone in the down-sweep
    "cg1", "cg2", "cg4", "cg8", "cg16",  # cg == 1 skips the LDS sum
    "split", "parts_gt4", "parts_not_multiple_of_4", "split_kb32",  # the last arriver's read-back loop takes four parts per round
    "split_cg1", "split_cg_gt1",  # a part's partial comes from one wave, or from wave 0 after the LDS sum of cg waves
    "fold_empty_row", "fold_gt4", "fold_not_multiple_of_4",  # fc_nd_fold_b takes four sources per round
    "nontemporal",  # fc_nd_block_b<KB, true>
    "xcd_order", "node_major_order",  # the two task orders of a launch (FC_BATCH_XCD)
)


@dataclass
class Task:
    node: int  # row of the node table
    nrows: int
    ncols: int  # columns of this task (a part: of its run of chunks)
    ld: int  # columns of the whole block
    op: int  # offset of the task's operand rows in olist
    dst: int  # first destination buffer row
    part: int = 0
    parts: int = 1
    chunk0: int = 0  # first chunk of the tile this task covers

    @property
    def nchunk(self) -> int:
        return (self.ncols + 31) // 32


@dataclass
class Launch:
    kind: int  # 0 block, 1 fold
    level: int
    up: bool = False
    tasks: list = field(default_factory=list)
    row0: int = 0
    nrows: int = 0
    sources: np.ndarray | None = None  # fold: source rows per destination row

    @property
    def any_split(self) -> bool:
        return any(t.parts > 1 for t in self.tasks)

    @property
    def mean_chunks(self) -> float:
        # (the same operations in the same order as build_batch_tables: products of integers summed in double)
        tcols = trows = 0.0
        for t in self.tasks:
            tcols += float(t.nrows) * t.ncols
            trows += float(t.nrows)
        return tcols / max(trows, 1.0) / 32.0


@dataclass
class Model:
    N: int
    nodes: np.ndarray  # (G, 7): level, n, i0, ni, nb, voff, ioff
    soff: np.ndarray  # first scratch row of every node
    zero_row: int
    olist: np.ndarray
    ooff: np.ndarray
    ooff_up: np.ndarray
    fptr: np.ndarray
    fsrc: np.ndarray
    launches: list
    pslots: int
    factor_values: int


def _int_knob(knobs: dict, name: str, default: int) -> int:
    return int(knobs[name]) if name in knobs else default


def split_chunks(knobs: dict) -> int:
    return max(0, _int_knob(knobs, "FC_BATCH_SPLIT", 16))


def part_ranges(nchunk: int, split: int) -> list[tuple[int, int]]:
    """Chunk ranges of the parts a tile of ``nchunk`` 32-column chunks is cut into under FC_BATCH_SPLIT = ``split`` (one range: not split)."""
    parts = min(255, (nchunk + split // 2) // split) if split > 0 and 2 * nchunk >= 3 * split else 1
    if parts <= 1:
        return [(0, nchunk)]
    return [(nchunk * q // parts, nchunk * (q + 1) // parts) for q in range(parts)]


def model(tree: NDTree, knobs: dict | None = None) -> Model:
    knobs = knobs or {}
    fac = ndsolver.factorize_blocks(None, tree)
    nodes, idx = fac.nodes, fac.idx.astype(np.int64)
    N, G = fac.N, nodes.shape[0]
    nb_all = nodes[:, 4]
    soff = np.concatenate([[0], np.cumsum(nb_all)[:-1]]).astype(np.int64)
    S = int(nb_all.sum())
    # fold lists: destination row -> scratch rows, nodes in table order
    dest = [idx[int(io) : int(io) + int(nb)] - N for _, _, _, _, nb, _, io in nodes]
    src = [2 * N + int(soff[g]) + np.arange(int(nodes[g, 4])) for g in range(G)]
    dest_all = np.concatenate(dest) if dest else np.zeros(0, np.int64)
    src_all = np.concatenate(src) if src else np.zeros(0, np.int64)
    order = np.argsort(dest_all, kind="stable")
    fptr = np.concatenate([[0], np.cumsum(np.bincount(dest_all, minlength=N))]).astype(np.int64)
    fsrc = src_all[order]
    # operand lists
    zero_row = 2 * N + S
    olist = [np.full(32, zero_row, dtype=np.int64)]
    pos = 32
    ooff, ooff_up = np.zeros(G, np.int64), np.zeros(G, np.int64)

    def push(a):
        nonlocal pos
        olist.append(np.asarray(a, dtype=np.int64))
        pos += len(a)

    for g, (_, _, i0, ni, nb, _, io) in enumerate(nodes):
        own = np.arange(int(i0), int(i0 + ni))
        ooff[g] = pos
        push(own)
        push(idx[int(io) : int(io) + int(nb)] if nb else [])
        push([zero_row] * (-pos % 32))
        ooff_up[g] = ooff[g]
        if nb > 0 and ni & 31:
            ooff_up[g] = pos
            push(own)
            push([zero_row] * (-pos % 32))
    split = split_chunks(knobs)
    launches: list[Launch] = []
    pslots = 0
    values = 0

    def emit(level: int, up: bool):
        nonlocal pslots, values
        sel = [g for g in range(G) if nodes[g, 0] == level and nodes[g, 3] > 0 and (not up or nodes[g, 4] > 0)]
        if not sel:
            return
        L = Launch(0, level, up)
        for g in sel:
            _, _, i0, ni, nb, _, _ = (int(v) for v in nodes[g])
            rows, ld = (nb, ni) if up else (ni, ni + nb)
            for r0 in range(0, rows, 16):
                whole = Task(g, min(16, rows - r0), ld, ld, int(ooff_up[g] if up else ooff[g]), (2 * N + int(soff[g]) + r0) if up else (N + i0 + r0))
                rng = part_ranges(whole.nchunk, split)
                for q, (c0, c1) in enumerate(rng):
                    L.tasks.append(Task(g, whole.nrows, min(ld, 32 * c1) - 32 * c0, ld, whole.op + 32 * c0, whole.dst, q, len(rng), c0))
                if len(rng) > 1:
                    pslots += len(rng)
            values += rows * ld
        launches.append(L)

    for k in range(tree.depth, 0, -1):
        emit(k, True)
        r0, r1 = int(tree.node_ptr[k - 1][0]), int(tree.node_ptr[k - 1][-1])
        if r1 > r0:
            launches.append(Launch(1, k - 1, row0=r0, nrows=r1 - r0, sources=np.diff(fptr[r0 : r1 + 1])))
    for k in range(0, tree.depth + 1):
        emit(k, False)
    return Model(N, nodes, soff, zero_row, np.concatenate(olist), ooff, ooff_up, fptr, fsrc, launches, pslots, values)


def launch_cg(L: Launch, KB: int, knobs: dict | None = None) -> int:
    """batch_launch_cg: the forced count, or the smallest power of two <= 16 that leaves a wave at most `want` chunks of the launch's mean
    tile — 1.5 (3 at KB = 32; FC_BATCH_CPW), launches with split tiles 3 (4 at KB = 32)."""
    knobs = knobs or {}
    force = _int_knob(knobs, "FC_BATCH_CG", 0)
    if force in (1, 2, 4, 8, 16):
        return force
    cpw = max(0.5, float(knobs["FC_BATCH_CPW"])) if "FC_BATCH_CPW" in knobs else (3.0 if KB > 16 else 1.5)
    want = (4.0 if KB > 16 else 3.0) if L.any_split else cpw
    mean, cg = L.mean_chunks, 1
    while cg < 16 and mean / cg > want:
        cg *= 2
    return cg


def nontemporal(m: Model, knobs: dict | None = None) -> bool:
    knobs = knobs or {}
    total = int(sum(ni * (ni + nb) + nb * ni for _, _, _, ni, nb, _, _ in m.nodes))
    return 8.0 * total > (float(knobs["FC_NT_BYTES"]) if "FC_NT_BYTES" in knobs else NT_BYTES)


def predicted_launches(m: Model, KB: int, knobs: dict | None = None) -> np.ndarray:
    """The rows fc_get_batch_launches must report (LAUNCH_COLS)."""
    nt = int(nontemporal(m, knobs))
    out = []
    for L in m.launches:
        if L.kind == 0:
            ch = [t.nchunk for t in L.tasks]
            out.append([0, len(L.tasks), launch_cg(L, KB, knobs), min(ch), max(ch), int(L.any_split), max(t.parts for t in L.tasks), nt])
        else:
            out.append([1, L.nrows, 0, int(L.sources.min()), int(L.sources.max()), 0, 0, 0])
    return np.array(out, dtype=np.int32).reshape(-1, len(LAUNCH_COLS))


def census(tree: NDTree, knobs: dict | None, KB: int, m: Model | None = None) -> set[str]:
    """Labels (LABELS) of the branches the batched apply takes on ``tree`` under ``knobs`` at batch width ``KB``."""
    knobs = knobs or {}
    m = m or model(tree, knobs)
    got = set()
    for L in m.launches:
        if L.kind == 1:
            s = L.sources
            if np.any(s == 0):
                got.add("fold_empty_row")
            if np.any(s > 4):
                got.add("fold_gt4")
            if np.any(s % 4 != 0):
                got.add("fold_not_multiple_of_4")
            continue
        cg = launch_cg(L, KB, knobs)
        got.add(f"cg{cg}")
        for t in L.tasks:
            for grp in range(cg):
                nw = (t.nchunk - grp + cg - 1) // cg if t.nchunk > grp else 0
                got.add(("nw0", "nw1", "nw2")[nw] if nw <= 2 else "nw_gt2")
                if KB <= 16 and nw > 2 and nw % 3:
                    got.add(f"overrun{3 - nw % 3}")
                if KB > 16 and nw % 2:
                    got.add("overrun1_kb32")
            if t.nrows < 16:
                got.add("short_tile")
            if t.ld & 1:
                got.add("odd_cols")
            if t.ld & 31:
                got.add("cols_not_32")
            if t.parts > 1:
                got.add("split")
                got.add("split_cg1" if cg == 1 else "split_cg_gt1")
                if KB > 16:
                    got.add("split_kb32")
                if t.parts > 4:
                    got.add("parts_gt4")
                if t.parts % 4:
                    got.add("parts_not_multiple_of_4")
    for g in range(m.nodes.shape[0]):
        if m.nodes[g, 4] == 0:
            got.add("node_without_boundary")
        if m.ooff_up[g] != m.ooff[g]:
            got.add("up_list_separate")
    if nontemporal(m, knobs):
        got.add("nontemporal")
    got.add("node_major_order" if knobs.get("FC_BATCH_XCD", "1")[:1] == "0" else "xcd_order")
    assert got <= set(LABELS)
    return got


# The cases: the four small meshes of front_cases.CASES (name, nx, ny, bisections fused per tree level, depth and merge arguments of
# setup_solver) and one more, because none of the four has a fold row without sources: an 8 x 6 mesh cut down to leaves of one or two
# cells (505 rows, three levels below the root) has leaves whose dofs ALL sit in separators -- such a leaf has no rows, hence no node
# in the table, and 10 of the rows of level 2 are in the boundary of such leaves only.  (Cut finer still, e.g. 6 x 6 by the same tree,
# a leaf is left with pressure rows alone and its pivot block is singular.)
def cases() -> list[tuple]:
    from tests.support import front_cases

    return list(front_cases.CASES) + [("deep8x6", 8, 6, (2, 2, 2), 6, 2)]


# The knob sets of tests/test_batch_apply_gpu.py (one child process each), and the label each is there for that no other set reaches
# (tests/test_batch_cases_host.py asserts it):
#   default           cg8: wide tiles, unsplit, with the wave count the rule chooses (KB = 32 on the 8- to 21-chunk tiles)
#   cg1_nosplit       overrun1: one wave walks all of a tile's chunks (nw up to 21, every remainder of the pipeline period)
#   cg16_node_major   node_major_order (FC_BATCH_XCD=0); waves 12 .. 15 of a 12-chunk tile have nw = 0
#   cg4_split2        split_cg_gt1: parts of two or three chunks on four waves (nw = 0 and 1 inside a part)
#   split2_nt         nontemporal; split launches at the wave count the rule chooses for them (split_cg1)
KNOB_SETS = {
    "default": {},
    "cg1_nosplit": {"FC_BATCH_CG": "1", "FC_BATCH_SPLIT": "0"},
    "cg16_node_major": {"FC_BATCH_CG": "16", "FC_BATCH_XCD": "0"},
    "cg4_split2": {"FC_BATCH_CG": "4", "FC_BATCH_SPLIT": "2"},
    "split2_nt": {"FC_BATCH_SPLIT": "2", "FC_NT_BYTES": "0"},
}


# ──────────────────────────────────────────────────────────────────────────────────────────
# The operators and the reference of tests/test_batch_apply_gpu.py
OPERATORS = {"bdf1": 200.0, "bdf2": 300.0}  # slot -> mass coefficient (1 / dt and 1.5 / dt at dt = 0.005); nu = 0.01, smooth advection
NU = 0.01
N_RHS = 32
KS = (1, 4, 5, 8, 9, 16, 17, 32)  # both edges of every batch width


def smooth_advection(th) -> np.ndarray:
    """The advecting / linearisation field of tests/test_front_elimination_gpu.py."""
    x = th.node_coords
    return np.r_[1.0 + 0.3 * np.sin(x[:, 0]) * np.cos(0.7 * x[:, 1]), 0.2 * np.cos(0.5 * x[:, 0] + 0.1) * np.sin(x[:, 1])]


def host_operator(th, dofs, mass: float):
    """The operator the device assembles for (mass, NU, smooth advection) with Dirichlet rows and columns eliminated, formed by the numpy
    oracle: what the host constant of the GPU test was measured on."""
    from oracle import ns_oracle as O

    U0 = smooth_advection(th)
    A = O.assemble_matrix(O.Disc.from_taylor_hood(th), mass=mass, nu=NU, adv=U0, lin=U0)
    return O.apply_bc_symmetric(A, None, np.asarray(dofs, dtype=np.int64), np.zeros(len(dofs)))[0]


def rhs_pool(N: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((N_RHS, N))


def residual_longdouble(A, X: np.ndarray, B: np.ndarray) -> np.ndarray:
    """B - A X for the columns X[j], B[j] ([m][N]) with products and sums in np.longdouble."""
    A = A.tocsr()
    prod = A.data.astype(np.longdouble)[:, None] * X.T.astype(np.longdouble)[A.indices]
    assert np.all(np.diff(A.indptr) > 0)
    return (B.T.astype(np.longdouble) - np.add.reduceat(prod, A.indptr[:-1], axis=0)).T


def refined_solve(A, B: np.ndarray, sweeps: int = 2) -> np.ndarray:
    """A^-1 B[j] for every row of B: LAPACK LU in fp64, then ``sweeps`` refinements with the residual formed in np.longdouble and the
    iterate kept in np.longdouble; rounded to fp64 at the end."""
    import scipy.linalg as sla

    lu = sla.lu_factor(A.toarray())
    X = sla.lu_solve(lu, B.T).T.astype(np.longdouble)
    for _ in range(sweeps):
        R = residual_longdouble(A, X, B)
        X = X + sla.lu_solve(lu, R.T.astype(np.float64)).T
    return np.asarray(X, dtype=np.float64)


def cond1_estimate(A) -> float:
    """1-norm condition number of A: |A|_1 times Higham's estimate of |A^-1|_1 through a sparse LU."""
    import scipy.sparse.linalg as spla

    lu = spla.splu(A.tocsc())
    inv = spla.LinearOperator(A.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T"))
    return float(abs(A).sum(axis=0).max() * spla.onenormest(inv))


def batch_rhs(pool: np.ndarray, ref: np.ndarray, k: int):
    """k right-hand sides and their reference solutions from the pool: different columns; for k >= 4 the last one exactly zero and the one
    before it 2^40 times column 0.  Returns (B, Xref, zero column or None, (scaled column, its twin) or None)."""
    B, X = pool[:k].copy(), ref[:k].copy()
    if k < 4:
        return B, X, None, None
    B[k - 1], X[k - 1] = 0.0, 0.0
    B[k - 2], X[k - 2] = 2.0**40 * pool[0], 2.0**40 * ref[0]
    return B, X, k - 1, (k - 2, 0)
