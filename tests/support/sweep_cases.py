"""Host model of the single-vector factor apply's launch choices, and a census of the kernel instances and branches a tree, a knob
set and a storage width reach — TEST INFRASTRUCTURE (pure numpy: nothing here imports the device package).

  model(tree, knobs, bits)      what csrc/fc_hip.hip lays out for the node layout of ndsolver.factorize_blocks(None, tree): the stage
                                geometries of fc_solver_setup, the tiles of down_blocks / retile_flat / fc_solver_set_blocks, the levels
                                of build_up_column, the nontemporal / resident split
  predicted_launches(m)         what fc_get_sweep_launches must report (DeviceSolver.sweep_launches), in launch order
  census(m)                     labels of the template instances and kernel branches that run (LABELS)
  apply_longdouble(fac, v, B)   the stage-by-stage apply with products and sums in np.longdouble: the reference of the GPU test

The knobs are environment variables of the library (a dict of strings, as they would sit in os.environ).  HANDLE_KNOBS are read when a
handle is created or lays out its tables and may change inside one process; PROCESS_KNOBS are read once per process.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests.support import ndsolver
from tests.support.ndsolver import NDTree

LAUNCH_COLS = ("kernel", "direction", "p1", "p2", "workgroups", "nontemporal", "bits", "rows")  # DeviceSolver.SWEEP_LAUNCH_COLS
K_SWEEP, K_BLOCK, K_FLAT, K_FOLD, K_DIAG = range(5)

HANDLE_KNOBS = ("FC_SWEEP_GEOM", "FC_DOWN_DEPTH", "FC_BLOCK_KERNEL", "FC_BLOCK_TARGET", "FC_BLOCK_MIN", "FC_FLAT_ROW", "FC_FLAT_TILE", "FC_UP_FORM")
PROCESS_KNOBS = ("FC_NT_BYTES", "FC_RESIDENT_BYTES", "FC_WG_SORT", "FC_UP_THREADS", "FC_UPC_LPR_SHIFT", "FC_UPC_RC", "FC_UPC_TARGET", "FC_BLK_SORT")

# constants of csrc/fc_hip.hip and csrc/fc_kernels.hip.h
NT_BYTES = 268435456.0
UP_THREADS = 1048576.0
DOWN_DEPTH = 2.0
BLK_TILE = 2048  # FC_BLK_TILE: operand values of fc_nd_down_block held in LDS at a time
FLAT_CAP, FLAT_WD = 4096, 512  # FC_FLAT_CAP, FC_FLAT_WD

SWEEP_KEYS = ((8, 4), (8, 8), (16, 4), (16, 8), (16, 16), (32, 4), (32, 8), (32, 16), (32, 32), (64, 4), (64, 8), (64, 16), (64, 32), (64, 64),
              (256, 16), (256, 32), (256, 64), (256, 256))
BLOCK_DOWN_KEYS = ((16, 1), (16, 2), (32, 1), (32, 2), (32, 4), (64, 1), (64, 2), (64, 4), (64, 8))
BLOCK_UPC_KEYS = ((8, 1), (8, 2), (16, 1), (16, 2), (16, 4), (32, 1), (32, 2), (32, 4), (64, 1), (64, 2), (64, 4), (64, 8))
FLAT_LOADS = (4, 8, 12, 16)
LP_SWEEP = {16: 4, 64: 16, 256: 64}  # compressed storage: LANES -> SUB
LP_BLOCK = {16: 2, 32: 4, 64: 8}  # ... LPR -> RPS

INSTANCE_LABELS = (
    tuple(f"sweep_{l}_{s}_nt{nt}" for l, s in SWEEP_KEYS for nt in (0, 1))
    + tuple(f"sweep_lanes{l}_{d}" for l in (8, 16, 32, 64, 256) for d in ("up", "down"))
    + tuple(f"block_down_{l}_{r}" for l, r in BLOCK_DOWN_KEYS)
    + tuple(f"block_upc_{l}_{r}" for l, r in BLOCK_UPC_KEYS)
    + tuple(f"flat_{f}_{u}" for f in ("down", "upc") for u in FLAT_LOADS)
    + ("block_down_nt", "block_upc_nt", "flat_down_nt", "flat_upc_nt")
    + tuple(f"sweep_{vt}_{l}" for vt in ("f32", "bf16") for l in LP_SWEEP)
    + tuple(f"block_{vt}_{l}" for vt in ("f32", "bf16") for l in LP_BLOCK)
)
# The branches, from the kernels' text (csrc/fc_kernels.hip.h):
BRANCH_LABELS = (
    # fc_nd_sweep: a row with more segments than the shuffle width SW = min(LANES, 64) takes another round of descriptor loads
    "desc_rounds_sw8", "desc_rounds_sw16", "desc_rounds_sw32", "desc_rounds_sw64",
    "idle_subgroup",  # the last round of G = LANES / SUB segments has fewer than G: `if (sidx >= cnt) len = 0`
    "segment_trips_gt1",  # len > 4 * SUB: the 4-deep issue loop runs again
    "segment_indexed", "segment_contiguous",
    "empty_row",  # q0 == q1 for a row < nrows
    "partial_workgroup",  # nrows is no multiple of 256 / LANES: rows beyond nrows take part in the shuffles
    "wg_order_on", "wg_order_off",
    # fc_nd_down_block
    "block_single_trip", "block_loop",  # wd <= 4 * LPR: the values loaded before the operand gather are the whole row; else the loop
    "block_multi_tile",  # wd > FC_BLK_TILE: the operand goes through LDS in more than one tile
    "block_no_index_part",  # nb == 0 (the root; every block of the column form)
    "block_short",  # nrows < RPS * SLOTS: row slots without a row
    # fc_nd_flat_block
    "flat_partial_256",  # nrows * wd is no multiple of 256: the clamped loads of the last round
    "flat_rows_gt32",  # a second round of the 32 row groups
    "flat_wd_mod16_1to8",  # the `j + 8 < wd` guard fails for some lane
    "flat_wd_gt256",  # the operand gather loops
    # fc_nd_fold1: eight sources per round
    "fold_empty_row", "fold_gt8", "fold_not_multiple_of_8",
    "mixed_resident_nt",  # one apply with nontemporal and cached launches
)
LABELS = INSTANCE_LABELS + BRANCH_LABELS


def _f(knobs: dict, name: str, default: float) -> float:
    return float(knobs[name]) if name in knobs else default


def _i(knobs: dict, name: str, default: int) -> int:
    return int(knobs[name]) if name in knobs else default


def _pow2_ceil(v: float) -> int:
    p = 1
    while p < v:
        p <<= 1
    return p


def _pow2_floor(v: float) -> int:
    p = 1
    while 2 * p <= v:
        p <<= 1
    return p


def _nblocks(n: int, per: int) -> int:
    return (n + per - 1) // per


def block_target(N: int) -> int:
    t = 1024
    while t < 8192 and N / 128.0 > 1.4142 * t:
        t *= 2
    return t


def flat_loads(knobs: dict, max_row: int, max_tile: int) -> int:
    flat_row = _i(knobs, "FC_FLAT_ROW", 256)
    if flat_row <= 0 or max_row > flat_row or max_row > FLAT_WD or max_tile > FLAT_CAP or max_tile <= 0:
        return 0
    return 4 * ((max_tile + 1023) // 1024)


def flat_tile_values(knobs: dict) -> int:
    return min(FLAT_CAP, max(256, _i(knobs, "FC_FLAT_TILE", 2048))) if "FC_FLAT_TILE" in knobs else 2048


def sweep_geom(stages: list[tuple[int, int]]) -> str:
    """FC_SWEEP_GEOM for (lanes, sub) per stage in stage order ((0, 0): keep what the rule chooses)."""
    return ",".join(f"{l}:{s}" for l, s in stages)


@dataclass
class Blk:
    val: int
    row0: int
    nrows: int
    i0: int
    ni: int
    idx: int
    nb: int

    @property
    def wd(self) -> int:
        return self.ni + self.nb


@dataclass
class Stage:
    kind: int
    row0: int
    nrows: int
    seg_count: np.ndarray  # segments of every row
    seg_len: np.ndarray  # lengths, rows one after the other
    seg_indexed: np.ndarray
    lanes: int = 0
    sub: int = 0
    bytes: float = 0.0
    nt: bool = False
    wg_order: bool = False
    blk: list = field(default_factory=list)  # tiles after retile_flat
    blk_lpr: int = 64
    blk_rps: int = 1
    blk_flat: int = 0


@dataclass
class UpLevel:
    blk: list
    lpr: int
    rps: int
    flat: int
    rows: int
    fold_row0: int
    fold_nrows: int
    sources: np.ndarray  # fold: scratch rows per destination row


@dataclass
class Model:
    N: int
    bits: int
    n_val: int
    nt: bool  # OrderSys::nt
    stages: list
    up_column: bool  # a whole apply runs its up-sweep in column form
    levels: list  # UpLevel, deepest first (built whether or not the apply takes them)
    down_tables: tuple  # ndsolver.down_blocks for the knobs' target / minimum, before retile_flat


def _stage_geometry(st: Stage, s: int, knobs: dict) -> None:
    nseg, nz = int(st.seg_count.sum()), int(st.seg_len.sum())
    mean_seg = nz / nseg if nseg else 0.0
    mean_row = nz / st.nrows if st.nrows else 0.0
    segs_per_row = nseg / st.nrows if st.nrows else 0.0
    few_long_rows = st.nrows < 4096 and mean_row >= 1024
    if st.kind == 0:
        sub = min(64, max(4, _pow2_ceil(mean_seg / 4.0)))
        grp_fill = max(1, _pow2_floor(_f(knobs, "FC_UP_THREADS", UP_THREADS) / max(1.0, float(st.nrows) * sub)))
        grp = min(grp_fill, min(16, max(1, _pow2_floor(segs_per_row))))
        lanes = sub * grp
        if lanes > 64:
            if few_long_rows:
                lanes, sub = 256, max(sub, 16)
            else:
                lanes = 64
    else:
        dd = max(1.0, _f(knobs, "FC_DOWN_DEPTH", DOWN_DEPTH)) if "FC_DOWN_DEPTH" in knobs else DOWN_DEPTH
        lanes = 256 if few_long_rows else min(64, max(8, _pow2_ceil(mean_seg / dd)))
        sub = lanes
    lanes = max(lanes, 8)
    sub = min(sub, lanes)
    geom = knobs.get("FC_SWEEP_GEOM")
    if geom:
        ent = geom.split(",")
        if s < len(ent):
            l, _, sb = ent[s].partition(":")
            if int(l or 0) > 0 and int(sb or 0) > 0:
                lanes, sub = int(l), int(sb)
    st.lanes, st.sub = lanes, sub
    st.bytes = 8.0 * nz + 16.0 * nseg + 4.0 * float(st.seg_len[st.seg_indexed].sum()) + st.nrows * (8.0 + 8.0 + (8.0 if st.kind == 0 else 0.0))
    st.wg_order = knobs.get("FC_WG_SORT", "1")[:1] != "0" and st.nrows > 0


def _retile_flat(blks: list, knobs: dict) -> list:
    if not blks:
        return []
    flat = flat_loads(knobs, max(b.wd for b in blks), 1) > 0
    out = []
    for b in blks:
        parts = 1
        if flat and b.nrows * b.wd > flat_tile_values(knobs):
            fit = max(1, flat_tile_values(knobs) // b.wd)
            parts = (b.nrows + fit - 1) // fit
        rc = (b.nrows + parts - 1) // parts
        for r0 in range(0, b.nrows, rc):
            out.append(Blk(b.val + r0 * b.wd, b.row0 + r0, min(rc, b.nrows - r0), b.i0, b.ni, b.idx, b.nb))
    return out


def _up_levels(tree: NDTree, fac, knobs: dict) -> list:
    """build_up_column: per level, deepest first, the tiles of the nodes' -L blocks and the fold of the level above."""
    nodes, N = fac.nodes, fac.N
    idx = fac.idx.astype(np.int64)
    G = nodes.shape[0]
    soff = np.concatenate([[0], np.cumsum(nodes[:, 4])[:-1]]).astype(np.int64) if G else np.zeros(0, np.int64)
    dest = np.concatenate([idx[int(io) : int(io) + int(nb)] - N for _, _, _, _, nb, _, io in nodes]) if G else np.zeros(0, np.int64)
    fcount = np.bincount(dest, minlength=N)
    lpr_shift, rc_max = _i(knobs, "FC_UPC_LPR_SHIFT", 0), (max(8, _i(knobs, "FC_UPC_RC", 32)) if "FC_UPC_RC" in knobs else 32)
    upc_env = max(1, _i(knobs, "FC_UPC_TARGET", 0)) if "FC_UPC_TARGET" in knobs else 0
    levels = []
    for k in range(tree.depth, 0, -1):
        sel = [g for g in range(G) if nodes[g, 0] == k and nodes[g, 3] > 0 and nodes[g, 4] > 0]
        L = UpLevel([], 16, 1, 0, 0, 0, 0, np.zeros(0, np.int64))
        if sel:
            values = float(sum(float(nodes[g, 3]) * float(nodes[g, 4]) for g in sel))
            rows = int(sum(nodes[g, 4] for g in sel))
            wd = values / max(rows, 1)
            lpr = 8 if wd <= 32 else (16 if wd <= 64 else (32 if wd <= 128 else 64))
            for _ in range(max(0, lpr_shift)):
                lpr = min(64, lpr * 2)
            for _ in range(max(0, -lpr_shift)):
                lpr = max(8, lpr // 2)
            slots = 256 // lpr
            rc = rc_max
            target = upc_env if upc_env else max(2048, block_target(N) // 2)
            while rc > slots and rows // rc < target:
                rc //= 2
            rc = max(rc, 1)
            max_ni = max(int(nodes[g, 3]) for g in sel)
            flat = flat_loads(knobs, max_ni, 1) > 0
            for g in sel:
                _, _, i0, ni, nb, voff, _ = (int(v) for v in nodes[g])
                assert ni <= BLK_TILE * 64, "build_up_column: node too large"
                if flat:
                    fit = max(1, flat_tile_values(knobs) // ni)
                    parts = (nb + fit - 1) // fit
                    rc = (nb + parts - 1) // parts
                for r0 in range(0, nb, rc):
                    L.blk.append(Blk(voff + ni * (ni + nb) + r0 * ni, int(soff[g]) + r0, min(rc, nb - r0), i0, ni, 0, 0))
            L.blk.sort(key=lambda b: -(b.nrows * b.ni))  # (stable, as std::stable_sort)
            maxr = max(b.nrows for b in L.blk)
            rps = 1
            while rps * slots < maxr:
                rps *= 2
            L.lpr, L.rps, L.rows = lpr, rps, rows
            L.flat = flat_loads(knobs, max_ni, max(b.nrows * b.ni for b in L.blk)) if flat else 0
        r0, r1 = int(tree.node_ptr[k - 1][0]), int(tree.node_ptr[k - 1][-1])
        L.fold_row0, L.fold_nrows, L.sources = r0, r1 - r0, fcount[r0:r1]
        levels.append(L)
    return levels


def model(tree: NDTree, knobs: dict | None = None, bits: int = 64, fac=None) -> Model:
    """``fac``: ndsolver.factorize_blocks(None, tree), if the caller has it already."""
    knobs = knobs or {}
    fac = fac or ndsolver.factorize_blocks(None, tree)
    N = fac.N
    n_val = max(1, int(fac.vals.size))
    stages = []
    for s in range(len(fac.stage_kind)):
        r0, nr = int(fac.stage_begin[s]), int(fac.stage_nrows[s])
        q0, q1 = int(fac.seg_ptr[r0]), int(fac.seg_ptr[r0 + nr])
        st = Stage(int(fac.stage_kind[s]), int(fac.stage_row0[s]), nr, np.diff(fac.seg_ptr[r0 : r0 + nr + 1]).astype(np.int64),
                   fac.seg_len[q0:q1].astype(np.int64), fac.seg_col[q0:q1] < 0)
        _stage_geometry(st, s, knobs)
        stages.append(st)
    nt = 8.0 * n_val > _f(knobs, "FC_NT_BYTES", NT_BYTES)
    resident, kept = _f(knobs, "FC_RESIDENT_BYTES", 0.0), 0.0
    for st in stages:
        st.nt = nt
        if nt and kept + st.bytes <= resident:
            st.nt = False
            kept += st.bytes
    # the tiles of the down stages: down_blocks, retile_flat, fc_solver_set_blocks
    target = max(1, _i(knobs, "FC_BLOCK_TARGET", 0)) if "FC_BLOCK_TARGET" in knobs else block_target(N)
    minimum = max(1, _i(knobs, "FC_BLOCK_MIN", 0)) if "FC_BLOCK_MIN" in knobs else 512
    tables = ndsolver.down_blocks(fac, 0, 1, 32, target, minimum)
    begin, count, lpr = tables[0], tables[1].copy(), tables[2]
    if knobs.get("FC_BLOCK_KERNEL", "1")[:1] == "0":
        count[:] = 0
    for s, st in enumerate(stages):
        raw = [Blk(*(int(a[q]) for a in tables[3:])) for q in range(int(begin[s]), int(begin[s]) + int(count[s]))]
        st.blk = _retile_flat(raw, knobs)
        if knobs.get("FC_BLK_SORT", "1")[:1] != "0":
            st.blk.sort(key=lambda b: -(b.nrows * b.wd))
        st.blk_lpr = int(lpr[s])
        slots = 256 // max(16, st.blk_lpr)
        st.blk_rps = 1
        while st.blk and st.blk_rps * slots < max(b.nrows for b in st.blk):
            st.blk_rps *= 2
        st.blk_flat = flat_loads(knobs, max(b.wd for b in st.blk), max(b.nrows * b.wd for b in st.blk)) if st.blk and bits == 64 else 0
    form = {"row": 1, "column": 2}.get(knobs.get("FC_UP_FORM", "auto"), 0)
    levels = _up_levels(tree, fac, knobs)
    upc = (form == 2 or (form == 0 and nt)) and bits == 64 and any(L.blk for L in levels)
    return Model(N, bits, n_val, nt, stages, upc, levels, tables)


def _pick_stage(m: Model, st: Stage) -> list:
    d = 0 if st.kind == 0 else 1
    if m.bits != 64:
        if st.kind == 1 and st.blk:
            lpr = 16 if st.blk_lpr <= 16 else (32 if st.blk_lpr <= 32 else 64)
            return [K_BLOCK, 1, lpr, lpr // 8, len(st.blk), 0, m.bits, st.nrows]
        lanes = 16 if st.lanes <= 16 else (64 if st.lanes <= 64 else 256)
        return [K_SWEEP, d, lanes, lanes // 4, _nblocks(st.nrows, 256 // lanes), 0, m.bits, st.nrows]
    if st.kind == 1 and st.blk and st.blk_flat > 0:
        return [K_FLAT, 1, st.blk_flat, 0, len(st.blk), int(st.nt), 64, st.nrows]
    if st.kind == 1 and st.blk:
        return [K_BLOCK, 1, st.blk_lpr, st.blk_rps, len(st.blk), int(st.nt), 64, st.nrows]
    return [K_SWEEP, d, st.lanes, st.sub, _nblocks(st.nrows, 256 // st.lanes), int(st.nt), 64, st.nrows]


def predicted_launches(m: Model) -> np.ndarray:
    """The rows fc_get_sweep_launches must report (LAUNCH_COLS).  Raises for a geometry without a template instance: the launcher
    would reject it."""
    out = []
    if m.up_column:
        for L in m.levels:
            if L.blk:
                out.append([K_FLAT, 0, L.flat, 0, len(L.blk), int(m.nt), 64, L.rows] if L.flat > 0 else [K_BLOCK, 0, L.lpr, L.rps, len(L.blk), int(m.nt), 64, L.rows])
            if L.fold_nrows > 0:
                out.append([K_FOLD, 0, 0, 0, _nblocks(L.fold_nrows, 256), 0, 64, L.fold_nrows])
    for st in m.stages:
        if st.nrows > 0 and not (m.up_column and st.kind == 0):
            out.append(_pick_stage(m, st))
    for kernel, d, p1, p2, *_ in out:
        if kernel == K_SWEEP:
            assert (p1, p2) in SWEEP_KEYS, f"no fc_nd_sweep<{p1}, {p2}>"
        if kernel == K_BLOCK:
            assert (p1, p2) in (BLOCK_DOWN_KEYS if d else BLOCK_UPC_KEYS), f"no fc_nd_down_block<{p1}, {p2}> in the {'down' if d else 'column'} form"
        if kernel == K_FLAT:
            assert p1 in FLAT_LOADS
    return np.array(out, dtype=np.int32).reshape(-1, len(LAUNCH_COLS))


def _census_blocks(got: set, blks: list, lpr: int, rps: int) -> None:
    slots = 256 // lpr
    for b in blks:
        got.add("block_single_trip" if b.wd <= 4 * lpr else "block_loop")
        if b.wd > BLK_TILE:
            got.add("block_multi_tile")
        if b.nb == 0:
            got.add("block_no_index_part")
        if b.nrows < rps * slots:
            got.add("block_short")


def _census_flat(got: set, blks: list) -> None:
    for b in blks:
        if (b.nrows * b.wd) % 256:
            got.add("flat_partial_256")
        if b.nrows > 32:
            got.add("flat_rows_gt32")
        if 1 <= b.wd % 16 <= 8:
            got.add("flat_wd_mod16_1to8")
        if b.wd > 256:
            got.add("flat_wd_gt256")


def census(m: Model) -> set[str]:
    """Labels (LABELS) of the instances and branches one whole apply of the model runs."""
    got = set()
    rows = predicted_launches(m)
    vt = {32: "f32", 16: "bf16"}.get(m.bits)
    for kernel, d, p1, p2, _, nt, _, _ in rows.tolist():
        form = "down" if d else "upc"
        if kernel == K_SWEEP:
            got.add(f"sweep_{vt}_{p1}" if vt else f"sweep_{p1}_{p2}_nt{nt}")
            if not vt:
                got.add(f"sweep_lanes{p1}_{'down' if d else 'up'}")
        elif kernel == K_BLOCK:
            got.add(f"block_{vt}_{p1}" if vt else f"block_{form}_{p1}_{p2}")
            if nt:
                got.add(f"block_{form}_nt")
        elif kernel == K_FLAT:
            got.add(f"flat_{form}_{p1}")
            if nt:
                got.add(f"flat_{form}_nt")
    reading = rows[rows[:, 0] <= K_FLAT]
    if reading.size and reading[:, 5].min() != reading[:, 5].max():
        got.add("mixed_resident_nt")
    if m.up_column:
        for L in m.levels:
            if L.blk and L.flat > 0:
                _census_flat(got, L.blk)
            elif L.blk:
                _census_blocks(got, L.blk, L.lpr, L.rps)
            if L.fold_nrows > 0:
                s = L.sources
                if np.any(s == 0):
                    got.add("fold_empty_row")
                if np.any(s > 8):
                    got.add("fold_gt8")
                if np.any(s % 8 != 0):
                    got.add("fold_not_multiple_of_8")
    for st in m.stages:
        if st.nrows == 0 or (m.up_column and st.kind == 0):
            continue
        kernel, _, p1, p2 = _pick_stage(m, st)[:4]
        if kernel == K_FLAT:
            _census_flat(got, st.blk)
        elif kernel == K_BLOCK:
            _census_blocks(got, st.blk, p1, p2)
        elif kernel == K_SWEEP:
            lanes, sub = p1, p2
            sw, G = min(lanes, 64), lanes // sub
            if np.any(st.seg_count > sw):
                got.add(f"desc_rounds_sw{sw}")
            if np.any(st.seg_count == 0):
                got.add("empty_row")
            last = st.seg_count[st.seg_count > 0] % sw  # segments of the last descriptor round (0: a full one)
            if G > 1 and np.any(np.where(last == 0, sw, last) % G != 0):
                got.add("idle_subgroup")
            if np.any(st.seg_len > 4 * sub):
                got.add("segment_trips_gt1")
            if np.any(st.seg_indexed & (st.seg_len > 0)):
                got.add("segment_indexed")
            if np.any(~st.seg_indexed & (st.seg_len > 0)):
                got.add("segment_contiguous")
            if st.nrows % (256 // lanes):
                got.add("partial_workgroup")
            if m.bits == 64:  # (the compressed launches pass no workgroup order)
                got.add("wg_order_on" if st.wg_order else "wg_order_off")
            else:
                got.add("wg_order_off")
    assert got <= set(LABELS), got - set(LABELS)
    return got


# ──────────────────────────────────────────────────────────────────────────────────────────
# The reference of tests/test_sweep_apply_gpu.py


def round_values(vals: np.ndarray, bits: int) -> np.ndarray:
    """fp64 values as a storage width holds them (fc_pack: round to nearest even), widened back to fp64."""
    if bits == 64:
        return np.asarray(vals, dtype=np.float64)
    f = np.asarray(vals, dtype=np.float32)
    if bits == 32:
        return f.astype(np.float64)
    b = f.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def apply_longdouble(fac, vals: np.ndarray, B: np.ndarray) -> np.ndarray:
    """The factor apply of nd_numeric.block_solve for the rows of B ([m][N]) on the factor values ``vals`` (the layout of ``fac``), stage by
    stage, every product and sum in np.longdouble; rounded to fp64 at the end."""
    t, N = fac.tree, fac.N
    v = np.asarray(vals, dtype=np.longdouble)
    m = B.shape[0]
    buf = np.zeros((2 * N, m), dtype=np.longdouble)
    buf[:N] = B[:, t.perm].T
    for s in range(len(fac.stage_kind)):
        r0, nr, d0 = int(fac.stage_begin[s]), int(fac.stage_nrows[s]), int(fac.stage_row0[s])
        acc = np.zeros((nr, m), dtype=np.longdouble)
        # rows that share a segment shape are taken together: all rows of a node have the same columns
        r = 0
        while r < nr:
            qs = range(int(fac.seg_ptr[r0 + r]), int(fac.seg_ptr[r0 + r + 1]))
            shape = [(int(fac.seg_col[q]), int(fac.seg_len[q])) for q in qs]
            e = r + 1
            while e < nr and [(int(fac.seg_col[q]), int(fac.seg_len[q])) for q in range(int(fac.seg_ptr[r0 + e]), int(fac.seg_ptr[r0 + e + 1]))] == shape:
                e += 1
            for j, (c, n) in enumerate(shape):
                if n == 0:
                    continue
                cols = np.arange(c, c + n) if c >= 0 else fac.idx[-(c + 1) : -(c + 1) + n].astype(np.int64)
                offs = np.array([int(fac.seg_val[int(fac.seg_ptr[r0 + i]) + j]) for i in range(r, e)], dtype=np.int64)
                M = v[offs[:, None] + np.arange(n)[None, :]]
                acc[r:e] += M @ buf[cols]
            r = e
        if fac.stage_kind[s] == 0:
            buf[d0 : d0 + nr] += acc
        else:
            buf[N + d0 : N + d0 + nr] = acc
    X = np.empty((m, N))
    X[:, t.perm] = np.asarray(buf[N:], dtype=np.float64).T
    return X


# ──────────────────────────────────────────────────────────────────────────────────────────
# The cases, the knob sets and the runs of tests/test_sweep_apply_gpu.py
#
# The cases of batch_cases and three more, found by a search over front_cases.host_case with N <= 6000 (name, nx, ny, bisections fused
# per tree level, depth and merge arguments of setup_solver):
#   bin8x6        the 8 x 6 mesh of deep8x6 under a BINARY tree of six levels (505 rows): a row of the root separator sits in the boundary
#                 of up to 20 nodes -- the smallest case found with more than 16 segments in an up row (a second descriptor round at
#                 shuffle width 16)
#   bin32x16      32 x 16 cells under nine binary levels (4851 rows): up rows of 34 segments, a second descriptor round at shuffle width
#                 32.  The smallest solvable one found: 8 x 8 ... 28 x 16 cells under seven to nine binary levels, and a tenth level on
#                 this mesh or on 24 x 24 cells, leave a leaf with pressure rows alone (singular pivot block); 16 x 16 cells under eight
#                 levels is solvable and stops at 30 segments, 24 x 24 under nine (5427 rows) reaches 34 as well.  35 (24 x 24, ten levels,
#                 singular) is the most seen at all
#   twoleaf22x20  two leaves under the root (4173 rows): rows of 2138 values, the smallest such mesh whose leaf rows exceed FC_BLK_TILE
def cases() -> list[tuple]:
    from tests.support import batch_cases

    return batch_cases.cases() + [("bin8x6", 8, 6, (1,) * 6, 6, 1), ("twoleaf22x20", 22, 20, (1,), 1, 1), ("bin32x16", 32, 16, (1,) * 9, 9, 1)]


N_RHS = 8  # right-hand sides of the pool (batch_cases.rhs_pool) every handle solves for; rhs_set adds two


def rhs_set(tree: NDTree, pool: np.ndarray, dofs=()) -> np.ndarray:
    """The right-hand sides of one operator: N_RHS rows of the pool, then one supported on a single leaf row and one on a single root
    row (the first of each that is no Dirichlet row)."""
    is_bc = np.zeros(pool.shape[1], dtype=bool)
    is_bc[np.asarray(dofs, dtype=np.int64)] = True
    B = np.zeros((N_RHS + 2, pool.shape[1]))
    B[:N_RHS] = pool[:N_RHS]
    for j, k in ((N_RHS, tree.depth), (N_RHS + 1, 0)):
        rows = tree.perm[int(tree.node_ptr[k][0]) : int(tree.node_ptr[k][-1])]
        B[j, rows[~is_bc[rows]][0]] = 1.0
    return B


# Labels no case within N <= 6000 reaches:
UNREACHED = (
    ("desc_rounds_sw64", "needs an up row of more than 64 segments: the most found is 35 (24 x 24 cells, ten binary levels)"),
)

# Knobs read once per process: one child process each.  What each is there for that no other set reaches
# (tests/test_sweep_cases_host.py asserts it):
#   default         the compressed-storage instances (fp32 and bf16 sweeps and blocks); the column-form block <64, 1> (the rule's rows per
#                   tile); the multi-tile block row of twoleaf22x20; the second descriptor round at shuffle width 32 of bin32x16
#   nt_upc32        FC_UPC_TARGET=1 keeps the column-form tiles at 32 rows: block_upc <16, 2>, <32, 4>, <64, 8>; everything nontemporal
#   resident_upc16  a resident budget that splits an apply into cached and nontemporal launches (mixed_resident_nt); column-form tiles of 16
#                   rows: block_upc <32, 2>, <64, 4>
#   wgoff_upc8      column-form tiles of 8 rows: block_upc <64, 2>; FC_WG_SORT=0 (launch order = row order) and a small FC_UP_THREADS
#   upc64           column-form tiles of 64 rows: block_upc <8, 2>, <16, 4> (only handles whose levels stay at 16 lanes per row or below:
#                   <32, 8> and <64, 16> do not exist)
KNOB_SETS = {
    "default": {},
    "nt_upc32": {"FC_NT_BYTES": "0", "FC_UPC_TARGET": "1"},
    "resident_upc16": {"FC_NT_BYTES": "0", "FC_RESIDENT_BYTES": "150000", "FC_UPC_RC": "16", "FC_UPC_TARGET": "1"},
    "wgoff_upc8": {"FC_WG_SORT": "0", "FC_UP_THREADS": "4096", "FC_UPC_RC": "8", "FC_UPC_TARGET": "1"},
    "upc64": {"FC_UPC_RC": "64", "FC_UPC_TARGET": "1"},
}


def _blk(target: int) -> dict:  # the row-lane block kernel on every level, down form and column form
    return {"FC_BLOCK_MIN": "1", "FC_FLAT_ROW": "0", "FC_BLOCK_TARGET": str(target), "FC_UP_FORM": "column"}


def _flat(row: int, tile: int) -> dict:  # the flat kernel on every level whose rows fit `row`, tiles of `tile` values
    return {"FC_BLOCK_MIN": "1", "FC_BLOCK_TARGET": "1", "FC_FLAT_ROW": str(row), "FC_FLAT_TILE": str(tile), "FC_UP_FORM": "column"}


# Knobs read per handle.  ("geom", r): the segment kernel on every stage in row form, stage s with the geometry SWEEP_KEYS[(s + r) % 18].
HANDLE_SETS = {
    "default": {},
    "segment": {"FC_BLOCK_KERNEL": "0"},
    "segment_dd1": {"FC_BLOCK_KERNEL": "0", "FC_DOWN_DEPTH": "1", "FC_UP_FORM": "row"},
    "column": {"FC_UP_FORM": "column"},
    "geom0": ("geom", 0), "geom2": ("geom", 2), "geom6": ("geom", 6), "geom15": ("geom", 15),
    "blk_t1": _blk(1), "blk_t4": _blk(4), "blk_t8": _blk(8), "blk_t32": _blk(32),
    "flat_256_2048": _flat(256, 2048), "flat_512_3072": _flat(512, 3072), "flat_512_4096": _flat(512, 4096),
}


def handle_knobs(name: str, n_stages: int) -> dict:
    hk = HANDLE_SETS[name]
    if isinstance(hk, tuple):
        return {"FC_SWEEP_GEOM": sweep_geom([SWEEP_KEYS[(s + hk[1]) % len(SWEEP_KEYS)] for s in range(n_stages)]), "FC_BLOCK_KERNEL": "0", "FC_UP_FORM": "row"}
    return dict(hk)


# (handle set, storage bits, case) per child, in the order they run
RUNS = {
    "default": [("default", 64, c) for c in ("square8", "wide16x9", "huge20x9", "huge16x16", "deep8x6", "bin8x6", "twoleaf22x20")] + [
        ("segment_dd1", 64, "square8"), ("blk_t8", 64, "wide16x9"), ("flat_512_4096", 64, "wide16x9"), ("flat_512_3072", 64, "huge20x9"),
        ("column", 64, "huge20x9"),
        ("blk_t1", 32, "square8"), ("blk_t1", 16, "square8"), ("blk_t1", 32, "wide16x9"), ("blk_t1", 16, "wide16x9"),
        ("geom2", 32, "bin8x6"), ("geom2", 16, "bin8x6"), ("default", 32, "deep8x6"), ("default", 16, "huge16x16"),
        ("geom15", 64, "bin32x16")],
    "nt_upc32": [("default", 64, "square8"), ("geom0", 64, "bin8x6"), ("blk_t4", 64, "deep8x6"), ("flat_256_2048", 64, "deep8x6"),
                 ("blk_t32", 64, "wide16x9"), ("segment", 64, "huge20x9")],
    "resident_upc16": [("default", 64, "wide16x9"), ("geom15", 64, "bin8x6"), ("geom6", 64, "bin8x6"), ("blk_t1", 64, "wide16x9"),
                       ("segment", 64, "huge20x9")],
    "wgoff_upc8": [("default", 64, "deep8x6"), ("geom2", 64, "bin8x6"), ("column", 64, "huge20x9"), ("segment", 64, "huge16x16")],
    "upc64": [("default", 64, "square8"), ("blk_t8", 64, "square8"), ("column", 64, "deep8x6")],
}
