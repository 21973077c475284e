"""Cases, knob sets, runs and the route model of ONE BATCHED time step: the forward batched step of csrc/fc_batch.hip.h --
fc_rhs_elem_breg<KB, FORCE>, fc_rhs_elem_b<KB>, fc_rhs_gather_b, fc_rhs_ctrl_b, fc_tail_b (row blocks and fc_energy_b_block), fc_final_b,
fc_early_b, fc_wait_solved_b, fc_final_late_b, fc_b_interleave, fc_b_zero_column -- and the dispatch around them (batch_enqueue,
batch_launches, batch_launches_side, build_tail_blocks, build_ctrl_rows of csrc/fc_hip.hip).  No GPU import:
tests/test_batch_step_cases_host.py runs everything here on the host, tests/test_batch_step_routes_gpu.py and
tests/support/batch_step_child.py run it against the device.  The host model of the step itself (np.longdouble right-hand side, sensors,
energy, residual and their bounds) is step_cases.HostModel.

  MESHES / star_mesh / host_case    the three structured meshes of step_cases and a star that reaches what no structured mesh does
  WIDTHS / PAIRS / geometry         batch widths, the (mesh, k) pairs in use and the launch geometry each pair meets
  KNOB_SETS / HANDLE_SETS           knobs read once per process (a child process each) / when a handle is created (a fresh handle each)
  predicted_tail_blocks             host model of build_tail_blocks: block count, which cut ended each block
  predicted_route / History         host model of the dispatch conditions: what fc_get_batch_step_route must report
  scenario / RUNS / walk            the operations of a run, as data: the child executes them, walk() only predicts their routes
  census / LABELS / UNREACHED       the branches a set of runs reaches"""
from __future__ import annotations

from collections import Counter

import numpy as np

from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from tests.support import front_cases as fcs
from tests.support import step_cases as sc

cdiv = sc.cdiv

# ── meshes ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
MESHES = ("5x3", "9x9", "12x11", "star")
STAR_VALENCE, STAR_RINGS = 10, 4


def star_mesh(valence: int = STAR_VALENCE, rings: int = STAR_RINGS):
    """A centre vertex of ``valence`` cells and ``rings`` rings of ``valence`` vertices, every second ring turned by half a sector:
    valence (2 rings - 1) cells.  The centre's velocity rows collect ``valence`` element contributions and couple to every dof of the
    fan: 2 (1 + 3 valence) velocities + (1 + valence) pressures = 73 entries at valence 10.  The even rings are the turned ones, so the
    outermost ring has a facet on x = xmax: front_cases.dirichlet_dofs leaves its midpoint free and the flow is not enclosed."""
    from flowcontrol_amd.fem.mesh import Mesh

    pts = [(0.5, 0.5)]
    for r in range(1, rings + 1):
        for i in range(valence):
            a = 2 * np.pi * (i + 0.5 * ((r + 1) % 2)) / valence
            pts.append((0.5 + 0.45 * r / rings * np.cos(a), 0.5 + 0.45 * r / rings * np.sin(a)))
    v = lambda r, i: 1 + (r - 1) * valence + i % valence  # noqa: E731
    cells = [(0, v(1, i), v(1, i + 1)) for i in range(valence)]
    for r in range(1, rings):
        for i in range(valence):
            a, b, c, d = v(r, i), v(r, i + 1), v(r + 1, i), v(r + 1, i + 1)
            cells += [(a, c, b), (b, c, d)] if r % 2 == 1 else [(a, c, d), (a, d, b)]
    return Mesh.from_arrays(np.array(pts), np.array(cells))  # (orients every cell counter-clockwise)


def host_case(mesh: str):
    """(TaylorHood space, Dirichlet dofs, their two profiles) of a mesh; cached, and handed to step_cases' cache so that
    step_cases.HostModel finds the star (the trick of adjoint_march_cases.host_case)."""
    if mesh == "star" and mesh not in sc._host:
        from flowcontrol_amd.fem.spaces import TaylorHood

        th = TaylorHood(star_mesh())
        dofs = fcs.dirichlet_dofs(th)
        x = th.node_coords[dofs % th.nn]
        isx = dofs < th.nn
        prof = np.stack([np.where(isx, np.sin(x[:, 0] + 2 * x[:, 1]), 0.0), np.where(isx, 0.0, np.cos(3 * x[:, 0] - x[:, 1]))], axis=1)
        sc._host[mesh] = (th, dofs, prof)
        return sc._host[mesh]
    return sc.host_case(mesh)


def pattern(th):
    """(rowptr, colidx) of the device's CSR pattern."""
    return fcs.taylor_hood_pattern(th)


def contributions(th) -> np.ndarray:
    """Element contributions the gather collects per velocity row (W numbering)."""
    return np.bincount(th.cell_dofs[:, :12].ravel(), minlength=th.N)


# ── widths ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
WIDTHS = (3, 4, 5, 12, 20, 32)  # KB 4 with and without a padded column, 8, 16, 32 twice


def batch_width(k: int) -> int:
    return 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32


# the (mesh, k) pairs of the runs, chosen (not the full product) so that every KB meets
#   element loop (256 / KB cells per workgroup)   a ragged single workgroup where one holds 30 cells (KB 4, 8) and several workgroups with
#                                                 a ragged last one (all four KB)
#   energy blocks (4 x 256 / KB cells, 4 trips)   a ragged single workgroup (30 cells: all four KB) and a second workgroup with empty
#                                                 trips (KB 4: 264 = 256 + 8 cells, three empty trips; KB 8: 162 = 128 + 34; KB 16: 162 =
#                                                 2 x 64 + 34; KB 32: 70 = 2 x 32 + 6)
#   gather (256 / (KB / 2) rows per workgroup)    several workgroups with a ragged last one (all four KB)
# and the star runs at KB 4 and KB 32.  geometry() computes all of it; tests/test_batch_step_cases_host.py asserts it.
PAIRS = (("5x3", 3), ("5x3", 4), ("12x11", 3), ("star", 4), ("5x3", 5), ("9x9", 5), ("5x3", 12), ("9x9", 12), ("5x3", 20), ("star", 32))


def geometry(mesh: str, k: int) -> dict:
    th = host_case(mesh)[0]
    KB = batch_width(k)
    return dict(KB=KB, nc=th.nc, N=th.N, elem_cpb=256 // KB, g_elem=cdiv(th.nc, 256 // KB), elem_lds_cpb=256 // (8 * (KB // 2)),
                g_elem_lds=cdiv(th.nc, 256 // (8 * (KB // 2))), energy_cpb=4 * (256 // KB), g_energy=cdiv(th.nc, 4 * (256 // KB)),
                g_gather=cdiv(th.N * (KB // 2), 256), NT=cdiv(16 * KB, 256), JL=16 // (KB // 2), padded=KB - k)


# ── knobs ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
PROCESS_KNOBS = ("FC_SPECULATE", "FC_SPECULATE_GATHER", "FC_LATE_GATE", "FC_BATCH_ELEM", "FC_BATCH_GRAPH", "FC_TB_COLS")
HANDLE_KNOBS = ("FC_OVERLAP_TAIL",)
KNOB_SETS = {
    "default": {},
    "no_speculate": {"FC_SPECULATE": "0"},
    "no_gather_ahead": {"FC_SPECULATE_GATHER": "0"},
    "no_late_gate": {"FC_LATE_GATE": "0"},
    "elem_lds": {"FC_BATCH_ELEM": "lds"},
    "graph": {"FC_BATCH_GRAPH": "1"},
    "tb64": {"FC_TB_COLS": "64"},
    "tb128": {"FC_TB_COLS": "128"},
}
HANDLE_SETS = {"overlapped": {}, "one_stream": {"FC_OVERLAP_TAIL": "0"}}
# children whose right-hand sides, solutions and records must agree bit for bit, step by step and column by column: the sources state
# the same operations in the same order (fc_rhs_ctrl_b after the gather ahead against the full gather; the same kernels behind another
# gate or replayed from a graph)
BITWISE_PAIRS = (("default", "no_gather_ahead"), ("default", "no_speculate"), ("default", "no_late_gate"), ("default", "graph"))
ELEM_PAIR = ("default", "elem_lds")  # promised by the comment above fc_rhs_elem_breg: asserted if it holds, the count reported otherwise

SENSOR_SETS = ("none", "limit64", "long150", "single_entry")  # of step_cases.sensor_rows

# ── the tail's row blocks ─────────────────────────────────────────────────────────────────────────────────────────────────────────────
TB_ROWS, TB_COLS_DEFAULT, TB_NNZ = 16, 128, 768  # FC_TB_ROWS, FC_TB_COLS, FC_TB_NNZ of csrc/fc_batch.hip.h
REFUSAL = "a matrix row has more entries than a row block holds"


def tb_cols(KB: int, knobs: dict) -> int:
    """fc_ctx::Batch::tb_cols as build_tail_blocks chooses it (the meshes here are far below factors that stream from HBM)."""
    if "FC_TB_COLS" in knobs:
        v = int(knobs["FC_TB_COLS"])
    else:
        v = (144 if KB > 16 else 256) if knobs.get("FC_OVERLAP_TAIL", "1")[0] != "0" else TB_COLS_DEFAULT
    return min(384 * 16 // max(16, KB), max(TB_ROWS, v))


_blocks = {}


def predicted_tail_blocks(th, cols: int) -> dict:
    """build_tail_blocks on the host: the rows in cell order (a node's two velocity rows next to each other, then the cell's pressures),
    cut into blocks of at most 16 rows, ``cols`` distinct columns and FC_TB_NNZ entries.  Returns the block count, how each block ended
    (Counter over "rows16", "cols", "nnz", "short_last"), the most distinct columns and entries of a block; raises ValueError with the
    library's message when a single row does not fit.  (Distinct columns are counted in the W numbering: a permutation keeps them.)"""
    key = (id(th), cols)
    if key in _blocks:
        return _blocks[key]
    rp, ci = pattern(th)
    seen, order = np.zeros(th.N, dtype=bool), []
    for cell in th.cell_dofs:
        for w in [d for a in range(6) for d in (cell[a], cell[6 + a])] + list(cell[12:15]):
            if not seen[w]:
                seen[w] = True
                order.append(int(w))
    order += [w for w in range(th.N) if not seen[w]]
    cuts, n_blocks, max_cols, max_nnz, q0 = Counter(), 0, 0, 0, 0
    while q0 < th.N:
        cur, q, nnz, why = set(), q0, 0, "rows16"
        while q < th.N and q - q0 < TB_ROWS:
            row = ci[rp[order[q]]:rp[order[q] + 1]]
            if q > q0 and nnz + len(row) > TB_NNZ:
                why = "nnz"
                break
            new = cur | set(row.tolist())
            if len(new) > cols and q > q0:
                why = "cols"
                break
            cur, nnz, q = new, nnz + len(row), q + 1
        if len(cur) > cols or nnz > TB_NNZ:
            raise ValueError(REFUSAL)
        if q == th.N and q - q0 < TB_ROWS and why == "rows16":
            why = "short_last"
        cuts[why] += 1
        n_blocks, max_cols, max_nnz, q0 = n_blocks + 1, max(max_cols, len(cur)), max(max_nnz, nnz), q
    _blocks[key] = dict(n=n_blocks, cuts=cuts, max_cols=max_cols, max_nnz=max_nnz)
    return _blocks[key]


# ── route model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
ROUTE_COLS = ("lead", "elem", "spec", "spec_gather", "overlapped", "late_gate", "monitored", "n_row_blocks", "n_cell_blocks", "tb_cols", "KB",
              "n_ctrl_rows", "graph")  # DeviceSolver.BATCH_ROUTE_COLS
ELEM_NONE, ELEM_LDS, ELEM_BREG, ELEM_BREG_FORCE = 0, 1, 2, 3


class History:
    """What the dispatch of the next batched step depends on beyond its own arguments (fc_ctx::Batch)."""

    def __init__(self):
        self.pre_slot, self.pre_gather, self.pre_overlapped = -1, False, False
        self.cur = 0  # ring phase: the right-hand side of an overlapped step lives in quarter cur % 4 of the store, a one-stream step's in quarter 0
        self.step_count = 0
        self.ctrl_ok = {SLOT_BDF1: False, SLOT_BDF2: False}
        self.have_c = {SLOT_BDF1: False, SLOT_BDF2: False}
        self.have_force = False

    def invalidate(self):
        self.pre_slot = -1


def _off(knobs: dict, name: str) -> bool:
    return knobs.get(name, "1")[0] == "0"


def predicted_route(mesh: str, k: int, knobs: dict, settings: dict, hist: History, n_ctrl_rows: int = 0) -> np.ndarray:
    """The vector fc_get_batch_step_route must report for a step with ``settings`` (order, energy, mode, check) on a handle of ``mesh``
    with a batch of ``k``, created under ``knobs`` (process and handle knobs together), whose past is ``hist``.  The conditions are those
    of step_batch_begin, batch_enqueue, batch_launches and batch_tail_geometry, read from csrc/fc_hip.hip.  ``n_ctrl_rows``: what
    build_ctrl_rows lists for a slot (the child counts them from the device's own operator; the host test passes 0)."""
    th = host_case(mesh)[0]
    KB = batch_width(k)
    slot = SLOT_BDF1 if settings["order"] == 1 else SLOT_BDF2
    overlapped = not _off(knobs, "FC_OVERLAP_TAIL") and settings["mode"] == "early"  # fc_step_batch asks for everything: one stream
    check = settings["check"]
    monitored = check != 0 and hist.step_count % check == 0
    spec = -1
    if not _off(knobs, "FC_SPECULATE") and not hist.have_force:
        spec = slot if hist.have_c[slot] else SLOT_BDF2  # (both slots are set up in every run)
    spec_gather = spec >= 0 and not _off(knobs, "FC_SPECULATE_GATHER") and not hist.have_c[spec]
    ctrl_ok = dict(hist.ctrl_ok)
    if spec_gather:
        ctrl_ok[spec] = True  # build_ctrl_rows, before the launches
    have_ev = hist.pre_slot == slot and not hist.have_force
    # the gathered right-hand side counts only if it sits where this step reads it
    same_place = (hist.cur % 4 if hist.pre_overlapped else 0) == (hist.cur % 4 if overlapped else 0)
    lead = 2 if not have_ev else (0 if (hist.pre_gather and ctrl_ok[slot] and same_place) else 1)
    kernel = ELEM_LDS if knobs.get("FC_BATCH_ELEM") == "lds" else (ELEM_BREG_FORCE if hist.have_force else ELEM_BREG)
    elem = kernel if (lead == 2 or spec >= 0) else ELEM_NONE
    late_gate = not _off(knobs, "FC_LATE_GATE") and overlapped and spec_gather
    cols = tb_cols(KB, knobs)
    n_rows = predicted_tail_blocks(th, cols)["n"] if monitored else 0
    n_cells = cdiv(th.nc, 4 * (256 // KB)) if settings["energy"] else 0
    graph = knobs.get("FC_BATCH_GRAPH", "0")[0] == "1"
    return np.array([lead, elem, spec + 1, int(spec_gather), int(overlapped), int(late_gate), int(monitored), n_rows, n_cells, cols, KB,
                     n_ctrl_rows if ctrl_ok[slot] else -1, int(graph)], dtype=np.int32)


def advance(hist: History, route: np.ndarray) -> None:
    """The handle after a step that took ``route``."""
    r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
    hist.pre_slot, hist.pre_gather, hist.pre_overlapped = r["spec"] - 1, bool(r["spec_gather"]), bool(r["overlapped"])
    if r["spec_gather"]:
        hist.ctrl_ok[r["spec"] - 1] = True
    hist.cur += 1
    hist.step_count += 1


# ── columns ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def ident(s: int, k: int) -> int:
    """Which scenario column s of a batch of k carries: its own, except that the LAST column of a batch of four or more repeats column
    0 -- the same scenario in two columns of one batch, and columns 0 to 2 of k = 3 and k = 4 carry the same three."""
    return 0 if (k >= 4 and s == k - 1) else s


def column_state(th, s: int, k: int, seed: int):
    """(u_n, u_nn, p_n) of column s: every scenario its own initial state."""
    return sc.initial_state(th, 1000 * seed + ident(s, k))


def controls(k: int, shift: int) -> np.ndarray:
    """(k, N_ACT): every scenario its own controls, changing from step to step with ``shift``."""
    return np.stack([sc.CONTROLS[(ident(s, k) + shift) % 4] * (1.0 + 0.125 * ident(s, k)) for s in range(k)])


def force_amplitudes(k: int, shift: int) -> np.ndarray:
    """(k, N_ACT) body-force amplitudes that differ from the controls of the same step."""
    return np.stack([-0.7 * sc.CONTROLS[(ident(s, k) + shift + 1) % 4] + 0.05 * ident(s, k) for s in range(k)])


# ── scenarios: the operations of a run, as data ──────────────────────────────────────────────────────────────────────────────────────
# ("opts", check)                          set_solver_options(refine = 0, check_residual = check)
# ("step", order, energy, mode, shift)     mode "block": fc_step_batch (one stream); "early": fc_step_batch_begin / _end_early / _collect
#                                          (overlapped unless FC_OVERLAP_TAIL=0); controls(k, shift); with force profiles set:
#                                          force_amplitudes(k, shift) as u_force
# ("set_state", seed)                      fc_set_state_batch: the speculation is dropped
# ("cop", order, on)                       fc_set_rhs_operator with the explicit operator of a Crank-Nicolson slot / without
# ("force", variant | None)                fc_set_force
# ("nonfinite", order, energy, mode, shift)   the step twice from one state: clean, then with a NaN in one velocity entry of column k // 2;
#                                          the other columns equal the clean step bit for bit, the flag is set for that column only; then
#                                          fc_reset_sim_batch on it (its state is zero from there on)
def step(order, energy=True, mode="block", shift=0):
    return ("step", order, bool(energy), mode, shift)


def scenario(name: str) -> list[tuple]:
    if name == "main":
        # BDF1, then BDF2; lead 2 -> 0 (gather ahead) -> 1 (the form switches: gathers again) -> 0 overlapped -> 1 (switch back) -> 2
        # (fc_set_state_batch); then check_residual = 3 with the energy off on some steps: no tail at all (G = 0), a cells-only grid,
        # a rows-only grid, an overlapped step off the cadence
        return [("opts", 1), step(1, True, "block", 0), step(2, True, "block", 1), step(2, False, "early", 2), step(2, True, "early", 3),
                step(2, True, "early", 0), step(2, True, "block", 1), ("set_state", 2), step(2, True, "block", 2),
                ("opts", 3), step(2, False, "block", 3), step(2, True, "block", 0), step(2, False, "block", 1), step(2, True, "early", 2),
                step(2, False, "early", 3)]
    if name == "cn":
        # an explicit operator on the BDF1 slot: the speculation goes to the same slot, nothing is gathered ahead; then the operator is
        # set on a slot whose control-independent right-hand side the previous step HAS gathered ahead without it
        return [("opts", 1), ("cop", 1, True), step(1, True, "block", 0), step(1, True, "early", 1), step(1, False, "block", 2), step(2, True, "block", 3),
                step(2, True, "block", 0), ("cop", 2, True), step(2, True, "block", 1), step(2, True, "block", 2), ("cop", 2, False), ("cop", 1, False),
                step(2, True, "block", 3), step(1, True, "block", 0)]
    if name == "force":
        # body-force profiles: the FORCE kernel, no speculation, u_force different from u_ctrl; then without them again
        return [("opts", 1), step(2, True, "block", 0), ("force", 0), step(2, True, "block", 1), step(1, True, "early", 2), step(2, False, "block", 3),
                ("force", None), step(2, True, "block", 0), step(2, True, "block", 1)]
    if name == "nonfinite":
        # the flag once on the tail's route (one stream, monitored: fc_tail_b tests the velocity rows it finishes) and once on the
        # down-sweep's (overlapped, or off the monitor's cadence: the tiles test what they write)
        return [("opts", 1), step(2, True, "block", 0), ("nonfinite", 2, True, "block", 1), step(2, True, "block", 2),
                ("set_state", 3), ("nonfinite", 2, True, "early", 3), step(2, True, "early", 0),
                ("opts", 0), ("set_state", 4), ("nonfinite", 2, False, "block", 1), step(2, True, "block", 2)]
    raise KeyError(name)


SCENARIOS = ("main", "cn", "force", "nonfinite")
# runs of a child: (scenario, mesh, k, handle knob set, sensor set)
_SHARED = [("main", "5x3", 4, "overlapped", "limit64"), ("main", "9x9", 5, "overlapped", "long150"), ("main", "5x3", 12, "one_stream", "single_entry"),
           ("main", "star", 32, "overlapped", "long150"), ("cn", "5x3", 5, "overlapped", "none")]
RUNS = {
    "default": _SHARED + [("main", "5x3", 3, "overlapped", "limit64"), ("main", "12x11", 3, "overlapped", "single_entry"), ("main", "star", 4, "one_stream", "limit64"),
                          ("main", "5x3", 5, "one_stream", "none"), ("main", "9x9", 12, "overlapped", "none"), ("main", "5x3", 20, "overlapped", "limit64"),
                          ("force", "5x3", 4, "overlapped", "single_entry"), ("force", "star", 32, "one_stream", "none"),
                          ("nonfinite", "5x3", 5, "overlapped", "single_entry"), ("nonfinite", "star", 32, "one_stream", "long150")],
    "no_speculate": _SHARED,
    "no_gather_ahead": _SHARED,
    "no_late_gate": _SHARED,
    "graph": _SHARED + [("nonfinite", "5x3", 5, "overlapped", "single_entry")],
    "elem_lds": _SHARED + [("main", "5x3", 20, "overlapped", "limit64"), ("force", "5x3", 4, "overlapped", "single_entry"), ("force", "star", 32, "one_stream", "none")],
    "tb64": [("main", "5x3", 4, "overlapped", "limit64"), ("main", "9x9", 5, "overlapped", "long150"), ("main", "12x11", 3, "one_stream", "single_entry"),
             ("main", "5x3", 20, "overlapped", "none")],
    "tb128": [("main", "9x9", 5, "overlapped", "long150"), ("main", "9x9", 12, "one_stream", "none")],
}
# runs the default child repeats WITHOUT the capture: right-hand side copies off, records bit for bit those of the captured run
UNCAPTURED = [("main", "5x3", 4, "overlapped", "limit64"), ("main", "5x3", 12, "one_stream", "single_entry")]
# fc_set_batch must refuse with REFUSAL: (knob set, mesh, k)
REFUSED = [("tb64", "star", 4), ("tb64", "star", 32)]


def run_name(run: tuple) -> str:
    return "/".join(str(v) for v in run)


def apply_op(hist: History, op: tuple) -> None:
    """What an operation other than a step does to the History."""
    kind = op[0]
    if kind == "set_state":  # fc_set_state_batch: element vectors of the old state
        hist.invalidate()
    elif kind == "reset":  # fc_reset_sim_batch
        hist.invalidate()
    elif kind == "force":  # fc_set_force: with profiles the element loop depends on the amplitudes, nothing left behind is used
        hist.have_force = op[1] is not None
    elif kind == "cop":  # fc_set_rhs_operator: the element vectors do not depend on C, a right-hand side gathered ahead does
        hist.have_c[SLOT_BDF1 if op[1] == 1 else SLOT_BDF2] = bool(op[2])
        hist.pre_gather = False
    elif kind != "opts":
        raise KeyError(kind)


def walk(run: tuple, knobs: dict):
    """The steps of a run with their predicted routes, without a device: yields (index of the operation, operation, settings or None,
    route or None, flag route or None).  A "nonfinite" operation yields its two steps (clean, bad)."""
    name, mesh, k, hs, _ = run
    kn = {**knobs, **HANDLE_SETS[hs]}
    hist, check = History(), 1
    for i, op in enumerate(scenario(name)):
        if op[0] == "opts":
            check = op[1]
            yield i, op, None, None, None
        elif op[0] == "step":
            settings = dict(order=op[1], energy=op[2], mode=op[3], check=check)
            route = predicted_route(mesh, k, kn, settings, hist)
            advance(hist, route)
            yield i, op, settings, route, None
        elif op[0] == "nonfinite":
            settings = dict(order=op[1], energy=op[2], mode=op[3], check=check)
            for bad in (False, True):
                apply_op(hist, ("set_state", 0))
                route = predicted_route(mesh, k, kn, settings, hist)
                advance(hist, route)
                # overlapped, or off the cadence: the down-sweep's tiles raise the flag; else the row blocks of fc_tail_b do
                yield i, op, settings, route, (("sweep" if (route[4] or not route[6]) else "tail") if bad else None)
            apply_op(hist, ("reset",))
        else:
            apply_op(hist, op)
            yield i, op, None, None, None


# ── census ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
LABELS = (
    # element loop
    "fc_rhs_elem_breg<false>", "fc_rhs_elem_breg<true>", "fc_rhs_elem_b", "fc_rhs_elem_b:force", "elem:ragged_single_workgroup", "elem:several_workgroups_ragged",
    "elem:lds:inactive_cells", "elem:ahead", "elem:u_force!=u_ctrl",
    # gather and control rows
    "fc_rhs_gather_b:with_ctrl", "gather:ahead", "gather:second_trip_clamped", "gather:C", "gather:opens_gate", "gather:several_workgroups_ragged", "fc_rhs_ctrl_b",
    "pair:padded_column",
    # tail
    "fc_tail_b:row_blocks", "tail:row>64", "tail:NT=1", "tail:NT=2", "tail:JL>1", "tail:JL=1", "tail:short_last_block", "tail:cut:rows16", "tail:cut:cols",
    "tail:one_cut_at_128", "tail:flag", "fc_energy_b_block", "energy:ragged_single_workgroup", "energy:second_workgroup_empty_trips", "tail:G=0", "tail:cells_only",
    "tail:rows_only", "tail:cut:nnz", "tail:staging_cap",
    # final kernels
    "fc_final_b", "fc_early_b", "fc_wait_solved_b", "fc_final_late_b", "final:sensor_wave_loop", "early:sensor_wave_loop", "sensor:none", "sensor:stride_loop",
    "sensor:single_entry", "sensor:limit64", "early:opens_gate", "monitor:off_cadence",
    # layout kernels
    "fc_b_interleave:padded", "fc_b_interleave:full", "fc_b_zero_column",
    # dispatch
    "lead:2", "lead:1", "lead:0", "lead:1:form_switch", "lead:1:no_gather_ahead", "spec:bdf2", "spec:same_slot", "spec:none:force", "spec:none:knob", "spec_gather:off:knob",
    "spec_gather:off:C", "overlapped", "one_stream", "late_gate:off:knob", "graph", "plain", "flag:sweep", "ctrl_rows:not_tabulated",
)
UNREACHED = {
    "tail:cut:nnz": "build_tail_blocks' FC_TB_NNZ cut: the most entries of a 16-row block on these meshes is 522 < 768 (9x9 at 128 columns; 501 on the star); a mesh that reaches it "
                    "needs sixteen rows of 48 entries on average next to each other in cell order, i.e. a high-valence fan of its own for every block",
    "tail:staging_cap": "the column cap of fc_tail_b's 12 staging trips (192 columns at KB 32, 384 at KB 16): blocks stay at or below 138 distinct columns on these meshes",
}


def census(runs: list[tuple], knobs: dict) -> set[str]:
    """Labels the steps of ``runs`` reach under the process knobs ``knobs`` (read from the kernels' text and the dispatch)."""
    out = set()

    def add(cond, label):
        if cond:
            out.add(label)

    for run in runs:
        name, mesh, k, hs, sens = run
        kn = {**knobs, **HANDLE_SETS[hs]}
        th = host_case(mesh)[0]
        g = geometry(mesh, k)
        KB = g["KB"]
        rows = sc.sensor_rows(th, sens)
        rp, _ = pattern(th)
        long_row, many = bool((np.diff(rp) > 64).any()), bool((contributions(th) > 8).any())
        hist_c, hist_f = {1: False, 2: False}, False
        out.add("fc_b_interleave:padded" if g["padded"] else "fc_b_interleave:full")
        prev = None
        for _, op, settings, route, flag_route in walk(run, knobs):
            if op[0] == "cop":
                hist_c[op[1]] = bool(op[2])
            elif op[0] == "force":
                hist_f = op[1] is not None
            if route is None:
                continue
            r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
            out |= {f"lead:{r['lead']}", "overlapped" if r["overlapped"] else "one_stream", "graph" if r["graph"] else "plain"}
            add(g["padded"], "pair:padded_column")
            if r["elem"]:
                out.add({ELEM_LDS: "fc_rhs_elem_b", ELEM_BREG: "fc_rhs_elem_breg<false>", ELEM_BREG_FORCE: "fc_rhs_elem_breg<true>"}[r["elem"]])
                add(r["elem"] == ELEM_LDS and hist_f, "fc_rhs_elem_b:force"), add(hist_f, "elem:u_force!=u_ctrl")
                if r["elem"] == ELEM_LDS:
                    add(th.nc % g["elem_lds_cpb"], "elem:lds:inactive_cells")
                    add(g["g_elem_lds"] > 1 and th.nc % g["elem_lds_cpb"], "elem:several_workgroups_ragged")
                else:
                    add(g["g_elem"] == 1 and th.nc % g["elem_cpb"], "elem:ragged_single_workgroup")
                    add(g["g_elem"] > 1 and th.nc % g["elem_cpb"], "elem:several_workgroups_ragged")
            add(r["spec"], "elem:ahead")
            if r["lead"] >= 1:
                out.add("fc_rhs_gather_b:with_ctrl")
                add(hist_c[settings["order"]], "gather:C")
            if r["lead"] >= 1 or r["spec_gather"]:
                add(many, "gather:second_trip_clamped")
                add(g["g_gather"] > 1 and (th.N * (KB // 2)) % 256, "gather:several_workgroups_ragged")
            add(r["lead"] == 0 and r["n_ctrl_rows"] != -1, "fc_rhs_ctrl_b")
            add(r["n_ctrl_rows"] == -1, "ctrl_rows:not_tabulated")
            add(r["spec_gather"], "gather:ahead"), add(r["late_gate"], "gather:opens_gate")
            if prev is not None and r["lead"] == 1 and prev["spec_gather"]:
                out.add("lead:1:form_switch" if prev["overlapped"] != r["overlapped"] else "lead:1")
            add(r["lead"] == 1 and prev is not None and prev["spec"] and not prev["spec_gather"], "lead:1:no_gather_ahead")
            if r["spec"]:
                out.add("spec:same_slot" if hist_c[settings["order"]] else "spec:bdf2")
                if not r["spec_gather"]:
                    out.add("spec_gather:off:C" if hist_c[{SLOT_BDF1: 1, SLOT_BDF2: 2}[r["spec"] - 1]] else "spec_gather:off:knob")
            else:
                out.add("spec:none:force" if hist_f else "spec:none:knob")
            if r["overlapped"]:
                out |= {"fc_early_b", "fc_wait_solved_b", "fc_final_late_b"}
                add(not r["late_gate"], "early:opens_gate")
                add(not r["late_gate"] and r["spec_gather"], "late_gate:off:knob")
                add(len(rows) > 4, "early:sensor_wave_loop")
            else:
                out.add("fc_final_b")
                add(len(rows) > 16, "final:sensor_wave_loop")
            G = r["n_row_blocks"] + r["n_cell_blocks"]
            add(G == 0, "tail:G=0"), add(G and not r["n_row_blocks"], "tail:cells_only"), add(G and not r["n_cell_blocks"], "tail:rows_only")
            add(settings["check"] > 1 and not r["monitored"], "monitor:off_cadence")
            if r["n_row_blocks"]:
                tb = predicted_tail_blocks(th, r["tb_cols"])
                out |= {"fc_tail_b:row_blocks", f"tail:NT={g['NT']}", "tail:JL>1" if g["JL"] > 1 else "tail:JL=1"}
                add(long_row, "tail:row>64"), add(tb["cuts"]["short_last"], "tail:short_last_block"), add(tb["cuts"]["rows16"], "tail:cut:rows16")
                add(tb["cuts"]["cols"], "tail:cut:cols"), add(tb["cuts"]["nnz"], "tail:cut:nnz"), add(r["tb_cols"] == 128 and tb["cuts"]["cols"] == 1, "tail:one_cut_at_128")
                add(tb["max_cols"] > 12 * 256 // (KB // 2), "tail:staging_cap")
            if r["n_cell_blocks"]:
                out.add("fc_energy_b_block")
                add(r["n_cell_blocks"] == 1 and th.nc % g["energy_cpb"], "energy:ragged_single_workgroup")
                add(r["n_cell_blocks"] > 1 and 0 < th.nc % g["energy_cpb"] <= 3 * (256 // KB), "energy:second_workgroup_empty_trips")
            if flag_route is not None:
                out |= {"tail:flag" if flag_route == "tail" else "flag:sweep", "fc_b_zero_column"}
            n_s = len(rows)
            add(n_s == 0, "sensor:none"), add(n_s == sc.MAX_SENSORS, "sensor:limit64")
            add(any(len(i) > 64 for i, _ in rows), "sensor:stride_loop"), add(any(len(i) == 1 for i, _ in rows), "sensor:single_entry")
            prev = r
    return out
