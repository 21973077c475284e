"""Cases, runs, route model, census and the host model (np.longdouble) of ONE backward step of the adjoint march, single and batched: the
right-hand side in front of the transposed sweeps (the forward element loops on the two masked levels or fc_adj_elem_nl / _reg / _b,
fc_adj_rhs_gather, fc_adj_rhs_gather_b), the control columns (fc_adj_control_columns) and the tail behind the sweeps (fc_adj_tail,
fc_adj_tail_b, fc_adj_reduce, fc_adj_reduce_b; dispatched by adj_enqueue_rhs / adj_enqueue_step and their batched forms in
csrc/fc_adjoint_run.hpp and csrc/fc_adjoint_batch_run.hpp).  No GPU import: tests/test_adjoint_march_cases_host.py runs everything here
on the host, tests/test_adjoint_march_gpu.py and tests/support/adjoint_march_child.py run it against the device.

  MESHES / TABLE                the meshes and the launch geometry each one reaches
  profiles / force_set          actuator sets: n_act Dirichlet profiles, `mixed` with load vectors of body-force profiles (fc_set_force)
  SENSOR_SETS / sensor_rows     step_cases' sets and two new ones: shared_rows, on_dirichlet
  SINGLE_RUNS / BATCH_RUNS      the runs, as data: the child executes them, walk() predicts the route of every backward step
  predicted_route               host model of the dispatch: what fc_get_adjoint_route must report
  census / LABELS / UNREACHED   the branches a set of runs reaches
  MarchModel                    one function per kernel in np.longdouble: rhs, masked, control_columns, partials, fold (+ fold_bitwise,
                                ct_chain: the two sums whose ORDER the sources state, reproduced bit for bit)"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from tests.support import step_cases as sc

L = np.longdouble
EPS = sc.EPS
DT, RE = sc.DT, sc.RE

# ── meshes ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
# the five edge meshes of the step tests; a square with N > 8192 (second, ragged trip of fc_adj_tail_b<32>: 8 rows per workgroup, grid
# capped at 1024); one with ceil(N / 256) > 64 (second, ragged trip of fc_adj_reduce's q += 64 loop)
MESHES = {**sc.CASES, "33x29": (33, 29), "64x32": (64, 32)}
# mesh -> (cells, unknowns)
TABLE = {"5x3": (30, 178), "9x9": (162, 822), "12x7": (168, 854), "12x11": (264, 1306), "23x12": (552, 2662), "33x29": (1914, 8926), "64x32": (4096, 18915)}
N_ACT = (0, 1, 2, 4, 5, 9, 32)
KBS = (4, 8, 16, 32)
TAIL_CAP, TAIL_B_CAP = 2048, 1024  # adj_tail_grid / adjb_tail_grid
ELEM_REG_MIN = sc.ELEM_REG_MIN
HANDLE_SETS = {"default": {}, "reg": {"FC_ELEM_REG_MIN": "1"}}
HANDLE_KNOBS = ("FC_ELEM_REG_MIN",)
TAPE_SETS = {"default": {}, "plain": {"FC_ADJ_TAPE_NT": "0"}}

# Largest relative distance of an fp64 numpy evaluation of MarchModel.rhs (the same expression, every table and operand rounded to fp64)
# from the np.longdouble one, 2-norm / max-norm over the velocity rows of a step whose two masked levels are not zero; measured per mesh
# by tests/test_adjoint_march_cases_host.py::test_host_constants, which asserts that these constants bound what it measures and exceed it
# by less than a factor of two.  (linearised: the mass product alone; nonlinear: with the transposed convection at a taped state.)
#            linearised                nonlinear
#   5x3      6.79e-17 / 9.12e-17       7.69e-17 / 1.01e-16
#   9x9      6.12e-17 / 1.20e-16       5.54e-17 / 7.48e-17
#   12x7     5.67e-17 / 7.57e-17       6.31e-17 / 1.22e-16
#   12x11    6.27e-17 / 1.44e-16       6.27e-17 / 1.72e-16
#   23x12    5.56e-17 / 1.04e-16       5.29e-17 / 1.15e-16
#   33x29    5.07e-17 / 9.79e-17       4.90e-17 / 1.40e-16
#   64x32    4.79e-17 / 7.29e-17       4.77e-17 / 8.01e-17
HOST_ADJ_RHS_ERROR = (7.69e-17, 1.72e-16)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def kb_of(k: int) -> int:
    return next(kb for kb in KBS if k <= kb)


_host = {}


def host_case(mesh: str):
    """(TaylorHood space, Dirichlet dofs) of a mesh; cached (and handed to step_cases' cache, so that step_cases.HostModel finds the two
    meshes its own table does not hold)."""
    if mesh not in _host:
        if mesh in sc.CASES:
            th, dofs, _ = sc.host_case(mesh)
        else:
            th, dofs, _ = sc.fcs.host_case(*MESHES[mesh], sc.TREE_BITS)
            sc._host[mesh] = (th, dofs, profiles(th, dofs, 2))
        _host[mesh] = (th, dofs)
    return _host[mesh]


# ── actuator sets ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def profiles(th, dofs, n_act: int) -> np.ndarray:
    """(n_bc, n_act) Dirichlet profiles: the two of step_cases.host_case, then smooth ones of other wave numbers on alternating
    components -- no two columns equal or proportional."""
    x = th.node_coords[dofs % th.nn]
    isx = dofs < th.nn
    cols = [np.where(isx, np.sin(x[:, 0] + 2 * x[:, 1]), 0.0), np.where(isx, 0.0, np.cos(3 * x[:, 0] - x[:, 1]))]
    for k in range(2, n_act):
        f = np.sin((0.7 + 0.45 * k) * x[:, 0] + 0.3 * k) * np.cos((1.1 + 0.3 * k) * x[:, 1] - 0.2 * k) + 0.05 * k
        cols.append(np.where(isx == (k % 2 == 0), f, 0.1 * f))
    return np.stack(cols[:n_act], axis=1) if n_act else np.zeros((len(dofs), 0))


def force_set(th, n_act: int) -> np.ndarray:
    """(n_act, 2 nn) nodal body-force profiles: step_cases.force_profiles, then more bumps and waves."""
    x = th.node_coords
    rows = list(sc.force_profiles(th, 0))
    for k in range(2, n_act):
        bump = np.exp(-((x[:, 0] - (0.15 + 0.025 * k)) ** 2 + (x[:, 1] - (0.8 - 0.02 * k)) ** 2) / 0.03)
        wave = np.sin((1 + 0.5 * k) * x[:, 0]) * np.cos((0.5 + 0.25 * k) * x[:, 1])
        rows.append(np.r_[bump, 0.3 * wave] if k % 2 == 0 else np.r_[0.3 * wave, bump])
    return np.stack(rows[:n_act]) if n_act else np.zeros((0, 2 * th.nn))


# ── sensor sets ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
SENSOR_SETS = sc.SENSOR_SETS + ("shared_rows", "on_dirichlet")


def sensor_rows(th, dofs, name: str) -> list[tuple[np.ndarray, np.ndarray]]:
    if name in sc.SENSOR_SETS:
        return sc.sensor_rows(th, name)
    rng = np.random.default_rng(len(name))
    free = np.setdiff1d(np.arange(2 * th.nn), dofs)
    if name == "shared_rows":
        # four sensors that overlap on the rows `sh` (five of them, each in three sensors at least); sensor 2 lists sh[0] twice with
        # different weights; every sensor also has rows of its own
        sh = free[rng.choice(free.size, size=5, replace=False)]
        own = [free[rng.choice(free.size, size=n, replace=False)] for n in (3, 2, 4, 1)]
        idx = [np.r_[sh[[0, 1, 2, 3]], own[0]], np.r_[own[1], sh[[4, 2, 1, 0]]], np.r_[sh[0], own[2], sh[[3, 4]], sh[0]], np.r_[sh[[4, 3, 2, 1, 0]], own[3]]]
        # (weights over seven decades: the ORDER of a row's sum then shows in its last bits)
        return [(i.astype(np.int32), (rng.standard_normal(i.size) + 0.5) * 10.0 ** rng.integers(-3, 4, i.size)) for i in idx]
    if name == "on_dirichlet":
        # entries on Dirichlet rows, pressure rows and free velocity rows in one sensor; a second one on Dirichlet rows only
        d = dofs[rng.choice(len(dofs), size=6, replace=False)]
        p = 2 * th.nn + rng.choice(th.nv, size=4, replace=False)
        f = free[rng.choice(free.size, size=3, replace=False)]
        return [(np.r_[d[:4], p, f].astype(np.int32), rng.standard_normal(11) + 0.5), (d[2:].astype(np.int32), rng.standard_normal(4) - 0.5)]
    raise KeyError(name)


def ct_table(rows, N: int):
    """The sensor table by row as adj_march_setup fills it (W numbering of the rows): per row the list of (sensor, weight), sensors
    ascending, a sensor's entries in the caller's order.  ``descending``: see MarchModel.ct_chain."""
    table = [[] for _ in range(N)]
    for s, (idx, w) in enumerate(rows):
        for i, v in zip(idx, w):
            table[int(i)].append((s, float(v)))
    return table


# ── runs, as data ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
# A single run: (mesh, n_act, variant, sensor set, handle set, nonlinear, first order, refine, steps, with_w)
#   linearised handles march step by step (fc_adjoint_reset with a terminal vector, `steps` fc_step_adjoint calls with the coefficients
#   of a run that starts on `first order`); nonlinear handles run fc_run_adjoint over a taped forward run of `steps` steps and of every
#   shorter length, so that the last backward step of each is seen -- under both FC_ADJ_TAPE_NT settings, which must agree bit for bit.
SINGLE_RUNS = [
    ("5x3", 0, "dirichlet", "one", "default", False, 1, 0, 3, True),
    ("5x3", 1, "dirichlet", "shared_rows", "reg", False, 2, 1, 3, True),
    ("9x9", 2, "mixed", "on_dirichlet", "default", False, 1, 0, 4, True),
    ("9x9", 9, "dirichlet", "none", "default", False, 2, 0, 3, False),
    ("12x7", 4, "dirichlet", "five", "default", True, 1, 0, 3, True),
    ("12x7", 2, "mixed", "shared_rows", "default", False, 1, 0, 3, False),
    ("12x11", 5, "mixed", "limit64", "reg", True, 2, 0, 3, True),
    ("12x11", 5, "mixed", "limit64", "default", True, 2, 0, 3, True),
    ("23x12", 9, "mixed", "long150", "default", False, 1, 1, 3, True),
    ("23x12", 32, "dirichlet", "single_entry", "default", True, 1, 0, 3, True),
    ("23x12", 9, "mixed", "long150", "reg", False, 1, 1, 3, True),
    ("33x29", 5, "mixed", "shared_rows", "default", False, 2, 0, 2, True),
    ("64x32", 5, "dirichlet", "on_dirichlet", "default", False, 1, 0, 1, True),
]
# A batched run: (mesh, k, n_act, variant, sensor set, nonlinear, first order, steps): fc_run_adjoint_batch of `steps` steps and of every
# shorter length.  Column k - 1 has w = 0, z = 0; columns 0 and k - 2 are equal (k >= 3).
BATCH_RUNS = [
    ("5x3", 3, 5, "mixed", "shared_rows", False, 1, 3),
    ("9x9", 5, 9, "dirichlet", "on_dirichlet", True, 2, 3),
    ("12x7", 9, 0, "dirichlet", "five", False, 1, 2),
    ("12x11", 17, 2, "mixed", "limit64", True, 1, 3),
    ("23x12", 32, 4, "mixed", "one", False, 2, 3),
    ("33x29", 32, 5, "dirichlet", "shared_rows", False, 1, 2),
    ("33x29", 17, 1, "dirichlet", "one", False, 1, 1),
]


def run_name(run: tuple) -> str:
    return "/".join(str(v) for v in run)


def step_coeffs(m: int, n: int, nonlinear: bool, dt: float = DT):
    """(cm_n, cm_nn, cc_n, cc_nn) of backward step m of an n-step run: forward step m + 1 read x_m with BDF2's (cm_n, cc_n), forward
    step m + 2 with (cm_nn, cc_nn), both gated by the horizon (fc_run_adjoint)."""
    nxt, nxt2 = m + 1 <= n, m + 2 <= n
    nl = 1.0 if nonlinear else 0.0
    return (2.0 / dt if nxt else 0.0, -0.5 / dt if nxt2 else 0.0, -2.0 * nl if nxt else 0.0, 1.0 * nl if nxt2 else 0.0)


# ── route model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
ROUTE_COLS = ("elem", "g_elem", "g_gather", "w", "term", "KB", "k", "g_tail", "passes", "reduced", "gx", "tape_nt")  # DeviceSolver.ADJ_ROUTE_COLS
ELEM_LANES, ELEM_REG, ELEM_BREG, ELEM_NL, ELEM_NL_REG, ELEM_NL_B = 1, 2, 3, 4, 5, 6
ELEM_NAMES = ("none", "fc_rhs_elem", "fc_rhs_elem_reg", "fc_rhs_elem_breg", "fc_adj_elem_nl", "fc_adj_elem_nl_reg", "fc_adj_elem_nl_b")


def predicted_route(mesh: str, n_act: int, n_sens: int, knobs: dict, nonlinear: bool, have_w: bool, have_term: bool, k: int = 0,
                    tape: int = -1, reduce: bool = True) -> np.ndarray:
    """What fc_get_adjoint_route must report for a backward step of a handle of ``mesh`` created under the handle knobs ``knobs``;
    ``k`` > 0: a batched step of k columns; ``tape``: -1 no copy into the state tape yet, 0 plain, 1 nontemporal.  The conditions are
    those of adj_enqueue_rhs / adj_enqueue_step, adjb_enqueue_rhs / adjb_enqueue_step and launch_elem_on."""
    nc, N = TABLE[mesh]
    passes = max(1, cdiv(n_act, 4))
    w = int(bool(have_w) and n_sens > 0)
    if k:
        KB = kb_of(k)
        g_tail = min(TAIL_B_CAP, cdiv(N, 256 // KB))
        red = int(n_act > 0 and reduce)
        return np.array([ELEM_NL_B if nonlinear else ELEM_BREG, cdiv(nc, 256 // KB), cdiv(N * (KB // 2), 256), w, int(have_term), KB, k, g_tail, passes,
                         red, g_tail if red else 0, tape], dtype=np.int32)
    reg_min = int(knobs.get("FC_ELEM_REG_MIN", ELEM_REG_MIN))
    reg = reg_min > 0 and nc >= reg_min
    elem = (ELEM_NL_REG if reg else ELEM_NL) if nonlinear else (ELEM_REG if reg else ELEM_LANES)
    g_tail = min(TAIL_CAP, cdiv(N, 256))
    return np.array([elem, cdiv(nc, 256) if reg else cdiv(8 * nc, 256), cdiv(N, 256), w, int(have_term), 0, 0, g_tail, passes, int(n_act > 0),
                     g_tail if n_act > 0 else 0, tape], dtype=np.int32)


def walk_single(run: tuple, tape_set: str = "default"):
    """The backward steps of a single run the child looks at, with their predicted routes: yields (n of the march, m, have_w, have_term,
    route).  Linearised: every step of the one march; nonlinear: the last step (m = 1) of the marches of length 1 .. steps."""
    mesh, n_act, _, sens, hs, nl, _, _, steps, with_w = run
    th, dofs = host_case(mesh)
    n_sens = len(sensor_rows(th, dofs, sens))
    kn = HANDLE_SETS[hs]
    if nl:
        tape = 0 if "FC_ADJ_TAPE_NT" in TAPE_SETS[tape_set] else 1
        for n in range(1, steps + 1):
            yield n, 1, with_w, n == 1, predicted_route(mesh, n_act, n_sens, kn, True, with_w, n == 1, tape=tape)
    else:
        for m in range(steps, 0, -1):
            yield steps, m, with_w, m == steps, predicted_route(mesh, n_act, n_sens, kn, False, with_w, m == steps)


def walk_batch(run: tuple, tape_set: str = "default"):
    mesh, k, n_act, _, sens, nl, _, steps = run
    th, dofs = host_case(mesh)
    n_sens = len(sensor_rows(th, dofs, sens))
    tape = (0 if "FC_ADJ_TAPE_NT" in TAPE_SETS[tape_set] else 1) if nl else -1
    for n in range(1, steps + 1):
        yield n, 1, True, n == 1, predicted_route(mesh, n_act, n_sens, {}, nl, True, n == 1, k=k, tape=tape)


# ── census ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
LABELS = (
    "fc_rhs_elem", "fc_rhs_elem_reg", "fc_rhs_elem_breg", "fc_adj_elem_nl", "fc_adj_elem_nl_reg", "fc_adj_elem_nl_b", "elem:ragged_workgroup",
    "elem:one_workgroup", "elem:several_workgroups", "fc_adj_rhs_gather", "gather:w", "gather:no_w", "gather:term", "gather:no_term",
    "fc_adj_rhs_gather_b<4>", "fc_adj_rhs_gather_b<8>", "fc_adj_rhs_gather_b<16>", "fc_adj_rhs_gather_b<32>", "batch:padding_columns", "batch:full_width",
    "ct:none", "ct:row_with_two_entries", "ct:row_twice_in_one_sensor", "ct:dirichlet_row", "ct:pressure_row", "ct:limit64",
    "columns:dirichlet_only", "columns:fvec",
    "fc_adj_tail", "tail:n_act=0", "tail:one_pass", "tail:later_passes", "tail:ragged_last_pass", "tail:full_last_pass", "tail:ragged_workgroup",
    "fc_adj_tail_b", "tail_b:n_act=0", "tail_b:one_pass", "tail_b:later_passes", "tail_b<32>:second_trip", "tail_b:grid_cap",
    "fc_adj_reduce", "reduce:skipped", "reduce:one_trip", "reduce:second_trip", "fc_adj_reduce_b", "reduce_b:second_trip",
    "fc_adj_tape_copy<true>", "fc_adj_tape_copy<false>", "solve:refined",
    "tail:second_trip", "tail_b<16>:second_trip", "tail_b<8>:second_trip", "tail_b<4>:second_trip",  # UNREACHED
)
UNREACHED = {
    "tail:second_trip": "the grid-stride trip of the single fc_adj_tail needs more than 2048 workgroups of 256 rows, N > 524288: beyond any host model; "
                        "the loop is the one fc_adj_tail_b<32> runs its second trip through",
    "tail_b<16>:second_trip": "16 rows per workgroup and a grid capped at 1024: N > 16384; the one mesh of the table beyond it (64x32) is kept to the single "
                              "march, a batched march of it at KB = 16 holds 2 x 18915 x 16 doubles per level and a dense-free host model of 16 columns",
    "tail_b<8>:second_trip": "32 rows per workgroup: N > 32768, no mesh of the table",
    "tail_b<4>:second_trip": "64 rows per workgroup: N > 65536, no mesh of the table",
}


def census(single: list[tuple], batch: list[tuple], tape_sets=tuple(TAPE_SETS)) -> set[str]:
    """Labels the backward steps of the runs reach (nonlinear runs: under each of ``tape_sets``)."""
    out = set()

    def add(cond, label):
        if cond:
            out.add(label)

    def sensors(mesh, sens, have_w):
        th, dofs = host_case(mesh)
        rows = sensor_rows(th, dofs, sens)
        if not rows or not have_w:
            out.add("ct:none")
            return
        tab = ct_table(rows, th.N)
        isd = np.zeros(th.N, dtype=bool)
        isd[dofs] = True
        for i, ent in enumerate(tab):
            add(len(ent) >= 2, "ct:row_with_two_entries")
            add(len({s for s, _ in ent}) < len(ent), "ct:row_twice_in_one_sensor")
            add(bool(ent) and isd[i], "ct:dirichlet_row")
            add(bool(ent) and i >= 2 * th.nn, "ct:pressure_row")
        add(len(rows) == sc.MAX_SENSORS, "ct:limit64")

    for run in single:
        mesh, n_act, variant, sens, hs, nl, _, refine, _, with_w = run
        nc, N = TABLE[mesh]
        sensors(mesh, sens, with_w)
        add(n_act > 0, "columns:fvec" if variant == "mixed" else "columns:dirichlet_only")
        add(refine > 0, "solve:refined")
        for ts in (tape_sets if nl else ("default",)):
            for _, _, _, _, route in walk_single(run, ts):
                r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
                out |= {ELEM_NAMES[r["elem"]], "fc_adj_rhs_gather", "fc_adj_tail", "gather:w" if r["w"] else "gather:no_w", "gather:term" if r["term"] else "gather:no_term"}
                per = 256 if r["elem"] in (ELEM_REG, ELEM_NL_REG) else 32
                add(nc % per, "elem:ragged_workgroup"), add(r["g_elem"] == 1, "elem:one_workgroup"), add(r["g_elem"] > 1, "elem:several_workgroups")
                add(N % 256, "tail:ragged_workgroup"), add(cdiv(N, 256) > TAIL_CAP, "tail:second_trip")
                add(n_act == 0, "tail:n_act=0"), add(r["passes"] == 1 and n_act > 0, "tail:one_pass"), add(r["passes"] > 1, "tail:later_passes")
                add(n_act % 4, "tail:ragged_last_pass"), add(n_act > 0 and n_act % 4 == 0, "tail:full_last_pass")
                if r["reduced"]:
                    out |= {"fc_adj_reduce", "reduce:second_trip" if r["gx"] > 64 else "reduce:one_trip"}
                else:
                    out.add("reduce:skipped")
                add(r["tape_nt"] == 1, "fc_adj_tape_copy<true>"), add(r["tape_nt"] == 0, "fc_adj_tape_copy<false>")
    for run in batch:
        mesh, k, n_act, variant, sens, nl, _, _ = run
        nc, N = TABLE[mesh]
        sensors(mesh, sens, True)
        add(n_act > 0, "columns:fvec" if variant == "mixed" else "columns:dirichlet_only")
        for ts in (tape_sets if nl else ("default",)):
            for _, _, _, _, route in walk_batch(run, ts):
                r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
                KB = r["KB"]
                out |= {ELEM_NAMES[r["elem"]], f"fc_adj_rhs_gather_b<{KB}>", "fc_adj_tail_b", "gather:w", "gather:term" if r["term"] else "gather:no_term"}
                add(k < KB, "batch:padding_columns"), add(k == KB, "batch:full_width")
                add(nc % (256 // KB), "elem:ragged_workgroup")
                add(n_act == 0, "tail_b:n_act=0"), add(r["passes"] == 1 and n_act > 0, "tail_b:one_pass"), add(r["passes"] > 1, "tail_b:later_passes")
                add(cdiv(N, 256 // KB) > TAIL_B_CAP, f"tail_b<{KB}>:second_trip"), add(r["g_tail"] == TAIL_B_CAP, "tail_b:grid_cap")
                if r["reduced"]:
                    out |= {"fc_adj_reduce_b"} | ({"reduce_b:second_trip"} if r["gx"] > 64 else set())
                else:
                    out.add("reduce:skipped")
                add(r["tape_nt"] == 1, "fc_adj_tape_copy<true>"), add(r["tape_nt"] == 0, "fc_adj_tape_copy<false>")
    return out


# ── operators on the host (the device assembles its own; these serve the host test) ──────────────────────────────────────────────────
def host_operators(mesh: str):
    """{order: (operator before the elimination of the Dirichlet dofs, after it)} and the mass matrix, from the numpy oracle."""
    from oracle import ns_oracle as O

    th, dofs = host_case(mesh)
    d = O.Disc.from_taylor_hood(th)
    free = np.ones(th.N)
    free[dofs] = 0.0
    Zf, Zd = sp.diags(free), sp.diags(1.0 - free)
    full, bc = {}, {}
    for order in (1, 2):
        full[order] = O.assemble_matrix(d, **sc.operator_args(th, order)).tocsr()
        bc[order] = (Zf @ full[order] @ Zf + Zd).tocsr()
    M = sp.block_diag([O.velocity_mass(d), sp.csr_matrix((th.nv, th.nv))]).tocsr()
    return full, bc, M


class RefinedT:
    """A^-T b: sparse LU in fp64, then refinements with the residual formed in np.longdouble and the iterate kept in np.longdouble (the
    scheme of batch_cases.refined_solve on the transposed operator; a sparse factorisation, so that the two large meshes stay at seconds)."""

    def __init__(self, A, sweeps: int = 2):
        import scipy.sparse.linalg as spla

        self.At = sp.csr_matrix(A.T)
        self.At.sort_indices()
        self.lu, self.sweeps = spla.splu(sp.csc_matrix(A)), sweeps

    def __call__(self, b, longdouble: bool = False):
        b = np.asarray(b, dtype=L)
        x = self.lu.solve(np.asarray(b, dtype=np.float64), trans="T").astype(L)
        for _ in range(self.sweeps):
            r = b - sc.spmv_longdouble(self.At, x)
            x = x + self.lu.solve(np.asarray(r, dtype=np.float64), trans="T")
        return x if longdouble else np.asarray(x, dtype=np.float64)


# ── the host model, one function per kernel ──────────────────────────────────────────────────────────────────────────────────────────
class MarchModel:
    """One (mesh, actuator set, sensor set) in np.longdouble, W numbering.  ``A_full``: {order: the slot's operator WITHOUT boundary
    conditions} -- the device's own (the child) or the oracle's (the host test); its Dirichlet columns are the lifting."""

    def __init__(self, mesh: str, n_act: int, variant: str, sens: str, A_full: dict):
        self.mesh, self.n_act, self.variant = mesh, n_act, variant
        self.th, self.dofs = host_case(mesh)
        th = self.th
        self.N, self.nn = th.N, th.nn
        self.hm = sc.HostModel(mesh)
        self.prof = profiles(th, self.dofs, n_act)
        self.fprof = force_set(th, n_act) if (variant == "mixed" and n_act > 0) else None
        self.rows = sensor_rows(th, self.dofs, sens)
        self.ct = ct_table(self.rows, self.N)
        self.free = np.ones(self.N, dtype=bool)
        self.free[self.dofs] = False
        self.A_full = {o: A.tocsr() for o, A in A_full.items()}
        self._cols = {}

    # fc_adj_control_columns ----------------------------------------------------------------------------------------------------------
    def control_columns(self, order: int, wrong: str | None = None):
        """(bt [n_act][N] in longdouble, lift, F, lift_bound): the profile on a Dirichlet row, -lift + F elsewhere.  lift = A_full G in
        longdouble; lift_bound = (L + 2) eps sum |a_ij| |g_j| per row bounds an fp64 row sum of any order (L the row's entries).
        ``wrong="fvec"``: the load vectors dropped."""
        if (order, wrong) in self._cols:
            return self._cols[order, wrong]
        A, N, na = self.A_full[order], self.N, self.n_act
        bt, lift, F, lb = (np.zeros((na, N), dtype=L) for _ in range(4))
        Aabs, nrow = abs(A), np.diff(A.indptr)
        for k in range(na):
            g = np.zeros(N, dtype=L)
            g[self.dofs] = self.prof[:, k].astype(L)
            lift[k] = sc.spmv_longdouble(A, g)
            lb[k] = (nrow + 2) * EPS * sc.spmv_longdouble(Aabs, np.abs(g))
            if self.fprof is not None and wrong != "fvec":
                F[k] = self.hm.load(self.hm._at_q(self.fprof[k].astype(L))[0])
            bt[k] = F[k] - lift[k]
            bt[k][self.dofs] = self.prof[:, k].astype(L)
        self._cols[order, wrong] = (bt, lift, F, lb)
        return self._cols[order, wrong]

    # element loop + fc_adj_rhs_gather -------------------------------------------------------------------------------------------------
    def _at_q(self, u, T):
        hm = self.hm
        u = np.asarray(u, dtype=T)
        ue = np.stack([u[hm.cn], u[hm.nn + hm.cn]], axis=2)
        return np.einsum("qa,caj->cqj", hm.PHI2.astype(T), ue), np.einsum("cqai,caj->cqij", hm.G2.astype(T), ue)

    def elem_part(self, zm1, zm2, coeffs, x_taped=None, T=L, wrong=None):
        """M Z (cm_n zm1 + cm_nn zm2) + J(x)^T Z (cc_n zm1 + cc_nn zm2) on every row, evaluated in the type ``T`` with the quadrature
        tables of step_cases.HostModel (the oracle's, cast): per cell and point V = sum_a v_a phi_a,
            (M v)[b, j] = sum_q w V_j phi_b,     (J^T v)[b, j] = sum_q w (phi_b sum_i V_i d_j u_i + V_j (u . grad phi_b))."""
        hm = self.hm
        cm_n, cm_nn, cc_n, cc_nn = (T(c) for c in coeffs)
        z1, z2 = (np.where(self.free, np.asarray(z, dtype=T), T(0)) for z in (zm1, zm2))
        am = cm_n * z1 + cm_nn * z2
        w, PHI = hm.w.astype(T), hm.PHI2.astype(T)
        Vm = self._at_q(am[: 2 * self.nn], T)[0]
        Le = np.einsum("cq,qb,cqj->cbj", w, PHI, Vm)
        if x_taped is not None and (cc_n != 0 or cc_nn != 0):
            ac = cc_n * z1 + cc_nn * z2
            Vc = self._at_q(ac[: 2 * self.nn], T)[0]
            uq, gu = self._at_q(np.asarray(x_taped, dtype=T)[: 2 * self.nn], T)  # gu[c, q, i, j] = d_i u_j
            Le = Le + np.einsum("cq,qb,cqi,cqji->cbj", w, PHI, Vc, gu) + np.einsum("cq,cqj,cql,cqbl->cbj", w, Vc, uq, hm.G2.astype(T))
        out = np.zeros(self.N, dtype=T)
        np.add.at(out, hm.cn.reshape(-1), Le[:, :, 0].reshape(-1))
        np.add.at(out, self.nn + hm.cn.reshape(-1), Le[:, :, 1].reshape(-1))
        if wrong == "mask_out":
            out = np.where(self.free, out, T(0))
        return out

    def ct_part(self, w, T=L, wrong=None):
        """(C^T w, sum |c w| per row, entries per row).  ``wrong="first_weight"``: every entry of a row takes the first entry's weight."""
        out, mag, cnt = np.zeros(self.N, dtype=T), np.zeros(self.N, dtype=L), np.zeros(self.N, dtype=np.int64)
        if w is None:
            return out, mag, cnt
        for i, ent in enumerate(self.ct):
            for s, c in ent:
                c = ent[0][1] if wrong == "first_weight" else c
                out[i] += T(c) * T(w[s])
                mag[i] += abs(L(c) * L(w[s]))
            cnt[i] = len(ent)
        return out, mag, cnt

    def rhs(self, zm1, zm2, coeffs, w, term, x_taped=None, T=L, wrong=None):
        """The right-hand side of a backward step on every row: M Z (..) (+ J(x_taped)^T Z (..)) + C^T w + term.  Not masked."""
        b = self.elem_part(zm1, zm2, coeffs, x_taped, T, wrong) + self.ct_part(w, T, wrong)[0]
        return b if term is None else b + np.asarray(term, dtype=T)

    def ct_chain(self, i: int, w, term=None, descending: bool = False) -> tuple[float, float]:
        """Row i of a FIRST backward step (both masked levels zero: the element sum is 0.0) as fc_adj_rhs_gather forms it in fp64, bit
        for bit: the row's entries c * w[sensor] added from 0.0 in the table's order, then ``term``.  Returns (with every product rounded
        before its add, with fused multiply-adds): the compiler may contract ``s += c * w`` or not, the order is the source's.
        ``descending``: the table filled sensors-descending (a mistake the test must see)."""
        ent = self.ct[i]
        if descending:
            ent = [e for s in sorted({s for s, _ in self.ct[i]}, reverse=True) for e in self.ct[i] if e[0] == s]
        plain, fused = 0.0, 0.0
        for s, c in ent:
            plain = plain + c * float(w[s])
            fused = float(Fraction(fused) + Fraction(c) * Fraction(float(w[s])))
        return (plain, fused) if term is None else (plain + float(term), fused + float(term))

    # fc_adj_tail -----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def masked(mu, free):
        """zm: mu off the Dirichlet rows, 0 on them (``free`` in the numbering of ``mu``)."""
        return np.where(free[(...,) + (None,) * (np.ndim(mu) - 1)], mu, 0.0)

    @staticmethod
    def partials(bt, mu, grid: int, rows_per_group: int, wrong=None):
        """(shares [n_act][grid], bounds): workgroup q takes the rows q R + r, (q + grid) R + r, .. (r < R = rows_per_group) of the
        numbering ``bt`` and ``mu`` come in.  bound = 2 (rows in the share + 8) eps sum |bt| |mu| holds for any summation order (the + 8:
        the tree over the workgroup's threads).  ``wrong="first4"``: actuators beyond the first four dropped."""
        bt, mu = np.asarray(bt, dtype=L), np.asarray(mu, dtype=L)
        na, N = bt.shape
        owner = (np.arange(N) // rows_per_group) % grid
        rows = np.bincount(owner, minlength=grid)
        prod = bt * mu[None, :]
        share, mag = np.zeros((na, grid), dtype=L), np.zeros((na, grid), dtype=L)
        for a in range(na):
            if wrong == "first4" and a >= 4:
                continue
            np.add.at(share[a], owner, prod[a])
            np.add.at(mag[a], owner, np.abs(prod[a]))
        return share, 2 * (rows[None, :] + 8) * EPS * mag

    # fc_adj_reduce ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def fold(partial):
        """g = the sum of an actuator's partials, in longdouble (last axis)."""
        return np.sum(np.asarray(partial, dtype=L), axis=-1)

    @staticmethod
    def fold_bitwise(partial) -> np.ndarray:
        """The same in fp64 in the order the source states: lane l takes partials l, l + 64, .. in order, then the shuffle tree
        (offsets 32, 16, .. 1: lane l adds lane l + off).  Bit for bit what fc_adj_reduce / fc_adj_reduce_b leave in g.
        ``partial``: (.., gx); returns (..)."""
        p = np.asarray(partial, dtype=np.float64)
        gx = p.shape[-1]
        lanes = np.zeros(p.shape[:-1] + (64,))
        for t in range(cdiv(gx, 64)):
            chunk = p[..., 64 * t: 64 * (t + 1)]
            lanes[..., : chunk.shape[-1]] = lanes[..., : chunk.shape[-1]] + chunk
        for off in (32, 16, 8, 4, 2, 1):
            lanes[..., :off] = lanes[..., :off] + lanes[..., off: 2 * off]
        return lanes[..., 0].copy()

    @staticmethod
    def dot(bt, mu):
        """(B~_k . mu in longdouble, its bound 2 (N + 2) eps sum |bt| |mu|) per actuator."""
        prod = np.asarray(bt, dtype=L) * np.asarray(mu, dtype=L)[None, :]
        return prod.sum(axis=1), 2 * (prod.shape[1] + 2) * EPS * np.abs(prod).sum(axis=1)


def host_march(model: MarchModel, solve_t: dict, first_order: int, n: int, w, z, X=None):
    """The whole backward march through the functions above, in longdouble: (g [n][n_act], mu [n][N]).  ``solve_t``: {order: RefinedT};
    ``X`` [n + 2][N]: the forward states x_{-1}, x_0, .. x_n of a nonlinear run (None: linearised)."""
    N = model.N
    zm = [np.zeros(N, dtype=L), np.zeros(N, dtype=L)]  # (newer, older)
    g, mus = np.zeros((n, model.n_act), dtype=L), np.zeros((n, N), dtype=L)
    for m in range(n, 0, -1):
        order = first_order if m == 1 else 2
        b = model.rhs(zm[0], zm[1], step_coeffs(m, n, X is not None), None if w is None else w[m - 1], z if m == n else None,
                      None if X is None else X[m + 1])
        mu = solve_t[order](b, longdouble=True)
        g[m - 1] = model.dot(model.control_columns(order)[0], mu)[0]
        mus[m - 1] = mu
        zm = [model.masked(mu, model.free), zm[0]]
    return g, mus


def rel2(a, ref) -> float:
    a, ref = np.asarray(a, dtype=L), np.asarray(ref, dtype=L)
    d = np.sum(ref**2)
    return float(np.sqrt(np.sum((a - ref) ** 2) / d)) if d > 0 else float(np.abs(a - ref).max())


def relmax(a, ref) -> float:
    a, ref = np.asarray(a, dtype=L), np.asarray(ref, dtype=L)
    d = np.abs(ref).max()
    return float(np.abs(a - ref).max() / d) if d > 0 else float(np.abs(a - ref).max())


def inputs(N: int, n_sens: int, steps: int, seed: int, k: int = 0):
    """(w [steps][n_sens] or [steps][k][n_sens], z [N] or [k][N]): smooth-free random inputs; batched: column k - 1 all zero, column
    k - 2 a copy of column 0 (k >= 3)."""
    rng = np.random.default_rng(seed)
    if not k:
        return rng.standard_normal((steps, n_sens)), rng.standard_normal(N)
    w, z = rng.standard_normal((steps, k, n_sens)), rng.standard_normal((k, N))
    w[:, k - 1], z[k - 1] = 0.0, 0.0
    if k >= 3:
        w[:, k - 2], z[k - 2] = w[:, 0], z[0]
    return w, z
