"""Cases, knob sets, runs, route model and the host model (np.longdouble) of ONE time step of the single simulation: the right-hand side in
front of the factor sweeps (fc_rhs_elem, fc_rhs_elem_reg, fc_rhs_gather, fc_force_rows) and the tail behind them (fc_tail<false|true>,
fc_finish, fc_final, fc_early, fc_wait_solved, fc_final_late; dispatched by enqueue_rhs, launch_tail, enqueue_step_launches and
step_enqueue_overlapped of csrc/fc_hip.hip).  No GPU import: tests/test_step_cases_host.py runs everything here on the host,
tests/test_step_routes_gpu.py and tests/support/step_child.py run it against the device.

  CASES / TABLE                 the meshes and the launch geometry each one reaches
  KNOB_SETS / HANDLE_SETS       knobs read once per process (a child process each) / when a handle is created (a fresh handle each)
  SENSOR_SETS / sensor_rows     the sensor rows of a run
  predicted_route               host model of the dispatch conditions: what fc_get_step_route must report
  History                       what that model remembers of a handle (speculated slot, step count, C operators, force vectors)
  scenario / RUNS               the operations of a run, as data: the child executes them, walk() only predicts their routes
  census / LABELS / UNREACHED   the branches a set of runs reaches
  HostModel                     the step in np.longdouble: right-hand side, sensors, energy, residual norms and their bounds"""
from __future__ import annotations

import numpy as np

from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from tests.support import batch_cases as bc
from tests.support import front_cases as fcs

L = np.longdouble
EPS = 2.0**-53  # unit round-off of fp64

# ── meshes ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
CASES = {"5x3": (5, 3), "9x9": (9, 9), "12x7": (12, 7), "12x11": (12, 11), "23x12": (23, 12)}
TREE_BITS = (2,)
# case -> (cells, unknowns, row workgroups, cell workgroups of a monitored step with energy at reps = 1, check workgroups of an unmonitored one)
TABLE = {
    "5x3": (30, 178, 6, 1, 1),       # one ragged cell workgroup (< 32 cells), g = 7 < one arrival group, one check workgroup
    "9x9": (162, 822, 26, 6, 1),     # g = 32: the arrival groups exactly full
    "12x7": (168, 854, 27, 6, 1),    # g = 33: a last arrival group of ONE workgroup
    "12x11": (264, 1306, 41, 9, 2),  # fc_rhs_elem_reg: second workgroup nearly empty (264 = 256 + 8), 2 check workgroups, g = 50
    "23x12": (552, 2662, 84, 18, 3),  # 3 check workgroups (last ragged), g = 102 = 3 full groups + 6; FC_TAIL_REPS=3: ragged row and cell groups
}
DT, RE = 0.005, 100.0
N_ACT = 2
GROUP = 32  # workgroups per arrival group of the fused final (launch_tail: kGroup)
TAIL_CHECK_ROWS = 1024  # rows per check workgroup: 256 threads x FC_TAIL_CHECK
ELEM_REG_MIN = 40000  # fc_ctx::elem_reg_min


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


_host = {}


def host_case(case: str):
    """(TaylorHood space, Dirichlet dofs, their two profiles) of a case; cached."""
    if case not in _host:
        nx, ny = CASES[case]
        th, dofs, _ = fcs.host_case(nx, ny, TREE_BITS)
        x = th.node_coords[dofs % th.nn]
        isx = dofs < th.nn
        prof = np.stack([np.where(isx, np.sin(x[:, 0] + 2 * x[:, 1]), 0.0), np.where(isx, 0.0, np.cos(3 * x[:, 0] - x[:, 1]))], axis=1)
        _host[case] = (th, dofs, prof)
    return _host[case]


def smooth_velocity(th, k: float = 1.0) -> np.ndarray:
    x = th.node_coords
    return np.r_[1.0 + 0.3 * np.sin(k * x[:, 0]) * np.cos(0.7 * k * x[:, 1]), 0.2 * np.cos(0.5 * k * x[:, 0] + 0.1) * np.sin(k * x[:, 1])]


def initial_state(th, seed: int):
    """(u_n, u_nn, p_n): smooth fields plus noise, so that no two dofs cancel by symmetry."""
    rng = np.random.default_rng(seed)
    u_n = 0.1 * smooth_velocity(th, 2.0) + 0.01 * rng.standard_normal(2 * th.nn)
    u_nn = 0.1 * smooth_velocity(th, 1.5) + 0.01 * rng.standard_normal(2 * th.nn)
    return u_n, u_nn, 0.01 * rng.standard_normal(th.nv)


def force_profiles(th, variant: int = 0) -> np.ndarray:
    """(N_ACT, 2 nn) nodal body-force profiles (as tests/test_hip_kernels.py::test_crank_nicolson_step; variant 1: other ones)."""
    x = th.node_coords
    c = 0.4 + 0.2 * variant
    return np.stack([np.r_[np.exp(-((x[:, 0] - c) ** 2 + (x[:, 1] - 0.5) ** 2) / 0.02), 0 * x[:, 0]],
                     np.r_[0 * x[:, 0], np.sin((1 + variant) * x[:, 0]) * np.cos(x[:, 1])]])


CONTROLS = np.array([[0.3, -0.2], [-0.1, 0.4], [0.25, 0.15], [-0.35, 0.05]])


def operator_args(th, order: int, dt: float = DT, lagged: bool = False) -> dict:
    """Arguments of assemble_matrix for the BDF operator of ``order``; ``lagged``: the operator A1 the residual monitor is tested on --
    dt halved and a stronger, rotated advection (as tests/test_hip_kernels.py::test_bicgstab_with_exact_and_lagged_factors)."""
    U = 1.6 * smooth_velocity(th, 1.3) if lagged else smooth_velocity(th)
    a = (1.0 if order == 1 else 1.5) / (0.5 * dt if lagged else dt)
    return dict(mass=a, nu=1.0 / RE, adv=U, lin=U)


def cn_operator_args(th) -> dict:
    """The explicit operator C of tests/test_hip_kernels.py::test_crank_nicolson_step (velocity columns are taken by the caller)."""
    U = smooth_velocity(th)
    return dict(mass=0.0, nu=0.5 / RE, adv=U, lin=U, adv_scale=0.5, lin_scale=0.5, pressure=0.0, divergence=0.0)


# ── knobs ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
PROCESS_KNOBS = ("FC_FUSED_FINAL", "FC_FUSED_TAIL", "FC_SPECULATE", "FC_TAIL_REPS")
HANDLE_KNOBS = ("FC_ELEM_REG_MIN", "FC_OVERLAP_TAIL")
KNOB_SETS = {
    "default": {},
    "fused_final": {"FC_FUSED_FINAL": "1"},
    "unfused_tail": {"FC_FUSED_TAIL": "0"},
    "no_speculate": {"FC_SPECULATE": "0"},
    "reps3": {"FC_TAIL_REPS": "3"},
    "reps3_fused_final": {"FC_TAIL_REPS": "3", "FC_FUSED_FINAL": "1"},
}
HANDLE_SETS = {"default": {}, "reg": {"FC_ELEM_REG_MIN": "1"}, "one_stream": {"FC_OVERLAP_TAIL": "0"}}
# children whose records must agree bit for bit, step by step (the sources state the same fold order / the same element vectors)
BITWISE_PAIRS = (("default", "fused_final"), ("default", "no_speculate"), ("reps3", "reps3_fused_final"))

# ── sensors ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
SENSOR_SETS = ("none", "one", "five", "limit64", "long150", "single_entry")
MAX_SENSORS = 64  # fc_set_sensors refuses more (ysh[64] of fc_final_body / fc_early)


def sensor_rows(th, name: str) -> list[tuple[np.ndarray, np.ndarray]]:
    rng = np.random.default_rng(len(name))
    pe = lambda p, c: tuple(np.asarray(a) for a in th.point_eval_row(p, c))
    rnd = lambda n: (rng.choice(th.N, size=n, replace=False).astype(np.int32), rng.standard_normal(n))
    if name == "none":
        return []
    if name == "one":
        return [pe((0.31, 0.42), 1)]
    if name == "five":  # more rows than the 4 waves of the workgroup; one of them a point evaluation
        return [pe((0.5, 0.5), 0)] + [rnd(n) for n in (3, 17, 64, 65)]
    if name == "limit64":
        return [rnd(1 + (7 * s) % 23) for s in range(MAX_SENSORS)]
    if name == "long150":  # the 64-lane stride loop runs 3 trips, the last one ragged
        return [rnd(150)]
    if name == "single_entry":
        return [(np.array([th.N // 3], dtype=np.int32), np.array([1.75]))]
    raise KeyError(name)


# ── route model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
ROUTE_COLS = ("elem", "speculated", "solver", "tail", "monitored", "g_rows", "g_check", "g_cells", "reps")  # DeviceSolver.STEP_ROUTE_COLS
ELEM_REUSED, ELEM_LANES, ELEM_REG = 0, 1, 2
SOLVER_APPLY, SOLVER_REFINE, SOLVER_BICGSTAB, SOLVER_GMRES = 0, 1, 2, 3
TAIL_FUSED, TAIL_FUSED_FINAL, TAIL_FINISH, TAIL_OVERLAPPED = 0, 1, 2, 3
DEFAULT_OPTS = dict(refine=0, check=1, method="refine")


class History:
    """What the dispatch of the next step depends on beyond its own arguments."""

    def __init__(self):
        self.pre_slot = -1  # fc_ctx::pre_slot: slot whose element vectors the previous step left behind
        self.step_count = 0  # fc_ctx::step_count: the cadence of the residual monitor counts the handle's steps
        self.have_c = {SLOT_BDF1: False, SLOT_BDF2: False}
        self.ready = {SLOT_BDF1: True, SLOT_BDF2: True}
        self.have_force = self.fvec_ok = False

    def invalidate(self):
        self.pre_slot = -1


def _knob(knobs: dict, name: str, default: int) -> int:
    return int(knobs[name]) if name in knobs else default


def predicted_route(case: str, knobs: dict, settings: dict, history: History) -> np.ndarray:
    """The vector fc_get_step_route must report for a step with ``settings`` (order, energy, blocking, refine, check, method) on a handle
    of ``case`` created under ``knobs`` (process and handle knobs together) whose past is ``history``.  The conditions are those of
    use_fused_tail, step_can_overlap, residual_every, launch_elem_on, speculate_next_rhs and launch_tail, read from csrc/fc_hip.hip; the
    meshes here are far below the sizes where factors stream from HBM (OrderSys::nt) and their factors are exact fp64 ones."""
    nc, N = TABLE[case][:2]
    slot = SLOT_BDF1 if settings["order"] == 1 else SLOT_BDF2
    refine, check, method = settings["refine"], int(settings["check"]), settings["method"]
    # check_step_ready: new body-force profiles are turned into load vectors with the element vectors as scratch (build_force_vectors)
    pre = -1 if (history.have_force and not history.fvec_ok) else history.pre_slot
    reg_min = _knob(knobs, "FC_ELEM_REG_MIN", ELEM_REG_MIN)
    elem = ELEM_REUSED if pre == slot else (ELEM_REG if reg_min > 0 and nc >= reg_min else ELEM_LANES)
    fused_tail = knobs.get("FC_FUSED_TAIL", "1")[0] != "0" and refine == 0  # use_fused_tail (refine = fc_ctx::max_iter)
    overlap = (knobs.get("FC_OVERLAP_TAIL", "1")[0] != "0" and not settings["blocking"] and method == "refine" and fused_tail)  # step_can_overlap
    res = check != 0 and history.step_count % check == 0  # residual_every = check_residual (>= 0 here)
    energy = bool(settings["energy"])
    if overlap:
        reps = max(1, cdiv(N, 32 * 2048))  # (FC_TAIL_REPS is launch_tail's)
        route = [elem, -1, SOLVER_APPLY, TAIL_OVERLAPPED, int(res), cdiv(N, 32 * reps) if res else 0, 0, cdiv(nc, 32 * reps) if energy else 0, reps]
    elif method != "refine" or fused_tail:
        reps = _knob(knobs, "FC_TAIL_REPS", 0) or max(1, cdiv(N, 32 * 2048))
        fused_final = knobs.get("FC_FUSED_FINAL", "0")[0] == "1"
        solver = SOLVER_APPLY if method == "refine" else (SOLVER_GMRES if method == "gmres" else SOLVER_BICGSTAB)
        route = [elem, -1, solver, TAIL_FUSED_FINAL if fused_final else TAIL_FUSED, int(res), cdiv(N, 32 * reps) if res else 0,
                 0 if res else cdiv(N, TAIL_CHECK_ROWS), cdiv(nc, 32 * reps) if energy else 0, reps]
    else:
        # solve_permuted + fc_finish + fc_final: the residual partials come from the driver's first SpMV whenever check_residual != 0 --
        # on EVERY step, the cadence is the fused tail's
        g = cdiv(N, 32)
        route = [elem, -1, SOLVER_REFINE, TAIL_FINISH, int(check != 0), g, 0, g if energy else 0, 1]
    # speculate_next_rhs: BDF2 follows, or the same slot when it carries an explicit operator (Crank-Nicolson)
    if knobs.get("FC_SPECULATE", "1")[0] != "0" and nc > 0:
        nxt = slot if history.have_c[slot] else SLOT_BDF2
        if history.ready[nxt]:
            route[1] = nxt
    return np.array(route, dtype=np.int32)


def advance(history: History, route: np.ndarray) -> None:
    """The handle after a step that took ``route``."""
    history.pre_slot = int(route[1])
    history.step_count += 1
    if history.have_force:
        history.fvec_ok = True


# ── scenarios: the operations of a run, as data ──────────────────────────────────────────────────────────────────────────────────────
# ("opts", dict)                      set_solver_options(refine, check_residual, method)
# ("step", order, energy, mode, uc)   mode "block": step(); "early": step_begin + step_end(early=True) + step_collect; uc: row of CONTROLS
# ("bad_step", order, mode, what)     what "nan_u": NaN in one velocity entry of u_n; "inf_ctrl": inf in u_ctrl -> FC_ERR_DIVERGED, flag 1
# ("set_state", seed, what)           what None / "nan_p": NaN in one entry of p_n (the right-hand side does not read the pressure)
# ("rhs", order, uc)                  assemble_rhs against the longdouble right-hand side (resets the speculation, by design)
# ("time_scheme", dt, nonlinear, refactor)   ("undo",)   ("batch",)   ("force", variant | None)   ("cop", order, on)
# ("solve_energy",)                   a dev.solve() and a dev.energy() between two steps
# ("lagged", order)                   the slot's operator replaced by A1 behind the factors of A0 (update_operator): residual monitor
# ("mark",) ("raw_step", order, energy, uc) ... ("raw_collect",) ("rewind",) steps ... ("same_as_raw",)
#                                     steps begun and ended early back to back, nothing read in between; then the state of the mark again
#                                     and the same steps through the checks: records equal bit for bit
def step(order, energy=True, mode="block", uc=0):
    return ("step", order, bool(energy), mode, uc)


def scenario(name: str) -> list[tuple]:
    if name == "tail":
        # (b)-(d), (h): at least 5 consecutive steps with the energy and the monitor's cadence alternating, so that the tail's grid changes
        # from step to step; route switches overlapped -> blocking -> refine = 1 -> overlapped -> GMRES on one handle (the 4-slot ring and
        # both parities of the right-hand side store are cycled)
        return [("opts", dict(refine=0, check=1, method="refine")), step(1, True, "early", 0), step(2, False, "block", 1),
                ("opts", dict(refine=0, check=3, method="refine")), step(2, True, "block", 2), step(2, True, "block", 3), step(2, False, "block", 0),
                step(2, True, "early", 1), step(2, False, "early", 2),
                ("opts", dict(refine=1, check=1, method="refine")), step(2, True, "block", 3),
                ("opts", dict(refine=0, check=0, method="refine")), step(2, True, "early", 0), step(2, False, "early", 2), step(2, True, "block", 1),
                ("opts", dict(refine=30, check=1, method="gmres")), step(2, True, "block", 2),
                ("opts", dict(refine=0, check=1, method="refine")), step(2, True, "early", 3), step(1, True, "block", 0),
                # three steps back to back with nothing in between (the late tail of one runs beside the launches of the next, both
                # parities of the right-hand side store and of the late record in flight), then the same steps one by one through the
                # checks above: bit for bit the same
                ("mark",), ("raw_step", 2, True, 1), ("raw_step", 2, False, 2), ("raw_step", 2, True, 3), ("raw_collect",), ("rewind",),
                step(2, True, "block", 1), step(2, False, "block", 2), step(2, True, "block", 3), ("same_as_raw",)]
    if name == "rhs":
        # (a): both orders, nonlinear on / off, body forces, the explicit operator C; then a step on each order for the route
        ops = []
        for nl in (True, False):
            ops += [("time_scheme", DT, nl, False), ("rhs", 1, 0), ("rhs", 2, 1)]
        ops += [("time_scheme", DT, True, False), ("force", 0), ("rhs", 1, 2), ("rhs", 2, 3), ("cop", 1, True), ("rhs", 1, 0), ("rhs", 2, 1),
                step(1, True, "block", 2), step(1, True, "block", 3), ("force", None), ("cop", 1, False), ("rhs", 1, 0), step(1, True, "block", 1),
                step(2, True, "block", 2)]
        return ops
    if name == "speculate":
        # (f): the invalidation points of the speculated element loop, in the issue's order
        return [("opts", dict(refine=0, check=1, method="refine")), step(1, uc=0), step(2, uc=1), step(2, uc=2), ("set_state", 7, None),
                step(1, uc=3), step(2, uc=0), ("time_scheme", 0.004, True, True), step(2, uc=1), ("undo",), step(2, uc=2), ("batch",),
                step(2, uc=3), ("force", 1), step(2, uc=0), step(2, uc=1), ("force", None), ("cop", 2, True), step(2, uc=2), step(2, uc=3), ("cop", 2, False),
                step(2, uc=0), ("solve_energy",), step(2, uc=1), step(2, True, "early", 2), step(2, True, "early", 3)]
    if name == "nonfinite":
        # (g): on every tail kind this process reaches, with the monitor on, off and between its cadence
        ops = []
        for opts, mode in ((dict(refine=0, check=1, method="refine"), "block"), (dict(refine=0, check=0, method="refine"), "block"),
                           (dict(refine=0, check=3, method="refine"), "block"), (dict(refine=0, check=1, method="refine"), "early"),
                           (dict(refine=1, check=1, method="refine"), "block")):
            ops += [("opts", opts), ("bad_step", 2, mode, "nan_u"), ("set_state", 11, None), step(2, True, mode, 1), ("set_state", 12, "nan_p"),
                    step(2, True, mode, 2), ("bad_step", 2, mode, "inf_ctrl"), ("set_state", 13, None), step(2, False, mode, 3)]
        return ops
    if name == "residual":
        # (e): the monitor on a residual that is not round-off: factors of A0, monitor on A1
        return [("lagged", 2), ("opts", dict(refine=0, check=1, method="refine")), step(2, True, "block", 0), step(2, True, "early", 1),
                step(2, False, "block", 2), ("opts", dict(refine=1, check=1, method="refine")), step(2, True, "block", 3)]
    raise KeyError(name)


SCENARIOS = ("tail", "rhs", "speculate", "nonfinite", "residual")
# runs of a child: (scenario, case, handle knob set, sensor set).  Every child runs the tail scenario on every mesh of the table (a
# sensor set each, so that every set meets every tail kind) and the non-finite flag; the right-hand side does not depend on the process
# knobs and is checked in the default child; the speculation sequence runs in the two children that are compared, and in the one-stream
# form; the residual monitor on the routes the issue names.
_TAIL_RUNS = [("tail", "5x3", "default", "limit64"), ("tail", "9x9", "default", "five"), ("tail", "12x7", "default", "long150"),
              ("tail", "12x11", "reg", "single_entry"), ("tail", "23x12", "default", "one"), ("tail", "12x7", "one_stream", "none")]
RUNS = {
    "default": _TAIL_RUNS + [("rhs", c, hs, "none") for c in CASES for hs in ("default", "reg")]
    + [("speculate", "12x11", "default", "one"), ("speculate", "9x9", "one_stream", "five"), ("nonfinite", "12x7", "default", "one"),
       ("residual", "12x7", "default", "five"), ("residual", "23x12", "default", "one")],
    "fused_final": _TAIL_RUNS + [("nonfinite", "12x7", "default", "one"), ("residual", "12x7", "default", "five"), ("residual", "23x12", "default", "one")],
    "unfused_tail": _TAIL_RUNS + [("nonfinite", "12x7", "default", "one"), ("residual", "12x7", "default", "five")],
    "no_speculate": _TAIL_RUNS + [("speculate", "12x11", "default", "one"), ("speculate", "9x9", "one_stream", "five"), ("nonfinite", "12x7", "default", "one")],
    "reps3": _TAIL_RUNS + [("nonfinite", "23x12", "default", "one"), ("residual", "23x12", "default", "one")],
    "reps3_fused_final": _TAIL_RUNS + [("nonfinite", "23x12", "default", "one"), ("residual", "23x12", "default", "one")],
}


def run_name(run: tuple) -> str:
    return "/".join(run)


def walk(run: tuple, knobs: dict):
    """The steps of a run with their predicted routes, without a device: yields (index of the operation, operation, settings or None,
    route or None).  The child keeps its own History in the same way; this is what census() and the host test read."""
    name, case, hs, _ = run
    kn = {**knobs, **HANDLE_SETS[hs]}
    hist, opts = History(), dict(DEFAULT_OPTS)
    for i, op in enumerate(scenario(name)):
        settings = route = None
        if op[0] == "opts":
            opts = dict(op[1])
        elif op[0] in ("step", "bad_step", "raw_step"):
            order, energy, mode = (op[1], op[2], op[3]) if op[0] == "step" else (op[1], op[2], "early") if op[0] == "raw_step" else (op[1], True, op[2])
            settings = dict(order=order, energy=energy, blocking=mode == "block", **opts)
            route = predicted_route(case, kn, settings, hist)
            advance(hist, route)
        else:
            apply_op(hist, op)
        yield i, op, settings, route


def apply_op(hist: History, op: tuple) -> None:
    """What an operation other than a step does to the History (the invalidation points of the speculated element loop)."""
    kind = op[0]
    if kind in ("set_state", "rewind", "time_scheme", "undo", "batch", "rhs"):  # fc_set_state, fc_set_time_scheme, fc_undo_step, fc_step_batch, enqueue_rhs
        hist.invalidate()
        if kind == "rhs" and hist.have_force:
            hist.fvec_ok = True  # (check_step_ready of fc_assemble_rhs built them)
    elif kind == "force":  # fc_set_force: the load vectors are rebuilt by the next step, with the element vectors as scratch
        hist.have_force, hist.fvec_ok = op[1] is not None, False
    elif kind == "cop":  # fc_set_rhs_operator: the element vectors do not depend on C; the NEXT speculation follows the slot
        hist.have_c[SLOT_BDF1 if op[1] == 1 else SLOT_BDF2] = bool(op[2])
    elif kind in ("solve_energy", "lagged", "opts", "mark", "raw_collect", "same_as_raw"):  # fc_solve, fc_energy, fc_update_operator: none of them touches the element vectors
        pass
    else:
        raise KeyError(kind)


# ── census ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
LABELS = (
    "fc_rhs_elem", "fc_rhs_elem_reg", "elem:reused", "elem:ragged_workgroup", "fc_rhs_gather", "gather:force", "gather:C", "fc_force_rows",
    "fc_tail<false>", "fc_tail<true>", "fc_finish", "fc_final", "fc_early", "fc_wait_solved", "fc_final_late", "late:empty_tail",
    "tail:row_blocks", "tail:check_blocks", "tail:check_ragged", "tail:cell_blocks", "tail:no_energy", "reps>1", "reps:ragged_rows", "reps:ragged_cells",
    "final:single_group", "final:full_groups", "final:ragged_group", "final:group_of_one", "final:partials>256",  # (the last: UNREACHED)
    "sensor:none", "sensor:stride_loop", "sensor:round_robin", "sensor:limit64", "sensor:single_entry",
    "solver:apply", "solver:refine", "solver:gmres", "monitor:cadence_off_step",
    "rowkind", "cell_list", "fc_energy_elem", "fc_publish_tail", "final:fold_beyond_2048", "solver:bicgstab",  # UNREACHED
)
UNREACHED = {
    "rowkind": "the rows of other ranks: partitioned handles need several GPUs (tests/test_partitioned_gpu.py)",
    "cell_list": "a rank's share of the cells: partitioned handles (tests/test_partitioned_gpu.py)",
    "fc_energy_elem": "the energy share of a rank's cells: partitioned handles (tests/test_partitioned_gpu.py)",
    "fc_publish_tail": "the all-reduced tail record: partitioned handles (tests/test_partitioned_gpu.py)",
    "final:fold_beyond_2048": "the strided fold loop of fc_final_body behind its 8 x 256 preloaded partials needs more than 2048 tail workgroups: N > 65536",
    "final:partials>256": "the second preloaded partial of a thread of fc_final_body needs more than 256 tail workgroups, N > 8192: beyond a dense host solve; "
                          "the O1 mesh of tests/test_hip_kernels.py runs it against the fp64 oracle",
    "solver:bicgstab": "the driver is pinned by tests/test_krylov_counts_gpu.py; the step dispatches both Krylov drivers on one line and the tail behind them is the one GMRES meets",
}


def census(runs: list[tuple], knobs: dict) -> set[str]:
    """Labels the steps of ``runs`` reach under the process knobs ``knobs``."""
    out = set()

    def add(cond, label):
        if cond:
            out.add(label)

    for run in runs:
        name, case, hs, sens = run
        nc, N = TABLE[case][:2]
        th = host_case(case)[0]
        rows = sensor_rows(th, sens)
        for _, op, settings, route in walk(run, knobs):
            if op[0] == "rhs":
                out |= {"fc_rhs_gather", "fc_rhs_elem_reg" if "FC_ELEM_REG_MIN" in HANDLE_SETS[hs] else "fc_rhs_elem"}
            if op[0] == "force" and op[1] is not None:
                out.add("fc_force_rows")
            if route is None:
                continue
            r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
            out |= {("elem:reused", "fc_rhs_elem", "fc_rhs_elem_reg")[r["elem"]], "fc_rhs_gather", ("solver:apply", "solver:refine", "solver:bicgstab", "solver:gmres")[r["solver"]]}
            if r["elem"] and (nc % 256 if r["elem"] == ELEM_REG else (8 * nc) % 256):
                out.add("elem:ragged_workgroup")
            g = r["g_rows"] + r["g_check"] + r["g_cells"]
            if r["tail"] == TAIL_OVERLAPPED:
                out |= {"fc_early", "fc_wait_solved", "fc_final_late", "fc_tail<false>" if g else "late:empty_tail"}
            elif r["tail"] == TAIL_FINISH:
                out |= {"fc_finish", "fc_final"}
            elif r["tail"] == TAIL_FUSED:
                out |= {"fc_tail<false>", "fc_final"}
            else:
                out.add("fc_tail<true>")
                ng, last = cdiv(g, GROUP), g % GROUP
                out.add("final:full_groups" if last == 0 else "final:single_group" if ng == 1 else "final:group_of_one" if last == 1 else "final:ragged_group")
            if r["tail"] != TAIL_FINISH:
                add(r["g_rows"], "tail:row_blocks"), add(r["g_check"], "tail:check_blocks"), add(r["g_cells"], "tail:cell_blocks")
                if r["g_check"] and N % TAIL_CHECK_ROWS:
                    out.add("tail:check_ragged")
                if r["reps"] > 1:
                    out.add("reps>1")
                    if r["g_rows"] and cdiv(N, 32) % r["reps"]:
                        out.add("reps:ragged_rows")
                    if r["g_cells"] and cdiv(nc, 32) % r["reps"]:
                        out.add("reps:ragged_cells")
            if not r["g_cells"]:
                out.add("tail:no_energy")
            if g > 256 or (r["tail"] == TAIL_FINISH and r["g_rows"] > 256):
                out.add("final:partials>256")
            if settings["check"] > 1 and not r["monitored"]:
                out.add("monitor:cadence_off_step")
            n_s = len(rows)
            add(n_s == 0, "sensor:none"), add(n_s > 4, "sensor:round_robin"), add(n_s == MAX_SENSORS, "sensor:limit64")
            add(any(len(i) > 64 for i, _ in rows), "sensor:stride_loop"), add(any(len(i) == 1 for i, _ in rows), "sensor:single_entry")
        # the gather's optional terms: a step or a right-hand side while they are switched on
        force = cop = False
        for op in scenario(name):
            if op[0] == "force":
                force = op[1] is not None
            elif op[0] == "cop":
                cop = bool(op[2])
            elif op[0] in ("step", "rhs"):
                add(force, "gather:force"), add(cop, "gather:C")
    return out


# ── the host model in np.longdouble ───────────────────────────────────────────────────────────────────────────────────────────────────
def spmv_longdouble(A, x) -> np.ndarray:
    """A x with products and sums in np.longdouble (every row of A holds an entry)."""
    A = A.tocsr()
    assert np.all(np.diff(A.indptr) > 0)
    return np.add.reduceat(A.data.astype(L) * np.asarray(x, dtype=L)[A.indices], A.indptr[:-1])


class Refined:
    """batch_cases.refined_solve with the LU factors kept: many right-hand sides of one operator, one at a time."""

    def __init__(self, A, sweeps: int = 2):
        import scipy.linalg as sla

        self.A, self.sweeps, self.sla = A.tocsr(), sweeps, sla
        self.lu = sla.lu_factor(self.A.toarray())

    def __call__(self, b: np.ndarray) -> np.ndarray:
        B = np.asarray(b, dtype=np.float64)[None, :]
        X = self.sla.lu_solve(self.lu, B.T).T.astype(L)
        for _ in range(self.sweeps):
            R = bc.residual_longdouble(self.A, X, B)
            X = X + self.sla.lu_solve(self.lu, R.T.astype(np.float64)).T
        return np.asarray(X, dtype=np.float64)[0]


class HostModel:
    """One case in np.longdouble: the element loop of oracle/ns_oracle.py::rhs_transient with the same quadrature tables cast up, the
    gather, the lifting, the Dirichlet rows, the load vectors of the force profiles and the explicit operator; sensors, energy, residual."""

    def __init__(self, case: str):
        from oracle import ns_oracle as O

        self.th, self.dofs, self.prof = host_case(case)
        th = self.th
        self.d = d = O.Disc.from_taylor_hood(th)
        self.nn, self.N = th.nn, th.N
        p = d.coords.astype(L)[d.cells]
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]  # columns of J
        det = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
        Jinv = np.empty((d.nc, 2, 2), dtype=L)  # inverse of [[e1x, e2x], [e1y, e2y]]
        Jinv[:, 0, 0], Jinv[:, 0, 1], Jinv[:, 1, 0], Jinv[:, 1, 1] = e2[:, 1] / det, -e2[:, 0] / det, -e1[:, 1] / det, e1[:, 0] / det
        self.PHI2 = O._PHI2.astype(L)
        self.G2 = np.einsum("qar,crd->cqad", O._DPHI2.astype(L), Jinv)
        self.w = O._QW.astype(L)[None, :] * (det / 2)[:, None]
        self.cn = d.cell_nodes.astype(np.int64)
        Mab = np.einsum("cq,qa,qb->cab", self.w, self.PHI2, self.PHI2)  # the velocity mass matrix of O.velocity_mass, entries in longdouble
        self._m_rows, self._m_cols, self._m_vals = np.repeat(self.cn, 6, axis=1).reshape(-1), np.tile(self.cn, (1, 6)).reshape(-1), Mab.reshape(-1)

    def _at_q(self, u):
        u = np.asarray(u, dtype=L)
        ue = np.stack([u[self.cn], u[self.nn + self.cn]], axis=2)
        return np.einsum("qa,caj->cqj", self.PHI2, ue), np.einsum("cqai,caj->cqij", self.G2, ue)

    def load(self, gq) -> np.ndarray:
        Le = np.einsum("cq,qa,cqj->caj", self.w, self.PHI2, gq)
        b = np.zeros(self.N, dtype=L)
        np.add.at(b, self.cn.reshape(-1), Le[:, :, 0].reshape(-1))
        np.add.at(b, self.nn + self.cn.reshape(-1), Le[:, :, 1].reshape(-1))
        return b

    def rhs(self, order, dt, nonlinear, u_n, u_nn, uc, A_full, fprof=None, uforce=None, Cmat=None) -> np.ndarray:
        """The vector fc_assemble_rhs returns, in longdouble.  ``A_full``: the operator of the slot WITHOUT boundary conditions (its
        Dirichlet columns are the lifting), ``fprof`` (N_ACT, 2 nn) nodal force profiles, ``Cmat`` (N, 2 nn) the explicit operator."""
        dt, nl = L(dt), L(1.0 if nonlinear else 0.0)
        vn, gn = self._at_q(u_n)
        conv = lambda v, g: np.einsum("cqi,cqij->cqj", v, g)
        if order == 1:
            gq = vn / dt - nl * conv(vn, gn)
        else:
            vnn, gnn = self._at_q(u_nn)
            gq = (4 * vn - vnn) / (2 * dt) - 2 * nl * conv(vn, gn) + nl * conv(vnn, gnn)
        uc = np.asarray(uc, dtype=L)
        if fprof is not None:
            gq = gq + self._at_q(np.asarray(uc if uforce is None else uforce, dtype=L) @ np.asarray(fprof, dtype=L))[0]
        b = self.load(gq)
        if Cmat is not None:
            b = b - spmv_longdouble(Cmat, np.asarray(u_n, dtype=L))
        g = np.zeros(self.N, dtype=L)
        g[self.dofs] = self.prof.astype(L) @ uc
        b = b - spmv_longdouble(A_full, g)
        b[self.dofs] = g[self.dofs]
        return b

    def energy(self, u) -> np.longdouble:
        """1/2 u^T M u."""
        u = np.asarray(u, dtype=L)
        return sum(L(0.5) * np.sum(u[o + self._m_rows] * self._m_vals * u[o + self._m_cols]) for o in (0, self.nn))

    @staticmethod
    def sensors(rows, x):
        """(y_s, its bound 2 (n_s + 6) eps sum_k |w_k x_k|) per row: a 64-lane partial plus a 6-level shuffle tree, times 2."""
        y = np.array([np.sum(np.asarray(w, dtype=L) * np.asarray(x, dtype=L)[i]) for i, w in rows], dtype=L)
        bound = np.array([2 * (len(i) + 6) * EPS * np.sum(np.abs(np.asarray(w, dtype=L) * np.asarray(x, dtype=L)[i])) for i, w in rows], dtype=L)
        return y, bound

    @staticmethod
    def residual(A, x, b):
        """(|b - A x|_2, |b|_2, bound of the monitor's |r|_2): 2 (L + 2) eps | |b| + |A| |x| |_2 with L the longest row -- the running
        error bound of the row sums, times 2."""
        A = A.tocsr()
        r = np.asarray(b, dtype=L) - spmv_longdouble(A, x)
        longest = int(np.diff(A.indptr).max())
        mag = np.abs(np.asarray(b, dtype=L)) + spmv_longdouble(abs(A), np.abs(np.asarray(x, dtype=L)))
        nrm = lambda v: np.sqrt(np.sum(v * v))
        return nrm(r), nrm(np.asarray(b, dtype=L)), 2 * (longest + 2) * EPS * nrm(mag)


def rel2(a, ref) -> float:
    a, ref = np.asarray(a, dtype=L), np.asarray(ref, dtype=L)
    return float(np.sqrt(np.sum((a - ref) ** 2) / np.sum(ref**2)))


def relmax(a, ref) -> float:
    a, ref = np.asarray(a, dtype=L), np.asarray(ref, dtype=L)
    return float(np.abs(a - ref).max() / np.abs(ref).max())
