"""Runs, route model, census and the host model (np.longdouble) of ONE step of the tangent-linear march, single and batched: the element
loops fc_tan_elem_nl / fc_tan_elem_nl_reg / fc_tan_elem_nl_b<KB, SHARED>, the forward step's gathers with the control columns
(fc_rhs_gather, fc_rhs_gather_b<KB>, fc_tan_force_b<KB>) and the tails fc_tan_tail / fc_tan_tail_b<KB> (dispatched by tan_enqueue_step /
tanb_enqueue_step of csrc/fc_tangent_run.hpp).  No GPU import: tests/test_tangent_march_cases_host.py runs everything here on the host,
tests/test_tangent_march_gpu.py and tests/support/tangent_march_child.py run it against the device.

  TABLE                         the meshes and the launch geometry each one reaches
  SINGLE_RUNS / BATCH_RUNS      the runs, as data: the child executes them, walk_single / walk_batch predict the route of every step
  predicted_route               host model of the dispatch: what fc_get_tangent_route must report
  census / LABELS / UNREACHED   the kernel instances and loop trips a set of runs reaches
  TangentMarchModel             one function per kernel in np.longdouble: elem_part, rhs, tail

Actuator sets, force sets, sensor sets and the control columns are those of tests/support/adjoint_march_cases.py."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2
from tests.support import adjoint_march_cases as mc
from tests.support import step_cases as sc

L = np.longdouble
EPS = sc.EPS
DT = sc.DT
cdiv, kb_of, run_name, rel2, relmax = mc.cdiv, mc.kb_of, mc.run_name, mc.rel2, mc.relmax

# ── meshes ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
# The five edge meshes of the step tests.  No tangent kernel has a grid cap or a grid-stride loop (every launch is sized by its rows,
# cells or (row, column) pairs), so the two large squares of the adjoint table would add no path.
MESHES = dict(sc.CASES)
TABLE = {m: mc.TABLE[m] for m in MESHES}  # mesh -> (cells, unknowns)
N_ACT = (0, 1, 5, 9)
KBS = mc.KBS
SENSOR_SETS = mc.SENSOR_SETS
HANDLE_SETS, HANDLE_KNOBS = mc.HANDLE_SETS, mc.HANDLE_KNOBS
ELEM_REG_MIN = sc.ELEM_REG_MIN

# Largest relative distance of an fp64 numpy evaluation of TangentMarchModel.rhs (the same expression, every table and operand rounded
# to fp64) from the np.longdouble one, 2-norm / max-norm over the velocity rows, of a step with both tangent levels, both taped states
# and two actuators; measured per mesh and first order by tests/test_tangent_march_cases_host.py::test_host_constants, which asserts that
# these constants bound what it measures and exceed it by less than a factor of two.
#            order 1 (BDF1 step)       order 2 (BDF2 step)
#   5x3      1.76e-16 / 2.29e-16       1.83e-16 / 3.02e-16
#   9x9      1.37e-16 / 3.09e-16       1.37e-16 / 2.86e-16
#   12x7     1.39e-16 / 2.69e-16       1.42e-16 / 1.93e-16
#   12x11    1.25e-16 / 2.51e-16       1.49e-16 / 2.63e-16
#   23x12    1.08e-16 / 2.37e-16       1.35e-16 / 3.18e-16
# (above the adjoint marches' constant: the tangent levels of the runs are random on every row, so the mass term cancels between nodes)
HOST_TAN_RHS_ERROR = (1.84e-16, 3.19e-16)

host_case, profiles, force_set, sensor_rows = mc.host_case, mc.profiles, mc.force_set, mc.sensor_rows

# ── runs, as data ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
# A single run: (mesh, n_act, variant, sensor set, handle set, first order, refine, steps, (du, dx0, dxm1 given)).  The handles are
# nonlinear (the march refuses linearised ones).  fc_run_tangent over a taped forward run of `steps` steps and of every shorter length,
# so that the last step of each is seen.
SINGLE_RUNS = [
    ("5x3", 0, "dirichlet", "none", "default", 1, 0, 3, (False, True, True)),
    ("5x3", 1, "dirichlet", "single_entry", "reg", 2, 1, 2, (True, True, False)),
    ("9x9", 5, "mixed", "five", "default", 2, 0, 3, (True, True, True)),
    ("12x7", 9, "dirichlet", "long150", "default", 1, 1, 3, (True, True, True)),
    ("12x7", 1, "mixed", "one", "default", 2, 1, 2, (True, False, True)),
    ("12x11", 5, "mixed", "limit64", "default", 2, 0, 2, (True, True, True)),
    ("23x12", 9, "mixed", "on_dirichlet", "reg", 1, 0, 3, (True, True, True)),
    ("23x12", 9, "mixed", "on_dirichlet", "default", 1, 0, 3, (True, True, True)),
]
# A batched run: (mesh, k, n_act, variant, sensor set, first order, steps, ref_col).  Column k - 1 has zero inputs; columns 0 and k - 2
# are equal (k >= 3), their trajectories included.
BATCH_RUNS = [
    ("5x3", 3, 5, "mixed", "one", 1, 3, -1),
    ("5x3", 3, 1, "dirichlet", "none", 2, 2, 2),
    ("9x9", 5, 9, "mixed", "five", 2, 3, 0),
    ("12x7", 5, 0, "dirichlet", "on_dirichlet", 1, 2, -1),
    ("12x7", 9, 5, "mixed", "single_entry", 1, 3, -1),
    ("9x9", 9, 1, "dirichlet", "one", 2, 2, 8),
    ("12x11", 17, 5, "dirichlet", "limit64", 2, 2, -1),
    ("5x3", 32, 5, "mixed", "long150", 1, 3, 0),
]


def step_coeffs(order: int, dt: float = DT):
    """(cm_n, cm_nn, cc_n, cc_nn) of a forward step of ``order`` on a nonlinear handle (coeffs_for)."""
    return (1.0 / dt, 0.0, -1.0, 0.0) if order == 1 else (2.0 / dt, -0.5 / dt, -2.0, 1.0)


def order_of(j: int, first: int) -> int:
    return first if j == 1 else 2


# ── route model ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
ROUTE_COLS = ("elem", "g_elem", "g_gather", "KB", "k", "ref_col", "force_b", "fvec", "refined", "g_tail", "l1", "l2", "t2", "slot")  # DeviceSolver.TAN_ROUTE_COLS
ELEM_LANES, ELEM_REG, ELEM_B, ELEM_B_SHARED = 1, 2, 3, 4


def predicted_route(mesh: str, n_act: int, variant: str, knobs: dict, order: int, refine: int = 0, k: int = 0, ref_col: int = -1) -> np.ndarray:
    """What fc_get_tangent_route must report for a step of ``order`` on a handle of ``mesh`` created under the handle knobs ``knobs``;
    ``k`` > 0: a batched step of k columns.  The conditions are those of tan_enqueue_step, tanb_enqueue_step and launch_elem_on's rule."""
    nc, N = TABLE[mesh]
    c = step_coeffs(order)
    gate = [int(c[2] != 0), int(c[3] != 0), int(c[3] != 0 or c[1] != 0)]
    slot = SLOT_BDF1 if order == 1 else SLOT_BDF2
    force = int(variant == "mixed" and n_act > 0)  # (fc_set_force is called with profiles only)
    if k:
        KB = kb_of(k)
        return np.array([ELEM_B_SHARED if ref_col >= 0 else ELEM_B, cdiv(nc, 256 // KB), cdiv(N * (KB // 2), 256), KB, k, ref_col, force, 0, 0, cdiv(N * KB, 256),
                         *gate, slot], dtype=np.int32)
    reg_min = int(knobs.get("FC_ELEM_REG_MIN", ELEM_REG_MIN))
    reg = reg_min > 0 and nc >= reg_min
    return np.array([ELEM_REG if reg else ELEM_LANES, cdiv(nc, 256) if reg else cdiv(8 * nc, 256), cdiv(N, 256), 0, 0, -1, 0, force, int(refine > 0), cdiv(N, 256),
                     *gate, slot], dtype=np.int32)


def walk_single(run: tuple):
    """The steps of a single run the child looks at: yields (n of the march, order of its last step, route)."""
    mesh, n_act, variant, _, hs, first, refine, steps, _ = run
    for n in range(1, steps + 1):
        o = order_of(n, first)
        yield n, o, predicted_route(mesh, n_act, variant, HANDLE_SETS[hs], o, refine)


def walk_batch(run: tuple):
    mesh, k, n_act, variant, _, first, steps, ref_col = run
    for n in range(1, steps + 1):
        o = order_of(n, first)
        yield n, o, predicted_route(mesh, n_act, variant, {}, o, 0, k=k, ref_col=ref_col)


# ── census ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
LABELS = (
    "fc_tan_elem_nl", "fc_tan_elem_nl_reg", *(f"fc_tan_elem_nl_b<{kb},{s}>" for kb in KBS for s in ("false", "true")),
    "elem:ragged_workgroup", "elem:one_workgroup", "elem:several_workgroups", "elem_reg:several_workgroups",
    "fc_rhs_gather", "gather:fvec", "gather:no_fvec", "gather:n_act=0", *(f"fc_rhs_gather_b<{kb}>" for kb in KBS), *(f"fc_tan_force_b<{kb}>" for kb in KBS),
    "force_b:not_launched",
    "fc_tan_tail", "fc_tan_tail:wave_second_trip", "fc_tan_tail:lane_second_trip", "fc_tan_tail:no_sensors", "fc_tan_tail:dx", "fc_tan_tail:no_dx",
    *(f"fc_tan_tail_b<{kb}>" for kb in KBS), "fc_tan_tail_b:several_sensors", "fc_tan_tail_b:no_sensors",
    "batch:padding_columns", "batch:full_width", "ref_col:none", "ref_col:first", "ref_col:last",
    "gate:bdf1", "gate:bdf2", "gate:bdf2_first_step", "given:all", "given:no_du", "given:no_dx0", "given:no_dxm1",
    "gate:cc_n=0", "gate:cm_nn_without_cc_nn", "rows:partitioned", "tape:checkpointed",  # UNREACHED
)
UNREACHED = {
    "gate:cc_n=0": "cc_n == 0 (l1 off: the taped state x1 is not loaded) is a linearised handle's coefficient set, and the march refuses linearised handles",
    "gate:cm_nn_without_cc_nn": "cm_nn != 0 with cc_nn == 0 (t2 on, l2 off) is the BDF2 step of a linearised handle, which the march refuses",
    "rows:partitioned": "both marches and fc_tangent_reserve refuse partitioned handles before anything else (tests/test_tangent_gpu.py holds the refusals)",
    "tape:checkpointed": "a tangent march over a checkpointed state tape is refused by design (tests/test_tangent_gpu.py holds the refusal)",
}


def census(single: list[tuple], batch: list[tuple]) -> set[str]:
    """Labels the steps of the runs reach."""
    out = set()

    def add(cond, label):
        if cond:
            out.add(label)

    def gates(n, first, r):
        g = (r["l1"], r["l2"], r["t2"])
        assert g in ((1, 0, 0), (1, 1, 1)), g
        out.add("gate:bdf1" if g == (1, 0, 0) else "gate:bdf2_first_step" if n == 1 else "gate:bdf2")

    for run in single:
        mesh, n_act, variant, sens, hs, first, refine, steps, given = run
        nc, N = TABLE[mesh]
        th, dofs = host_case(mesh)
        rows = sensor_rows(th, dofs, sens)
        add(all(given), "given:all")
        for g, name in zip(given, ("du", "dx0", "dxm1")):
            add(not g, f"given:no_{name}")
        for n, _, route in walk_single(run):
            r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
            reg = r["elem"] == ELEM_REG
            out |= {"fc_tan_elem_nl_reg" if reg else "fc_tan_elem_nl", "fc_rhs_gather", "fc_tan_tail", "gather:fvec" if r["fvec"] else "gather:no_fvec",
                    "fc_tan_tail:dx" if r["refined"] else "fc_tan_tail:no_dx"}
            add(nc % (256 if reg else 32), "elem:ragged_workgroup"), add(r["g_elem"] == 1, "elem:one_workgroup")
            add(r["g_elem"] > 1, "elem_reg:several_workgroups" if reg else "elem:several_workgroups")
            add(n_act == 0, "gather:n_act=0"), add(not rows, "fc_tan_tail:no_sensors"), add(len(rows) > 4, "fc_tan_tail:wave_second_trip")
            add(any(len(i) > 64 for i, _ in rows), "fc_tan_tail:lane_second_trip")
            gates(n, first, r)
    for run in batch:
        mesh, k, n_act, variant, sens, first, steps, ref_col = run
        nc, N = TABLE[mesh]
        th, dofs = host_case(mesh)
        rows = sensor_rows(th, dofs, sens)
        for n, _, route in walk_batch(run):
            r = dict(zip(ROUTE_COLS, (int(v) for v in route)))
            KB = r["KB"]
            out |= {f"fc_tan_elem_nl_b<{KB},{'true' if r['elem'] == ELEM_B_SHARED else 'false'}>", f"fc_rhs_gather_b<{KB}>", f"fc_tan_tail_b<{KB}>",
                    f"fc_tan_force_b<{KB}>" if r["force_b"] else "force_b:not_launched"}
            add(k < KB, "batch:padding_columns"), add(k == KB, "batch:full_width"), add(nc % (256 // KB), "elem:ragged_workgroup")
            add(ref_col < 0, "ref_col:none"), add(ref_col == 0, "ref_col:first"), add(ref_col == k - 1, "ref_col:last")
            add(n_act == 0, "gather:n_act=0"), add(len(rows) > 1, "fc_tan_tail_b:several_sensors"), add(not rows, "fc_tan_tail_b:no_sensors")
            gates(n, first, r)
    return out


# ── the refined host solve on the untransposed operator ──────────────────────────────────────────────────────────────────────────────
class Refined(mc.RefinedT):
    """A^-1 b by adjoint_march_cases.RefinedT's scheme (sparse LU in fp64, refinements with the residual and the iterate in
    np.longdouble) on the untransposed operator."""

    def __init__(self, A, sweeps: int = 2):
        import scipy.sparse.linalg as spla

        self.A = sp.csr_matrix(A)
        self.A.sort_indices()
        self.lu, self.sweeps = spla.splu(sp.csc_matrix(A)), sweeps

    def __call__(self, b, longdouble: bool = False):
        b = np.asarray(b, dtype=L)
        x = self.lu.solve(np.asarray(b, dtype=np.float64)).astype(L)
        for _ in range(self.sweeps):
            r = b - sc.spmv_longdouble(self.A, x)
            x = x + self.lu.solve(np.asarray(r, dtype=np.float64))
        return x if longdouble else np.asarray(x, dtype=np.float64)


def lagged_operator(mesh: str):
    """The BDF2 operator A1 of step_cases.operator_args(lagged=True) with the Dirichlet rows eliminated, from the numpy oracle: behind
    the factors of A0 (update_operator) one refinement sweep returns a correction dx that is no rounding effect."""
    from oracle import ns_oracle as O

    th, dofs = host_case(mesh)
    free = np.ones(th.N)
    free[dofs] = 0.0
    Zf, Zd = sp.diags(free), sp.diags(1.0 - free)
    return (Zf @ O.assemble_matrix(O.Disc.from_taylor_hood(th), **sc.operator_args(th, 2, lagged=True)).tocsr() @ Zf + Zd).tocsr()


# ── the host model, one function per kernel ──────────────────────────────────────────────────────────────────────────────────────────
WRONG = ("drop_ud", "nn_d1", "mask_d", "own_trajectory", "fvec", "no_dx", "first_weight")


class TangentMarchModel(mc.MarchModel):
    """One (mesh, actuator set, sensor set) in np.longdouble, W numbering, on step_cases.HostModel's quadrature tables (the oracle's,
    cast up).  ``A_full``: {order: the slot's operator WITHOUT boundary conditions}, the device's own (the child) or the oracle's."""

    # fc_tan_elem_nl / _reg / _b ------------------------------------------------------------------------------------------------------
    def elem_part(self, d1, d2, x1, x2, coeffs, T=L, wrong=None):
        """(ev [12][nc], their row sums [N]): per cell and point  w (zeta_m + sum_l cc_l ((d_l . grad) u_l + (u_l . grad) d_l))  tested
        with phi_a; zeta_m = cm_n d1 + cm_nn d2, u_l the velocity of x_l.  Both tangent levels are read UNMASKED.  ev[a] / ev[6 + a]:
        the x / y share of local node a, as the device lays them out.
        ``wrong``: "drop_ud" (u . grad) d left out; "nn_d1" the cc_nn term fed d1; "mask_d" Dirichlet rows of d zeroed."""
        hm = self.hm
        cm_n, cm_nn, cc_n, cc_nn = (T(c) for c in coeffs)
        nn2 = 2 * self.nn
        d1, d2 = (np.asarray(d, dtype=T)[:nn2] for d in (d1, d2))
        if wrong == "mask_d":
            d1, d2 = (np.where(self.free[:nn2], d, T(0)) for d in (d1, d2))
        w, PHI = hm.w.astype(T), hm.PHI2.astype(T)
        g = self._at_q(cm_n * d1 + cm_nn * d2, T)[0]
        for cc, x, d in ((cc_n, x1, d1), (cc_nn, x2, d1 if wrong == "nn_d1" else d2)):
            if cc == 0:
                continue
            uq, gu = self._at_q(np.asarray(x, dtype=T)[:nn2], T)  # gu[c, q, i, j] = d_i u_j
            dq, gd = self._at_q(d, T)
            conv = np.einsum("cqi,cqij->cqj", dq, gu)
            if wrong != "drop_ud":
                conv = conv + np.einsum("cqi,cqij->cqj", uq, gd)
            g = g + cc * conv
        Le = np.einsum("cq,qa,cqj->caj", w, PHI, g)
        ev = np.concatenate([Le[:, :, 0].T, Le[:, :, 1].T], axis=0)
        rows = np.zeros(self.N, dtype=T)
        np.add.at(rows, hm.cn.reshape(-1), Le[:, :, 0].reshape(-1))
        np.add.at(rows, self.nn + hm.cn.reshape(-1), Le[:, :, 1].reshape(-1))
        return ev, rows

    def gather(self, ev, T=L):
        """Row sums of given element vectors [12][nc] (the gather's first half, on the device's own ev)."""
        hm = self.hm
        ev = np.asarray(ev, dtype=T)
        rows = np.zeros(self.N, dtype=T)
        np.add.at(rows, hm.cn.T.reshape(-1), ev[:6].reshape(-1))
        np.add.at(rows, self.nn + hm.cn.T.reshape(-1), ev[6:].reshape(-1))
        return rows

    def touched(self) -> np.ndarray:
        """Rows some cell contributes to (every velocity row of these meshes; no pressure row)."""
        t = np.zeros(self.N, dtype=bool)
        t[self.hm.cn.reshape(-1)] = t[self.nn + self.hm.cn.reshape(-1)] = True
        return t

    # fc_rhs_gather / fc_rhs_gather_b + fc_tan_force_b --------------------------------------------------------------------------------
    def rhs(self, rows, du, order, T=L, wrong=None, lift=None, fvec=None):
        """The right-hand side on every row from the element row sums: the profile times du on a Dirichlet row; elsewhere the row sum
        - lift du + fvec du.  ``lift`` / ``fvec`` [n_act][N]: the device's own operands (default: the model's, in longdouble).
        ``wrong="fvec"``: the load vectors dropped."""
        b = np.array(rows, dtype=T)
        du = np.zeros(self.n_act, dtype=T) if du is None else np.asarray(du, dtype=T)
        _, ml, mf, _ = self.control_columns(order)
        lift = ml if lift is None else lift
        fvec = (mf if self.fprof is not None else None) if fvec is None else fvec
        if self.n_act:
            b = b - du @ np.asarray(lift, dtype=T)
            if fvec is not None and wrong != "fvec":
                b = b + du @ np.asarray(fvec, dtype=T)
        b[self.dofs] = self.prof.astype(T) @ du if self.n_act else T(0)
        return b

    def dirichlet_bound(self, du):
        """(n_act + 2) eps sum |prof| |du| per Dirichlet dof: an fp64 sum of n_act products in any order."""
        du = np.zeros(self.n_act) if du is None else np.asarray(du, dtype=L)
        return (self.n_act + 2) * EPS * (np.abs(self.prof.astype(L)) @ np.abs(du))

    # fc_tan_tail / fc_tan_tail_b ------------------------------------------------------------------------------------------------------
    def tail(self, x, dx=None, wrong=None):
        """(new level, dy, bound): the level is x + dx in fp64 (ONE add: bit for bit) or x; dy_s = C_s . (x + dx) in longdouble on that
        fp64 level; bound_s = (entries + 2) eps sum |c| |x + dx|, an fp64 sum of the entries' products in any order.
        ``wrong``: "no_dx" the sensors read x; "first_weight" a sensor row takes its first weight throughout."""
        x = np.asarray(x, dtype=np.float64)
        lev = x if dx is None else x + np.asarray(dx, dtype=np.float64)
        seen = x if wrong == "no_dx" else lev
        dy, bound = np.zeros(len(self.rows), dtype=L), np.zeros(len(self.rows), dtype=L)
        for s, (idx, w) in enumerate(self.rows):
            c = np.full(len(w), w[0], dtype=L) if wrong == "first_weight" else np.asarray(w, dtype=L)
            prod = c * seen[idx].astype(L)
            dy[s], bound[s] = prod.sum(), (len(idx) + 2) * EPS * np.abs(prod).sum()
        return lev, dy, bound


def host_march(model: TangentMarchModel, solve: dict, first: int, X, du=None, dx0=None, dxm1=None):
    """The whole march through the functions above, in longdouble: (D [n + 2][N] = dx_{-1}, dx_0, .. dx_n; dy [n][n_sens]).
    ``solve``: {order: Refined}; ``X`` [n + 2][N]: the forward states x_{-1}, x_0, .. x_n."""
    n, N = X.shape[0] - 2, model.N
    zero = np.zeros(N, dtype=L)
    D = [zero if dxm1 is None else np.asarray(dxm1, dtype=L), zero if dx0 is None else np.asarray(dx0, dtype=L)]
    dys = np.zeros((n, len(model.rows)), dtype=L)
    for j in range(1, n + 1):
        o = order_of(j, first)
        _, rows = model.elem_part(D[-1], D[-2], X[j], X[j - 1], step_coeffs(o))
        b = model.rhs(rows, None if du is None else du[j - 1], o)
        x = solve[o](b, longdouble=True)
        D.append(x)
        dys[j - 1] = np.array([np.sum(np.asarray(w, dtype=L) * x[i]) for i, w in model.rows], dtype=L)
    return np.array(D), dys


def inputs(N: int, n_act: int, steps: int, seed: int, k: int = 0):
    """(du [steps][n_act], dx0 [N], dxm1 [N]) or their batched forms ([steps][k][n_act], [k][N]): random on EVERY row, the Dirichlet and
    the pressure rows included (the levels are read unmasked, the pressure rows are the caller's); batched: column k - 1 all zero, column
    k - 2 a copy of column 0 (k >= 3)."""
    rng = np.random.default_rng(seed)
    if not k:
        return rng.standard_normal((steps, n_act)), rng.standard_normal(N), rng.standard_normal(N)
    du, d0, dm1 = rng.standard_normal((steps, k, n_act)), rng.standard_normal((k, N)), rng.standard_normal((k, N))
    du[:, k - 1], d0[k - 1], dm1[k - 1] = 0.0, 0.0, 0.0
    if k >= 3:
        du[:, k - 2], d0[k - 2], dm1[k - 2] = du[:, 0], d0[0], dm1[0]
    return du, d0, dm1
