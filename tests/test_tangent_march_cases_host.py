"""Host side of tests/test_tangent_march_gpu.py (no GPU): the runs of tests/support/tangent_march_cases.py reach every label outside
UNREACHED, the mesh table holds, the np.longdouble model of a tangent step agrees with the fp64 scipy model of the whole march
(tests/support/tangent_model.py), every seeded model mistake moves the quantity it touches by at least 1000 x that quantity's tolerance in
the GPU test, and the host constant the GPU test's tolerance stands on is re-measured."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import adjoint_march_cases as mc
from tests.support import step_cases as sc
from tests.support import tangent_march_cases as tc
from tests.support.adjoint_nl_model import NonlinearStepModel
from tests.support.tangent_model import TangentModel

L = np.longdouble


@pytest.fixture(scope="module")
def ops():
    """Per mesh the oracle's operators, assembled once and left unchanged."""
    cache = {}

    def get(mesh):
        if mesh not in cache:
            cache[mesh] = mc.host_operators(mesh)
        return cache[mesh]

    return get


def test_the_runs_reach_every_label_outside_unreached():
    reached = tc.census(tc.SINGLE_RUNS, tc.BATCH_RUNS)
    assert reached <= set(tc.LABELS), reached - set(tc.LABELS)
    assert set(tc.UNREACHED) <= set(tc.LABELS)
    missing = set(tc.LABELS) - set(tc.UNREACHED) - reached
    assert not missing, f"no run reaches {sorted(missing)}"
    assert not reached & set(tc.UNREACHED)
    assert all(len(why) > 20 for why in tc.UNREACHED.values())
    print(f"{len(reached)} of {len(tc.LABELS)} labels reached, {len(tc.UNREACHED)} unreached with a reason")
    # the sets the runs must cover between them
    S, B = tc.SINGLE_RUNS, tc.BATCH_RUNS
    assert {r[1] for r in S} == set(tc.N_ACT) and {r[2] for r in S} == {"dirichlet", "mixed"}
    assert {r[3] for r in S} >= {"none", "one", "five", "long150", "limit64", "single_entry", "on_dirichlet"}
    assert {r[6] for r in S} == {0, 1} and {r[5] for r in S} == {1, 2} and all(r[7] <= 3 for r in S) and all(r[6] <= 3 for r in B)
    assert ("5x3", "default") in {(r[0], r[4]) for r in S} and ("23x12", "reg") in {(r[0], r[4]) for r in S}
    assert {r[1] for r in B} == {3, 5, 9, 17, 32} and {tc.kb_of(r[1]) for r in B} == set(tc.KBS)
    assert {(-1 if r[7] < 0 else 0 if r[7] == 0 else "last") for r in B if r[7] in (-1, 0, r[1] - 1)} == {-1, 0, "last"}
    assert all(r[7] in (-1, 0, r[1] - 1) for r in B)
    assert sum(r[2] == 0 for r in B) == 1 and len({tc.kb_of(r[1]) for r in B if r[3] == "mixed"}) >= 2 and any(r[4] in ("five", "limit64") for r in B)
    assert any(r[1] == tc.kb_of(r[1]) for r in B)
    assert set(tc.MESHES) == {r[0] for r in S}


def test_no_handle_set_is_redundant():
    full = tc.census(tc.SINGLE_RUNS, tc.BATCH_RUNS)
    for hs in tc.HANDLE_SETS:
        rest = tc.census([r for r in tc.SINGLE_RUNS if r[4] != hs], tc.BATCH_RUNS)
        assert full - rest, f"handle set {hs!r} reaches nothing of its own"
        print(f"only under handle set {hs!r}: {sorted(full - rest)}")
    assert full - tc.census([], tc.BATCH_RUNS) and full - tc.census(tc.SINGLE_RUNS, [])


def test_the_mesh_table_holds():
    """cells, N and the grids of every launch."""
    for mesh, (nc, N) in tc.TABLE.items():
        th, _ = tc.host_case(mesh)
        assert (th.mesh.cells.shape[0], th.N) == (nc, N), mesh
    r = lambda *a, **k: dict(zip(tc.ROUTE_COLS, (int(v) for v in tc.predicted_route(*a, **k))))  # noqa: E731
    # eight lanes per cell: 5x3 is ONE ragged workgroup (30 cells of 32); 9x9 six, the last one with two cells; 23x12 eighteen
    a = r("5x3", 0, "dirichlet", {}, 1)
    assert (a["elem"], a["g_elem"], a["g_gather"], a["g_tail"], a["fvec"], a["refined"], a["l1"], a["l2"], a["t2"]) == (1, 1, 1, 1, 0, 0, 1, 0, 0)
    assert r("9x9", 5, "mixed", {}, 2)["g_elem"] == 6 and 162 % 32 == 2 and r("23x12", 9, "mixed", {}, 2)["g_elem"] == 18
    # a thread per cell on 23x12: three workgroups, the last one with 40 cells
    b = r("23x12", 9, "mixed", {"FC_ELEM_REG_MIN": "1"}, 2, 1)
    assert (b["elem"], b["g_elem"], b["g_gather"], b["g_tail"], b["fvec"], b["refined"], b["l1"], b["l2"], b["t2"]) == (2, 3, 11, 11, 1, 1, 1, 1, 1) and 552 - 512 == 40
    assert r("5x3", 1, "dirichlet", {"FC_ELEM_REG_MIN": "1"}, 2)["g_elem"] == 1
    # batched: cells per workgroup 256 / KB, row pairs and (row, column) threads
    c = r("12x11", 5, "dirichlet", {}, 2, k=17, ref_col=-1)
    assert (c["elem"], c["g_elem"], c["g_gather"], c["KB"], c["k"], c["ref_col"], c["force_b"], c["g_tail"]) == (3, 33, 82, 32, 17, -1, 0, 164)
    d = r("5x3", 5, "mixed", {}, 1, k=32, ref_col=0)
    assert (d["elem"], d["g_elem"], d["KB"], d["force_b"], d["fvec"]) == (4, 4, 32, 1, 0) and 30 % 8 == 6
    assert r("12x7", 0, "mixed", {}, 1, k=9)["force_b"] == 0  # (no actuators: no profiles are set)
    assert r("9x9", 1, "dirichlet", {}, 2, k=9, ref_col=8)["g_elem"] == mc.cdiv(162, 16)
    # the sensor sets are what the tail's loops need
    th, dofs = tc.host_case("12x7")
    assert len(tc.sensor_rows(th, dofs, "five")) == 5 and len(tc.sensor_rows(th, dofs, "long150")[0][0]) == 150 and len(tc.sensor_rows(th, dofs, "limit64")) == 64


def _scipy_model(mesh, n_act, variant, sens, ops):
    from oracle import ns_oracle as O

    full, bc, M = ops(mesh)
    m = tc.TangentMarchModel(mesh, n_act, variant, sens, full)
    G = np.zeros((m.N, n_act))
    G[m.dofs] = m.prof
    C = sp.lil_matrix((len(m.rows), m.N))
    for s, (idx, w) in enumerate(m.rows):
        for i, v in zip(idx, w):
            C[s, i] += v
    F = None
    if m.fprof is not None:
        F = np.stack([np.asarray(m.control_columns(1)[2][k], dtype=float) for k in range(n_act)], axis=1)
    model = NonlinearStepModel(O.Disc.from_taylor_hood(m.th), bc[1], bc[2], M, m.dofs, m.prof, full[1] @ G, full[2] @ G, C.tocsr(), tc.DT, F=F)
    return m, model, {o: tc.Refined(bc[o]) for o in (1, 2)}


def _trajectory(m, model, first, n, seed=5, state=1):
    u_n, u_nn, p = sc.initial_state(m.th, state)
    u = np.random.default_rng(seed).standard_normal((n, m.n_act)) * 0.1
    X, _ = model.forward(first, u, np.r_[u_n, p], np.r_[u_nn, p])
    return X


@pytest.mark.parametrize("mesh,n_act,variant,sens,first", [
    ("5x3", 5, "mixed", "five", 1), ("9x9", 1, "dirichlet", "on_dirichlet", 2), ("12x7", 9, "mixed", "long150", 1), ("23x12", 5, "mixed", "limit64", 2)])
def test_longdouble_model_against_the_fp64_scipy_model(mesh, n_act, variant, sens, first, ops):
    """One march of three steps through TangentMarchModel's per-kernel functions against tangent_model.TangentModel: relative."""
    m, model, solve = _scipy_model(mesh, n_act, variant, sens, ops)
    X = _trajectory(m, model, first, 3)
    du, d0, dm1 = tc.inputs(m.N, n_act, 3, 3)
    D, dy = tc.host_march(m, solve, first, X, du, d0, dm1)
    Dm, dym = TangentModel(model).tangent(first, X, du, d0, dm1)
    nn2 = 2 * m.nn
    ex, ey = tc.rel2(D[2:], Dm[2:]), tc.rel2(dy, dym)
    print(f"{mesh} n_act {n_act} {variant} {sens} first order {first}: dx {ex:.3e}, dy {ey:.3e} relative to the fp64 scipy model")
    assert ex <= 1e-10 and ey <= 1e-10 and np.any(D[2:, :nn2])


def test_every_seeded_mistake_is_visible(ops):
    """Each seeded model mistake moves the quantity it touches by at least 1000 x that quantity's tolerance in the GPU test, on the
    inputs the GPU test uses (tc.inputs, sc.initial_state trajectories)."""
    mesh = "12x7"
    m, model, solve = _scipy_model(mesh, 5, "mixed", "five", ops)
    X = _trajectory(m, model, 2, 2)
    X_other = _trajectory(m, model, 2, 2, state=2)  # (another column of a batch: sc.initial_state(th, 1 + s))
    du, d0, dm1 = tc.inputs(m.N, 5, 2, 7)
    nn2 = 2 * m.nn
    tol = 16 * tc.HOST_TAN_RHS_ERROR[1]
    for order in (1, 2):
        c = tc.step_coeffs(order)
        ev, rows = m.elem_part(d0, dm1, X[1], X[0], c)
        for wrong in ("drop_ud", "nn_d1", "mask_d"):
            if wrong == "nn_d1" and order == 1:
                continue  # (a BDF1 step has no cc_nn term)
            evw, rw = m.elem_part(d0, dm1, X[1], X[0], c, wrong=wrong)
            ratio = tc.relmax(rw[:nn2], rows[:nn2]) / tol
            re = tc.relmax(evw, ev) / tol
            print(f"order {order} {wrong}: b moves by {ratio:.2e} x, ev by {re:.2e} x the max-norm tolerance")
            assert ratio >= 1000 and re >= 1000
        # SHARED ignored: the column reads its own trajectory instead of ref_col's
        _, ro = m.elem_part(d0, dm1, X_other[1], X_other[0], c)
        ratio = tc.relmax(ro[:nn2], rows[:nn2]) / tol
        print(f"order {order} own trajectory: b moves by {ratio:.2e} x the max-norm tolerance")
        assert ratio >= 1000
        # fvec dropped: the free rows of b, against the tolerance of the control part (lifting bound + load vector tolerance)
        b = m.rhs(rows, du[0], order)
        bw = m.rhs(rows, du[0], order, wrong="fvec")
        _, lift, F, lb = m.control_columns(order)
        ctrl_tol = np.abs(du[0]) @ (lb + 16 * sc.EPS * 2 * np.abs(F).max(axis=1)[:, None]) + tol * np.abs(b[:nn2]).max()
        f = m.free & m.touched()
        ratio = float((np.abs(bw - b)[f] / ctrl_tol[f]).max())
        print(f"order {order} fvec dropped: b moves by {ratio:.2e} x its tolerance on the worst free row")
        assert ratio >= 1000
    # the tail: a sensor row that takes its first weight throughout, and sensors that read x without dx.  Behind exact factors a
    # refinement sweep's dx is a few ulps of x (measured here: |dx| / |x| = 6e-15, dy moves by 0.2 .. 56 x its bound), so the GPU test
    # runs its tail check on a slot whose operator was replaced behind its factors (tc.lagged_operator): this is that pair on the host
    b = m.rhs(m.elem_part(d0, dm1, X[1], X[0], tc.step_coeffs(2))[1], du[0], 2)
    A1 = tc.lagged_operator(mesh)
    x0 = solve[2].lu.solve(np.asarray(b, dtype=np.float64))
    dx = solve[2].lu.solve(np.asarray(b - sc.spmv_longdouble(A1, x0), dtype=np.float64))
    lev, dy, bound = m.tail(x0, dx)
    assert np.array_equal(lev, x0 + dx) and np.any(dx)
    first = np.abs(m.tail(x0, dx, wrong="first_weight")[1] - dy)
    multi = np.array([len(i) > 1 for i, _ in m.rows])
    r = (first / bound)[multi]
    print(f"first weight throughout: dy moves by {float(r.min()):.2e} .. {float(r.max()):.2e} x its bound on the {multi.sum()} sensors of several entries")
    assert multi.sum() >= 4 and r.min() >= 1000
    nodx = np.abs(m.tail(x0, dx, wrong="no_dx")[1] - dy) / bound
    print(f"sensors without dx (lagged operator, |dx| / |x| = {np.linalg.norm(dx) / np.linalg.norm(x0):.1e}): dy moves by {float(nodx.min()):.2e} .. {float(nodx.max()):.2e} x its bound")
    assert nodx.min() >= 1000


def test_host_constants(ops):
    """HOST_TAN_RHS_ERROR re-measured: an fp64 numpy evaluation of the right-hand side (element loop, gather, control columns) against
    the np.longdouble one, velocity rows, per mesh and order.  The constants bound what is measured and exceed it by less than two."""
    worst = [0.0, 0.0]
    for mesh in tc.MESHES:
        m, model, _ = _scipy_model(mesh, 2, "mixed", "five", ops)
        nn2 = 2 * m.nn
        du, d0, dm1 = tc.inputs(m.N, 2, 1, 2)
        x1 = np.r_[sc.initial_state(m.th, 1)[0], np.zeros(m.th.nv)]
        x2 = np.r_[sc.initial_state(m.th, 1)[1], np.zeros(m.th.nv)]
        line = f"#   {mesh:8s}"
        for order in (1, 2):
            c = tc.step_coeffs(order)
            ref = m.rhs(m.elem_part(d0, dm1, x1, x2, c)[1], du[0], order)
            f64 = m.rhs(m.elem_part(d0, dm1, x1, x2, c, T=np.float64)[1], du[0], order, T=np.float64)
            assert f64.dtype == np.float64 and ref.dtype == L
            e2, ei = tc.rel2(f64[:nn2], ref[:nn2]), tc.relmax(f64[:nn2], ref[:nn2])
            worst = [max(worst[0], e2), max(worst[1], ei)]
            line += f" {e2:.2e} / {ei:.2e}      "
        print(line)
    print(f"HOST_TAN_RHS_ERROR measured {worst[0]:.3e} / {worst[1]:.3e}, recorded {tc.HOST_TAN_RHS_ERROR}")
    for got, rec in zip(worst, tc.HOST_TAN_RHS_ERROR):
        assert got <= rec < 2 * got, (got, rec)
