"""Host side of tests/test_adjoint_march_gpu.py (no GPU): the runs of tests/support/adjoint_march_cases.py reach every branch label
outside UNREACHED, the mesh table holds, the np.longdouble model of a backward step agrees with the fp64 scipy models of the whole march,
the new actuator and sensor sets tell the seeded model mistakes apart, and the host constant the GPU test's tolerance stands on is
re-measured."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import adjoint_march_cases as mc
from tests.support import step_cases as sc
from tests.support.adjoint_nl_model import NonlinearStepModel
from tests.support.adjoint_step_model import StepModel

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
    reached = mc.census(mc.SINGLE_RUNS, mc.BATCH_RUNS)
    assert reached <= set(mc.LABELS), reached - set(mc.LABELS)
    assert set(mc.UNREACHED) <= set(mc.LABELS)
    missing = set(mc.LABELS) - set(mc.UNREACHED) - reached
    assert not missing, f"no run reaches {sorted(missing)}"
    assert not reached & set(mc.UNREACHED), f"reached although listed as unreached: {sorted(reached & set(mc.UNREACHED))}"
    assert all(len(why) > 20 for why in mc.UNREACHED.values())
    print(f"{len(reached)} of {len(mc.LABELS)} labels reached, {len(mc.UNREACHED)} unreached with a reason")
    # the issue's sets are all there
    assert {r[1] for r in mc.SINGLE_RUNS} == set(mc.N_ACT)
    assert {r[3] for r in mc.SINGLE_RUNS} | {r[4] for r in mc.BATCH_RUNS} == set(mc.SENSOR_SETS)
    assert {mc.kb_of(r[1]) for r in mc.BATCH_RUNS} == set(mc.KBS) and {r[1] for r in mc.BATCH_RUNS} == {3, 5, 9, 17, 32}
    assert {r[0] for r in mc.SINGLE_RUNS} == set(mc.MESHES) and "64x32" not in {r[0] for r in mc.BATCH_RUNS}
    assert {(r[2], r[5]) for r in mc.SINGLE_RUNS} == {(v, nl) for v in ("dirichlet", "mixed") for nl in (False, True)}
    assert {r[6] for r in mc.SINGLE_RUNS} == {1, 2} and {r[9] for r in mc.SINGLE_RUNS} == {True, False}


def test_no_knob_set_is_redundant():
    full = mc.census(mc.SINGLE_RUNS, mc.BATCH_RUNS)
    for hs in mc.HANDLE_SETS:
        rest = mc.census([r for r in mc.SINGLE_RUNS if r[4] != hs], mc.BATCH_RUNS)
        assert full - rest, f"handle set {hs!r} reaches nothing of its own"
        print(f"only under handle set {hs!r}: {sorted(full - rest)}")
    for ts in mc.TAPE_SETS:
        rest = mc.census(mc.SINGLE_RUNS, mc.BATCH_RUNS, tape_sets=tuple(t for t in mc.TAPE_SETS if t != ts))
        assert full - rest, f"tape set {ts!r} reaches nothing of its own"
        print(f"only under tape set {ts!r}: {sorted(full - rest)}")
    for what, runs in (("single", mc.SINGLE_RUNS), ("batched", mc.BATCH_RUNS)):
        rest = mc.census([] if what == "single" else mc.SINGLE_RUNS, [] if what == "batched" else mc.BATCH_RUNS)
        assert full - rest and runs


def test_the_mesh_table_holds():
    """cells, N, the grids of every launch and the tail's pass counts, as the comments of the table say."""
    for mesh, (nc, N) in mc.TABLE.items():
        th, dofs = mc.host_case(mesh)
        assert (th.mesh.cells.shape[0], th.N) == (nc, N), mesh
    # the two large squares lie beyond the two thresholds
    assert mc.TABLE["33x29"][1] > 8192 and mc.TABLE["64x32"][1] > 64 * 256
    r = lambda *a, **k: dict(zip(mc.ROUTE_COLS, (int(v) for v in mc.predicted_route(*a, **k))))  # noqa: E731
    # fc_adj_tail_b<32> on 33x29: the cap of 1024 workgroups of 8 rows; workgroups 0 .. 91 take a ragged second trip
    b = r("33x29", 5, 4, {}, False, True, True, k=32)
    assert (b["KB"], b["g_tail"], b["passes"], b["gx"]) == (32, 1024, 2, 1024)
    assert mc.cdiv(8926 - 8192, 8) == 92 and (8926 - 8192) % 8 == 6
    assert r("33x29", 1, 1, {}, False, True, True, k=17)["g_tail"] == 1024 and r("23x12", 4, 1, {}, False, True, True, k=32)["g_tail"] == 333
    # fc_adj_reduce on 64x32: gx = 74, lanes 0 .. 9 take a second partial
    s = r("64x32", 5, 2, {}, False, True, True)
    assert (s["g_tail"], s["gx"], s["passes"], s["g_gather"], s["g_elem"]) == (74, 74, 2, 74, 128)
    assert [r("5x3", n, 1, {}, False, True, False)["passes"] for n in mc.N_ACT] == [1, 1, 1, 1, 2, 3, 8]
    z = r("5x3", 0, 1, {}, False, True, False)
    assert (z["reduced"], z["gx"], z["g_tail"]) == (0, 0, 1)
    assert r("12x11", 5, 64, {"FC_ELEM_REG_MIN": "1"}, True, True, False, tape=1)["elem"] == mc.ELEM_NL_REG
    assert r("12x11", 5, 64, {"FC_ELEM_REG_MIN": "1"}, True, True, False, tape=1)["g_elem"] == 2  # 264 = 256 + 8 cells
    assert r("12x11", 2, 64, {}, True, True, False, k=17, tape=0)["g_elem"] == mc.cdiv(264, 8)
    assert r("5x3", 1, 0, {}, False, True, False)["w"] == 0  # no sensors: w is not handed on
    # the new sensor sets are what their names say
    th, dofs = mc.host_case("12x7")
    tab = mc.ct_table(mc.sensor_rows(th, dofs, "shared_rows"), th.N)
    shared = [e for e in tab if len({s for s, _ in e}) >= 3]
    assert len(shared) >= 3 and any(len(e) > len({s for s, _ in e}) for e in tab)
    rows = mc.sensor_rows(th, dofs, "on_dirichlet")
    assert np.isin(rows[0][0], dofs).sum() == 4 and (rows[0][0] >= 2 * th.nn).sum() == 4 and np.isin(rows[1][0], dofs).all()
    # no two actuator columns equal or proportional
    for fam in (mc.profiles(th, dofs, 32).T, mc.force_set(th, 32)):
        unit = fam / np.linalg.norm(fam, axis=1)[:, None]
        cosines = np.abs(unit @ unit.T) - np.eye(32)
        assert cosines.max() < 0.9999, cosines.max()


def _scipy_model(mesh, n_act, variant, sens, ops, nonlinear):
    from oracle import ns_oracle as O

    full, bc, M = ops(mesh)
    m = mc.MarchModel(mesh, n_act, variant, sens, full)
    G = np.zeros((m.N, n_act))
    G[m.dofs] = m.prof
    C = sp.lil_matrix((len(m.rows), m.N))
    for s, (idx, w) in enumerate(m.rows):
        for i, v in zip(idx, w):
            C[s, i] += v
    F = None
    if m.fprof is not None:
        F = np.stack([np.asarray(m.control_columns(1)[2][k], dtype=float) for k in range(n_act)], axis=1)
    args = (bc[1], bc[2], M, m.dofs, m.prof, full[1] @ G, full[2] @ G, C.tocsr(), mc.DT)
    model = NonlinearStepModel(O.Disc.from_taylor_hood(m.th), *args, F=F) if nonlinear else StepModel(*args, F=F)
    return m, model, {o: mc.RefinedT(bc[o]) for o in (1, 2)}


@pytest.mark.parametrize("mesh,n_act,variant,sens,nonlinear,first", [
    ("5x3", 5, "mixed", "shared_rows", True, 1), ("9x9", 2, "mixed", "on_dirichlet", True, 2), ("12x7", 4, "dirichlet", "five", True, 1),
    ("12x11", 5, "mixed", "limit64", False, 2), ("23x12", 9, "mixed", "long150", True, 1), ("33x29", 5, "mixed", "shared_rows", False, 2),
    ("64x32", 5, "dirichlet", "on_dirichlet", False, 1)])
def test_longdouble_model_against_the_fp64_scipy_model(mesh, n_act, variant, sens, nonlinear, first, ops):
    """One march of three steps per mesh through MarchModel's per-kernel functions against StepModel / NonlinearStepModel: relative."""
    m, model, solve_t = _scipy_model(mesh, n_act, variant, sens, ops, nonlinear)
    n = 3 if mesh != "64x32" else 2
    w, z = mc.inputs(m.N, len(m.rows), n, 3)
    X = None
    if nonlinear:
        u_n, u_nn, p = sc.initial_state(m.th, 1)
        u = np.random.default_rng(5).standard_normal((n, n_act)) * 0.1
        X, _ = model.forward(first, u, np.r_[u_n, p], np.r_[u_nn, p])
        gm, _, _, mum = model.adjoint(first, X, w, z)
    else:
        gm, _, _, mum = model.adjoint(first, n, w, z)
    g, mu = mc.host_march(m, solve_t, first, n, w, z, X)
    eg, em = mc.rel2(g, gm), mc.rel2(mu, mum)
    print(f"{mesh} n_act {n_act} {variant} {sens} {'nonlinear' if nonlinear else 'linearised'}: g {eg:.3e}, mu {em:.3e} relative to the fp64 scipy model")
    assert eg <= 1e-10 and em <= 1e-10


def test_the_new_sets_are_distinguishing(ops):
    """Each seeded model mistake moves the quantity it touches by at least 1000 x that quantity's tolerance in the GPU test."""
    mesh = "12x7"
    full, bc, _ = ops(mesh)
    rng = np.random.default_rng(8)
    # fvec dropped: bt off the Dirichlet rows
    m = mc.MarchModel(mesh, 9, "mixed", "shared_rows", full)
    bt, lift, F, lb = m.control_columns(2)
    tol = lb + 16 * sc.EPS * 2 * np.abs(F).max(axis=1)[:, None] + 2 * sc.EPS * (np.abs(lift) + np.abs(F))
    moved = np.abs(m.control_columns(2, wrong="fvec")[0] - bt)[:, m.free]
    ratio = (moved / tol[:, m.free]).max(axis=1)
    print(f"fvec dropped: bt moves by {ratio.min():.2e} .. {ratio.max():.2e} x its tolerance, per actuator")
    assert ratio.min() >= 1000
    # sensor entries of a row summed with the first entry's weight: b on the rows with two entries and more
    w = rng.standard_normal(len(m.rows))
    good, mag, cnt = m.ct_part(w)
    bad = m.ct_part(w, wrong="first_weight")[0]
    multi = cnt >= 2
    r = np.abs(bad - good)[multi] / ((cnt[multi] + 2) * sc.EPS * mag[multi])
    print(f"first entry's weight: b moves by {float(r.max()):.2e} x its bound on the worst of {multi.sum()} rows, {(r >= 1000).sum()} rows beyond 1000 x")
    assert multi.sum() >= 5 and r.max() >= 1000 and (r >= 1000).sum() >= 3
    z1 = rng.standard_normal(m.N)
    # ... and the ORDER of a row's sum shows in its bits (fc_adj_rhs_gather's chain, sensors ascending against descending)
    differ = sum(m.ct_chain(i, w, z1[i]) != m.ct_chain(i, w, z1[i], descending=True) for i in np.flatnonzero(multi))
    print(f"sensors descending: {differ} of {multi.sum()} rows differ in their bits")
    assert differ >= 1
    # Dirichlet mask put on the output: b on the Dirichlet rows
    z1, z2 = rng.standard_normal(m.N), rng.standard_normal(m.N)
    x = np.r_[sc.initial_state(m.th, 1)[0], np.zeros(m.th.nv)]
    for nl in (False, True):
        c = mc.step_coeffs(1, 3, nl)
        good = m.elem_part(z1, z2, c, x if nl else None)
        bad = m.elem_part(z1, z2, c, x if nl else None, wrong="mask_out")
        ratio = float(np.abs(bad - good).max() / np.abs(good).max()) / (16 * mc.HOST_ADJ_RHS_ERROR[1])
        print(f"mask on the output ({'nonlinear' if nl else 'linearised'}): b moves by {ratio:.2e} x its max-norm tolerance")
        assert ratio >= 1000 and np.abs(good[m.dofs]).min() > 0
    # actuators beyond the first four dropped: the partials and g
    mu = rng.standard_normal(m.N)
    share, bound = m.partials(bt, mu, 4, 256)
    lost = m.partials(bt, mu, 4, 256, wrong="first4")[0]
    ratio = np.abs(lost - share)[4:] / bound[4:]
    g, gb = m.dot(bt, mu)
    rg = np.abs(m.fold(lost) - g)[4:] / gb[4:]
    print(f"first four actuators only: partials move by at least {float(ratio.min()):.2e} x their bound, g by at least {float(rg.min()):.2e} x")
    assert ratio.min() >= 1000 and rg.min() >= 1000 and np.array_equal(lost[:4], share[:4])
    assert float(np.abs(m.fold(share) - g).max()) <= float(gb.max())


def test_the_sparse_refined_solve_is_the_dense_one(ops):
    """RefinedT (sparse LU, longdouble residuals) against batch_cases.refined_solve (LAPACK LU, the scheme HOST_BLOCK_SOLVE_ERROR was
    measured with) on the transposed operators of two small meshes: both refine to the fp64 rounding of the solution."""
    from tests.support import batch_cases as bcs

    for mesh in ("5x3", "12x7"):
        _, bc, _ = ops(mesh)
        B = np.random.default_rng(6).standard_normal((3, bc[2].shape[0]))
        for order in (1, 2):
            dense = bcs.refined_solve(sp.csr_matrix(bc[order].T), B)
            sparse = np.stack([mc.RefinedT(bc[order])(b) for b in B])
            e = max(mc.rel2(sparse[j], dense[j]) for j in range(3))
            print(f"{mesh} order {order}: sparse against dense refined transposed solve {e:.2e}")
            assert e <= 2.0**-52, e


def test_fold_bitwise_is_the_stated_order():
    """fold_bitwise against a scalar transcription of fc_adj_reduce: lane l sums partials l, l + 64, .., then the shuffle tree."""
    rng = np.random.default_rng(0)
    for gx in (1, 7, 64, 65, 74, 128, 333, 1024):
        p = rng.standard_normal(gx) * 10.0 ** rng.integers(-6, 6, gx)
        lanes = [0.0] * 64
        for l in range(64):
            for q in range(l, gx, 64):
                lanes[l] += p[q]
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + (lanes[l + off] if l + off < 64 else lanes[l]) for l in range(64)]  # (__shfl_down beyond the wave: the lane's own)
        assert mc.MarchModel.fold_bitwise(p) == lanes[0], gx
    assert mc.MarchModel.fold_bitwise(rng.standard_normal((3, 5, 74))).shape == (3, 5)


def test_host_constants(ops):
    """HOST_ADJ_RHS_ERROR re-measured: an fp64 numpy evaluation of the right-hand side against the np.longdouble one, velocity rows, per
    mesh, linearised and nonlinear.  The constants bound what is measured and exceed it by less than a factor of two."""
    worst = [0.0, 0.0]
    for mesh in mc.MESHES:
        full, _, _ = ops(mesh)
        m = mc.MarchModel(mesh, 2, "dirichlet", "five", full)
        rng = np.random.default_rng(1)
        nn2 = 2 * m.nn
        z1 = np.r_[0.1 * sc.smooth_velocity(m.th, 2.0) + 0.01 * rng.standard_normal(nn2), 0.01 * rng.standard_normal(m.th.nv)]
        z2 = np.r_[0.1 * sc.smooth_velocity(m.th, 1.5) + 0.01 * rng.standard_normal(nn2), 0.01 * rng.standard_normal(m.th.nv)]
        x = np.r_[sc.initial_state(m.th, 1)[0], np.zeros(m.th.nv)]
        w, z = mc.inputs(m.N, len(m.rows), 1, 2)
        line = f"#   {mesh:8s}"
        for nl in (False, True):
            c = mc.step_coeffs(1, 3, nl)
            ref = m.rhs(z1, z2, c, w[0], z, x if nl else None)
            f64 = m.rhs(z1, z2, c, w[0], z, x if nl else None, T=np.float64)
            assert f64.dtype == np.float64 and ref.dtype == L
            e2, ei = mc.rel2(f64[:nn2], ref[:nn2]), mc.relmax(f64[:nn2], ref[:nn2])
            worst = [max(worst[0], e2), max(worst[1], ei)]
            line += f" {e2:.2e} / {ei:.2e}      "
        print(line)
    print(f"HOST_ADJ_RHS_ERROR measured {worst[0]:.3e} / {worst[1]:.3e}, recorded {mc.HOST_ADJ_RHS_ERROR}")
    for got, rec in zip(worst, mc.HOST_ADJ_RHS_ERROR):
        assert got <= rec < 2 * got, (got, rec)
