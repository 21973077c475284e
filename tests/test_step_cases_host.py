"""Host side of tests/test_step_routes_gpu.py (no GPU): the cases, knob sets and runs of tests/support/step_cases.py reach every branch
label outside UNREACHED; the mesh table holds; the np.longdouble model of a step agrees with the fp64 oracle; the constants the GPU test
derives its tolerances from still bound what is measured here; the lagged operator of the residual-monitor runs leaves a residual with
digits to compare."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from tests.support import batch_cases as bc
from tests.support import step_cases as sc
from tests.test_step_routes_gpu import HOST_ENERGY_ERROR, HOST_RHS_ERROR


@pytest.fixture(scope="module")
def models():
    return {case: sc.HostModel(case) for case in sc.CASES}


def test_runs_reach_every_label_outside_unreached():
    reached = set()
    for kn, knobs in sc.KNOB_SETS.items():
        got = sc.census(sc.RUNS[kn], knobs)
        assert got <= set(sc.LABELS), got - set(sc.LABELS)
        reached |= got
    assert set(sc.UNREACHED) <= set(sc.LABELS) and all(sc.UNREACHED.values())
    assert not reached & set(sc.UNREACHED), f"reached after all, take them out of UNREACHED: {sorted(reached & set(sc.UNREACHED))}"
    missing = set(sc.LABELS) - reached - set(sc.UNREACHED)
    assert not missing, f"no run reaches {sorted(missing)}"
    # what the single children must reach on their own
    assert {"fc_tail<true>", "final:single_group", "final:full_groups", "final:group_of_one", "final:ragged_group"} <= sc.census(sc.RUNS["fused_final"], sc.KNOB_SETS["fused_final"])
    assert {"reps>1", "reps:ragged_rows", "reps:ragged_cells", "fc_tail<true>"} <= sc.census(sc.RUNS["reps3_fused_final"], sc.KNOB_SETS["reps3_fused_final"])
    assert {"fc_finish", "solver:refine"} <= sc.census(sc.RUNS["unfused_tail"], sc.KNOB_SETS["unfused_tail"])
    d = sc.census(sc.RUNS["default"], sc.KNOB_SETS["default"])
    assert {"elem:reused", "fc_rhs_elem", "fc_rhs_elem_reg", "fc_early", "fc_final_late", "fc_wait_solved", "late:empty_tail", "fc_force_rows", "gather:C", "gather:force",
            "tail:check_blocks", "tail:check_ragged", "monitor:cadence_off_step", "sensor:stride_loop", "sensor:round_robin", "sensor:limit64"} <= d
    assert "elem:reused" not in sc.census(sc.RUNS["no_speculate"], sc.KNOB_SETS["no_speculate"])
    # every sensor set meets every tail kind of its child; every knob set and every pair of compared children exists
    assert {r[3] for r in sc.RUNS["default"]} == set(sc.SENSOR_SETS)
    assert set(sc.RUNS) == set(sc.KNOB_SETS) and all(a in sc.RUNS and b in sc.RUNS for a, b in sc.BITWISE_PAIRS)
    for a, b in sc.BITWISE_PAIRS:
        assert set(sc.RUNS[b]) & set(sc.RUNS[a]), (a, b)


def test_mesh_table():
    """An edit of a mesh cannot silently lose an edge of the launch geometry."""
    for case, (nc, N, g_rows, g_cells, g_check) in sc.TABLE.items():
        th = sc.host_case(case)[0]
        assert (th.nc, th.N) == (nc, N)
        assert (sc.cdiv(N, 32), sc.cdiv(nc, 32), sc.cdiv(N, sc.TAIL_CHECK_ROWS)) == (g_rows, g_cells, g_check)
    g = {c: t[2] + t[3] for c, t in sc.TABLE.items()}
    assert g == {"5x3": 7, "9x9": 32, "12x7": 33, "12x11": 50, "23x12": 102}
    assert sc.TABLE["5x3"][0] < 32 and sc.TABLE["12x11"][0] == 256 + 8 and sc.TABLE["23x12"][1] % sc.TAIL_CHECK_ROWS
    assert sc.cdiv(84, 3) * 3 == 84 and sc.cdiv(18, 3) * 3 == 18 and sc.cdiv(2662, 96) == 28  # FC_TAIL_REPS=3 on 23x12: the last row group of 32 is ragged ...
    assert 2662 % 32 and 552 % 32  # ... inside its workgroup, and so is the last cell group
    assert sc.cdiv(1306, 96) * 3 > 41 and sc.cdiv(264, 96) * 3 == 9  # 12x11: a row workgroup whose last group lies past N altogether


def test_route_model_on_the_speculation_sequence():
    """elem:reused exactly behind a step that speculated the same slot with nothing invalidating in between."""
    run = ("speculate", "12x11", "default", "one")
    ops = sc.scenario("speculate")
    prev_spec, dirty = -1, True
    for i, op, settings, route in sc.walk(run, {}):
        if route is None:
            dirty = dirty or op[0] in ("set_state", "time_scheme", "undo", "batch") or (op[0] == "force" and op[1] is not None)
            continue
        slot = 0 if settings["order"] == 1 else 1
        assert (route[0] == sc.ELEM_REUSED) == (not dirty and prev_spec == slot), (i, op, route)
        prev_spec, dirty = int(route[1]), False
    assert [o[0] for o in ops].count("step") >= 14
    assert all(r is None or r[0] != sc.ELEM_REUSED for *_, r in sc.walk(run, {"FC_SPECULATE": "0"}))


def _oracle(m, fprof=None):
    from oracle import ns_oracle as O

    U0 = sc.smooth_velocity(m.th)
    ts = O.TimeStepper(m.d, sc.RE, sc.DT, U0, m.dofs, m.prof, force_profiles=None if fprof is None else fprof.T)
    cn = O.TimeStepperCN(m.d, sc.RE, sc.DT, U0, m.dofs, m.prof, force_profiles=None if fprof is None else fprof.T)
    return O, ts, cn


def test_longdouble_model_against_the_fp64_oracle_and_the_constants(models):
    """TimeStepper.rhs (both orders, nonlinear on / off, force profiles), TimeStepperCN.rhs (the explicit operator C) and velocity_mass on
    every case; the worst distances are the constants of the GPU test."""
    worst = {"rhs": [0.0, 0.0], "energy": 0.0}
    for case, m in models.items():
        th = m.th
        u_n, u_nn, _ = sc.initial_state(th, 1)
        fprof = sc.force_profiles(th)
        per = [0.0, 0.0]
        for forces in (None, fprof):
            O, ts, cn = _oracle(m, forces)
            for nl in (True, False):
                ts.nonlinear = cn.nonlinear = nl
                for order in (1, 2):
                    uc = sc.CONTROLS[order]
                    ref = m.rhs(order, sc.DT, nl, u_n, u_nn, uc, ts.A_full[order], fprof=forces)
                    got = ts.rhs(order, u_n, u_nn, uc)
                    per = [max(per[0], sc.rel2(got, ref)), max(per[1], sc.relmax(got, ref))]
                C = cn.C[:, : 2 * th.nn]
                ref = m.rhs(1, sc.DT, nl, u_n, None, sc.CONTROLS[0], cn.A_full, fprof=forces, uforce=0.5 * sc.CONTROLS[0], Cmat=C)
                got = cn.rhs(u_n, sc.CONTROLS[0])
                per = [max(per[0], sc.rel2(got, ref)), max(per[1], sc.relmax(got, ref))]
        M = O.velocity_mass(m.d)
        e = max(abs(float((0.5 * u @ (M @ u) - m.energy(u)) / m.energy(u))) for u in (u_n, u_nn, sc.smooth_velocity(th)))
        print(f"{case}: fp64 oracle against the longdouble model: rhs {per[0]:.2e} / {per[1]:.2e} (2-norm / max-norm), energy {e:.2e}")
        assert per[0] < 1e-15 and per[1] < 1e-15 and e < 1e-15  # the model IS the oracle's operation
        worst["rhs"] = [max(worst["rhs"][0], per[0]), max(worst["rhs"][1], per[1])]
        worst["energy"] = max(worst["energy"], e)
    print(f"worst: rhs {worst['rhs'][0]:.3e} / {worst['rhs'][1]:.3e}, energy {worst['energy']:.3e}")
    assert worst["rhs"][0] <= HOST_RHS_ERROR[0] and worst["rhs"][1] <= HOST_RHS_ERROR[1]
    assert worst["energy"] <= HOST_ENERGY_ERROR
    # ... and not by much: a constant ten times too generous would be a loosened tolerance
    assert HOST_RHS_ERROR[0] <= 2 * worst["rhs"][0] and HOST_RHS_ERROR[1] <= 2 * worst["rhs"][1] and HOST_ENERGY_ERROR <= 2 * worst["energy"]
    assert 16 * max(HOST_RHS_ERROR) <= 1e-12  # never looser than what tests/test_hip_kernels.py::test_rhs_solve_step asserts today


def test_refined_solver_is_batch_cases_refined_solve(models):
    """step_cases.Refined is batch_cases.refined_solve with the LU factors kept."""
    m = models["9x9"]
    O, ts, _ = _oracle(m)
    B = bc.rhs_pool(m.N, 3)[:2]
    R = sc.Refined(ts.A_bc[2])
    X, E = np.array([R(b) for b in B]), bc.refined_solve(ts.A_bc[2], B)  # (LAPACK's triangular solves of one and of two columns may round differently)
    assert max(sc.rel2(x, e) for x, e in zip(X, E)) <= 1e-15


@pytest.mark.parametrize("case", sorted({r[1] for runs in sc.RUNS.values() for r in runs if r[0] == "residual"}))
def test_the_lagged_operator_leaves_a_residual_with_digits(models, case):
    """The residual-monitor runs solve with the factors of A0 and monitor A1: |b - A1 x| / |b| must be far above round-off, and the
    monitor's bound far below it."""
    from oracle import ns_oracle as O

    m = models[case]
    th = m.th
    u_n, u_nn, _ = sc.initial_state(th, 3)
    A0 = O.apply_bc_symmetric(O.assemble_matrix(m.d, **sc.operator_args(th, 2)), None, m.dofs, np.zeros(m.dofs.size))[0]
    A1_full = O.assemble_matrix(m.d, **sc.operator_args(th, 2, lagged=True))
    A1 = O.apply_bc_symmetric(A1_full, None, m.dofs, np.zeros(m.dofs.size))[0]
    b = np.asarray(m.rhs(2, sc.DT, True, u_n, u_nn, sc.CONTROLS[0], A1_full), dtype=np.float64)
    x = spla.splu(A0.tocsc()).solve(b)
    r, bn, bound = m.residual(A1, x, b)
    print(f"{case}: |b - A1 x| / |b| = {float(r / bn):.3e}, bound of the monitor's |r| relative to |r|: {float(bound / r):.2e}")
    assert r / bn > 1e-6 and bound / r < 1e-6


def test_sensor_sets(models):
    th = models["12x7"].th
    rows = {name: sc.sensor_rows(th, name) for name in sc.SENSOR_SETS}
    assert len(rows["none"]) == 0 and len(rows["one"]) == 1 and len(rows["five"]) == 5 and len(rows["limit64"]) == sc.MAX_SENSORS
    assert [len(i) for i, _ in rows["long150"]] == [150] and [len(i) for i, _ in rows["single_entry"]] == [1]
    assert max(len(i) for i, _ in rows["five"]) == 65 and 64 in [len(i) for i, _ in rows["five"]]
    for rr in rows.values():
        for i, w in rr:
            assert len(i) == len(w) and i.min() >= 0 and i.max() < th.N and len(set(i.tolist())) == len(i)
    y, bound = sc.HostModel.sensors(rows["five"], np.cos(np.arange(th.N)))
    assert y.shape == (5,) and np.all(bound > 0) and np.all(bound < 1e-11)
