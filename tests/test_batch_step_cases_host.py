"""Host side of tests/test_batch_step_routes_gpu.py (no GPU): the runs and knob sets of tests/support/batch_step_cases.py reach every
branch label outside UNREACHED; the star mesh reaches what no structured mesh does; the (mesh, k) pairs meet the launch geometry they were
chosen for; predicted_tail_blocks reproduces the cut counts of build_tail_blocks; the route model follows the dispatch through the
scenarios; the np.longdouble model of a step agrees with the fp64 oracle on the star within the constants of the GPU test."""
import numpy as np
import pytest

from tests.support import batch_step_cases as bs
from tests.support import step_cases as sc
from tests.test_step_routes_gpu import HOST_ENERGY_ERROR, HOST_RHS_ERROR


def test_runs_reach_every_label_outside_unreached():
    reached, per = set(), {}
    for kn, knobs in bs.KNOB_SETS.items():
        per[kn] = bs.census(bs.RUNS[kn], knobs)
        assert per[kn] <= set(bs.LABELS), per[kn] - set(bs.LABELS)
        reached |= per[kn]
    assert len(set(bs.LABELS)) == len(bs.LABELS)
    assert set(bs.UNREACHED) <= set(bs.LABELS) and all(bs.UNREACHED.values())
    assert not reached & set(bs.UNREACHED), f"reached after all, take them out of UNREACHED: {sorted(reached & set(bs.UNREACHED))}"
    missing = set(bs.LABELS) - reached - set(bs.UNREACHED)
    assert not missing, f"no run reaches {sorted(missing)}"
    # what the single children must reach on their own
    d = per["default"]
    assert {"fc_rhs_elem_breg<false>", "fc_rhs_elem_breg<true>", "elem:ragged_single_workgroup", "elem:several_workgroups_ragged", "gather:second_trip_clamped",
            "gather:ahead", "gather:opens_gate", "gather:C", "fc_rhs_ctrl_b", "tail:row>64", "tail:NT=1", "tail:NT=2", "tail:JL=1", "tail:JL>1", "tail:G=0",
            "tail:cells_only", "tail:rows_only", "energy:ragged_single_workgroup", "energy:second_workgroup_empty_trips", "final:sensor_wave_loop",
            "early:sensor_wave_loop", "sensor:stride_loop", "lead:0", "lead:1:form_switch", "lead:2", "spec:same_slot", "spec:none:force", "spec_gather:off:C",
            "tail:flag", "flag:sweep", "fc_b_zero_column", "fc_b_interleave:padded", "fc_b_interleave:full", "monitor:off_cadence", "plain"} <= d
    assert "graph" not in d and {"graph", "flag:sweep"} <= per["graph"] and "plain" not in per["graph"]
    assert {"fc_rhs_elem_b", "fc_rhs_elem_b:force", "elem:lds:inactive_cells"} <= per["elem_lds"] and not {"fc_rhs_elem_breg<false>", "fc_rhs_elem_breg<true>"} & per["elem_lds"]
    assert "spec:none:knob" in per["no_speculate"] and not {"elem:ahead", "gather:ahead", "lead:0", "lead:1"} & per["no_speculate"]
    assert {"spec_gather:off:knob", "lead:1:no_gather_ahead"} <= per["no_gather_ahead"] and not {"gather:ahead", "lead:0", "fc_rhs_ctrl_b"} & per["no_gather_ahead"]
    assert {"late_gate:off:knob", "early:opens_gate"} <= per["no_late_gate"] and "gather:opens_gate" not in per["no_late_gate"]
    assert "tail:cut:cols" in per["tb64"] and "tail:one_cut_at_128" in per["tb128"] and "tail:cut:cols" not in d
    # every sensor set, scenario, width and pair is in use; the compared children share runs
    assert {r[4] for r in bs.RUNS["default"]} == set(bs.SENSOR_SETS) and {r[0] for r in bs.RUNS["default"]} == set(bs.SCENARIOS)
    assert {(r[1], r[2]) for r in bs.RUNS["default"]} == set(bs.PAIRS) and {r[2] for r in bs.RUNS["default"]} == set(bs.WIDTHS)
    assert set(bs.RUNS) == set(bs.KNOB_SETS)
    for a, b in bs.BITWISE_PAIRS + (bs.ELEM_PAIR,):
        assert len(set(bs.RUNS[a]) & set(bs.RUNS[b])) >= 4, (a, b)
    assert set(bs.UNCAPTURED) <= set(bs.RUNS["default"])


def test_the_star_reaches_what_no_structured_mesh_does():
    th, dofs, prof = bs.host_case("star")
    assert (th.nc, th.N, th.nn, th.nv) == (70, 343, 151, 41)
    assert prof.shape == (dofs.size, sc.N_ACT) and dofs.size == 38  # the 20 boundary nodes but the midpoint of the x = xmax facet
    lengths, contrib = np.diff(bs.pattern(th)[0]), bs.contributions(th)
    # the centre's two velocity rows: 2 x 31 velocities of the fan + 11 pressures; its pressure row couples to the 62 velocities only
    # (the device's pattern holds no pressure-pressure entries)
    assert lengths.max() == 73 and int((lengths > 64).sum()) == 2
    assert contrib.max() == 10 and int((contrib > 8).sum()) == 2
    for mesh in ("5x3", "9x9", "12x11"):
        t = bs.host_case(mesh)[0]
        assert np.diff(bs.pattern(t)[0]).max() == 45 and bs.contributions(t).max() == 6
    # every cell counter-clockwise and of positive area, every dof in a cell
    p = th.mesh.coords[th.mesh.cells]
    det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    assert det.min() > 1e-3 and np.unique(th.cell_dofs).size == th.N
    # the tree the device builds for it exists
    from tests.support import ndsolver

    skip = np.zeros(th.N, dtype=bool)
    skip[dofs] = True
    assert ndsolver.build_tree(th.cell_dofs, th.mesh.cell_centroids(), th.N, 2, skip, bits=list(sc.TREE_BITS)).depth >= 1


def test_pairs_meet_the_launch_geometry_they_were_chosen_for():
    g = {p: bs.geometry(*p) for p in bs.PAIRS}
    by_kb = {KB: [p for p in bs.PAIRS if g[p]["KB"] == KB] for KB in (4, 8, 16, 32)}
    assert [bs.batch_width(k) for k in bs.WIDTHS] == [4, 4, 8, 16, 32, 32] and all(by_kb.values())
    ragged = lambda n, per: n % per != 0  # noqa: E731
    for KB, pairs in by_kb.items():
        gs = [g[p] for p in pairs]
        assert any(x["g_elem"] > 1 and ragged(x["nc"], x["elem_cpb"]) for x in gs), KB
        assert any(x["g_energy"] == 1 and ragged(x["nc"], x["energy_cpb"]) for x in gs), KB
        assert any(x["g_energy"] > 1 and 0 < x["nc"] % x["energy_cpb"] <= 3 * (256 // KB) for x in gs), KB  # a last workgroup with empty trips
        assert any(x["g_gather"] > 1 and ragged(x["N"] * (KB // 2), 256) for x in gs), KB
        assert any(x["padded"] for x in gs) or KB == 32
    for KB in (4, 8):  # a workgroup of the register element loop holds the 30 cells of 5x3
        assert any(x["g_elem"] == 1 and ragged(x["nc"], x["elem_cpb"]) for x in (g[p] for p in by_kb[KB]))
    assert g[("12x11", 3)]["nc"] == 256 + 8 and g[("12x11", 3)]["g_energy"] == 2  # three empty trips in the second workgroup
    assert {g[p]["KB"] for p in bs.PAIRS if p[0] == "star"} == {4, 32}
    assert g[("5x3", 3)]["padded"] == 1 and g[("5x3", 4)]["padded"] == 0 and g[("star", 32)]["padded"] == 0
    assert {x["NT"] for x in g.values()} == {1, 2} and {x["JL"] for x in g.values()} == {8, 4, 2, 1}


def test_predicted_tail_blocks_reproduces_the_cut_counts():
    """The column cut happens only for FC_TB_COLS <= 128: once at 128 on 9x9, dozens of times at 64; no block exceeds 138 distinct
    columns; the FC_TB_NNZ cut is not reached; FC_TB_COLS=64 on the star is a refusal, not an overflow."""
    most_cols = most_nnz = 0
    for mesh in bs.MESHES:
        th = bs.host_case(mesh)[0]
        for cols in (128, 144, 192, 256, 384):
            tb = bs.predicted_tail_blocks(th, cols)
            assert tb["cuts"]["nnz"] == 0 and tb["cuts"]["short_last"] == 1 and sum(tb["cuts"].values()) == tb["n"]
            assert tb["cuts"]["cols"] == (1 if (mesh, cols) == ("9x9", 128) else 0), (mesh, cols)
            most_cols, most_nnz = max(most_cols, tb["max_cols"]), max(most_nnz, tb["max_nnz"])
    assert most_cols == 137 <= 138 and most_nnz == 522 < bs.TB_NNZ  # (9x9 at 128 columns; the star: 501)
    assert {m: bs.predicted_tail_blocks(bs.host_case(m)[0], 256)["n"] for m in bs.MESHES} == {"5x3": 12, "9x9": 52, "12x11": 82, "star": 22}
    at64 = {m: bs.predicted_tail_blocks(bs.host_case(m)[0], 64) for m in ("5x3", "9x9", "12x11")}
    assert {m: (t["n"], t["cuts"]["cols"]) for m, t in at64.items()} == {"5x3": (16, 9), "9x9": (90, 73), "12x11": (138, 118)}
    with pytest.raises(ValueError, match=bs.REFUSAL):
        bs.predicted_tail_blocks(bs.host_case("star")[0], 64)
    # tb_cols as build_tail_blocks chooses it
    assert [bs.tb_cols(KB, {}) for KB in (4, 8, 16, 32)] == [256, 256, 256, 144]
    assert [bs.tb_cols(KB, {"FC_OVERLAP_TAIL": "0"}) for KB in (4, 32)] == [128, 128]
    assert [bs.tb_cols(KB, {"FC_TB_COLS": "64"}) for KB in (4, 32)] == [64, 64] and bs.tb_cols(32, {"FC_TB_COLS": "384"}) == 192 and bs.tb_cols(4, {"FC_TB_COLS": "3"}) == 16
    assert all(bs.tb_cols(KB, {}) <= 12 * 256 // (KB // 2) for KB in (4, 8, 16, 32))  # the staging trips of fc_tail_b hold a block's columns
    for ks, mesh, k in bs.REFUSED:
        with pytest.raises(ValueError, match=bs.REFUSAL):
            bs.predicted_tail_blocks(bs.host_case(mesh)[0], bs.tb_cols(bs.batch_width(k), bs.KNOB_SETS[ks]))


def test_route_model_on_the_scenarios():
    """lead = 0 exactly behind a step that gathered ahead into the place this step reads, with nothing invalidating in between."""
    run = ("main", "5x3", 4, "overlapped", "limit64")
    leads = [int(r[0]) for *_, r, _ in bs.walk(run, {}) if r is not None]
    assert leads == [2, 0, 1, 0, 0, 1, 2, 0, 0, 0, 1, 0]
    assert all(int(r[0]) == 2 for *_, r, _ in bs.walk(run, {"FC_SPECULATE": "0"}) if r is not None)
    assert [int(r[0]) for *_, r, _ in bs.walk(run, {"FC_SPECULATE_GATHER": "0"}) if r is not None] == [2, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1]
    one = [r for *_, r, _ in bs.walk(("main", "5x3", 4, "one_stream", "limit64"), {}) if r is not None]
    assert not any(r[4] or r[5] for r in one) and [int(r[0]) for r in one] == [2, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0] and {int(r[9]) for r in one} == {128}
    # check_residual = 3 from the eighth step on: steps 7 and 8 off the cadence (no tail at all, then cells only), step 9 on it with the energy off
    tails = [(int(r[6]), int(r[7]) > 0, int(r[8]) > 0) for *_, r, _ in bs.walk(run, {}) if r is not None][7:]
    assert tails == [(0, False, False), (0, False, True), (1, True, False), (0, False, True), (0, False, False)]
    # Crank-Nicolson slot: speculation onto the same slot, no gather ahead; an operator set behind a gather ahead makes the next step gather in full
    cn = [r for *_, r, _ in bs.walk(("cn", "5x3", 5, "overlapped", "none"), {}) if r is not None]
    assert [(int(r[0]), int(r[2]), int(r[3])) for r in cn] == [(2, 1, 0), (1, 1, 0), (1, 1, 0), (2, 2, 1), (0, 2, 1), (1, 2, 0), (1, 2, 0), (1, 2, 1), (2, 2, 1)]
    # body forces: the FORCE kernel on every step, nothing speculated
    fo = [r for *_, r, _ in bs.walk(("force", "5x3", 4, "overlapped", "single_entry"), {}) if r is not None]
    assert [(int(r[0]), int(r[1]), int(r[2])) for r in fo] == [(2, 2, 2), (2, 3, 0), (2, 3, 0), (2, 3, 0), (2, 2, 2), (0, 2, 2)]
    # the non-finite column: once on the tail's flag route, then on the down-sweep's (overlapped; off the cadence)
    nf = [f for *_, f in bs.walk(("nonfinite", "5x3", 5, "overlapped", "single_entry"), {}) if f is not None]
    assert nf == ["tail", "sweep", "sweep"]
    assert [f for *_, f in bs.walk(("nonfinite", "star", 32, "one_stream", "long150"), {}) if f is not None] == ["tail", "tail", "sweep"]


def test_columns():
    assert [bs.ident(s, 3) for s in range(3)] == [0, 1, 2] and [bs.ident(s, 4) for s in range(4)] == [0, 1, 2, 0] and bs.ident(31, 32) == 0
    u, f = bs.controls(5, 1), bs.force_amplitudes(5, 1)
    assert u.shape == f.shape == (5, sc.N_ACT) and np.array_equal(u[4], u[0]) and len({tuple(r) for r in u[:4]}) == 4 and not np.any(u == f)
    assert np.array_equal(bs.controls(3, 2), bs.controls(4, 2)[:3])
    th = bs.host_case("5x3")[0]
    a, b = bs.column_state(th, 1, 4, 2), bs.column_state(th, 3, 4, 2)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(b[0], bs.column_state(th, 0, 4, 2)[0])


def test_longdouble_model_against_the_fp64_oracle_on_the_star():
    """As tests/test_step_cases_host.py::test_longdouble_model_against_the_fp64_oracle_and_the_constants, on the star: TimeStepper.rhs
    (both orders, nonlinear on / off, force profiles), TimeStepperCN.rhs and velocity_mass.  Measured: rhs 1.29e-16 / 3.35e-16 (2-norm /
    max-norm), energy 2.08e-16 -- within HOST_RHS_ERROR and HOST_ENERGY_ERROR of the structured meshes, so the star needs no constant of
    its own and the GPU test holds it to the same tolerances."""
    from oracle import ns_oracle as O

    bs.host_case("star")
    m = sc.HostModel("star")
    th = m.th
    u_n, u_nn, _ = sc.initial_state(th, 1)
    fprof = sc.force_profiles(th)
    per = [0.0, 0.0]
    U0 = sc.smooth_velocity(th)
    for forces in (None, fprof):
        ts = O.TimeStepper(m.d, sc.RE, sc.DT, U0, m.dofs, m.prof, force_profiles=None if forces is None else forces.T)
        cn = O.TimeStepperCN(m.d, sc.RE, sc.DT, U0, m.dofs, m.prof, force_profiles=None if forces is None else forces.T)
        for nl in (True, False):
            ts.nonlinear = cn.nonlinear = nl
            for order in (1, 2):
                uc = sc.CONTROLS[order]
                ref = m.rhs(order, sc.DT, nl, u_n, u_nn, uc, ts.A_full[order], fprof=forces)
                got = ts.rhs(order, u_n, u_nn, uc)
                per = [max(per[0], sc.rel2(got, ref)), max(per[1], sc.relmax(got, ref))]
            ref = m.rhs(1, sc.DT, nl, u_n, None, sc.CONTROLS[0], cn.A_full, fprof=forces, uforce=0.5 * sc.CONTROLS[0], Cmat=cn.C[:, : 2 * th.nn])
            got = cn.rhs(u_n, sc.CONTROLS[0])
            per = [max(per[0], sc.rel2(got, ref)), max(per[1], sc.relmax(got, ref))]
    M = O.velocity_mass(m.d)
    e = max(abs(float((0.5 * u @ (M @ u) - m.energy(u)) / m.energy(u))) for u in (u_n, u_nn, sc.smooth_velocity(th)))
    print(f"star: fp64 oracle against the longdouble model: rhs {per[0]:.3e} / {per[1]:.3e} (2-norm / max-norm), energy {e:.3e}")
    assert per[0] < 1e-15 and per[1] < 1e-15 and e < 1e-15  # the model IS the oracle's operation
    assert per[0] <= HOST_RHS_ERROR[0] and per[1] <= HOST_RHS_ERROR[1] and e <= HOST_ENERGY_ERROR
    # the constants of the structured meshes are those of tests/test_step_routes_gpu.py, unchanged
    assert HOST_RHS_ERROR == (1.61e-16, 3.63e-16) and HOST_ENERGY_ERROR == 3.71e-16
