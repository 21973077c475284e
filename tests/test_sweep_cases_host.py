"""The host model of the single-vector factor apply (tests/support/sweep_cases.py) on the cases, knob sets and runs that
tests/test_sweep_apply_gpu.py executes: together they reach every template instance of the sweep kernels and every branch label outside
UNREACHED, no knob set is redundant, the modelled tiles agree with ndsolver.down_blocks and stay inside the bounds the kernels rely on
(none of them checks an index)."""
import numpy as np
import pytest

from tests.support import front_cases as fcs
from tests.support import ndsolver
from tests.support import sweep_cases as sc


@pytest.fixture(scope="module")
def trees():
    return {name: fcs.host_case(nx, ny, bits)[2] for name, nx, ny, bits, _, _ in sc.cases()}


@pytest.fixture(scope="module")
def models(trees):
    out = {}
    for kn, runs in sc.RUNS.items():
        for hs, bits, case in runs:
            fac_stages = 2 * trees[case].depth + 1
            knobs = {**sc.KNOB_SETS[kn], **sc.handle_knobs(hs, fac_stages)}
            out[kn, hs, bits, case] = (knobs, sc.model(trees[case], knobs, bits))
    return out


@pytest.fixture(scope="module")
def censuses(models):
    return {key: sc.census(m) for key, (_, m) in models.items()}


def test_runs_reach_every_instance_and_every_label_outside_unreached(censuses):
    reached = set().union(*censuses.values())
    for lab in sc.LABELS:
        print(f"{lab:24s}", sorted("/".join(map(str, k)) for k, v in censuses.items() if lab in v)[:3])
    unreached = {lab for lab, _ in sc.UNREACHED}
    assert all(reason for _, reason in sc.UNREACHED)
    # what may stay unreached: branch labels, among them the descriptor rounds at shuffle widths 32 and 64 and the multi-tile block
    assert unreached <= set(sc.BRANCH_LABELS)
    assert set(sc.INSTANCE_LABELS) <= reached, f"instances not reached: {sorted(set(sc.INSTANCE_LABELS) - reached)}"
    assert reached == set(sc.LABELS) - unreached, f"not reached: {sorted(set(sc.LABELS) - unreached - reached)}; reached after all: {sorted(reached & unreached)}"
    assert len(sc.KNOB_SETS) <= 6 and set(sc.RUNS) == set(sc.KNOB_SETS)
    assert len(sc.INSTANCE_LABELS) == 36 + 10 + 9 + 12 + 8 + 4 + 12


def test_no_knob_set_is_redundant(censuses):
    for kn in sc.KNOB_SETS:
        mine = set().union(*[v for k, v in censuses.items() if k[0] == kn])
        others = set().union(*[v for k, v in censuses.items() if k[0] != kn])
        print(f"{kn:16s} only here: {sorted(mine - others)}")
        assert mine - others, f"knob set {kn} reaches nothing the others do not"


def test_knobs_are_where_the_library_reads_them(models):
    """Process-level knobs only in KNOB_SETS, handle-level ones only in HANDLE_SETS; every child starts with a default handle."""
    for kn, knobs in sc.KNOB_SETS.items():
        assert set(knobs) <= set(sc.PROCESS_KNOBS)
        assert sc.RUNS[kn][0][:2] == ("default", 64)
    for hs in sc.HANDLE_SETS:
        assert set(sc.handle_knobs(hs, 7)) <= set(sc.HANDLE_KNOBS)
    assert all(t <= 6000 for t in (m.N for _, m in models.values()))


def test_the_extra_cases_are_needed(censuses):
    """No case of batch_cases has an up row of more than 16 segments or a row wider than FC_BLK_TILE; the three added ones do."""
    from tests.support import batch_cases as bc

    old = {c[0] for c in bc.cases()}
    for lab, case in (("desc_rounds_sw16", "bin8x6"), ("desc_rounds_sw32", "bin32x16"), ("block_multi_tile", "twoleaf22x20")):
        reach = {k[3] for k, v in censuses.items() if lab in v}
        assert case in reach and not reach & old, (lab, reach)
    assert {k[3] for k, v in censuses.items() if "desc_rounds_sw32" in v} == {"bin32x16"}


def test_model_tiles_equal_down_blocks_and_stay_in_bounds(trees, models):
    for (kn, hs, bits, case), (knobs, m) in models.items():
        fac = ndsolver.factorize_blocks(None, trees[case])
        N, n_val = fac.N, fac.vals.size
        begin, count, lpr, val, row0, nrows, i0, ni, idx, nb = m.down_tables
        for s, st in enumerate(m.stages):
            assert (st.kind, st.row0, st.nrows) == (int(fac.stage_kind[s]), int(fac.stage_row0[s]), int(fac.stage_nrows[s]))
            if knobs.get("FC_BLOCK_KERNEL") == "0":
                assert not st.blk
                continue
            q = slice(int(begin[s]), int(begin[s]) + int(count[s]))
            # retile_flat only cuts tiles: the modelled tiles of a stage, merged per node, are down_blocks' tiles
            assert sum(b.nrows for b in st.blk) == int(nrows[q].sum()) == (st.nrows if count[s] else 0)
            assert {(b.i0, b.ni, b.idx, b.nb) for b in st.blk} == set(zip(i0[q].tolist(), ni[q].tolist(), idx[q].tolist(), nb[q].tolist()))
            assert {b.val for b in st.blk} >= set(val[q].tolist()) and {b.row0 for b in st.blk} >= set(row0[q].tolist())
            if st.blk:
                assert st.blk_lpr == int(lpr[s])
            rows = np.zeros(N, dtype=int)
            for b in st.blk:
                rows[b.row0 : b.row0 + b.nrows] += 1
                assert 1 <= b.nrows <= 32 and 0 <= b.val and b.val + b.nrows * b.wd <= n_val
                assert 0 <= b.i0 and b.i0 + b.ni <= N and b.idx + b.nb <= fac.idx.size
                if st.blk_flat:  # fc_nd_flat_block: vs[256 * U], xs[FC_FLAT_WD]
                    assert b.nrows * b.wd <= 256 * st.blk_flat and b.wd <= sc.FLAT_WD
                else:
                    assert b.nrows <= st.blk_rps * (256 // st.blk_lpr)
            if st.blk:
                assert np.all(rows[st.row0 : st.row0 + st.nrows] == 1) and rows.sum() == st.nrows
        S = int(fac.nodes[:, 4].sum())
        slots = np.zeros(S, dtype=int)
        for L in m.levels:
            for b in L.blk:
                slots[b.row0 : b.row0 + b.nrows] += 1
                assert b.nb == 0 and 0 <= b.val and b.val + b.nrows * b.ni <= n_val and b.i0 + b.ni <= N
                if L.flat:
                    assert b.nrows * b.ni <= 256 * L.flat and b.ni <= sc.FLAT_WD
                else:
                    assert b.nrows <= L.rps * (256 // L.lpr)
            assert L.sources.size == L.fold_nrows and sum(b.nrows for b in L.blk) == L.rows
        assert np.all(slots == 1)  # every scratch row is written by exactly one tile
        assert sum(int(L.sources.sum()) for L in m.levels) == S  # ... and folded exactly once
        got = sc.predicted_launches(m)
        assert got.shape[1] == len(sc.LAUNCH_COLS) and np.all(got[:, 4] >= 1)


def test_rule_examples():
    """The geometry rules against values worked out by hand from fc_solver_setup, flat_loads and block_target."""
    # 128 * 1.4142 * 1024 = 185 362.02, * 2048 = 370 724.05, * 4096 = 741 448.09
    assert [sc.block_target(n) for n in (1000, 185362, 185363, 370725, 741448, 741449, 2000000)] == [1024, 1024, 2048, 4096, 4096, 8192, 8192]
    assert sc.flat_loads({}, 256, 1024) == 4 and sc.flat_loads({}, 257, 1024) == 0 and sc.flat_loads({}, 100, 1025) == 8
    assert sc.flat_loads({"FC_FLAT_ROW": "512"}, 512, 4096) == 16 and sc.flat_loads({"FC_FLAT_ROW": "600"}, 513, 1) == 0
    assert sc.flat_loads({"FC_FLAT_ROW": "0"}, 8, 8) == 0 and sc.flat_loads({}, 8, 4097) == 0
    assert sc.flat_tile_values({}) == 2048 and sc.flat_tile_values({"FC_FLAT_TILE": "1"}) == 256 and sc.flat_tile_values({"FC_FLAT_TILE": "9999"}) == 4096
    # an up stage of 100 rows with 4 segments of 40 values each: sub = pow2_ceil(10) = 16, four segments side by side -> 64 lanes
    st = sc.Stage(0, 0, 100, np.full(100, 4), np.full(400, 40), np.zeros(400, bool))
    sc._stage_geometry(st, 0, {})
    assert (st.lanes, st.sub, st.bytes) == (64, 16, 8.0 * 16000 + 16.0 * 400 + 100 * 24.0)
    sc._stage_geometry(st, 0, {"FC_UP_THREADS": "3200"})  # 3200 / (100 * 16) = 2 segments side by side
    assert (st.lanes, st.sub) == (32, 16)
    sc._stage_geometry(st, 1, {"FC_SWEEP_GEOM": "8:4,256:32"})
    assert (st.lanes, st.sub) == (256, 32)
    # a down stage: rows of 30 + 50 values -> mean segment 40, lanes = pow2_ceil(40 / 2) = 32; FC_DOWN_DEPTH=1: 64
    dn = sc.Stage(1, 0, 10, np.full(10, 2), np.tile([30, 50], 10), np.tile([False, True], 10))
    sc._stage_geometry(dn, 0, {})
    assert (dn.lanes, dn.sub) == (32, 32)
    sc._stage_geometry(dn, 0, {"FC_DOWN_DEPTH": "1"})
    assert (dn.lanes, dn.sub) == (64, 64)
    # few long rows: a whole workgroup per row
    root = sc.Stage(1, 0, 1500, np.full(1500, 1), np.full(1500, 1500), np.zeros(1500, bool))
    sc._stage_geometry(root, 0, {})
    assert (root.lanes, root.sub) == (256, 256)


def test_round_values_is_round_to_nearest_even():
    v = np.array([1.0, 1.0 + 2.0**-8, 1.0 + 3 * 2.0**-8, 1.0 + 2.0**-8 + 2.0**-20, -(1.0 + 2.0**-24), 0.0, 3.0e-5])
    assert np.array_equal(sc.round_values(v, 64), v)
    assert np.array_equal(sc.round_values(v, 32), v.astype(np.float32).astype(np.float64))
    got = sc.round_values(v, 16)  # bf16: 8 significant bits -- ties go to the even neighbour
    assert np.array_equal(got[:6], [1.0, 1.0, 1.0 + 2.0**-6, 1.0 + 2.0**-7, -1.0, 0.0])
    assert abs(got[6] / v[6] - 1) <= 2.0**-8


def test_longdouble_apply_is_the_block_solve(trees):
    """apply_longdouble against nd_numeric.block_solve on host factors: the same operation, so they agree to fp64 round-off."""
    from tests.support import batch_cases as bc
    from tests.support import nd_numeric

    name, nx, ny, bits, _, _ = [c for c in sc.cases() if c[0] == "deep8x6"][0]
    th, dofs, tree = fcs.host_case(nx, ny, bits)
    A = bc.host_operator(th, dofs, 300.0)
    fac = nd_numeric.factorize_blocks(A, tree)
    B = sc.rhs_set(tree, bc.rhs_pool(A.shape[0], 5), dofs)
    assert np.count_nonzero(B[sc.N_RHS]) == 1 and np.count_nonzero(B[sc.N_RHS + 1]) == 1
    X = sc.apply_longdouble(fac, fac.vals, B)
    for j in range(B.shape[0]):
        assert np.linalg.norm(X[j] - nd_numeric.block_solve(fac, B[j])) <= 1e-13 * np.linalg.norm(X[j])
        assert np.linalg.norm(A @ X[j] - B[j]) <= 1e-12 * np.linalg.norm(B[j])
