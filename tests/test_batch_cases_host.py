"""The host model of the batched factor apply (tests/support/batch_cases.py) on the cases and knob sets that
tests/test_batch_apply_gpu.py runs: together they reach every branch label, no knob set is redundant, and the modelled tables keep
the invariants fc_nd_block_b relies on (it has no bounds checks in its pipeline)."""
import numpy as np
import pytest

from tests.support import batch_cases as bc
from tests.support import front_cases as fcs


@pytest.fixture(scope="module")
def trees():
    return {name: fcs.host_case(nx, ny, bits)[2] for name, nx, ny, bits, _, _ in bc.cases()}


@pytest.fixture(scope="module")
def censuses(trees):
    out = {}
    for name, tree in trees.items():
        for kn, knobs in bc.KNOB_SETS.items():
            m = bc.model(tree, knobs)
            for KB in bc.KBS:
                out[name, kn, KB] = bc.census(tree, knobs, KB, m)
    return out


def test_cases_and_knob_sets_reach_every_label(censuses):
    reached = set().union(*censuses.values())
    for lab in bc.LABELS:
        print(f"{lab:26s}", sorted({f"{c}/{kn}/{KB}" for (c, kn, KB), v in censuses.items() if lab in v})[:4])
    assert reached == set(bc.LABELS), f"not reached: {sorted(set(bc.LABELS) - reached)}"
    assert len(bc.KNOB_SETS) <= 8


def test_no_knob_set_is_redundant(censuses):
    for kn in bc.KNOB_SETS:
        mine = set().union(*[v for (_, k, _), v in censuses.items() if k == kn])
        others = set().union(*[v for (_, k, _), v in censuses.items() if k != kn])
        print(f"{kn:18s} only here: {sorted(mine - others)}")
        assert mine - others, f"knob set {kn} reaches nothing the others do not"


def test_the_extra_case_is_needed(trees, censuses):
    """front_cases.CASES alone never fold a row without sources; the added mesh does."""
    names = [c[0] for c in fcs.CASES]
    assert not any("fold_empty_row" in v for (c, _, _), v in censuses.items() if c in names)
    assert any("fold_empty_row" in v for (c, _, _), v in censuses.items() if c not in names)
    assert all(t.perm.size <= 2500 for t in trees.values())


@pytest.mark.parametrize("kn", list(bc.KNOB_SETS))
def test_model_tables_keep_the_kernel_invariants(trees, kn):
    knobs = bc.KNOB_SETS[kn]
    for name, tree in trees.items():
        m = bc.model(tree, knobs)
        N, S = m.N, int(m.nodes[:, 4].sum())
        assert m.zero_row == 2 * N + S and np.all(m.olist[:32] == m.zero_row)  # the null group
        assert m.olist.size % 32 == 0 and np.all(m.ooff % 32 == 0) and np.all(m.ooff_up % 32 == 0)
        assert np.all((m.olist >= 0) & (m.olist <= m.zero_row))
        tiles = {}
        pslots = 0
        for L in m.launches:
            if L.kind == 1:
                assert 0 <= L.row0 and L.row0 + L.nrows <= N and L.sources.size == L.nrows
                continue
            assert L.tasks
            for t in L.tasks:
                _, _, i0, ni, nb, _, _ = (int(v) for v in m.nodes[t.node])
                ops = m.olist[t.op : t.op + 32 * t.nchunk]
                assert ops.size == 32 * t.nchunk  # every chunk the pipeline reads lies inside the list ...
                first = 32 * t.chunk0
                want = np.r_[np.arange(i0, i0 + ni), [] if L.up else m.olist[m.ooff[t.node] + ni : m.ooff[t.node] + ni + nb]][first : first + t.ncols]
                assert np.array_equal(ops[: t.ncols], want)  # ... names the block's columns ...
                assert np.all(ops[t.ncols :] == m.zero_row), f"{name}: operand list of a task does not end with the zero row"  # ... and ends with padding
                if L.up:
                    assert np.all(ops[: t.ncols] < N)  # the -L block multiplies the node's own y rows only
                    assert 2 * N <= t.dst and t.dst + t.nrows <= 2 * N + S
                else:
                    assert N + i0 <= t.dst and t.dst + t.nrows <= N + i0 + ni
                assert 1 <= t.nrows <= 16 and 1 <= t.parts <= 255 and 0 <= t.part < t.parts
                tiles.setdefault((L.level, L.up, t.node, t.dst), []).append(t)
        for key, parts in tiles.items():
            assert [t.part for t in parts] == list(range(parts[0].parts))
            nchunk = (parts[0].ld + 31) // 32
            edges = [t.chunk0 for t in parts] + [nchunk]
            assert edges[0] == 0 and all(t.chunk0 + t.nchunk == e for t, e in zip(parts, edges[1:])), f"{name} {key}: parts leave a gap"
            assert all(t.nchunk >= 1 for t in parts) and sum(t.ncols for t in parts) == parts[0].ld
            pslots += len(parts) if len(parts) > 1 else 0
        assert pslots == m.pslots
        # fold lists: every scratch row is the source of exactly one destination row
        assert m.fptr[-1] == S and np.array_equal(np.sort(m.fsrc), 2 * N + np.arange(S))
        rows = bc.predicted_launches(m, 16, knobs)
        assert rows.shape == (len(m.launches), len(bc.LAUNCH_COLS)) and np.all(rows[rows[:, 0] == 0, 2] >= 1)


def test_cg_rule_examples():
    """launch_cg against values worked out by hand from batch_launch_cg's rule."""
    L = bc.Launch(0, 0, tasks=[bc.Task(0, 16, 384, 384, 32, 0)])  # 12 chunks
    assert [bc.launch_cg(L, KB) for KB in bc.KBS] == [8, 8, 8, 4]  # 12 / 8 = 1.5 <= 1.5; 12 / 4 = 3 <= 3
    assert bc.launch_cg(L, 16, {"FC_BATCH_CG": "16"}) == 16 and bc.launch_cg(L, 16, {"FC_BATCH_CG": "3"}) == 8
    assert bc.launch_cg(L, 16, {"FC_BATCH_CPW": "6"}) == 2
    P = bc.Launch(0, 0, tasks=[bc.Task(0, 16, 64, 384, 32 + 64 * q, 0, q, 6, 2 * q) for q in range(6)])
    assert bc.launch_cg(P, 16) == 1 and bc.launch_cg(P, 32) == 1  # parts of two chunks: 3 (4) chunks per wave wanted
    assert bc.part_ranges(12, 2) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12)] and bc.part_ranges(2, 2) == [(0, 2)]
    assert len(bc.part_ranges(21, 2)) == 11 and len(bc.part_ranges(23, 16)) == 1 and len(bc.part_ranges(24, 16)) == 2
