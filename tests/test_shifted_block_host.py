"""Host side of the block sweeps (flowcontrol_amd.linalg): the grouping of a frequency grid into factorisation groups and blocks, the
expansion of (inputs, shifts) into block columns, and the refusals of ShiftedOperator that need no device."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from flowcontrol_amd import linalg


def test_groups_are_factorised_at_their_geometric_middle():
    ww = np.logspace(-1, 1, 64)
    groups = linalg.sweep_groups(ww, 16, 2)
    assert [(g["start"], g["stop"]) for g in groups] == [(0, 16), (16, 32), (32, 48), (48, 64)]
    for g in groups:
        assert g["mid"] == pytest.approx(np.sqrt(ww[g["start"]] * ww[g["stop"] - 1]), rel=1e-15)
        assert ww[g["start"]] < g["mid"] < ww[g["stop"] - 1]
        assert g["blocks"] == [(g["start"], g["stop"])]  # 16 frequencies x 2 inputs = 32 columns: one block


def test_blocks_hold_at_most_32_columns_and_remainders_are_kept():
    ww = np.linspace(0.5, 2.0, 45)
    for every, nu in ((32, 2), (20, 3), (7, 1), (1, 4), (45, 32)):
        groups = linalg.sweep_groups(ww, every, nu)
        seen = []
        for g in groups:
            assert g["stop"] - g["start"] == min(every, ww.size - g["start"])
            assert g["blocks"][0][0] == g["start"] and g["blocks"][-1][1] == g["stop"]
            for (j0, j1), nxt in zip(g["blocks"], g["blocks"][1:] + [None]):
                assert 1 <= (j1 - j0) * nu <= linalg.MAX_BLOCK
                assert nxt is None or nxt[0] == j1
                if nxt is not None:  # only a group's last block may be short
                    assert j1 - j0 == linalg.MAX_BLOCK // nu
                seen.extend(range(j0, j1))
        assert seen == list(range(ww.size))
    # a remainder group: 45 = 2 x 20 + 5
    g = linalg.sweep_groups(ww, 20, 3)[-1]
    assert (g["start"], g["stop"]) == (40, 45) and g["blocks"] == [(40, 45)]
    assert linalg.sweep_groups(ww, 20, 3)[0]["blocks"] == [(0, 10), (10, 20)]


def test_middle_of_a_group_with_a_nonpositive_frequency_is_arithmetic():
    g = linalg.sweep_groups([0.0, 1.0, 2.0], 3, 1)[0]
    assert g["mid"] == 1.0
    assert linalg.sweep_groups([2.0], 4, 1)[0]["mid"] == 2.0


def test_group_arguments_are_checked():
    with pytest.raises(ValueError, match="refactor_every"):
        linalg.sweep_groups([1.0], 0, 1)
    with pytest.raises(ValueError, match="inputs"):
        linalg.sweep_groups([1.0], 1, 33)


def test_column_expansion():
    n = 6
    b = np.arange(2 * n, dtype=float).reshape(n, 2)
    # [n, k] with k shifts: as given
    cols, sig = linalg.expand_block_columns(b, [1j, 2j], 2)
    assert np.array_equal(cols, b) and np.array_equal(sig, [1j, 2j])
    # [n, nu] with 3 shifts, k = 6: every input at every shift, shift-major
    cols, sig = linalg.expand_block_columns(b, [1j, 2j, 3j], 6)
    assert cols.shape == (n, 6) and cols.dtype == complex
    assert np.array_equal(sig, [1j, 1j, 2j, 2j, 3j, 3j])
    for s in range(3):
        assert np.array_equal(cols[:, 2 * s:2 * s + 2], b)
    # the same count of shifts and inputs, but a block of 4: the expansion
    cols, sig = linalg.expand_block_columns(b, [1j, 2j], 4)
    assert cols.shape == (n, 4) and np.array_equal(sig, [1j, 1j, 2j, 2j])
    # one vector, one shift
    cols, sig = linalg.expand_block_columns(np.ones(n), 0.5j, 1)
    assert cols.shape == (n, 1) and sig.shape == (1,)
    with pytest.raises(ValueError, match="block width"):
        linalg.expand_block_columns(b, [1j, 2j, 3j], 5)
    with pytest.raises(ValueError, match="finite"):
        linalg.expand_block_columns(b, [1j, np.nan], 2)
    with pytest.raises(ValueError, match="1 .. 32"):
        linalg.expand_block_columns(np.ones((n, 3)), np.arange(11) * 1j)
    with pytest.raises(ValueError, match="empty"):
        linalg.expand_block_columns(b, [], 2)


def _hosted(n=5):
    """A ShiftedOperator on a stand-in for the device: nothing below reaches the library."""
    A = sp.identity(n, format="csr")
    dev = types.SimpleNamespace(lib=None, N=n, nn=1, _h=None, rowptr=np.arange(n + 1, dtype=np.int32), colidx=np.arange(n, dtype=np.int32))
    return types.SimpleNamespace(th=types.SimpleNamespace(device=lambda: dev)), A


def test_solve_block_refusals_without_a_device():
    fs, A = _hosted()
    with pytest.raises(ValueError, match="krylov"):
        linalg.ShiftedOperator(fs, A, A, block=4)
    with pytest.raises(ValueError, match="block must be in"):
        linalg.ShiftedOperator(fs, A, A, krylov=True, block=33)
    op = linalg.ShiftedOperator(fs, A, A)
    with pytest.raises(ValueError, match="Krylov"):
        op.solve_block(np.ones((5, 2)), [1j, 2j])
    with pytest.raises(ValueError, match="Krylov"):
        op.set_block(2)
    with pytest.raises(ValueError, match="block=True"):
        linalg.frequency_response(op, np.ones((5, 1)), np.ones((1, 5)), [1.0], verbose=False, block=True)
    op = linalg.ShiftedOperator(fs, A, A, krylov=True, block=4)
    with pytest.raises(ValueError, match="factor"):
        op.set_block(4)
    with pytest.raises(ValueError, match="rows"):
        op.solve_block(np.ones((4, 4)), [1j] * 4)
    with pytest.raises(ValueError, match="block width"):
        op.solve_block(np.ones((5, 3)), [1j, 2j])
    with pytest.raises(ValueError, match="no block is set"):
        op.solve_block(np.ones((5, 4)), [1j, 2j, 3j, 4j])
    with pytest.raises(ValueError, match="0 .. 32"):
        op.set_block(40)
