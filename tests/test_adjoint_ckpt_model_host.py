"""The index arithmetic of the checkpointed state tape, pinned without a GPU: the numpy model of the closed-loop adjoint
(``tests/support/adjoint_loop_model.py`` around the nonlinear plant of ``tests/support/adjoint_nl_model.py``) marched over a
``SegmentedTape`` (``tests/support/adjoint_ckpt_model.py``) -- checkpoints every c steps, one dense segment, recomputation from the
taped controls -- must return the gradients of the march over the full trajectory, ``array_equal``, for n = 7 and c in 1, 2, 3, 7, 9."""
import numpy as np
import pytest

from tests.support import adjoint_ckpt_model as cm
from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm

N_STEPS = 7
SPACINGS = (1, 2, 3, 7, 9)


@pytest.fixture(scope="module")
def plant():
    return lc.host_plant(True)


@pytest.fixture(scope="module", params=[1, 2], ids=["bdf1", "bdf2"])
def full(plant, request):
    """One forward run and the full walk, computed once and left unchanged: (loop, forward run, w, r, z, gradients)."""
    model, x0, xm1 = plant
    loop, w, r, z = lc.make_case(model, x0, xm1, request.param, N_STEPS)
    f = loop.forward()
    lm.assert_limits_tell(f["v"], loop.lo, loop.hi)  # (the clamp is active on some control values and inactive on others)
    return loop, f, w, r, z, loop.adjoint(f, w, r, z)


@pytest.mark.parametrize("c", SPACINGS)
def test_segmented_walk_equals_the_full_walk(full, c):
    loop, f, w, r, z, want = full
    got, tape = cm.segmented_adjoint(loop, f, c, w, r, z)
    for k in lm.GROUPS + ("ubar",):
        assert np.array_equal(got[k], want[k]), f"c = {c}: {k}"
    n = N_STEPS
    segs = -(-n // c)
    assert tape.columns_held == 2 * segs + c + 2
    assert tape.replayed == n - (n - (segs - 1) * c)  # all but the last segment's steps
    # backward step m < n reads x_m (column m + 1), in descending order, then the two products read x_0 and x_{-1}
    assert tape.reads == list(range(n, 1, -1)) + [1, 0]
    assert tape.resident == 0


def test_a_wrong_column_map_is_seen(full):
    """The comparison has teeth: a tape whose buffer is read one column off gives other gradients."""
    loop, f, w, r, z, want = full

    class OffByOne(cm.SegmentedTape):
        def __getitem__(self, col):
            return super().__getitem__(min(col + 1, self.n + 1))

    got = loop.adjoint({**f, "X": OffByOne(loop, f, 3)}, w, r, z)
    assert not np.array_equal(got["dx0"], want["dx0"])
