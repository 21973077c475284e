"""A checkpointed walk over the numpy models of the adjoint marches (``adjoint_nl_model`` as the plant of ``adjoint_loop_model.Loop``)
-- TEST INFRASTRUCTURE for the checkpointed state tape (``fc_adjoint_tape_reserve_sparse``; DESIGN section 5.4 "Checkpointed tape").

``SegmentedTape`` stands where a forward run's ``X [n + 2, N]`` stands in ``Loop.adjoint``: the model reads its states only as
``X[col]`` (col 0 = x_{-1}, col m + 1 = x_m), and this object answers from what a checkpointed tape holds --

  * checkpoint j = the pair (x_{jc-1}, x_{jc}), j = 0 .. ceil(n / c) - 1,
  * one buffer of c + 2 columns: while it holds segment j, column 0 = x_{jc-1}, column 1 = x_{jc}, column i + 1 = x_{jc+i},
  * the control u_m every step read --

restated here from the layout alone, not from csrc/fc_adjoint_segments.hpp.  The forward run writes it step by step as the device
does; a read of a column whose segment the buffer does not hold recomputes that segment from its checkpoint with the model's own
``plant_step`` on the taped controls (no controller runs), which is why the walk's gradients are ``array_equal`` to the full walk's."""
from __future__ import annotations

import numpy as np


class SegmentedTape:
    def __init__(self, loop, f, c: int):
        """``f``: the dict of ``loop.forward()``; its ``X`` is consumed one row per step and not kept."""
        self.loop, self.c, self.n = loop, int(c), int(loop.n)
        n, c = self.n, self.c
        X = f["X"]
        self.u = np.array(f["u"], dtype=float)  # the control tape: what the plant step read, behind signals and limits
        self.ckpt = [None] * -(-n // c)
        self.buf = [None] * (c + 2)
        self.buf[0], self.buf[1] = X[0].copy(), X[1].copy()  # begin(): (x_{-1}, x_0) into the buffer and into checkpoint 0
        self.ckpt[0] = (self.buf[0].copy(), self.buf[1].copy())
        for m in range(1, n + 1):
            j, i = divmod(m - 1, c)  # step m is step i + 1 of segment j
            if i == 0 and j > 0:  # it opens the segment: the buffer's last pair goes to the store and to columns 0, 1
                self.ckpt[j] = (self.buf[c].copy(), self.buf[c + 1].copy())
                self.buf[0], self.buf[1] = self.ckpt[j][0].copy(), self.ckpt[j][1].copy()
            self.buf[i + 2] = X[m + 1].copy()
        self.resident = (n - 1) // c  # the segment the buffer holds: the forward run's last one
        self.replayed = 0
        self.reads = []

    @property
    def columns_held(self) -> int:
        return 2 * len(self.ckpt) + len(self.buf)

    def _replay(self, j: int) -> None:
        p, c = self.loop.plant, self.c
        self.buf[0], self.buf[1] = self.ckpt[j][0].copy(), self.ckpt[j][1].copy()
        for m in range(j * c + 1, min((j + 1) * c, self.n) + 1):
            i = m - j * c  # x_m -> column i + 1, from columns i (x_{m-1}) and i - 1 (x_{m-2})
            self.buf[i + 1] = self.loop.plant_step(p.order_of(m, self.loop.first_order), self.buf[i], self.buf[i - 1], self.u[m - 1])
            self.replayed += 1
        self.resident = j

    def __getitem__(self, col: int):
        """Global column ``col``: x_{col - 1}.  Columns 0 and 1 are read in segment 0."""
        col = int(col)
        if not 0 <= col <= self.n + 1:
            raise IndexError(col)
        j = 0 if col < 2 else (col - 2) // self.c
        if j != self.resident:
            self._replay(j)
        self.reads.append(col)
        return self.buf[col - j * self.c]


def segmented_adjoint(loop, f, c: int, w, r, z=None):
    """``loop.adjoint`` over a checkpointed tape of spacing ``c``: (gradients, the tape)."""
    tape = SegmentedTape(loop, f, c)
    g = loop.adjoint({**f, "X": tape}, w, r, z)
    return g, tape
