"""numpy model of the adjoint factor layout of the shifted solver (``fc_fe_export_t``) — TEST INFRASTRUCTURE.

The factor values of a tree node are the rows ``[D^-1 | -U]`` (``ni x (ni + nb)``) followed by the block ``-L`` (``nb x ni``).  With
``P M P^T = (I + L) D (I + U)`` the transpose is ``(I + U^T) D^T (I + L^T)``, so the values of the transposed system in the SAME layout
are, node by node,

    rows [D^-1 | -U]  <-  [(D^-1)^T | (-L)^T]
    block -L          <-  (-U)^T

Signs and offsets stay as they are.  ``transpose_values`` applies that to a value array; it takes the node table either as the
``plan_nodes`` of ``fc_sym_build_shifted`` / ``FactorPlan.nodes`` ([g, 7]: level, front offset, nf, ni, value offset, parent, slot) or as
``BlockFactors.nodes`` ([g, 7]: level, node, i0, ni, nb, value offset, index offset)."""
from __future__ import annotations

import numpy as np


def node_shapes(nodes, table: str = "plan") -> list[tuple[int, int, int]]:
    """(ni, nb, value offset) per node with a pivot block.  ``table="plan"``: ``plan_nodes`` ([g, 7] or flat); ``"block"``:
    ``BlockFactors.nodes``.  (Both are [g, 7] integer tables: the caller says which one it passes.)"""
    tab = np.asarray(nodes, dtype=np.int64).reshape(-1, 7)
    if table == "plan":
        return [(int(ni), int(nf - ni), int(vo)) for _, _, nf, ni, vo, _, _ in tab if ni > 0]
    if table == "block":
        return [(int(ni), int(nb), int(vo)) for _, _, _, ni, nb, vo, _ in tab if ni > 0]
    raise ValueError(f"table must be 'plan' or 'block', got {table!r}")


def transpose_values(vals: np.ndarray, nodes, table: str = "plan") -> np.ndarray:
    """The value array of the transposed system in the same layout (entries outside the nodes are copied)."""
    out = np.array(vals, dtype=np.float64, copy=True)
    for ni, nb, vo in node_shapes(nodes, table):
        nf = ni + nb
        W = vals[vo : vo + ni * nf].reshape(ni, nf)
        if nb:
            L = vals[vo + ni * nf : vo + ni * nf + nb * ni].reshape(nb, ni)
            out[vo : vo + ni * nf] = np.concatenate([W[:, :ni].T, L.T], axis=1).ravel()
            out[vo + ni * nf : vo + ni * nf + nb * ni] = W[:, ni:].T.ravel()
        else:
            out[vo : vo + ni * ni] = W.T.ravel()
    return out


def transpose_positions(rowptr: np.ndarray, col: np.ndarray) -> np.ndarray:
    """tpos[k] = position of the entry (j, i) for every entry k = (i, j) of a CSR pattern with sorted rows (the rule of
    ``fc_shifted_set_adjoint``); ValueError for an entry without a partner."""
    n = rowptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    keys = rows * n + col.astype(np.int64)
    want = col.astype(np.int64) * n + rows
    pos = np.searchsorted(keys, want)
    bad = (pos >= keys.size) | (keys[np.minimum(pos, keys.size - 1)] != want)
    if np.any(bad):
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"entry ({rows[k]}, {col[k]}) has no partner: the pattern is not structurally symmetric")
    return pos.astype(np.int32)
