"""Inputs and device helpers of the batched adjoint march tests (tests/test_adjoint_batch_host.py, tests/test_adjoint_batch_gpu.py) --
TEST INFRASTRUCTURE.

What is batch-specific about ``fc_run_adjoint_batch`` is that column s must see ITS trajectory, ITS weights and ITS terminal vector, and
that nothing is averaged before the march.  So every column gets its own initial state, control sequence, weights and terminal vector;
the seeds are fixed here (the host test shows on the scipy models that these inputs tell the mistakes apart)."""
from __future__ import annotations

import numpy as np

#: the project's series tolerance against its oracle, and central differences of a forward run at EPS
TOL, EPS, TOL_FD = 1e-8, 1e-4, 1e-6
#: seeds of the per-column inputs (chosen on the CPU: tests/test_adjoint_batch_host.py)
SEED_INPUTS, SEED_STATES = 41, 43


def column_inputs(n, k, n_act, n_sens, N, seed=SEED_INPUTS):
    """(u [n, k, n_act], w [n, k, n_sens], z [k, N]), all different per column."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k, n_act)), rng.standard_normal((n, k, n_sens)), rng.standard_normal((k, N))


def column_states(u_n, u_nn, p, k, seed=SEED_STATES):
    """(u_n [k, .], u_nn [k, .], p [k, .]): column s starts from the case's state scaled by 1 + 0.5 s / k and perturbed by its own noise."""
    rng = np.random.default_rng(seed)
    scale = 1.0 + 0.5 * np.arange(k) / max(k, 1)
    amp = float(np.max(np.abs(u_n)))
    un = scale[:, None] * u_n[None, :] + 0.05 * amp * rng.standard_normal((k, u_n.size))
    unn = scale[:, None] * u_nn[None, :] + 0.05 * amp * rng.standard_normal((k, u_nn.size))
    pp = np.tile(p, (k, 1)) + 0.01 * rng.standard_normal((k, p.size))
    return un, unn, pp


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(ref)) / np.linalg.norm(ref))


def rel_columns(a, ref, axis_k):
    """Relative defect of every column (axis ``axis_k``) on its own: the worst one."""
    a, ref = np.moveaxis(np.asarray(a), axis_k, 0), np.moveaxis(np.asarray(ref), axis_k, 0)
    return max(rel(a[s], ref[s]) for s in range(a.shape[0]))


# ── the model, column by column ────────────────────────────────────────────────────────────────────────────────────────────────────
def model_forward_nl(model, first_order, u, x0, xm1):
    """X [k, n + 2, N], y [n, k, n_sens] of the nonlinear model, one run per column."""
    k = u.shape[1]
    runs = [model.forward(first_order, u[:, s], x0[s], xm1[s]) for s in range(k)]
    return np.array([r[0] for r in runs]), np.stack([r[1] for r in runs], axis=1)


def model_adjoint_nl(model, first_order, X, w, z):
    """(g [n, k, n_act], dx0 [k, N], dxm1 [k, N]) of the nonlinear model, one march per column."""
    k = X.shape[0]
    out = [model.adjoint(first_order, X[s], w[:, s], None if z is None else z[s]) for s in range(k)]
    return np.stack([o[0] for o in out], axis=1), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def model_adjoint_lin(model, first_order, n, w, z):
    """The same for the linearised model."""
    k = w.shape[1]
    out = [model.adjoint(first_order, n, w[:, s], None if z is None else z[s]) for s in range(k)]
    return np.stack([o[0] for o in out], axis=1), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ── device side ────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def batch_on(sq, k, tape=0):
    """The square's handle with a batch of k, direct factor apply, transposed factors of both slots and the batched adjoint setup."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    dev = sq.dev
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(k)
    for s in (SLOT_BDF1, SLOT_BDF2):
        dev.set_adjoint_factors(s, 1)
        dev.set_adjoint_batch(s, 1)
    if tape:
        dev.adjoint_tape_reserve_batch(tape)


def batch_off(sq, refine=1):
    """Everything of batch_on released: the handle steps single runs as before."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    dev = sq.dev
    dev.adjoint_tape_reserve_batch(0)
    for s in (SLOT_BDF1, SLOT_BDF2):
        dev.set_adjoint_batch(s, -1)
        dev.set_adjoint_factors(s, -1)
    dev.set_batch(0)
    dev.set_solver_options(refine=refine, check_residual=1)
    sq.restart()


def forward_batch(dev, first_order, u, tape=False):
    """n batched steps with u [n, k, n_act] from the present batched state: y [n, k, n_sens]."""
    from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2

    if tape:
        dev.adjoint_tape_begin_batch()
    y = np.empty((u.shape[0], dev.batch_k, dev.n_sens))
    for m in range(u.shape[0]):
        y[m], _, _ = dev.step_batch(SLOT_BDF1 if (m == 0 and first_order == 1) else SLOT_BDF2, u[m], compute_energy=False)
    return y
