"""Device handles and shared inputs of tests/test_optpert_gpu.py -- TEST INFRASTRUCTURE.

Two linearised handles: the 8 x 8 square of tests/support/adjoint_step_child.py (``Square``, N = 659) and the 7 x 5 rectangle with the
same boundary conditions and base field (N = 378, 70 cells: the last workgroup of the row-lane kernels is partial), each with the scipy
``StepModel`` of its device-assembled matrices; ``batch_on`` / ``batch_off`` of tests/support/adjoint_batch_cases.py switch the batch,
the transposed factors and the batched adjoint setup on and off."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.support import optpert_model as om
from tests.support.adjoint_batch_cases import batch_off, batch_on  # noqa: F401  (the tests' switches)
from tests.support.adjoint_step_child import Square, bc_setup, smooth_velocity


class Rect(Square):
    """``Square`` on an nx x ny mesh."""

    def __init__(self, nx=7, ny=5, refine=1):
        from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS
        from flowcontrol_amd.device import DeviceSolver
        from flowcontrol_amd.fem.mesh import Mesh
        from flowcontrol_amd.fem.spaces import TaylorHood
        from tests.support import adjoint_step_model as am

        th = self.th = TaylorHood(Mesh.unit_square(nx, ny))
        dev = self.dev = DeviceSolver(th)
        self.dt, Re = om.DT, om.RE
        U0 = smooth_velocity(th)
        dofs, prof = bc_setup(th)
        self.dofs, self.prof = dofs, prof
        dev.set_bc(dofs, prof)
        dev.set_time_scheme(self.dt, False)
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        self.M = dev.matrix(SLOT_MASS)
        raw, A = {}, {}
        for order, slot, c in ((1, SLOT_BDF1, 1.0 / self.dt), (2, SLOT_BDF2, 1.5 / self.dt)):
            dev.assemble_matrix(slot, mass=c, nu=1.0 / Re, adv=U0, lin=U0)
            raw[order] = dev.matrix(slot)
            dev.apply_bc(slot)
            A[order] = dev.matrix(slot)
            dev.setup_solver(slot, refine=refine)
        row = th.point_eval_row((0.31, 0.42), 1)
        dev.set_sensors([row])
        G = np.zeros((dev.N, 2))
        G[dofs] = prof
        C = sp.csr_matrix((row[1], (np.zeros(len(row[0]), dtype=int), row[0])), shape=(1, dev.N))
        self.model = am.StepModel(A[1], A[2], self.M, dofs, prof, raw[1] @ G, raw[2] @ G, C, self.dt)
        rng = np.random.default_rng(2)
        self.u_n = 0.1 * smooth_velocity(th, 2.0) + 0.01 * rng.standard_normal(2 * th.nn)
        self.u_nn = 0.1 * smooth_velocity(th, 1.5)
        self.p = 0.01 * rng.standard_normal(th.nv)


def bare_handle(nx=4, ny=3, mass=False):
    """A small linearised handle with the BDF2 slot set up and, unless ``mass``, NO assembled mass slot (the refusal tests)."""
    from flowcontrol_amd._lib import SLOT_BDF2, SLOT_MASS
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    th = TaylorHood(Mesh.unit_square(nx, ny))
    dev = DeviceSolver(th)
    dofs, prof = bc_setup(th)
    dev.set_bc(dofs, prof)
    dev.set_time_scheme(om.DT, False)
    U0 = smooth_velocity(th)
    dev.assemble_matrix(SLOT_BDF2, mass=1.5 / om.DT, nu=1.0 / om.RE, adv=U0, lin=U0)
    dev.apply_bc(SLOT_BDF2)
    dev.setup_solver(SLOT_BDF2, refine=1)
    dev.set_sensors([th.point_eval_row((0.31, 0.42), 1)])
    if mass:
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
    return dev


def padding_is_zero(dev, block, k) -> bool:
    """Columns k .. KB - 1 of a resident block as it lies on the device are exactly zero."""
    return not np.any(dev.optpert_block_raw(block)[:, k:])


def model_blocks(sq, k):
    return om.ModelBlocks(sq.model, k, 2 * sq.th.nn)


def random_block(sq, k, seed, garbage=True):
    """(k, N) random; with ``garbage`` the pressure and Dirichlet rows hold values a load must zero."""
    X = np.random.default_rng(seed).standard_normal((k, sq.dev.N))
    if not garbage:
        X *= model_blocks(sq, k).fmask
    return X


def mass_rhs(sq, k, seed=7):
    """b (k, N) random on all N rows; column 1 is zero (k >= 3) and the last column repeats column 0 (k >= 2)."""
    b = np.random.default_rng(seed).standard_normal((k, sq.dev.N))
    if k >= 3:
        b[1] = 0.0
    if k >= 2:
        b[-1] = b[0]
    return b
