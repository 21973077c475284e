"""The snapshot bank of the time-stepping handle (``fc_state_snap_*``, csrc/fc_modal.hip.h) and POD / DMD on it
(flowcontrol_amd/modal.py) on the MI355X: the Gram kernel against a long-double product, the capture against downloaded states,
the untouched trajectories, POD / DMD against the numpy model of tests/support/modal_model.py, the refusals.

Small problem: ``Mesh.unit_square(8, 8)``, N = 659 (odd; three slices of 256 / 256 / 147 rows in the Gram kernel).  The step pipeline
itself (capture sites, overlapped tail, closed loop) runs on the cylinder's O1 mesh."""
import tempfile
import time

import numpy as np
import pytest

from flowcontrol_amd import _lib, linalg, modal
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS, SLOT_SCRATCH, FcError
from flowcontrol_amd.controller import Controller
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.examples.data import controller_file
from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import Function, TaylorHood
from flowcontrol_amd.flowsolverparameters import ParamIC
from flowcontrol_amd.operatorgetter import OperatorGetter
from tests.support import modal_model as mm

pytestmark = pytest.mark.gpu

#: reference examples/operators/compute_eigenvalues.py: the leading eigenvalue of the cylinder at Re = 100 (where get_mat_vp looks)
_EIG_TARGET = 0.13 + 0.77j


# ── the 8 x 8 square: Gram kernel, POD, synthetic DMD, refusals ─────────────────────────────────────────────────────────────────
def _smooth_velocity(th, k=1.0):
    x = th.node_coords
    return np.r_[1.0 + 0.3 * np.sin(k * x[:, 0]) * np.cos(0.7 * k * x[:, 1]), 0.2 * np.cos(0.5 * k * x[:, 0] + 0.1) * np.sin(k * x[:, 1])]


def _bc_setup(th):
    """Dirichlet everywhere but on the x = xmax side, two 'actuators' with smooth profiles (as tests/test_hip_kernels.py)."""
    m = th.mesh
    be = m.boundary_edges()
    be = be[m.edge_midpoints()[be, 0] < m.coords[:, 0].max() - 1e-9]
    nodes = np.unique(np.r_[m.edges[be].reshape(-1), th.nv + be])
    dofs = np.r_[nodes, nodes + th.nn]
    x = th.node_coords[nodes]
    p0 = np.r_[np.sin(x[:, 0] + 2 * x[:, 1]), 0 * x[:, 0]]
    p1 = np.r_[0 * x[:, 0], np.cos(3 * x[:, 0] - x[:, 1])]
    order = np.argsort(dofs)
    return dofs[order], np.stack([p0, p1], axis=1)[order]


@pytest.fixture(scope="module")
def square():
    """The stepping problem of tests/test_hip_kernels.py::test_rhs_solve_step (order 2) on the 8 x 8 square, ready to step."""
    from flowcontrol_amd.device import DeviceSolver

    th = TaylorHood(Mesh.unit_square(8, 8))
    dev = DeviceSolver(th)
    dt, Re = 0.005, 100.0
    U0 = _smooth_velocity(th)
    dofs, prof = _bc_setup(th)
    dev.set_bc(dofs, prof)
    dev.set_time_scheme(dt, True)
    dev.assemble_matrix(SLOT_BDF2, mass=1.5 / dt, nu=1.0 / Re, adv=U0, lin=U0)
    dev.apply_bc(SLOT_BDF2)
    dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
    dev.setup_solver(SLOT_BDF2, refine=1)
    dev.set_sensors([th.point_eval_row((0.31, 0.42), 1)])
    M = dev.matrix(SLOT_MASS)
    yield th, dev, M
    dev.close()


@pytest.fixture(scope="module")
def gram_data(square):
    """130 random columns for each set and the long-double products every Gram test compares with (computed once)."""
    th, dev, M = square
    rng = np.random.default_rng(7)
    X0 = rng.standard_normal((130, dev.N)) * np.exp(rng.uniform(-2.0, 2.0, size=(130, 1)))
    X1 = rng.standard_normal((130, dev.N))
    ref = {None: mm.gram_longdouble(X0, X1), "energy": mm.gram_longdouble(X0, X1, M)}
    bound = {None: mm.gram_bound(X0, X1), "energy": mm.gram_bound(X0, X1, M)}
    return X0, X1, ref, bound


def _raw_gram(dev, lset, a0, a1, rset, b0, b1, slot, pad=7):
    """fc_state_snap_gram into a buffer with `pad` sentinel entries behind the result."""
    out = np.full((a1 - a0) * (b1 - b0) + pad, -7.25)
    _lib.check(dev.lib.fc_state_snap_gram(dev._h, lset, a0, a1, rset, b0, b1, slot, out))
    return out


@pytest.mark.parametrize("weight", [None, "energy"])
@pytest.mark.parametrize("rng_", [(0, 1, 0, 1), (0, 63, 0, 63), (0, 64, 0, 64), (0, 65, 0, 65), (0, 130, 0, 130), (3, 70, 0, 37), (66, 130, 129, 130)])
def test_gram_on_known_data(square, gram_data, weight, rng_):
    """1. L[:, a0:a1]^T Wt R[:, b0:b1] for column counts around the 64-column tile, offset ranges, identity and mass weight: every
    entry within 2 (N + m) 2^-53 |L|^T |Wt| |R| of the long-double product, three calls bit-identical, nothing written behind the
    (a1 - a0)(b1 - b0) entries asked for."""
    th, dev, M = square
    X0, X1, ref, bound = gram_data
    a0, a1, b0, b1 = rng_
    bank = modal.SnapshotBank(dev, 130)
    try:
        bank.load(X0, set=0)
        bank.load(X1, set=1)
        assert (bank.count, bank.kept) == (130, 130)
        slot = modal._weight_slot(weight)
        outs = [_raw_gram(dev, 0, a0, a1, 1, b0, b1, slot) for _ in range(3)]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
        cnt = (a1 - a0) * (b1 - b0)
        assert np.all(outs[0][cnt:] == -7.25)
        G = outs[0][:cnt].reshape(a1 - a0, b1 - b0)
        assert np.array_equal(G, bank.gram(a=(a0, a1), b=(b0, b1), weight=weight, lset=0, rset=1))
        err = np.abs(G.astype(np.longdouble) - ref[weight][a0:a1, b0:b1]).astype(float)
        # the bound of the WHOLE product (m = 130) restricted to the block is no smaller than the block's own (m = its column count)
        N = dev.N
        blk = bound[weight][a0:a1, b0:b1] * (N + max(a1 - a0, b1 - b0)) / (N + 130)
        ratio = float(np.max(err / blk))
        print(f"gram {rng_} weight={weight}: max error / bound = {ratio:.3e}")
        assert ratio <= 1.0
    finally:
        bank.close()


def _square_run(dev, th, n, bank_args=None):
    """n steps of the square's stepping problem from its fixed initial state through fc_run; returns (bank or None, y, dE)."""
    rng = np.random.default_rng(2)
    u_n = 0.1 * _smooth_velocity(th, 2.0) + 0.01 * rng.standard_normal(2 * th.nn)
    u_nn = 0.1 * _smooth_velocity(th, 1.5)
    bank = modal.SnapshotBank(dev, *bank_args) if bank_args else None
    dev.set_state(u_n, u_nn, np.zeros(th.nv))
    y, dE = dev.run(SLOT_BDF2, n, np.array([0.3, -0.2]))
    return bank, y, dE


@pytest.fixture(scope="module")
def pod_run(square):
    """40 captured states of a short run on the square, centred by pod(); the device result and the model's, computed once."""
    th, dev, M = square
    bank, _, _ = _square_run(dev, th, 40, (40, 1, 0))
    try:
        assert bank.count == 40
        X = bank.get()
        assert np.array_equal(X[-1], dev.get_solution())
        res = modal.pod(bank, center=True, weight="energy", modes=True)
        # kept modes: the coefficients of the (centred) snapshots on them are one Gram call, and equal S V^T
        res3 = modal.pod(bank, r=3, modes=False, keep=True)
        assert res3.modes is None and res3.kept_at == 0 and bank.kept == 3
        coef = modal.project(bank)
        bank.clear(1)
        res_one = modal.pod(bank, refine=False)  # the single Gram matrix alone, as the numpy model
    finally:
        bank.close()
    return X, res, res3, coef, res_one, mm.pod(X, M, center=True)


def test_pod_parity(square, pod_run):
    """5. sigma^2 within the Frobenius norm of test 1's bound of the model's Gram eigenvalues (Weyl); Phi^T M Phi = I to 1e-8 for the
    modes with sigma_i >= 1e-3 sigma_0 (2^-53 (sigma_0 / sigma_i)^2 with a margin of 100); the coefficients on kept modes are S V^T."""
    th, dev, M = square
    X, res, res3, coef, _, (sig_m, V_m, Phi_m, mean_m) = pod_run
    Xc = X - mean_m
    weyl = np.linalg.norm(mm.gram_bound(Xc, Xc, M))
    d = np.max(np.abs(res.sigma ** 2 - sig_m ** 2))
    print(f"pod: rank {res.r} of 40, sigma_0 = {res.sigma[0]:.3e}, sigma_r / sigma_0 = {res.sigma[res.r - 1] / res.sigma[0]:.3e}, "
          f"max |sigma^2 - model| = {d:.3e} (bound {weyl:.3e})")
    assert d <= weyl
    assert np.allclose(res.mean, mean_m, rtol=0, atol=1e-14 * np.abs(X).max())
    big = res.sigma[: res.r] >= 1e-3 * res.sigma[0]
    P = res.modes[big]
    orth = np.max(np.abs(P @ (M @ P.T) - np.eye(P.shape[0])))
    print(f"pod: {P.shape[0]} modes above 1e-3 sigma_0, |Phi^T M Phi - I| = {orth:.3e}")
    assert orth <= 1e-8
    assert np.isclose(res.energy.sum(), 1.0)
    assert coef.shape == (3, 40)
    assert np.max(np.abs(coef - (res3.V * res3.sigma[:3]).T)) <= 1e-10 * res3.sigma[0]


def _recon_errors(X, res, M):
    """Relative error of Phi S V^T + mean against the snapshots: in the energy norm the POD is optimal in, and entry-wise (Frobenius,
    pressure included)."""
    D = (res.V * res.sigma[: res.r]) @ res.modes + res.mean - X
    en = lambda Y: np.sqrt(np.sum(Y * (M @ Y.T).T))  # noqa: E731
    return en(D) / en(X), np.linalg.norm(D) / np.linalg.norm(X)


def test_pod_reconstruction(square, pod_run):
    """5. Phi S V^T + mean reproduces the snapshots to 1e-10 relative when r = rank, in the energy norm (the norm this POD is optimal
    in; the weight vanishes on the pressure rows).  The singular values of these 40 states fall without a gap (sigma_13 / sigma_0 =
    3.1e-7), below what ONE Gram matrix in fp64 resolves (sqrt(m eps) sigma_0): the single pass and the numpy model stop at rank 14
    and miss 1e-10 (2.2e-9 measured); pod()'s deflated second pass follows them further down and is what is asserted."""
    th, dev, M = square
    X, res, _, _, res_one, (sig_m, V_m, Phi_m, mean_m) = pod_run
    e_rank = _recon_errors(X, res, M)
    e_one = _recon_errors(X, res_one, M)
    Dm = (V_m * sig_m[: V_m.shape[1]]) @ Phi_m + mean_m - X
    e_model = np.sqrt(np.sum(Dm * (M @ Dm.T).T)) / np.sqrt(np.sum(X * (M @ X.T).T))
    print(f"pod reconstruction: r = rank = {res.r}: energy norm {e_rank[0]:.3e}, Frobenius {e_rank[1]:.3e}; single pass, r = {res_one.r}: "
          f"energy norm {e_one[0]:.3e}, Frobenius {e_one[1]:.3e}; numpy model at its rank {V_m.shape[1]}: energy norm {e_model:.3e}; "
          f"sigma / sigma_0 = {np.array2string(res.sigma[:30] / res.sigma[0], precision=2)}")
    assert res.r > res_one.r
    assert e_rank[0] <= 1e-10


def test_dmd_of_a_synthetic_sequence(square):
    """6a. The synthetic sequence of the host test, loaded into the bank: dmd(r = 6) returns its mu to 1e-10, in both weights."""
    th, dev, M = square
    X, mus = mm.synthetic_sequence(dev.N, 40, seed=5, nvel=2 * th.nn)
    bank = modal.SnapshotBank(dev, 40, every=4)
    try:
        bank.load(X, set=0)
        for weight in ("energy", None):
            res = modal.dmd(bank, r=6, dt=0.01, weight=weight, modes=(weight is None))
            err = mm.match(res.mu, mus)
            print(f"dmd synthetic weight={weight}: max |mu - known| = {err:.3e}")
            assert err <= 1e-10
            assert np.allclose(res.lam, np.log(res.mu) / 0.04) and np.allclose(res.lam_bdf2, mm.bdf2_rate(res.mu, 0.01, 4))
        # exact-DMD modes are eigenvectors of the map x_j -> x_{j+1}: X2 = A X1 on the span, so the columns advance by mu
        Phi = res.modes
        assert Phi.shape == (6, dev.N)
        k = int(np.argmin(np.abs(res.mu - mus[0])))
        coef = np.linalg.lstsq(Phi.T, X[3].astype(complex), rcond=None)[0]
        assert np.linalg.norm(Phi.T @ (coef * res.mu) - X[4]) <= 1e-8 * np.linalg.norm(X[4]) and abs(res.mu[k] - mus[0]) <= 1e-10
    finally:
        bank.close()


def test_refusals(square):
    """7. Each refusal is FC_ERR_INVALID / FC_ERR_NOT_READY with a message, and leaves the bank as it was."""
    th, dev, M = square

    def refused(code, fn, *args):
        with pytest.raises(FcError) as e:
            fn(*args)
        assert e.value.code == code and len(str(e.value)) > 30, str(e.value)

    refused(_lib.FC_ERR_NOT_READY, dev.snap_get, 0, 0, 1)  # no bank
    refused(_lib.FC_ERR_INVALID, dev.snap_reserve, 8, 0, 0)  # every = 0
    refused(_lib.FC_ERR_INVALID, dev.snap_reserve, 8, 1, -1)
    assert dev.snap_info()["capacity"] == 0 and dev.snap_info()["bytes"] == 0
    dev.set_batch(2)
    try:
        refused(_lib.FC_ERR_INVALID, dev.snap_reserve, 8, 1, 0)  # a batch set
        with pytest.raises(RuntimeError, match="batch"):
            modal.SnapshotBank(dev, 8)
    finally:
        dev.set_batch(0)
    bank = modal.SnapshotBank(dev, 8)
    try:
        X = np.random.default_rng(0).standard_normal((5, dev.N))
        bank.load(X, set=0)
        refused(_lib.FC_ERR_INVALID, dev.snap_get, 0, 3, 3)  # get past the count
        refused(_lib.FC_ERR_INVALID, dev.snap_gram, 0, 0, 6, 0, 0, 5, -1)  # ranges past the counts
        refused(_lib.FC_ERR_INVALID, dev.snap_gram, 0, 0, 5, 1, 0, 1, -1)  # an empty set 1
        refused(_lib.FC_ERR_INVALID, dev.snap_mean, 0, 2, 2)
        refused(_lib.FC_ERR_INVALID, dev.snap_load, 0, 6, X[:1])  # a hole behind the count
        refused(_lib.FC_ERR_INVALID, dev.snap_load, 0, 5, X[:4])  # past the capacity
        from flowcontrol_amd.device import DeviceSolver

        fresh = DeviceSolver(th)  # (no slot assembled)
        try:
            fresh.snap_reserve(4)
            fresh.snap_load(0, 0, X[:2])
            refused(_lib.FC_ERR_NOT_READY, fresh.snap_gram, 0, 0, 2, 0, 0, 2, SLOT_SCRATCH)  # an unassembled weight slot
            refused(_lib.FC_ERR_NOT_READY, fresh.snap_push)  # no state on the device
        finally:
            fresh.close()
        Q = np.ones((5, 5))
        bank.combine(Q, keep=True, download=False)
        refused(_lib.FC_ERR_INVALID, dev.snap_combine, 0, 0, 5, Q[:, :4], True, False)  # combine(keep) past the capacity
        refused(_lib.FC_ERR_INVALID, dev.snap_combine, 0, 0, 5, Q, False, False)  # nowhere to put the result
        assert (bank.count, bank.kept) == (5, 5) and np.array_equal(bank.get(), X)
        assert np.allclose(bank.get(set=1), X.sum(axis=0))
    finally:
        bank.close()
    assert dev.snap_info()["bytes"] == 0


def test_partitioned_handle_is_refused():
    """7. A thread-rank (host exchange) handle keeps no bank."""
    from flowcontrol_amd.device import DeviceSolver

    th = TaylorHood(Mesh.unit_square(4, 4))
    dev = DeviceSolver(th)
    try:
        fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
        _lib.check(dev.lib.fc_set_host_exchange(dev._h, 2, 0, fn, None))
        with pytest.raises(FcError) as e:
            dev.snap_reserve(4)
        assert e.value.code == _lib.FC_ERR_INVALID and "partitioned" in str(e.value)
    finally:
        dev.close()


# ── the cylinder (O1): the capture sites of the step pipeline ───────────────────────────────────────────────────────────────────
def _solver(golden_dir, linear=False):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    if linear:
        fs.params_solver.is_eq_nonlinear = False
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


class _O1:
    """A prepared cylinder solver that every test restarts from the same initial state."""

    def __init__(self, fs):
        self.fs, self.dev = fs, fs.th.device()
        self.state0 = [np.array(a, copy=True) for a in self.dev.get_state()]
        self.u0 = np.zeros(self.dev.n_act)

    def restart(self):
        self.dev.set_state(*self.state0)

    def states_at(self, steps):
        """fc_get_solution after the given (increasing, 1-based) step numbers of a run cut into pieces, without a bank."""
        self.restart()
        out, done = [], 0
        for s in steps:
            self.dev.run(SLOT_BDF1 if done == 0 else SLOT_BDF2, s - done, self.u0)
            done = s
            out.append(self.dev.get_solution())
        return np.array(out)


@pytest.fixture(scope="module")
def o1(golden_dir):
    fs = _solver(golden_dir)
    fs.initialize_time_stepping(ic=None)
    fs._begin_stepping()
    yield _O1(fs)
    fs.th.release_device()


def test_capture_is_the_state(o1):
    """2. reserve(8, every = 3, first = 2), 20 steps: the six columns are, bit for bit, fc_get_solution after steps 5, 8, .. 20 of a
    run without a bank -- through fc_run, through 20 single steps (overlapped tail), and through fc_run_closed_loop (against fc_run
    with the controls the loop used); 12 more steps fill the set and drop two; fc_undo_step withdraws count and column."""
    dev = o1.dev
    twin = o1.states_at([5, 8, 11, 14, 17, 20])
    # fc_run
    o1.restart()
    bank = modal.SnapshotBank(dev, 8, every=3, first=2)
    try:
        dev.run(SLOT_BDF1, 20, o1.u0)
        assert bank.count == 6 and bank.dropped == 0 and bank.info()["steps"] == 20
        assert np.array_equal(bank.get(), twin)
        dev.run(SLOT_BDF2, 12, o1.u0)
        info = bank.info()
        assert (info["count"], info["dropped"], info["steps"]) == (8, 2, 32)
        assert np.array_equal(bank.get(0, 6), twin)
        bank.close()
        # 20 single steps, the host back as soon as y is there (the overlapped form of the step)
        o1.restart()
        bank = modal.SnapshotBank(dev, 8, every=3, first=2)
        for s in range(20):
            dev.step_begin(SLOT_BDF1 if s == 0 else SLOT_BDF2, o1.u0)
            dev.step_end(early=True)
        assert bank.count == 6
        assert np.array_equal(bank.get(), twin)
        # undo: steps 21, 22 capture nothing, step 23 is captured and withdrawn
        for _ in range(2):
            dev.step(SLOT_BDF2, o1.u0)
        assert bank.count == 6
        dev.step(SLOT_BDF2, o1.u0)
        assert bank.count == 7 and bank.info()["steps"] == 23
        col7 = bank.get(6, 7)[0]
        assert np.array_equal(col7, dev.get_solution())
        dev.undo_step()
        assert bank.count == 6 and bank.info()["steps"] == 22 and np.array_equal(bank.get(), twin)
        dev.step_begin(SLOT_BDF2, o1.u0)  # ... and the overlapped form of the same step brings the same column back
        dev.step_end(early=True)
        assert bank.count == 7 and np.array_equal(bank.get(6, 7)[0], col7)
        dev.undo_step()
        assert bank.count == 6 and bank.info()["steps"] == 22
        # fc_set_state captures nothing; a push captures now
        o1.restart()
        assert bank.count == 6
        bank.push()
        assert bank.count == 7 and np.array_equal(bank.get(6, 7)[0], np.r_[o1.state0[0], o1.state0[2]])
        bank.close()
        # closed loop on the device
        K0 = Controller.from_file(file=controller_file(), x0=None)
        o1.restart()
        bank = modal.SnapshotBank(dev, 8, every=3, first=2)
        dev.set_controllers([Controller(A=K0.A, B=K0.B, C=K0.C, D=K0.D)], o1.fs.params_time.dt, None)
        y, u, dE = dev.run_closed_loop(SLOT_BDF1, 20, np.array([0.1, 0.0, 0.0]))
        dev.set_controllers(None, o1.fs.params_time.dt)
        assert bank.count == 6 and np.abs(u).max() > 0
        loop_cols = bank.get()
        bank.clear()
        o1.restart()
        bank.close()
        bank = modal.SnapshotBank(dev, 8, every=3, first=2)
        dev.run(SLOT_BDF1, 20, u)
        assert np.array_equal(bank.get(), loop_cols)
        assert not np.array_equal(loop_cols, twin)
    finally:
        bank.close()
        dev.set_controllers(None, o1.fs.params_time.dt)


def test_nothing_else_moved(o1):
    """3. y and dE of 20 steps with a bank reserved == without one == after reserve(0), bit for bit; the bank's bytes return to 0."""
    dev = o1.dev

    def run20():
        o1.restart()
        return dev.run(SLOT_BDF1, 20, o1.u0)

    y0, dE0 = run20()
    bank = modal.SnapshotBank(dev, 20)
    y1, dE1 = run20()
    assert bank.count == 20 and bank.info()["bytes"] >= 20 * dev.N * 8
    bank.close()
    assert dev.snap_info() == dict(capacity=0, count=0, kept=0, every=1, first=0, steps=0, dropped=0, bytes=0)
    y2, dE2 = run20()
    assert np.array_equal(y0, y1) and np.array_equal(dE0, dE1)
    assert np.array_equal(y0, y2) and np.array_equal(dE0, dE2)
    # single steps too (the capture launch sits between the step's tail and the next step's speculated element loop)
    ys = []
    for with_bank in (False, True):
        o1.restart()
        b = modal.SnapshotBank(dev, 8) if with_bank else None
        ys.append([dev.step(SLOT_BDF1 if s == 0 else SLOT_BDF2, o1.u0)[:2] for s in range(6)])
        if b:
            b.close()
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(*ys))


def test_energy_of_the_captured_columns(o1):
    """4. diag(X^T M X) / 2 of the captured columns is the dE the steps reported: both are 1/2 u^T M u summed in different orders,
    N 2^-53 ~ 6e-12 at worst, 1e-12 relative asserted."""
    dev = o1.dev
    o1.restart()
    bank = modal.SnapshotBank(dev, 20)
    try:
        _, dE = dev.run(SLOT_BDF1, 20, o1.u0)
        G = bank.gram(weight="energy")
        assert np.array_equal(G, bank.gram(weight="energy"))
        rel = np.max(np.abs(0.5 * np.diag(G) - dE) / dE)
        print(f"energy: max relative difference of diag(G) / 2 and dE over 20 steps = {rel:.3e}; symmetry {np.max(np.abs(G - G.T)):.3e}")
        assert rel <= 1e-12
    finally:
        bank.close()


def test_flowsolver_records_through_step_and_run(golden_dir):
    """FlowSolver.record_snapshots: the bank follows step(), run() and run_closed_loop() of the solver; the columns are its fields."""
    fs = _solver(golden_dir)
    try:
        fs.initialize_time_stepping(ic=None)
        bank = fs.record_snapshots(12, every=2)
        for _ in range(4):
            fs.step(u_ctrl=[0.0, 0.0])
        fs.run(4, np.zeros(2))
        K0 = Controller.from_file(file=controller_file(), x0=None)
        fs.run_closed_loop(4, Controller(A=K0.A, B=K0.B, C=K0.C, D=K0.D))
        assert bank.count == 6 and bank.info()["steps"] == 12
        last = bank.get(5, 6)[0]
        nn2 = 2 * fs.th.nn
        assert np.array_equal(last[:nn2], fs.fields.u_n.vector().get_local()) and np.array_equal(last[nn2:], fs.fields.p_n.vector().get_local())
        res = modal.pod(bank, modes=False)
        assert res.modes is None and res.sigma.shape == (6,) and res.r >= 1
        bank.close()
    finally:
        fs.th.release_device()


def test_dmd_of_the_linearised_cylinder(golden_dir):
    """6b. Linear equations on O1 from the usual initial condition: 6000 steps of transient skipped, 100 snapshots every 20 steps,
    dmd(r = 2).  The device mu match the numpy model's on the downloaded snapshots to 1e-8, and the leading lam_bdf2 is no farther
    from get_mat_vp's eigenvalue than twice the model's own distance (a property of the data: the decaying modes still present after
    the transient and the two-mode projection; the measured figure is in DESIGN section 5.3)."""
    fs = _solver(golden_dir, linear=True)
    try:
        fs.initialize_time_stepping(ic=None)
        fs._begin_stepping()
        dev = fs.th.device()
        dt = fs.params_time.dt
        u0 = np.zeros(dev.n_act)
        bank = modal.SnapshotBank(dev, 100, every=20, first=6000)
        dev.run(SLOT_BDF1, 4000, u0)
        dev.run(SLOT_BDF2, 4000, u0)
        assert bank.count == 100 and bank.dropped == 0
        res = modal.dmd(bank, r=2, dt=dt, weight="energy")
        X = bank.get()
        assert np.all(np.isfinite(X))
        mu_m, lam_m, lam2_m = mm.dmd(X, dev.matrix(SLOT_MASS), r=2, dt=dt, every=20)
        d_mu = mm.match(res.mu, mu_m)
        A, E, _, _ = OperatorGetter(fs).get_all()
        valp, _ = linalg.get_mat_vp(A.tocsr(), E.tocsr(), n=2, target=_EIG_TARGET, tol=1e-10, flowsolver=fs)
        lead = valp[0]  # (nearest the target first: the leading eigenvalue, 0.1326 + 0.7700i)
        assert abs(lead - (0.132643 + 0.770015j)) <= 1e-5
        pick = lambda lam: lam[np.argmax(lam.imag)]  # noqa: E731  (the member of the pair in the upper half plane)
        d_dev, d_model = abs(pick(res.lam_bdf2) - lead), abs(pick(lam2_m) - lead)
        print(f"dmd O1 linear: mu = {res.mu}, |mu - model| = {d_mu:.3e}; get_mat_vp {lead:.6f}, lam_bdf2 {pick(res.lam_bdf2):.6f} "
              f"(distance {d_dev:.3e}), model {pick(lam2_m):.6f} (distance {d_model:.3e}), lam = log(mu) / (every dt) {pick(res.lam):.6f}; "
              f"sigma_1 / sigma_0 = {res.sigma[1] / res.sigma[0]:.3e}, sigma_2 / sigma_0 = {res.sigma[2] / res.sigma[0]:.3e}")
        assert d_mu <= 1e-8
        assert d_dev <= 2.0 * d_model
        bank.close()
    finally:
        fs.th.release_device()


def test_device_gram_beats_download_and_host_product(o1):
    """Measurements, condition 2: X^T M X of 256 columns on O1, operator pass included, takes less wall time on the device than
    downloading the 256 columns and forming the product with scipy / numpy on the host."""
    dev = o1.dev
    bank = modal.SnapshotBank(dev, 256)
    try:
        rng = np.random.default_rng(1)
        for c in range(0, 256, 64):
            bank.load(rng.standard_normal((64, dev.N)), set=0)
        M = dev.matrix(SLOT_MASS)
        bank.gram(weight="energy")  # (the work buffers are sized by the first call)
        t0 = time.perf_counter()
        G = bank.gram(weight="energy")
        t_dev = time.perf_counter() - t0
        last = dev.snap_gram_last()
        t0 = time.perf_counter()
        X = bank.get()
        t_get = time.perf_counter() - t0
        Gh = X @ (M @ X.T)
        t_host = time.perf_counter() - t0
        print(f"O1 gram 256 x 256 (N = {dev.N}): device {1e3 * t_dev:.2f} ms wall, {last['ms']:.3f} ms by HIP events "
              f"({last['flops'] / last['ms'] * 1e-9:.2f} TFLOP/s, {last['bytes'] / 1e6:.1f} MB); host {1e3 * t_host:.1f} ms of which the download "
              f"{1e3 * t_get:.1f} ms")
        assert np.max(np.abs(G - Gh)) <= 1e-10 * np.abs(Gh).max()
        assert t_dev < t_host
    finally:
        bank.close()
