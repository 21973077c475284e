"""Optimal perturbations on the MI355X (``fc_mass_solve_batch``, ``fc_optpert_*``; csrc/fc_optpert.hip.h, csrc/fc_optpert_run.hpp,
flowcontrol_amd/transient.py) against the numpy block backend of tests/support/optpert_model.py and scipy.

Small problems: the linearised 8 x 8 square (N = 659) and the 7 x 5 rectangle (N = 378, last workgroup partial) of
tests/support/optpert_cases.py; the FlowSolver level runs on the cylinder's O1 mesh."""
import tempfile

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib
from flowcontrol_amd import transient as tr
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS, FcDiverged, FcError
from tests.support import adjoint_batch_cases as bc
from tests.support import optpert_cases as oc
from tests.support import optpert_model as om

pytestmark = pytest.mark.gpu

INV, NOT_READY, NOT_CONV = _lib.FC_ERR_INVALID, _lib.FC_ERR_NOT_READY, _lib.FC_ERR_NOT_CONVERGED
TOL = bc.TOL
RTOL = 1e-12
CHUNK = 8  # kOptpertCgChunk


@pytest.fixture(scope="module")
def sq8():
    sq = oc.Square()
    assert sq.dev.N == 659
    yield sq
    sq.close()


@pytest.fixture(scope="module")
def sq75():
    sq = oc.Rect(7, 5)
    assert sq.th.mesh.cells.shape[0] == 70 and sq.dev.N == 378
    yield sq
    sq.close()


def refused(code, fn, *args, match=None):
    with pytest.raises(FcError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    if match:
        assert match in str(e.value), str(e.value)


def slot_of(order):
    return SLOT_BDF1 if order == 1 else SLOT_BDF2


def rel(a, ref):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(ref)) / np.linalg.norm(ref))


# ── 1. block mass solve ────────────────────────────────────────────────────────────────────────────────────────────────────────────
def check_mass_solve(sq, k):
    dev = sq.dev
    mb = oc.model_blocks(sq, k)
    f, Mff = mb.fidx, mb.Mff
    M = dev.matrix(SLOT_MASS)
    assert abs(M[f][:, f] - Mff).max() == 0.0
    d = 1.0 / np.sqrt(Mff.diagonal())
    kappa = np.linalg.cond((Mff.toarray() * d[:, None]) * d[None, :]) if k == 1 else None
    kappa_M = np.linalg.cond(Mff.toarray())
    b = oc.mass_rhs(sq, k)
    dev.set_batch(k)
    try:
        x, info = dev.mass_solve_batch(b, RTOL, 500)
        x2, info2 = dev.mass_solve_batch(b, RTOL, 500)
        assert np.array_equal(x, x2) and np.array_equal(info, info2), "two identical mass solves differ"
        assert np.all(np.isfinite(x))
        out = np.setdiff1d(np.arange(dev.N), f)
        assert not np.any(x[:, out]), "rows outside f are not exactly zero"
        lu = spla.splu(Mff.tocsc())
        worst_r = worst_e = 0.0
        for c in range(k):
            bf = b[c, f]
            if not np.any(bf):
                assert not np.any(x[c]) and info[c, 0] == 0 and info[c, 1] == 0.0
                continue
            r = np.linalg.norm(Mff @ x[c, f] - bf) / np.linalg.norm(bf)
            e = np.linalg.norm(x[c, f] - lu.solve(bf)) / np.linalg.norm(lu.solve(bf))
            worst_r, worst_e = max(worst_r, r), max(worst_e, e)
            _, it_np, _ = om.jacobi_cg(Mff, bf, RTOL)
            assert info[c, 0] <= it_np + CHUNK, (c, info[c], it_np)
            assert info[c, 1] <= RTOL
        print(f"N = {dev.N}, k = {k}: true residual {worst_r:.2e}, error vs splu {worst_e:.2e}, cond(M_ff) {kappa_M:.1f}, iterations {info[:, 0]}"
              + (f", cond(D^-1/2 M_ff D^-1/2) {kappa:.2f}" if kappa else ""))
        assert worst_r <= 2 * RTOL and worst_e <= kappa_M * 2 * RTOL
        if k >= 2:
            assert np.array_equal(x[0], x[-1]) and np.array_equal(info[0], info[-1]), "equal columns are not bit-equal"
        assert dev.optpert_info()["cg_iterations"] == int(info[:, 0].max())
        # max_iter exhausted: FC_ERR_NOT_CONVERGED, info filled, x finite
        refused(NOT_CONV, dev.mass_solve_batch, b, RTOL, 3)
        x3, info3 = dev.mass_solve_last
        assert np.all(np.isfinite(x3)) and np.all(info3[np.any(b[:, f], axis=1), 0] == 3) and np.all(info3[:, 1] < 1.0)
    finally:
        dev.optpert_reserve(False)
        dev.set_batch(0)
    assert dev.optpert_info()["bytes"] == 0


@pytest.mark.parametrize("k", [1, 4, 5, 9, 17, 32])
def test_mass_solve_square(sq8, k):
    check_mass_solve(sq8, k)


@pytest.mark.parametrize("k", [5, 17])
def test_mass_solve_partial_workgroup(sq75, k):
    check_mass_solve(sq75, k)


# ── 2. apply ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def check_apply(sq, k):
    dev = sq.dev
    mb = oc.model_blocks(sq, k)
    out = np.flatnonzero(mb.fmask == 0.0)
    oc.batch_on(sq, k)
    try:
        dev.optpert_reserve(True)
        U = oc.random_block(sq, k, seed=11 + k)
        dev.optpert_load("U", U)
        Ud = dev.optpert_get("U")
        assert not np.any(Ud[:, out]) and np.array_equal(Ud[:, mb.fidx], U[:, mb.fidx])
        mb.load("U", U)
        for first_order in (1, 2):
            for n in (1, 2, 7):
                H, E = dev.optpert_apply(slot_of(first_order), n)
                G, Y = dev.optpert_get("G"), dev.optpert_get("Y")
                H2, E2 = dev.optpert_apply(slot_of(first_order), n)
                assert np.array_equal(H, H2) and np.array_equal(E, E2) and np.array_equal(G, dev.optpert_get("G")), "two identical applies differ"
                Hm, Em = mb.apply(n, first_order)
                figs = {"G": rel(G, mb.blocks["G"]), "H": rel(H, Hm), "E": rel(E, Em), "Y": rel(Y, mb.blocks["Y"])}
                sym = float(np.max(np.abs(H - H.T)) / np.max(np.abs(H)))
                print(f"N = {dev.N}, k = {k}, first order {first_order}, n = {n}: " + ", ".join(f"{a} {v:.2e}" for a, v in figs.items()) + f", asymmetry {sym:.2e}")
                assert all(v <= TOL for v in figs.values()), figs
                assert sym <= TOL
                assert not np.any(G[:, out]), "G is not exactly zero outside f"
                assert all(oc.padding_is_zero(dev, blk, k) for blk in ("U", "G", "Y")), "a padding column of U, G or the response is not zero"
                u_n, _, p_n = dev.get_state_batch()
                assert np.array_equal(np.c_[u_n, p_n], Y), "the response block is not the batched state"
                info = dev.optpert_info()
                assert info["forward_steps"] == n and info["backward_steps"] == n and info["reserved"]
        # one column seeded with NaN is flagged alone, the others stay within tolerance
        if k >= 5:
            bad = 2
            Ub = U.copy()
            Ub[bad, mb.fidx[3]] = np.nan
            dev.optpert_load("U", Ub)
            with pytest.raises(FcDiverged):
                dev.optpert_apply(SLOT_BDF1, 2)
            assert list(np.flatnonzero(dev.optpert_flags)) == [bad]
            H, E = dev.optpert_last
            G = dev.optpert_get("G")
            Hm, Em = mb.apply(2, 1)
            good = np.setdiff1d(np.arange(k), [bad])
            assert rel(G[good], mb.blocks["G"][good]) <= TOL and rel(E[good], Em[good]) <= TOL and rel(H[np.ix_(good, good)], Hm[np.ix_(good, good)]) <= TOL
    finally:
        dev.optpert_reserve(False)
        oc.batch_off(sq)


@pytest.mark.parametrize("k", [1, 5, 8, 17])
def test_apply_square(sq8, k):
    check_apply(sq8, k)


def test_apply_partial_workgroup(sq75):
    check_apply(sq75, 5)


# ── 3. Gram / combine ──────────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("k", [5, 32])
def test_gram_and_combine(sq75, k):
    sq, dev = sq75, sq75.dev
    mb = oc.model_blocks(sq, k)
    oc.batch_on(sq, k)
    try:
        dev.optpert_reserve(True)
        X, Y = oc.random_block(sq, k, 21, garbage=False), oc.random_block(sq, k, 22, garbage=False)
        dev.optpert_load("U", X)
        dev.optpert_load("V", Y)
        M, u = abs(mb.M), 2.0**-53
        for weighted in (False, True):
            Gd = dev.optpert_gram("U", "V", weighted)
            assert np.array_equal(Gd, dev.optpert_gram("U", "V", weighted)), "a repeated Gram differs"
            ref = X @ ((mb.M @ Y.T) if weighted else Y.T)
            bound = 2 * (dev.N + k) * u * (np.abs(X) @ ((M @ np.abs(Y).T) if weighted else np.abs(Y).T))
            assert np.all(np.abs(Gd - ref) <= bound), float(np.max(np.abs(Gd - ref) / bound))
        # a permutation matrix permutes the columns bit-exactly; an accumulate onto it doubles them; the scale scales
        perm = np.random.default_rng(5).permutation(k)
        Q = np.zeros((k, k))
        Q[perm, np.arange(k)] = 1.0
        dev.optpert_combine("R", "U", Q)
        assert np.array_equal(dev.optpert_get("R"), X[perm])
        dev.optpert_combine("R", "U", Q, accumulate=True)
        assert np.array_equal(dev.optpert_get("R"), 2.0 * X[perm])
        s = 1.0 + np.arange(k)
        dev.optpert_combine("S", "U", Q, scale=s)
        assert np.array_equal(dev.optpert_get("S"), X[perm] * s[:, None])
        Qr = np.random.default_rng(6).standard_normal((k, k))
        dev.optpert_combine("S", "U", Qr)
        assert rel(dev.optpert_get("S"), Qr.T @ X) <= 1e-13
        # padding columns stay zero, read off the device as the blocks lie there ([N][KB]; k = 5: three padding columns): behind a load,
        # a combine, an accumulating and a scaled one, and behind the resident mass solve, which must not iterate on them
        assert dev.optpert_info()["KB"] == (8 if k == 5 else 32) and dev.optpert_block_raw("U").shape == (dev.N, dev.optpert_info()["KB"])
        assert all(oc.padding_is_zero(dev, blk, k) for blk in ("U", "V", "R", "S"))
        refused(INV, dev.optpert_combine, "U", "U", Q, match="different blocks")
        refused(INV, dev.optpert_mass_solve, "V", "V", RTOL, 10, match="different blocks")
        info = dev.optpert_mass_solve("G", "S", RTOL, 500)
        assert oc.padding_is_zero(dev, "G", k)
        Xs = dev.optpert_get("G")
        lu = spla.splu(mb.Mff.tocsc())
        want = np.zeros_like(Xs)
        want[:, mb.fidx] = lu.solve((Qr.T @ X)[:, mb.fidx].T).T
        assert rel(Xs, want) <= np.linalg.cond(mb.Mff.toarray()) * 2 * RTOL and np.all(info[:, 0] > 0)
    finally:
        dev.optpert_reserve(False)
        oc.batch_off(sq)


# ── 4. the whole iteration ─────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name", list(om.CASES))
def test_whole_iteration(sq8, sq75, name):
    c = om.CASES[name]
    sq = sq8 if (c["nx"], c["ny"]) == (8, 8) else sq75
    dev, k = sq.dev, c["k"]
    mb = oc.model_blocks(sq, k)
    X0 = tr.start_block(k, dev.N, None, om.SEED, mb.free)
    tr.orthonormalise_start(mb, X0)
    host = tr.subspace_iteration(mb, c["n"], c["n_modes"], c["tol"], 60, om.FIRST_ORDER, RTOL)
    w, _ = om.dense_reference(mb, c["n"], om.FIRST_ORDER)
    oc.batch_on(sq, k)
    try:
        dev.optpert_reserve(True)
        be = tr.DeviceBlocks(dev)
        assert np.array_equal(be.free, mb.free)
        tr.orthonormalise_start(be, X0)
        res = tr.subspace_iteration(be, c["n"], c["n_modes"], c["tol"], 60, om.FIRST_ORDER, RTOL)
    finally:
        dev.optpert_reserve(False)
        oc.batch_off(sq)
    m = c["n_modes"]
    gap = float(np.max(np.abs(res.gains - w[:m])) / w[0])
    V = res.block
    orth = float(np.max(np.abs(V @ (mb.M @ V.T) - np.eye(k))))
    print(f"{name}: device {res.iterations} iterations (host model {host.iterations}), gains {res.gains}, |gain - dense| / theta_0 {gap:.2e}, "
          f"|U^T M U - I| {orth:.2e}, residuals {res.residuals}")
    assert res.converged and np.all(res.residuals <= c["tol"])
    assert gap <= 1e-8
    assert res.iterations <= host.iterations + 2
    assert orth <= 1e-10


# ── 5. refusals and staleness ──────────────────────────────────────────────────────────────────────────────────────────────────────
def test_refusals_and_staleness(sq75):
    sq, dev = sq75, sq75.dev
    k = 4
    b = oc.mass_rhs(sq, k)
    assert dev.optpert_info()["bytes"] == 0 and not dev.optpert_info()["reserved"]
    refused(NOT_READY, dev.optpert_reserve, True, match="fc_set_batch")
    dev.batch_k = k
    refused(NOT_READY, dev.mass_solve_batch, b, match="fc_set_batch")
    dev.set_solver_options(refine=0, check_residual=1)
    dev.set_batch(k)
    try:
        refused(NOT_READY, dev.optpert_reserve, True, match="fc_set_adjoint_batch")
        refused(NOT_READY, dev.optpert_load, "U", b, match="fc_optpert_reserve")
    finally:
        dev.set_batch(0)
        dev.set_solver_options(refine=1, check_residual=1)
    oc.batch_on(sq, k)
    try:
        dev.optpert_reserve(True)
        assert dev.optpert_info()["reserved"] and dev.optpert_info()["bytes"] > 0 and dev.optpert_info()["KB"] == 4
        dev.optpert_load("U", oc.random_block(sq, k, 3))
        refused(INV, dev.optpert_apply, SLOT_BDF1, 0, match="n_steps")
        refused(INV, dev.optpert_load, 9, b, match="no such block")
        dev.batch_k = 3
        refused(INV, dev.optpert_apply, SLOT_BDF1, 2, match="k differs")
        dev.batch_k = k
        dev.set_adjoint_energy(np.ones((2, k)))
        refused(INV, dev.optpert_apply, SLOT_BDF1, 2, match="energy weights")
        dev.set_adjoint_energy(None)
        dev.set_time_scheme(sq.dt, True)
        refused(INV, dev.optpert_apply, SLOT_BDF1, 2, match="nonlinear")
        refused(INV, dev.optpert_reserve, True, match="nonlinear")
        dev.set_time_scheme(sq.dt, False)
        refused(INV, dev.mass_solve_batch, b, 0.0, 10, match="rtol")
        refused(INV, dev.optpert_apply, 5, 2, match="first_order_slot")
        # what fc_set_adjoint_batch refuses, reserve refuses: refinement sweeps in the solver options
        dev.set_solver_options(refine=1, check_residual=1)
        refused(INV, dev.optpert_reserve, True, match="refinement sweeps")
        refused(INV, dev.optpert_apply, SLOT_BDF1, 2, match="refinement sweeps")
        dev.set_solver_options(refine=0, check_residual=1)
        # a step in flight
        un, unn, pp = bc.column_states(sq.u_n, sq.u_nn, sq.p, k)
        dev.set_state_batch(un, unn, pp)
        dev.step_batch_begin(SLOT_BDF2, np.zeros((k, dev.n_act)), compute_energy=False)
        try:
            refused(INV, dev.optpert_reserve, True, match="in flight")
            refused(INV, dev.optpert_apply, SLOT_BDF1, 2, match="in flight")
            refused(INV, dev.mass_solve_batch, b, match="in flight")
            refused(INV, dev.optpert_gram, "U", "U", match="in flight")
        finally:
            dev.step_batch_end_early()
        # the reserve survives a forward batched step and a plain batched march
        H0, E0 = dev.optpert_apply(SLOT_BDF1, 3)
        un, unn, pp = bc.column_states(sq.u_n, sq.u_nn, sq.p, k)
        dev.set_state_batch(un, unn, pp)
        dev.step_batch(SLOT_BDF2, np.zeros((k, dev.n_act)), compute_energy=False)
        dev.run_adjoint_batch(SLOT_BDF1, 3, None, np.ones((k, dev.N)))
        H1, E1 = dev.optpert_apply(SLOT_BDF1, 3)
        assert np.array_equal(H0, H1) and np.array_equal(E0, E1) and dev.optpert_info()["applies"] == 2
        # reassembling FC_SLOT_MASS with another coefficient marks the tables stale; the next solve uses the new values
        x1, _ = dev.mass_solve_batch(b, RTOL, 500)
        dev.assemble_matrix(SLOT_MASS, mass=2.5, nu=0.0, pressure=0.0, divergence=0.0)
        assert dev.optpert_info()["stale"]
        x2, _ = dev.mass_solve_batch(b, RTOL, 500)
        assert not dev.optpert_info()["stale"]
        mb = oc.model_blocks(sq, k)
        want = np.zeros_like(x2)
        want[:, mb.fidx] = spla.splu((2.5 * mb.Mff).tocsc()).solve(b[:, mb.fidx].T).T
        assert rel(x2, want) <= np.linalg.cond(mb.Mff.toarray()) * 2 * RTOL and rel(x1, 2.5 * want) <= np.linalg.cond(mb.Mff.toarray()) * 2 * RTOL
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        # dropped by fc_set_batch
        dev.set_batch(k)
        assert not dev.optpert_info()["reserved"] and dev.optpert_info()["bytes"] == 0
        refused(NOT_READY, dev.optpert_get, "U", match="fc_optpert_reserve")
    finally:
        dev.set_adjoint_energy(None)
        dev.set_time_scheme(sq.dt, False)
        dev.optpert_reserve(False)
        oc.batch_off(sq)


def test_refusals_on_partitioned_handles_and_after_a_new_permutation():
    """FC_ERR_INVALID on a handle with an exchange; a permutation other than the
    present one releases the reserve -- and a later mass solve, which rebuilds the tables in the new numbering, does not make the old
    blocks valid again."""
    from flowcontrol_amd.device import DeviceSolver
    from flowcontrol_amd.fem.mesh import Mesh
    from flowcontrol_amd.fem.spaces import TaylorHood

    dev = oc.bare_handle()
    try:
        k = 3
        b = np.random.default_rng(1).standard_normal((k, dev.N))
        dev.set_solver_options(refine=0, check_residual=1)
        dev.set_batch(k)
        dev.set_adjoint_factors(SLOT_BDF2, 1)
        dev.set_adjoint_batch(SLOT_BDF2, 1)
        # (FC_ERR_NOT_READY without FC_SLOT_MASS cannot be provoked through DeviceSolver: its setup_solver assembles the slot for the
        #  energy matrix, and a batch needs a solver)
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        dev.optpert_reserve(True)  # (one slot set up: a run of BDF2 steps only)
        dev.optpert_load("U", b)
        H, _ = dev.optpert_apply(SLOT_BDF2, 2)
        assert np.all(np.isfinite(H))
        perm = np.empty(dev.N, dtype=np.int32)
        _lib.check(dev.lib.fc_get_permutation(dev._h, perm))
        _lib.check(dev.lib.fc_set_permutation(dev._h, perm))  # the same permutation: nothing is dropped
        assert dev.optpert_info()["reserved"]
        _lib.check(dev.lib.fc_set_permutation(dev._h, np.ascontiguousarray(perm[::-1])))
        info = dev.optpert_info()
        assert not info["reserved"] and info["bytes"] == 0
        refused(NOT_READY, dev.optpert_get, "U", match="fc_optpert_reserve")
        x, _ = dev.mass_solve_batch(b, RTOL, 500)  # the tables are rebuilt in the new numbering ...
        free = np.setdiff1d(np.arange(2 * dev.nn), dev.bc_dofs)
        Mff = dev.matrix(SLOT_MASS)[free][:, free]
        assert max(np.linalg.norm(Mff @ x[c, free] - b[c, free]) / np.linalg.norm(b[c, free]) for c in range(k)) <= 2 * RTOL
        for call in (lambda: dev.optpert_get("U"), lambda: dev.optpert_gram("U", "U"), lambda: dev.optpert_combine("V", "U", np.eye(k))):
            refused(NOT_READY, call, match="fc_optpert_reserve")  # ... and the blocks of the old one stay gone
    finally:
        dev.close()
    part = DeviceSolver(TaylorHood(Mesh.unit_square(4, 4)))
    try:
        fn = _lib.EXCHANGE_FN(lambda buf, n, user: None)
        _lib.check(part.lib.fc_set_host_exchange(part._h, 2, 0, fn, None))
        part.batch_k = 1
        refused(INV, part.mass_solve_batch, np.ones((1, part.N)), match="partitioned")
        refused(INV, part.optpert_reserve, True, match="partitioned")
    finally:
        part.close()


# ── 6. nothing else moved ──────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_nothing_else_moved(sq8):
    """Batched steps, a batched linearised march, a TAPED NONLINEAR batched march (the handle switched to the nonlinear scheme around a
    taped forward run, while the reserve is held and after applies that ended the tape and rewrote the march's buffers), a single
    march and a batched device closed loop (whose records live in device memory, as the apply's do) return the same bits before a
    reserve, with it, after applies and after the release; the march's bytes return to their earlier values and the
    optimal-perturbation bytes to zero."""
    from flowcontrol_amd.controller import Controller

    sq, dev = sq8, sq8.dev
    k, n = 5, 4
    oc.batch_on(sq, k)
    try:
        un, unn, pp = bc.column_states(sq.u_n, sq.u_nn, sq.p, k)
        u, w, z = bc.column_inputs(n, k, dev.n_act, dev.n_sens, dev.N)

        def probe():
            dev.set_state_batch(un, unn, pp)
            ys = [dev.step_batch(slot_of(1 if m == 0 else 2), u[m], compute_energy=True) for m in range(n)]
            state = dev.get_state_batch()
            g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF1, n, w, z)
            single = dev.run_adjoint(SLOT_BDF1, n, w[:, 0], z[0])
            dev.set_state_batch(un, unn, pp)
            dev.set_controllers([Controller(A=[[-100.0 - s]], B=[[1.0]], C=[[50.0]], D=[[0.0]]) for s in range(k)], sq.dt)
            try:
                loop = dev.run_closed_loop_batch(SLOT_BDF1, n, np.full((k, dev.n_sens), 0.01), compute_energy=True)
            finally:
                dev.set_controllers(None, sq.dt)
            return ([np.array(a, copy=True) for t in ys for a in t[:2]] + [np.array(a, copy=True) for a in state] + [g.copy(), dx0.copy(), dxm1.copy()]
                    + [np.array(a, copy=True) for a in single] + [np.array(a, copy=True) for a in loop])

        def probe_nl():
            dev.set_time_scheme(sq.dt, True)
            try:
                dev.adjoint_tape_reserve_batch(n)
                dev.set_state_batch(un, unn, pp)
                y = bc.forward_batch(dev, 1, u, tape=True)
                tape = dev.adjoint_tape_info_batch()
                assert tape["count"] == n and tape["begun"] and not tape["overflowed"], tape
                X = dev.adjoint_tape_states_batch()
                g, dx0, dxm1 = dev.run_adjoint_batch(SLOT_BDF1, n, w, z)
                assert dev.ADJ_ELEM[int(dev.adjoint_route()[0])] == "fc_adj_elem_nl_b", "the march did not run the nonlinear batched element loop"
                return [y.copy(), X.copy(), g.copy(), dx0.copy(), dxm1.copy()]
            finally:
                dev.adjoint_tape_reserve_batch(0)
                dev.set_time_scheme(sq.dt, False)

        before = probe() + probe_nl()
        bytes0 = {s: dev.adjoint_batch_info(s)["march_bytes"] for s in (SLOT_BDF1, SLOT_BDF2)}
        assert dev.optpert_info()["bytes"] == 0
        dev.optpert_reserve(True)
        dev.optpert_load("U", oc.random_block(sq, k, 31))
        dev.optpert_apply(SLOT_BDF1, 3)
        dev.optpert_mass_solve("V", "G", RTOL, 500)
        with_reserve = probe() + probe_nl()
        dev.optpert_apply(SLOT_BDF2, 2)
        dev.optpert_reserve(False)
        after = probe() + probe_nl()
        assert len(before) == len(with_reserve) == len(after) and np.any(before[-3]) and np.any(before[-2])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, with_reserve)), "a reserve moved a step or a march"
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after)), "a released reserve moved a step or a march"
        assert dev.optpert_info()["bytes"] == 0
        assert {s: dev.adjoint_batch_info(s)["march_bytes"] for s in (SLOT_BDF1, SLOT_BDF2)} == bytes0
    finally:
        dev.optpert_reserve(False)
        oc.batch_off(sq)


# ── 7. FlowSolver level: the linearised cylinder on O1 ───────────────────────────────────────────────────────────────────────────
def test_flowsolver_optimal_perturbations(golden_dir):
    """7. O1, is_eq_nonlinear=False: two iterations of ``fs.optimal_perturbations(n_steps=20, n_modes=2, k=8)``; a BatchedFlowSolver run
    from each returned mode through the public path reproduces the gain as dE_20 / dE_0 to 1e-8 (the Rayleigh property holds
    unconverged).  Everything is released, and ``fs.step`` returns the bits of the first step it returned before the call."""
    from flowcontrol_amd.batch import BatchedFlowSolver
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
    from flowcontrol_amd.fem.spaces import Function
    from flowcontrol_amd.flowsolverparameters import ParamIC

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(), num_steps=50)
    fs.params_solver.is_eq_nonlinear = False
    fs.params_ic = ParamIC(xloc=2.0, yloc=0.0, radius=0.5, amplitude=1.0)
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    n = 20
    try:
        fs.initialize_time_stepping(ic=None)
        y_first = np.array(fs.step([0.0, 0.0]), copy=True)
        fs.initialize_time_stepping(ic=None)
        res = fs.optimal_perturbations(n_steps=n, n_modes=2, k=8, max_iter=2)
        assert res.iterations == 2 and res.gains.shape == (2,) and res.modes.shape == (2, fs.th.N) and res.gains[0] >= res.gains[1] > 0.0
        dev = fs.th.device()
        assert dev.optpert_info()["bytes"] == 0 and all(dev.adjoint_info(s)["bytes"] == 0 for s in (SLOT_BDF1, SLOT_BDF2))
        # flu.mass_solve: the L2 projection M_ff^-1 b_f of one vector and of a block, on the same solver; released again
        from flowcontrol_amd import utils as flu

        free = np.setdiff1d(np.arange(2 * fs.th.nn), dev.bc_dofs)
        b = np.random.default_rng(4).standard_normal((3, fs.th.N))
        xb, x1 = flu.mass_solve(fs, b), flu.mass_solve(fs, b[1])
        Mff = dev.matrix(SLOT_MASS)[free][:, free]
        assert np.array_equal(xb[1], x1) and not np.any(xb[:, np.setdiff1d(np.arange(fs.th.N), free)])
        assert max(np.linalg.norm(Mff @ xb[c, free] - b[c, free]) / np.linalg.norm(b[c, free]) for c in range(3)) <= 2e-12
        assert dev.optpert_info()["bytes"] == 0
        assert np.array_equal(fs.step([0.0, 0.0]), y_first), "fs.step moved"
        bfs = BatchedFlowSolver(fs, 2)
        bfs.initialize_time_stepping(ics=[Function(fs.W, res.modes[i]) for i in range(2)])
        dE0 = bfs.initial_energy
        for _ in range(n):
            bfs.step(np.zeros((2, 2)))
        u_n = bfs.state()[0]
        dEn = np.array([0.5 * fs._velocity_l2_norm(u_n[i]) ** 2 for i in range(2)])
        bfs.close()
        ratio = dEn / dE0
        print(f"O1 linearised, n = {n}, 2 iterations: gains {res.gains}, dE_n / dE_0 {ratio}, residuals {res.residuals}")
        assert np.all(np.abs(ratio - res.gains) <= 1e-8 * res.gains)
        assert np.all(np.abs(dE0 - 0.5) <= 1e-10)
    finally:
        fs.th.release_device()
