"""The shifted solver's complex GMRES (``fc_shifted_set_krylov``): solves on lagged factors after ``fc_shifted_set_shift``, the
rescue of a solve on inexact factors, the untouched default, and a frequency sweep that factorises every third frequency only."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from flowcontrol_amd import _lib, linalg
from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver
from flowcontrol_amd.fem.spaces import Function
from flowcontrol_amd.operatorgetter import OperatorGetter
from tests.support.shifted_open import Open as _Open

pytestmark = pytest.mark.gpu

S1, S2 = 0.3 + 0.7j, 0.3 + 0.75j
#: GMRES tolerance of the sweep.  The true residual of a double-precision solve cannot go below about eps |M| |x| / |b|, and near the
#: cylinder's eigenvalue 0.13 + 0.77i the response x is some 1e3 to 1e4 times b: a floor of 1e-13 .. 1e-12, so 1e-12 cannot be asked
#: for there.  1e-11 lies above that floor and two orders below the 1e-9 the response is compared to.
SWEEP_RTOL = 1e-11


@pytest.fixture()
def prob():
    p = _Open()
    yield p
    p.lib.fc_destroy(p.h)


def test_lagged_factor_solve(prob):
    """Factors of sigma_1 = 0.3 + 0.7i, solves at sigma_2 = 0.3 + 0.75i by GMRES(60) on them: scipy's LU at sigma_2 to 1e-9, between 1
    and 200 iterations per column, one factorisation, and the same bits when the call is repeated.  scipy's gmres with the
    splu(sigma_1) preconditioner is run on the same pair of shifts first: the cap of 200 must be far away for it too."""
    p = prob
    M2 = (S2 * p.E - p.A).astype(complex).tocsc()
    count = [0]
    P = spla.LinearOperator(M2.shape, matvec=p.lu(S1).solve, dtype=complex)
    for c in range(2):
        count[0] = 0
        _, flag = spla.gmres(M2, p.b[c], M=P, rtol=1e-12, restart=60, maxiter=4, callback=lambda r: count.__setitem__(0, count[0] + 1),
                             callback_type="pr_norm")
        print("scipy gmres, splu(sigma_1) preconditioner: column", c, "iterations", count[0], "flag", flag)
        assert flag == 0 and count[0] <= 50
    p.setup(S1)
    p.ok(p.lib.fc_shifted_set_krylov(p.h, 200, 60, 1e-12))
    p.ok(p.lib.fc_shifted_set_shift(p.h, S2.real, S2.imag))
    rc, x, info = p.solve()
    p.ok(rc)
    it, cnt = p.krylov_info()
    print("lagged solve: error", p.rel_err(x, S2), "residuals", info, "iterations", it, "counters", cnt)
    assert p.rel_err(x, S2) <= 1e-9
    assert np.all(info <= 1e-12)
    assert np.all((1 <= it) & (it <= 200)) and cnt[0] == 1 and cnt[3] == 2 and cnt[4] == 0
    rc, x2, _ = p.solve()
    p.ok(rc)
    np.testing.assert_array_equal(x2, x)
    # fc_setup_shifted sets both shifts again: the direct solve at sigma_2, no iterations
    p.setup(S2)
    rc, x3, _ = p.solve()
    p.ok(rc)
    it, cnt = p.krylov_info()
    assert np.all(it == 0) and cnt[0] == 2 and p.rel_err(x3, S2) <= 1e-10


def test_set_shift_needs_krylov_and_the_default_is_untouched(prob):
    p = prob
    p.setup(S1)
    rc, x0, info0 = p.solve()
    p.ok(rc)
    assert p.lib.fc_shifted_set_shift(p.h, S2.real, S2.imag) == _lib.FC_ERR_INVALID
    assert b"Krylov" in p.lib.fc_last_error()
    # the new entry points called and switched off again: the same bits as a handle that never saw them
    q = _Open()
    try:
        q.ok(q.lib.fc_shifted_set_krylov(q.h, 200, 60, 1e-12))
        q.ok(q.lib.fc_shifted_set_pin(q.h, q.N - 1, 1.0))
        q.ok(q.lib.fc_shifted_set_pin(q.h, -1, 0.0))
        q.ok(q.lib.fc_shifted_set_krylov(q.h, 0, 0, 0.0))
        q.setup(S1)
        rc, x1, info1 = q.solve()
        q.ok(rc)
    finally:
        q.lib.fc_destroy(q.h)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(info1, info0)
    # Krylov on, accurate factors: nothing to rescue, the same bits again
    p.ok(p.lib.fc_shifted_set_krylov(p.h, 200, 60, 1e-12))
    rc, x2, _ = p.solve()
    p.ok(rc)
    np.testing.assert_array_equal(x2, x0)
    assert np.all(p.krylov_info()[0] == 0)


def test_rescue_of_a_solve_on_inexact_factors(prob):
    """refine = 0 and factor values off by a relative 1e-4 (fc_debug_scale_shifted_factors): the plain solve misses 1e-8 and fails;
    with Krylov on the same call continues with GMRES from that iterate, reaches rtol and equals scipy's LU to 1e-9."""
    p = prob
    p.setup(S1, refine=0)
    p.ok(p.lib.fc_shifted_set_krylov(p.h, 200, 60, 1e-12))
    p.setup(S1, refine=0)
    p.ok(p.lib.fc_debug_scale_shifted_factors(p.h, 1.0 + 1e-4))
    rc, x, info = p.solve()
    p.ok(rc)
    it, cnt = p.krylov_info()
    print("rescue: error", p.rel_err(x, S1), "residuals", info, "iterations", it)
    assert np.all(info <= 1e-12) and p.rel_err(x, S1) <= 1e-9
    assert np.all((1 <= it) & (it <= 200)) and cnt[0] == 2 and cnt[3] == 2 and cnt[4] == 2
    # an Arnoldi step solves on the same factors: counted as a rescue too, and the step is that of the exact operator
    v0 = np.random.default_rng(3).standard_normal(2 * p.N)
    p.ok(p.lib.fc_shifted_arnoldi_start(p.h, 4, v0))
    hcol, beta = np.zeros(2), C.c_double()
    p.ok(p.lib.fc_shifted_arnoldi_step(p.h, 0, hcol, C.byref(beta)))
    _, cnt = p.krylov_info()
    assert cnt[4] == 4 and cnt[3] == 4
    z = v0[0::2] + 1j * v0[1::2]
    q0 = -p.lu(S1).solve(p.E @ z)
    q0 /= np.linalg.norm(q0)
    w = -p.lu(S1).solve(p.E @ q0)
    assert abs((hcol[0] + 1j * hcol[1]) - np.vdot(q0, w)) <= 1e-9 * np.linalg.norm(w)
    p.ok(p.lib.fc_shifted_set_krylov(p.h, 0, 0, 0.0))
    rc, _, info = p.solve()
    print("plain solve on the same factors: residuals", info)
    assert rc == _lib.FC_ERR_NOT_CONVERGED and np.all(info > 1e-8)
    # the next numeric factorisation is exact again
    p.setup(S1, refine=0)
    rc, x, info = p.solve()
    p.ok(rc)
    assert p.rel_err(x, S1) <= 1e-9


@pytest.fixture(scope="module")
def cyl(tmp_path_factory, golden_dir):
    fs = CylinderFlowSolver.make_default(Re=100, path_out=tmp_path_factory.mktemp("krylov_cyl"))
    U0, P0 = Function(fs.W, np.load(golden_dir / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    A, E, B, Cm = OperatorGetter(fs).get_all()
    yield fs, A.tocsr(), E.tocsr(), np.asarray(B, dtype=float), np.asarray(Cm, dtype=float)
    fs.th.release_device()


def test_sweep_on_lagged_factors(cyl):
    """Cylinder O1, six frequencies 0.70 .. 0.80: factorising every third one only gives the H of factorising all six to 1e-9 max|H|,
    with two numeric factorisations instead of six."""
    fs, A, E, B, Cm = cyl
    ww = np.linspace(0.70, 0.80, 6)
    H, counts, iters = {}, {}, []
    for every in (1, 3):
        op = linalg.ShiftedOperator(fs, A, E, krylov={"max_iter": 200, "restart": 60, "rtol": SWEEP_RTOL} if every > 1 else None)
        try:
            if every == 1:
                H[every], _ = linalg.frequency_response(op, B, Cm, ww, verbose=False)
            else:
                Hs = np.zeros((Cm.shape[0], B.shape[1], ww.size), dtype=complex)
                for i, w in enumerate(ww):  # (frequency_response's own loop, with the iteration counts read in between)
                    Hi, _ = linalg.frequency_response(op, B, Cm, [w], verbose=False) if i % every == 0 else (None, None)
                    if Hi is None:
                        op.shift(1j * w)
                        Hi = op.transfer(B, Cm)[:, :, None]
                        iters.append(op.last_iterations.copy())
                    Hs[:, :, i] = Hi[:, :, 0]
                Hloop = Hs
                op.release()
                H[every], _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=every)
                np.testing.assert_array_equal(H[every], Hloop)
            counts[every] = op.krylov_info()["refactorisations"]
        finally:
            op.release()
    err = np.max(np.abs(H[3] - H[1])) / np.max(np.abs(H[1]))
    print("sweep: |dH| / max|H| =", err, "refactorisations", counts, "GMRES iterations per lagged frequency", [list(i) for i in iters])
    assert err <= 1e-9
    assert counts == {1: 6, 3: 2}
    assert all(np.all(i >= 1) for i in iters)
    # the public entry point with the keyword: the same numbers
    Hp, _ = linalg.get_frequency_response_sequential(A, B, Cm, E, ww, verbose=False, flowsolver=fs, refactor_every=3,
                                                     krylov={"max_iter": 200, "restart": 60, "rtol": SWEEP_RTOL})
    np.testing.assert_array_equal(Hp, H[3])
    with pytest.raises(ValueError, match="refactor_every"):
        linalg.frequency_response(linalg.ShiftedOperator(fs, A, E), B, Cm, ww, verbose=False, refactor_every=3)


def test_sweep_falls_back_to_refactorising(cyl, caplog):
    """One GMRES iteration is not enough on lagged factors: every second frequency logs the miss and is refactorised after all --
    the H of refactor_every = 1, bit for bit, with four numeric factorisations for four frequencies."""
    fs, A, E, B, Cm = cyl
    ww = np.linspace(0.70, 0.76, 4)
    op = linalg.ShiftedOperator(fs, A, E)
    try:
        Href, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False)
    finally:
        op.release()
    op = linalg.ShiftedOperator(fs, A, E, krylov={"max_iter": 1, "restart": 1, "rtol": 1e-11})
    try:
        with caplog.at_level("WARNING", logger="flowcontrol_amd.linalg"):
            H, _ = linalg.frequency_response(op, B, Cm, ww, verbose=False, refactor_every=2)
        info = op.krylov_info()
    finally:
        op.release()
    np.testing.assert_array_equal(H, Href)
    assert info["refactorisations"] == 4 and info["gmres_solves"] == 2 and info["rescues"] == 0
    assert sum("refactorising there" in r.getMessage() for r in caplog.records) == 2


def test_eigen_solve_reports_the_rescue(cyl):
    """ShiftedOperator.rescued after an eigen solve: False on exact factors, True when the Arnoldi steps ran on perturbed ones (the
    solves inside fc_shifted_arnoldi_step are counted by the library); the eigenvalue is the same."""
    fs, A, E, B, Cm = cyl
    lam = {}
    for scale in (None, 1.0 + 1e-4):
        # (exact factors: the default two refinement steps; perturbed ones: none, so that every solve misses 1e-8 before GMRES)
        op = linalg.ShiftedOperator(fs, A, E, refine=2 if scale is None else 0, krylov=True)  # (rtol 1e-10: sigma lies 0.04 from an eigenvalue)
        try:
            op.factor(0.1 + 0.8j)
            if scale is not None:
                _lib.check(op.lib.fc_debug_scale_shifted_factors(op._h, scale))
            kry = linalg.DeviceKrylov(op)
            v, _, _ = linalg.krylov_schur(kry, 1, 20, 0.1 + 0.8j, tol=1e-8)
            lam[scale] = v[0]
            assert op.rescued == (scale is not None), op.krylov_info()
        finally:
            op.release()
    assert abs(lam[None] - lam[1.0 + 1e-4]) <= 1e-7
