"""Balanced reduced models from frequency snapshots (``flowcontrol_amd.rom``), host side: the quadrature, the reduced matrices from the
small Gram matrices against the numpy / scipy model that forms them from explicit modes (tests/support/rom_model.py), the 2 * tail
error bound of balanced truncation on the 10 x 10 open-square operator, order selection, saving, and the argument checks."""
import numpy as np
import pytest

from flowcontrol_amd import rom
from flowcontrol_amd.controller import Controller
from tests.support import rom_model as M


@pytest.fixture(scope="module")
def model24():
    A, E, B, C = M.host_fixture()
    ww, weights = rom.log_quadrature(*M.BAND, 24)
    return M.Model(A, E, B, C, ww, weights)


@pytest.fixture(scope="module")
def full_H(model24):
    m = model24
    return M.full_response(m.A, m.E, m.B, m.C, M.CHECK_WW)


def test_quadrature_integrates_one_over_w():
    for lo, hi, nq in ((0.05, 200.0, 24), (0.05, 200.0, 6), (0.4, 1.5, 8), (1e-3, 1e3, 1)):
        ww, weights = rom.log_quadrature(lo, hi, nq)
        assert ww.shape == weights.shape == (nq,) and np.all(np.diff(ww) > 0) and lo < ww[0] and ww[-1] < hi
        assert abs(np.sum(weights / ww) - np.log(hi / lo)) <= 1e-13
        ww_m, weights_m = M.log_quadrature(lo, hi, nq)
        np.testing.assert_allclose(ww, ww_m, rtol=1e-14)
        np.testing.assert_allclose(weights, weights_m, rtol=1e-14)
    # exact for polynomials in log w up to degree 2 nq - 1: int (log w)^3 / w dw
    ww, weights = rom.log_quadrature(0.5, 8.0, 2)
    exact = (np.log(8.0) ** 4 - np.log(0.5) ** 4) / 4.0
    assert abs(np.sum(weights * np.log(ww) ** 3 / ww) - exact) <= 1e-12 * abs(exact)


def test_reduced_matrices_from_grams_equal_those_from_modes(model24):
    m = model24
    for r in (4, 8, 12):
        red = rom.reduced_from_grams(m.GE, m.GA, m.ZtB, m.CXs, m.ww, m.weights, H=m.H, r=r)
        assert red.r == r and red.A.shape == (r, r) and red.B.shape == (r, 2) and red.C.shape == (3, r) and not red.D.any()
        np.testing.assert_allclose(red.hsv, m.hsv, rtol=1e-12, atol=1e-14 * m.hsv[0])
        assert red.error_bound == pytest.approx(m.tail(r), rel=1e-12)
        # the transfer function does not depend on the signs of the singular vectors: compare through it and through the matrices
        # the model forms from explicit modes
        Am, Bm, Cm = m.from_modes(r)
        Ag, Bg, Cg = m.from_grams(r)
        for got, ref in ((Ag, Am), (Bg, Bm), (Cg, Cm), (red.A, Am), (red.B, Bm), (red.C, Cm)):  # (one SVD of one matrix: the same signs)
            assert np.max(np.abs(got - ref)) <= 1e-11 * max(1.0, np.max(np.abs(ref)))
        Hm = M.response(Am, Bm, Cm, M.CHECK_WW)
        Hp = red.frequency_response(M.CHECK_WW)
        assert np.max(np.abs(Hp - Hm)) <= 1e-11 * np.max(np.abs(Hm))
        np.testing.assert_allclose(np.sort_complex(red.eigenvalues()), np.sort_complex(np.linalg.eigvals(Am)), rtol=1e-9, atol=1e-9)


def test_modes_are_biorthogonal(model24):
    m = model24
    for r in (4, 8, 12):
        _, rr, TL, TR = rom.balancing_factors(m.GE, r)
        Phi, Psi = m.Xs @ TR, m.Zs @ TL.T
        err = np.max(np.abs(Psi.T @ (m.E @ Phi) - np.eye(r)))
        print(f"r = {r}: |Psi^T E Phi - I| = {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("r", [4, 8, 12])
def test_truncation_error_is_within_twice_the_tail(model24, full_H, r):
    m = model24
    red = rom.reduced_from_grams(m.GE, m.GA, m.ZtB, m.CXs, m.ww, m.weights, r=r)
    err = M.worst_error(full_H, red.frequency_response(M.CHECK_WW))
    print(f"r = {r}: max |H - H_r|_2 = {err:.4e} = {err / red.error_bound:.3f} x the bound {red.error_bound:.4e}")
    assert err <= red.error_bound
    assert np.all(red.eigenvalues().real < 0.0)


def test_order_selection_by_tolerance(model24):
    m = model24
    for tol in (1e-1, 1e-3, 1e-6):
        red = rom.reduced_from_grams(m.GE, m.GA, m.ZtB, m.CXs, m.ww, m.weights, tol=tol)
        r = red.r
        assert 2.0 * np.sum(m.hsv[r:]) <= tol * m.hsv[0] < 2.0 * np.sum(m.hsv[r - 1:])
    assert rom.select_order(np.array([1.0, 0.1, 0.01]), 0.3) == 1
    assert rom.select_order(np.array([1.0, 0.1, 0.01]), 0.02) == 2
    assert rom.select_order(np.array([1.0, 0.1, 0.01]), 0.0) == 3


def test_save_round_trips_through_controller(model24, tmp_path):
    m = model24
    red = rom.reduced_from_grams(m.GE, m.GA, m.ZtB, m.CXs, m.ww, m.weights, r=8)
    path = tmp_path / "rom8.mat"
    red.save(path)
    K = Controller.from_file(path)
    for name in "ABCD":
        np.testing.assert_array_equal(getattr(K, name), getattr(red, name))


def test_argument_checks(model24):
    m = model24
    A, E, B, C = m.A, m.E, m.B, m.C
    with pytest.raises(ValueError, match="weights"):
        rom.balanced_rom(A, B, C, E, m.ww, m.weights[:-1], r=4)
    with pytest.raises(ValueError, match="positive"):
        rom.balanced_rom(A, B, C, E, np.r_[0.0, m.ww[1:]], m.weights, r=4)
    with pytest.raises(ValueError, match="positive"):
        rom.balanced_rom(A, B, C, E, -m.ww, m.weights, r=4)
    with pytest.raises(ValueError, match="band"):
        rom.balanced_rom(A, B, C, E, r=4)
    with pytest.raises(ValueError, match="tol"):
        rom.balanced_rom(A, B, C, E, m.ww, m.weights)
    with pytest.raises(ValueError, match="flowsolver"):
        rom.balanced_rom(A, B, C, E, m.ww, m.weights, r=4)
    with pytest.raises(ValueError, match="rank"):
        rom.reduced_from_grams(m.GE, m.GA, m.ZtB, m.CXs, m.ww, m.weights, r=min(m.GE.shape) + 1)
    with pytest.raises(ValueError, match="rank"):
        rom.reduced_from_grams(m.GE[:, :4], m.GA[:, :4], m.ZtB, m.CXs[:, :4], m.ww, m.weights, r=5)
    with pytest.raises(ValueError):
        rom.log_quadrature(1.0, 0.5, 4)
