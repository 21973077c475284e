"""Loop signals and actuator limits, the host side: ``bank_step``'s keywords against a loop written out product by product, and the
estimator core of ``flowcontrol_amd.sysid`` on a synthetic closed loop with a known transfer function.  No GPU needed."""
import numpy as np
import pytest

from flowcontrol_amd import signal as fsignal
from flowcontrol_amd.controller import Controller, bank_step, pack_controllers
from flowcontrol_amd.sysid import frf_from_series

EPS = 2.0**-53
DT = 0.005


def _random_controller(rng, nx, nyc, nuc):
    if nx == 0:
        K = Controller(np.zeros((0, 0)), np.zeros((0, 1)), np.zeros((1, 0)), [[0.0]])  # (the constructor shapes static gains 1 x 1)
        K.B, K.C, K.D = np.zeros((0, nyc)), np.zeros((nuc, 0)), rng.standard_normal((nuc, nyc))
        K.ninputs, K.noutputs = nyc, nuc
        return K
    A = rng.standard_normal((nx, nx)) / np.sqrt(nx)
    A -= (np.max(np.linalg.eigvals(A).real) + 5.0) * np.eye(nx)
    return Controller(A, rng.standard_normal((nx, nyc)), rng.standard_normal((nuc, nx)), rng.standard_normal((nuc, nyc)))


def _dot(a, v):
    """sum_j a[j] v[j] in index order, one product and one addition at a time."""
    acc = 0.0
    for aj, vj in zip(a, v):
        acc += aj * vj
    return acc


def _plain_loop(bank, i, x, y, w_y, w_u, lo, hi):
    """One controller of the bank, every sum written out: (v before the clamp, u, x_new)."""
    Ad, Bd, C, D, G, g0, S = (bank[m][i] for m in ("Ad", "Bd", "C", "D", "G", "g0", "S"))
    nx, nyc, nuc, n_act = bank["nx"], bank["nyc"], bank["nuc"], S.shape[0]
    yc = [_dot(G[j], y) + g0[j] + w_y[j] for j in range(nyc)]
    uc = [_dot(C[r], x) + _dot(D[r], yc) for r in range(nuc)]
    xn = [_dot(Ad[r], x) + _dot(Bd[r], yc) for r in range(nx)]
    v = [_dot(S[a], uc) + w_u[a] for a in range(n_act)]
    u = [min(max(v[a], lo[a]), hi[a]) for a in range(n_act)]
    return np.array(v), np.array(u), np.array(xn)


@pytest.mark.parametrize("nx", [0, 13])
def test_bank_step_with_signals_and_limits_is_the_plain_loop(nx):
    """``bank_step(..., w_y, w_u, u_lo, u_hi)`` against the recursion written out sum by sum.  numpy's products and the written-out sums
    add the same terms in different orders: a sum of n products errs by at most n eps sum |a_j| |v_j| in any order (eps = 2^-53), so
    each stage is within (nx + nyc + 3) eps times its sum of absolute terms (the products, the constant and the signal), carried
    through the absolute values of the later stages -- the bound of the kernel test with one more addition in the yc and u stages.  The
    clamp is 1-Lipschitz, so it keeps the bound, and an entry beyond its limit by more than the bound equals the limit exactly."""
    rng = np.random.default_rng(7 + nx)
    k, nyc, nuc, n_sens, n_act = 3, 2, 2, 3, 2
    Ks = [_random_controller(rng, nx, nyc, nuc) for _ in range(k)]
    for K in Ks:
        K.x = rng.standard_normal(nx)
    bank = pack_controllers(Ks, DT, n_sens, n_act, feedback=(rng.standard_normal((k, nyc, n_sens)), rng.standard_normal((k, nyc))))
    x = bank["x0"].copy()
    c = (nx + nyc + 3) * EPS
    lo, hi = np.array([[-0.5, -np.inf]] * k), np.array([[0.7, 0.4]] * k)
    clamped = free = 0
    for step in range(30):
        y = rng.standard_normal((k, n_sens))
        w_y, w_u = rng.standard_normal((k, nyc)), rng.standard_normal((k, n_act))
        u, xn = bank_step(bank, x, y, w_y=w_y, w_u=w_u, u_lo=lo, u_hi=hi)
        # no signal, no limit: the bits of the call without keywords
        u0, x0 = bank_step(bank, x, y)
        uz, xz = bank_step(bank, x, y, w_y=np.zeros((k, nyc)), w_u=np.zeros((k, n_act)), u_lo=-np.inf, u_hi=np.inf)
        assert np.array_equal(u0, uz) and np.array_equal(x0, xz)
        for i in range(k):
            v_ref, u_ref, x_ref = _plain_loop(bank, i, x[i], y[i], w_y[i], w_u[i], lo[i], hi[i])
            aG, aC, aD, aAd, aBd, aS = (np.abs(bank[m][i]) for m in ("G", "C", "D", "Ad", "Bd", "S"))
            yc_abs = aG @ np.abs(y[i]) + np.abs(bank["g0"][i]) + np.abs(w_y[i])
            e_yc = c * yc_abs
            uc_abs = aC @ np.abs(x[i]) + aD @ yc_abs
            e_uc = c * uc_abs + aD @ e_yc
            e_u = c * (aS @ uc_abs + np.abs(w_u[i])) + aS @ e_uc
            e_x = c * (aAd @ np.abs(x[i]) + aBd @ yc_abs) + aBd @ e_yc
            assert np.all(np.abs(u[i] - u_ref) <= e_u), (step, i, np.abs(u[i] - u_ref).max(), e_u.max())
            assert np.all(np.abs(xn[i] - x_ref) <= e_x), (step, i)
            below, above = v_ref < lo[i] - e_u, v_ref > hi[i] + e_u
            assert np.array_equal(u[i][below], lo[i][below]) and np.array_equal(u[i][above], hi[i][above])
            clamped += int(below.sum() + above.sum())
            free += int(((v_ref > lo[i] + e_u) & (v_ref < hi[i] - e_u)).sum())
        x = xn
    assert clamped >= 20 and free >= 20, (clamped, free)  # (the limits bind for some entries and leave others alone)
    with pytest.raises(ValueError):
        bank_step(bank, x, y, u_lo=-1.0)


def _synthetic_loop(rng, A, B, C, gain, w):
    """The device loop's timing on a discrete plant: the controller at step s sees y of step s - 1, and y of step s includes u of
    step s.  x_s = A x_{s-1} + B u_s, y_s = C x_s, u_s = -gain y_{s-1}[0] + w_s.  Returns (y [n, 2], u [n])."""
    x = rng.standard_normal(A.shape[0])  # a transient to forget
    y_prev = C @ x
    ys, us = [], []
    for ws in w:
        u = -gain * y_prev[0] + ws
        x = A @ x + B[:, 0] * u
        y_prev = C @ x
        ys.append(y_prev), us.append(u)
    return np.array(ys), np.array(us)


def test_frf_from_series_recovers_the_plant_inside_a_closed_loop():
    """A stable discrete plant (4 states, spectral radius 0.9, 1 input, 2 outputs) under a static gain, excited by multisines of
    period N = 256 over P = 4 periods, the first two dropped.  Under the loop's timing the plant's transfer function from the applied
    u to y is G(z) = C (I - A / z)^-1 B.  The closed loop's spectral radius is at most 0.9 as well (asserted), so the transient left
    after two periods is below 0.9^512 = 4e-24 of its start and what remains is the rounding of the recursion and of a 512-term
    DFT: 1e-10 relative holds with room."""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((4, 4))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))
    B, C = rng.standard_normal((4, 1)), rng.standard_normal((2, 4))
    # the closed loop in this timing: x_s = (A - gain B C[0]) x_{s-1} + B w_s
    radius = lambda g: np.max(np.abs(np.linalg.eigvals(A - g * B @ C[:1])))  # noqa: E731
    gain = min((g for g in np.linspace(-0.5, 0.5, 41) if g != 0.0), key=radius)
    assert radius(gain) <= 0.9, radius(gain)
    N, P, P_skip, M = 256, 4, 2, 3
    np.random.seed(5)
    w = 0.1 * fsignal.multisine_MP(M, P, unwrap=False, N=N, Fs=1.0, fmin=0.05, fmax=0.5)  # harmonics in [0.025, 0.25] cycles per step
    ys, us = zip(*(_synthetic_loop(rng, A, B, C, gain, w[m]) for m in range(M)))
    res = frf_from_series(np.stack(ys), np.stack(us), w, N, P_skip)
    # only the excited harmonics are reported
    assert np.array_equal(res["bins"], np.arange(7, 65))
    assert res["G"].shape == (58, 2) and res["Y"].shape == (M, 58, 2) and res["U"].shape == (M, 58)
    z = np.exp(2j * np.pi * res["bins"] / N)
    G_ref = np.stack([C @ np.linalg.solve(np.eye(4) - A / zk, B[:, 0]) for zk in z])
    err = np.abs(res["G"] - G_ref) / np.abs(G_ref)
    print(f"largest relative error of G: {err.max():.3e}; largest G_std / |G|: {(res['G_std'] / np.abs(G_ref)).max():.3e}")
    assert err.max() <= 1e-10
    # the realisations differ in their phases only: their spread is rounding, at the same level
    assert np.all(res["G_std"] <= 1e-10 * np.abs(G_ref))
    # one realisation, without the leading axis; bins given: the same numbers, and no spread to report
    one = frf_from_series(ys[0], us[0], w[0], N, P_skip, bins=res["bins"][:5])
    assert np.array_equal(one["bins"], res["bins"][:5]) and not np.any(one["G_std"])
    assert np.abs(one["G"] - G_ref[:5]).max() <= 1e-10 * np.abs(G_ref[:5]).min()
    # an unexcited bin holds no information and is refused implicitly: asking for DC or the Nyquist bin is an error
    with pytest.raises(ValueError):
        frf_from_series(ys[0], us[0], w[0], N, P_skip, bins=[0])
    with pytest.raises(ValueError):
        frf_from_series(ys[0], us[0], w[0], N, P_skip, bins=[N // 2])
    with pytest.raises(ValueError):
        frf_from_series(ys[0][:-1], us[0][:-1], w[0][:-1], N, P_skip)
