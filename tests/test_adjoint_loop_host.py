"""The numpy / scipy model of a closed loop's adjoint (tests/support/adjoint_loop_model.py) against central differences of its own
forward run, the mistakes the inputs tell apart, the conditions on the limits of every clamped case (host and GPU), the model's own
accuracy for the inputs and step of the GPU test's central differences, and ``Controller.discrete_gradient``.  No GPU."""
import numpy as np
import pytest

from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import adjoint_step_model as am

#: step of the entry-by-entry central differences and their bound: truncation h^2 |J'''| / |J'| and round-off eps |J| / (h |J'|) are both
#: below 1e-7 for these O(1) .. O(100) quantities at h = 1e-5
H, TOL = 1e-5, 1e-6
#: a mistake must miss the central differences by at least this factor more than the correct form does
APART = 1e4
#: the groups in which each mistake shows
SHOWS = {"xi_after": ("Ad", "C"), "no_mask": ("Ad", "Bd", "C", "D", "G", "g0", "S", "x0", "y0", "w_y", "w_u", "dx0"),
         "G_late": ("G", "g0", "y0", "w_y", "w_u", "dx0")}


@pytest.fixture(scope="module")
def small():
    model, _ = am.random_problem()
    rng = np.random.default_rng(3)
    return model, rng.standard_normal(model.N), rng.standard_normal(model.N)


@pytest.fixture(scope="module")
def plants():
    return {nl: lc.host_plant(nl) for nl in (False, True)}


def _fd_all(loop, g, w, r, z):
    """Central differences of every group: entry by entry, the two state gradients along three random directions."""
    rng = np.random.default_rng(9)
    dirs = rng.standard_normal((3, loop.plant.N))
    out = {}
    for grp in lm.GROUPS:
        if grp in ("dx0", "dxm1"):
            out[grp] = (np.array([loop.fd_directional(grp, d, H, w, r, z) for d in dirs]), dirs)
        else:
            out[grp] = (loop.fd_gradient(grp, g[grp].shape, H, w, r, z), None)
    return out


def _err(g, grp, fd):
    ref, dirs = fd[grp]
    return lm.rel(g[grp] if dirs is None else dirs @ g[grp], ref)


@pytest.mark.parametrize("first_order,n", [(1, 6), (2, 3)])
def test_model_gradient_matches_central_differences(small, first_order, n):
    """n = 6 from a BDF1 first step and n = 3 from BDF2 with a non-zero x_{-1}: every group, with signals and limits that clamp part
    of the controls; and the three mistakes miss by orders of magnitude more than the correct form."""
    model, x0, xm1 = small
    assert np.any(xm1)
    loop, w, r, z = lc.make_case(model, x0, xm1, first_order, n)
    f = loop.forward()
    lm.assert_limits_tell(f["v"], loop.lo, loop.hi)
    assert np.array_equal(f["u"], np.minimum(np.maximum(f["v"], loop.lo), loop.hi))
    g = loop.adjoint(f, w, r, z)
    fd = _fd_all(loop, g, w, r, z)
    good = {}
    for grp in lm.GROUPS:
        if grp == "dxm1" and first_order == 1:  # a BDF1 first step never reads x_{-1}
            assert not np.any(g[grp]) and not np.any(fd[grp][0])
            continue
        good[grp] = _err(g, grp, fd)
        print(f"first order {first_order}, n = {n}, {grp}: {good[grp]:.2e}")
        assert good[grp] <= TOL, (grp, good[grp])
    for wrong, groups in SHOWS.items():
        gw = loop.adjoint(f, w, r, z, wrong=wrong)
        for grp in groups:
            miss = _err(gw, grp, fd)
            print(f"  {wrong} in {grp}: {miss:.2e}")
            assert miss >= APART * good[grp] and miss >= 1e-2, (wrong, grp, miss, good[grp])


def _all_cases():
    for fo, n in lc.MAIN_CASES:
        yield False, dict(first_order=fo, n=n)
    for fo, n in lc.NL_CASES:
        yield True, dict(first_order=fo, n=n)
    for c in lc.SHAPE_CASES + lc.SHORT_CASES:
        yield False, c


def test_limits_of_every_clamped_case_tell(plants):
    """At least two control values clamped, at least two free, no free value closer to a limit than 1e-3 of its magnitude -- for every
    case with limits of this file and of tests/test_adjoint_loop_gpu.py."""
    seen = 0
    for nl, c in _all_cases():
        model, x0, xm1 = plants[nl]
        loop, *_ = lc.make_case(model, x0, xm1, **c)
        if loop.lo is None:
            continue
        v = loop.forward()["v"]
        print(nl, c, lm.limits_report(v, loop.lo, loop.hi))
        lm.assert_limits_tell(v, loop.lo, loop.hi)
        seen += 1
    assert seen >= 4 + len(lc.SHAPE_CASES) // 2 + 2


@pytest.mark.parametrize("nonlinear", [False, True])
def test_model_meets_the_bound_of_the_device_central_differences(plants, nonlinear):
    """The GPU test compares central differences of the DEVICE's closed-loop cost at ``FD_EPS`` with the device's gradient at 1e-6.
    That is a check of the device only if the model's gradient and the model's central differences -- same inputs, same directions,
    same step -- agree to 1e-7."""
    model, x0, xm1 = plants[nonlinear]
    for first_order, n in (lc.NL_CASES if nonlinear else lc.MAIN_CASES):
        loop, w, r, z = lc.make_case(model, x0, xm1, first_order, n)
        f = loop.forward()
        g = loop.adjoint(f, w, r, z)
        for grp in lm.GROUPS:
            if grp == "dxm1" and first_order == 1:
                continue
            d = lc.fd_direction(grp, g[grp].shape, nn2=int(np.count_nonzero(model.M.diagonal())))  # (the velocity block)
            fd = loop.fd_directional(grp, d, lc.FD_EPS, w, r, z)
            err = abs(fd - float(np.sum(g[grp] * d))) / abs(fd)
            print(f"nonlinear {nonlinear}, first order {first_order}, n = {n}, {grp}: {err:.2e}")
            assert err <= lc.FD_MODEL_TOL, (grp, err)


def _discrete_gradient_error(K, dt, seed):
    rng = np.random.default_rng(seed)
    n, m = K.nstates, K.ninputs
    gAd, gBd = rng.standard_normal((n, n)), rng.standard_normal((n, m))
    gA, gB = K.discrete_gradient(dt, gAd, gBd)

    def phi(A, B):
        from flowcontrol_amd.controller import Controller

        Ad, Bd, _, _ = Controller(A, B, K.C, K.D).discrete(dt)
        return float(np.sum(gAd * Ad) + np.sum(gBd * Bd))

    errs = []
    for _ in range(3):
        dA, dB = rng.standard_normal((n, n)), rng.standard_normal((n, m))
        h = 1e-5 * max(1.0, float(np.abs(K.A).max()))
        fd = (phi(K.A + h * dA, K.B + h * dB) - phi(K.A - h * dA, K.B - h * dB)) / (2 * h)
        errs.append(abs(fd - float(np.sum(gA * dA) + np.sum(gB * dB))) / abs(fd))
    return max(errs)


def test_discrete_gradient_random_controller():
    from flowcontrol_amd.controller import Controller

    rng = np.random.default_rng(4)
    A = rng.standard_normal((5, 5))
    A -= (max(np.linalg.eigvals(A).real) + 0.5) * np.eye(5)  # stable
    K = Controller(A, rng.standard_normal((5, 2)), rng.standard_normal((1, 5)), np.zeros((1, 2)))
    err = _discrete_gradient_error(K, 0.05, 1)
    print(f"discrete_gradient, random 5-state controller: {err:.2e}")
    assert err <= 1e-8


def test_discrete_gradient_shipped_controller():
    from pathlib import Path

    import flowcontrol_amd
    from flowcontrol_amd.controller import Controller

    K = Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat")
    assert K.nstates == 13
    err = _discrete_gradient_error(K, 0.005, 2)
    print(f"discrete_gradient, shipped 13-state controller: {err:.2e}")
    assert err <= 1e-8
    gA, gB = K.discrete_gradient(0.005, np.zeros((13, 13)), np.zeros((13, K.ninputs)))
    assert not np.any(gA) and not np.any(gB)
