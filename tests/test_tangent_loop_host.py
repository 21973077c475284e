"""The numpy model of a closed loop's tangent (tests/support/tangent_loop_model.py) -- what tests/test_tangent_loop_gpu.py compares
``fc_run_tangent_closed_loop`` with -- pinned three ways without a GPU: against the model ADJOINT of the same loop through the
dot-product identity, against central differences of the model's own forward run, and against the mistakes the inputs must tell apart.
Then ``Controller.discrete_tangent`` against ``discrete_gradient`` and central differences, and the new names of the C ABI and of
``flu``."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests.support import adjoint_loop_cases as lc
from tests.support import adjoint_loop_model as lm
from tests.support import tangent_loop_model as tm

ROOT = Path(__file__).resolve().parents[1]
#: the identity holds to round-off: a defect of at most this share of the summed absolute terms
IDENTITY = 1e-12
#: a mistake must move dy or du by more than this, relative
APART = 1e-2


@pytest.fixture(scope="module")
def plants():
    return {nl: lc.host_plant(nl) for nl in (False, True)}


def _main_cases():
    for fo, n in lc.MAIN_CASES:
        yield False, dict(first_order=fo, n=n)
    for fo, n in lc.NL_CASES:
        yield True, dict(first_order=fo, n=n)


def _all_cases():
    yield from _main_cases()
    for c in lc.SHAPE_CASES + lc.SHORT_CASES:
        yield False, c


def _case(plants, nl, c):
    model, x0, xm1 = plants[nl]
    loop, w, r, z = lc.make_case(model, x0, xm1, **c)
    f = loop.forward()
    g = loop.adjoint(f, w, r, z)
    return loop, f, g, tm.directions(g), w, r, z


def test_identity_with_the_model_adjoint(plants):
    """sum w . dy + sum r . du + z . dx_n = sum_groups <g, d> for every main, nonlinear, shape and short case, all groups moved at once
    (directions ``fd_direction(grp, shape, seed=5)``): a defect of at most 1e-12 of the summed absolute terms."""
    worst = 0.0
    for nl, c in _all_cases():
        loop, f, g, d, w, r, z = _case(plants, nl, c)
        lhs, rhs, scale = tm.identity_terms(tm.tangent(loop, f, d), g, d, w, r, z)
        defect = abs(lhs - rhs) / scale
        worst = max(worst, defect)
        assert defect <= IDENTITY, (nl, c, lhs, rhs, defect)
    print(f"worst identity defect: {worst:.2e}")


def test_model_tangent_matches_central_differences(plants):
    """dy, du, xi_n, dx_n, dx_{n-1} against central differences of the model's own forward run at ``FD_EPS``, within ``FD_MODEL_TOL``,
    on the main and the nonlinear cases."""
    for nl, c in _main_cases():
        loop, f, g, d, *_ = _case(plants, nl, c)
        t = tm.tangent(loop, f, d)
        fp, fm = tm.perturbed(loop, d, lc.FD_EPS).forward(), tm.perturbed(loop, d, -lc.FD_EPS).forward()
        fd = lambda pick: (pick(fp) - pick(fm)) / (2 * lc.FD_EPS)  # noqa: E731
        errs = {"dy": lm.rel(t["dy"], fd(lambda q: q["y"][1:])), "du": lm.rel(t["du"], fd(lambda q: q["u"])),
                "xi": lm.rel(t["xi"], fd(lambda q: q["xi"][-1])), "dxn": lm.rel(t["dxn"], fd(lambda q: q["X"][-1])),
                "dxnm1": lm.rel(t["dxnm1"], fd(lambda q: q["X"][-2]))}
        print(nl, c, ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= lc.FD_MODEL_TOL, (nl, c, k, v)


@pytest.mark.parametrize("wrong", ["no_mask", "xi_after", "dy_late"])
def test_the_inputs_tell_the_mistakes_apart(plants, wrong):
    """Each mistake moves dy or du by more than 1e-2 relative on every main and nonlinear case."""
    for nl, c in _main_cases():
        loop, f, g, d, *_ = _case(plants, nl, c)
        t, tw = tm.tangent(loop, f, d), tm.tangent(loop, f, d, wrong=wrong)
        moved = max(lm.rel(tw["dy"], t["dy"]), lm.rel(tw["du"], t["du"]))
        print(f"{wrong}, nonlinear {nl}, {c}: {moved:.2e}")
        assert moved > APART, (wrong, nl, c, moved)


def _controllers():
    import flowcontrol_amd
    from flowcontrol_amd.controller import Controller

    rng = np.random.default_rng(4)
    A = rng.standard_normal((5, 5))
    A -= (max(np.linalg.eigvals(A).real) + 0.5) * np.eye(5)  # stable
    yield "random 5-state", Controller(A, rng.standard_normal((5, 2)), rng.standard_normal((1, 5)), np.zeros((1, 2))), 0.05
    yield "shipped 13-state", Controller.from_file(Path(flowcontrol_amd.__file__).parent / "examples" / "cylinder" / "data_input" / "Kopt_reduced13.mat"), 0.005


def test_discrete_tangent_is_the_transpose_of_discrete_gradient():
    """<(gAd, gBd), discrete_tangent(dA, dB)> = <discrete_gradient(gAd, gBd), (dA, dB)> to 1e-12 of the summed absolute terms."""
    for name, K, dt in _controllers():
        rng = np.random.default_rng(7)
        n, m = K.nstates, K.ninputs
        gAd, gBd, dA, dB = rng.standard_normal((n, n)), rng.standard_normal((n, m)), rng.standard_normal((n, n)), rng.standard_normal((n, m))
        tA, tB = K.discrete_tangent(dt, dA, dB)
        gA, gB = K.discrete_gradient(dt, gAd, gBd)
        terms = [np.sum(gAd * tA), np.sum(gBd * tB), np.sum(gA * dA), np.sum(gB * dB)]
        defect = abs(terms[0] + terms[1] - terms[2] - terms[3]) / sum(abs(x) for x in terms)
        print(f"discrete_tangent against discrete_gradient, {name}: {defect:.2e}")
        assert defect <= 1e-12
        zA, zB = K.discrete_tangent(dt, np.zeros((n, n)), np.zeros((n, m)))
        assert not np.any(zA) and not np.any(zB)


def test_discrete_tangent_matches_central_differences():
    """... and against central differences of ``discrete()`` (the step and the 1e-8 of the discrete_gradient tests)."""
    from flowcontrol_amd.controller import Controller

    for name, K, dt in _controllers():
        rng = np.random.default_rng(8)
        n, m = K.nstates, K.ninputs
        dA, dB = rng.standard_normal((n, n)), rng.standard_normal((n, m))
        tA, tB = K.discrete_tangent(dt, dA, dB)
        h = 1e-5 * max(1.0, float(np.abs(K.A).max()))
        plus, minus = (Controller(K.A + s * h * dA, K.B + s * h * dB, K.C, K.D).discrete(dt) for s in (1.0, -1.0))
        err = max(lm.rel(tA, (plus[0] - minus[0]) / (2 * h)), lm.rel(tB, (plus[1] - minus[1]) / (2 * h)))
        print(f"discrete_tangent against central differences, {name}: {err:.2e}")
        assert err <= 1e-8


def test_the_new_names_exist():
    """Both entry points are declared in include/fc_hip.h and bound in _lib.SIGNATURES; the drivers are reachable through ``flu``."""
    import flowcontrol_amd.utils as flu
    from flowcontrol_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "fc_hip.h").read_text(), flags=re.S)
    for name in ("fc_run_tangent_closed_loop", "fc_run_tangent_closed_loop_batch"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["fc_run_tangent_closed_loop"]) == 21 and len(_lib.SIGNATURES["fc_run_tangent_closed_loop_batch"]) == 24
    for name in ("closed_loop_tangent", "closed_loop_gauss_newton_product", "batched_closed_loop_tangent"):
        assert callable(getattr(flu, name)), name
