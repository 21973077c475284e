"""Closed loop on the device, the host side: the public ZOH discretisation, the packing of a controller bank and its numpy model,
and the declaration / binding of the new C entry points.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest
from scipy.signal import cont2discrete

from flowcontrol_amd import _lib
from flowcontrol_amd.controller import Controller, bank_step, bank_transposed, pack_controllers, unpack_controllers
from flowcontrol_amd.examples.data import controller_file

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["fc_set_controllers", "fc_get_controller_state", "fc_set_controller_state", "fc_ctrl_apply", "fc_run_closed_loop",
               "fc_run_closed_loop_batch", "fc_get_run_monitor"]


def _random_stable(rng, n, m, p):
    A = rng.standard_normal((n, n))
    A -= (np.max(np.linalg.eigvals(A).real) + 1.0) * np.eye(n)
    return Controller(A, rng.standard_normal((n, m)), rng.standard_normal((p, n)), rng.standard_normal((p, m)))


@pytest.mark.parametrize("case", ["kopt", "random"])
def test_discrete_is_the_zoh_discretisation(case):
    """``Controller.discrete(dt)`` against scipy's ZOH: two evaluations of the same matrix exponential, 1e-12 relative."""
    K = Controller.from_file(controller_file()) if case == "kopt" else _random_stable(np.random.default_rng(0), 6, 3, 2)
    dt = 0.005
    Ad, Bd, Cd, Dd = K.discrete(dt)
    rAd, rBd, rCd, rDd, _ = cont2discrete((K.A, K.B, K.C, K.D), dt, method="zoh")
    for mine, ref in ((Ad, rAd), (Bd, rBd), (Cd, rCd), (Dd, rDd)):
        assert mine.shape == ref.shape
        assert np.linalg.norm(mine - ref) <= 1e-12 * max(np.linalg.norm(ref), 1e-300)
    # the matrices `step` advances with
    x = np.random.default_rng(1).standard_normal(K.nstates)
    y = np.random.default_rng(2).standard_normal(K.ninputs)
    K.x = x.copy()
    u = K.step(y, dt)
    assert np.array_equal(u, Cd @ x + Dd @ y) and np.array_equal(K.x, Ad @ x + Bd @ y)


def test_bank_packing_round_trips_and_its_recursion_is_k_controller_loops():
    rng = np.random.default_rng(3)
    dt, n_sens, n_act = 0.005, 3, 2
    Ks = [Controller.from_file(controller_file()), _random_stable(rng, 4, 1, 1), _random_stable(rng, 7, 1, 2),
          Controller(np.zeros((0, 0)), np.zeros((0, 1)), np.zeros((1, 0)), [[0.7]])]  # a static gain: nx = 0
    for K in Ks:
        K.x = rng.standard_normal(K.nstates)
    G = rng.standard_normal((1, n_sens))
    g0 = rng.standard_normal(1)
    bank = pack_controllers(Ks, dt, n_sens, n_act, feedback=(G, g0))
    assert (bank["k"], bank["nx"], bank["nyc"], bank["nuc"]) == (4, 13, 1, 2)
    for K, (Ad, Bd, Cd, Dd, x) in zip(Ks, unpack_controllers(bank)):
        for mine, ref in zip((Ad, Bd, Cd, Dd), K.discrete(dt)):
            assert np.array_equal(mine, ref)
        assert np.array_equal(x, K.x)
    blocks = bank_transposed(bank)
    assert blocks.shape == (4, 13 * 13 + 13 * 1 + 2 * 13 + 2 * 1 + 1 * n_sens + 1 + n_act * 2)
    # the recursion on the packed (and on the transposed, device-layout) arrays against k independent Controller.step sequences
    x = bank["x0"].copy()
    xt = x.copy()
    for _ in range(40):
        y = rng.standard_normal((4, n_sens))
        u, x = bank_step(bank, x, y)
        ut, xt = bank_step(bank, xt, y, blocks=blocks)
        assert np.array_equal(u, ut) and np.array_equal(x, xt)
        for i, K in enumerate(Ks):
            cmd = np.atleast_1d(K.step(y=G @ y[i] + g0, dt=dt)).ravel()
            ref = cmd if cmd.size == n_act else np.full(n_act, cmd[0])
            scale = max(np.abs(ref).max(), 1e-300)
            assert np.abs(u[i] - ref).max() <= 1e-13 * scale + 1e-300
            assert np.abs(x[i, : K.nstates] - K.x).max() <= 1e-13 * max(np.abs(K.x).max(), 1.0) if K.nstates else True
            assert not np.any(x[i, K.nstates:])  # padded states stay zero
    # the reference loop
    ref_bank = pack_controllers(Ks[:1], dt, n_sens, n_act)
    assert np.array_equal(ref_bank["G"][0], [[-1.0, 0.0, 0.0]]) and np.array_equal(ref_bank["S"][0], [[1.0], [1.0]])
    with pytest.raises(TypeError):
        pack_controllers(Ks[:1], dt, n_sens, n_act, feedback=lambda y: -y[0])
    with pytest.raises(TypeError):
        pack_controllers([lambda y: y], dt, n_sens, n_act)
    with pytest.raises(ValueError):
        pack_controllers(Ks[:1], dt, n_sens, n_act, feedback=(np.zeros((2, n_sens)), np.zeros(2)))


def test_new_entry_points_are_declared_and_bound_with_matching_arity():
    header = (ROOT / "include" / "fc_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/fc_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert len(_lib.SIGNATURES[name]) == n_args, f"{name}: {n_args} parameters declared, {len(_lib.SIGNATURES[name])} bound"
    src = (ROOT / "flowcontrol_amd" / "csrc" / "fc_hip.hip").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not defined in fc_hip.hip"
    assert (ROOT / "flowcontrol_amd" / "csrc" / "fc_ctrl.hip.h").exists()
