"""Measurements of the optimal-perturbation driver on the cylinder's O1 mesh, linearised, n = 200 steps, at k = 8, 16 and
32, printed as ONE JSON line.  One process, `--passes` alternating passes of every route; median and spread (min, max) per figure.

  apply:     HIP-event ms and wall ms of one fc_optpert_apply, next to what the same work costs through the entry points that existed
             before it: 200 fc_step_batch calls (wall ms: each synchronises and downloads its records) plus one fc_run_adjoint_batch
             with a terminal block (its HIP-event ms and wall ms)
  iteration: wall ms of one whole subspace iteration (apply, Rayleigh-Ritz, block mass solve, residual block, two M-Cholesky-QR) on the
             device backend, against the host-staged route built only from the earlier entry points: the fc_step_batch loop,
             fc_get_state_batch, a host M x_n, fc_run_adjoint_batch(terminal), a scipy splu of M_ff (factorisation time excluded) and
             numpy for the block algebra
  cg:        block CG on M_ff: iterations, HIP-event us per iteration (three launches), the mass product's algorithmic bytes per pass
             (12 nnz(M_ff) + 4 (N + 1) + 16 N KB) and those bytes over the time of one iteration -- a lower bound of the product's rate

    python scripts/optpert_probe.py [--steps 200] [--passes 3] [--widths 8,16,32]
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import scipy.sparse.linalg as spla

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from flowcontrol_amd import transient as tr  # noqa: E402
from flowcontrol_amd._lib import SLOT_BDF1, SLOT_BDF2, SLOT_MASS  # noqa: E402
from flowcontrol_amd.adjoint import AdjointRun  # noqa: E402
from flowcontrol_amd.batch import BatchedFlowSolver  # noqa: E402
from flowcontrol_amd.fem.spaces import Function  # noqa: E402


def _cylinder():
    from flowcontrol_amd.examples.cylinder.cylinderflowsolver import CylinderFlowSolver

    fs = CylinderFlowSolver.make_default(Re=100, path_out=tempfile.mkdtemp(prefix="fc_optpert_"))
    fs.params_solver.is_eq_nonlinear = False
    U0, P0 = Function(fs.W, np.load(ROOT / "tests" / "golden" / "cylinder_O1.npz")["UP0"]).split()
    fs._assign_steady_state(U0, P0)
    return fs


class HostStaged:
    """The block backend through the entry points that existed before fc_optpert_*: blocks on the host, states through the host."""

    def __init__(self, dev, M, free, lu):
        self.dev, self.k, self.N, self.M, self.free, self.lu = dev, dev.batch_k, dev.N, M, free, lu
        self.fmask = np.zeros(dev.N)
        self.fmask[free] = 1.0
        self.blocks = {}

    def load(self, block, X):
        self.blocks[block] = np.asarray(X, dtype=float) * self.fmask

    def get(self, block):
        return self.blocks[block].copy()

    def forward(self, n, first_order):
        dev, nn2 = self.dev, 2 * self.dev.nn
        U = self.blocks["U"]
        dev.set_state_batch(U[:, :nn2], np.zeros((self.k, nn2)), np.zeros((self.k, self.N - nn2)))
        u0 = np.zeros((self.k, max(dev.n_act, 1)))
        for m in range(n):
            dev.step_batch(SLOT_BDF1 if (m == 0 and first_order == 1) else SLOT_BDF2, u0, compute_energy=False)

    def apply(self, n, first_order):
        dev = self.dev
        self.forward(n, first_order)
        u_n, _, p_n = dev.get_state_batch()
        X = np.c_[u_n, p_n]
        Z = (self.M @ X.T).T
        _, dx0, _ = dev.run_adjoint_batch(SLOT_BDF1 if first_order == 1 else SLOT_BDF2, n, None, Z)
        self.blocks["G"], self.blocks["Y"] = dx0 * self.fmask, X
        return self.blocks["U"] @ self.blocks["G"].T, 0.5 * np.einsum("ij,ij->i", X, Z)

    def mass_solve(self, dst, src, rtol):
        X = np.zeros((self.k, self.N))
        X[:, self.free] = self.lu.solve(self.blocks[src][:, self.free].T).T
        self.blocks[dst] = X

    def gram(self, a, b, weighted=False):
        B = self.blocks[b]
        return self.blocks[a] @ ((self.M @ B.T) if weighted else B.T)

    def combine(self, dst, src, Q, scale=None, accumulate=False):
        new = np.asarray(Q).T @ self.blocks[src]
        if scale is not None:
            new = new * np.asarray(scale)[:, None]
        self.blocks[dst] = self.blocks[dst] + new if accumulate else new


def one_iteration(be, n, first_order=1):
    """One whole iteration of flowcontrol_amd.transient.subspace_iteration, the block update included."""
    H, _ = be.apply(n, first_order)
    theta, S = np.linalg.eigh(0.5 * (H + H.T))
    theta, S = theta[::-1].copy(), np.ascontiguousarray(S[:, ::-1])
    be.mass_solve("V", "G", 1e-12)
    be.combine("R", "V", S)
    be.combine("R", "U", -S * theta[None, :], accumulate=True)
    res = np.sqrt(np.maximum(np.diag(be.gram("R", "R", True)), 0.0)) / theta[0]
    be.combine("S", "V", S, scale=1.0 / theta)
    tr._cholqr(be, "R", "S", "probe")
    tr._cholqr(be, "U", "R", "probe")
    return theta, res


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def probe_width(fs, k, n, passes):
    bfs = BatchedFlowSolver(fs, k)
    out = {}
    with AdjointRun(bfs) as run:
        dev = run.dev
        dev.assemble_matrix(SLOT_MASS, mass=1.0, nu=0.0, pressure=0.0, divergence=0.0)
        M = dev.matrix(SLOT_MASS)
        dev.optpert_reserve(True)
        be = tr.DeviceBlocks(dev)
        Mff = M[be.free][:, be.free].tocsc()
        t_lu, lu = wall_ms(lambda: spla.splu(Mff))
        hs = HostStaged(dev, M, be.free, lu)
        X0 = tr.start_block(k, dev.N, None, 0, be.free)
        tr.orthonormalise_start(be, X0)
        U = be.get("U")
        hs.load("U", U)
        slot = SLOT_BDF1
        fig = {q: [] for q in ("apply_event_ms", "apply_wall_ms", "steps_wall_ms", "march_event_ms", "march_wall_ms", "iter_device_ms", "iter_host_ms",
                               "cg_iterations", "cg_event_us_per_iteration")}
        Z = np.zeros((k, dev.N))
        for p in range(passes + 1):  # (pass 0 warms every route up and is dropped)
            be.load("U", U)
            w, _ = wall_ms(lambda: dev.optpert_apply(slot, n))
            a_ev = dev.optpert_info()["apply_ms"]
            hs.load("U", U)
            sw, _ = wall_ms(lambda: hs.forward(n, 1))
            mw, _ = wall_ms(lambda: dev.run_adjoint_batch(slot, n, None, Z + 1.0))
            m_ev = dev.adjoint_batch_info(slot)["run_ms"]
            be.load("U", U)
            di, (theta_d, _) = wall_ms(lambda: one_iteration(be, n))
            info = dev.optpert_info()
            hs.load("U", U)
            hi, (theta_h, _) = wall_ms(lambda: one_iteration(hs, n))
            assert np.allclose(theta_d, theta_h, rtol=1e-8), (theta_d, theta_h)
            if p == 0:
                continue
            for q, v in (("apply_event_ms", a_ev), ("apply_wall_ms", w), ("steps_wall_ms", sw), ("march_event_ms", m_ev), ("march_wall_ms", mw),
                         ("iter_device_ms", di), ("iter_host_ms", hi), ("cg_iterations", info["cg_iterations"]),
                         ("cg_event_us_per_iteration", 1e3 * info["mass_solve_ms"] / max(1, info["cg_iterations"]))):
                fig[q].append(v)
        KB = dev.optpert_info()["KB"]
        mass_bytes = 12 * Mff.nnz + 4 * (dev.N + 1) + 16 * dev.N * KB
        out = {q: stats(v) for q, v in fig.items()}
        out.update(k=k, KB=KB, N=int(dev.N), n_free=int(be.free.size), nnz_ff=int(Mff.nnz), splu_factor_ms=t_lu, mass_product_bytes=mass_bytes,
                   mass_product_GBps_lower_bound=mass_bytes / (1e3 * out["cg_event_us_per_iteration"]["median"]), device_bytes=dev.optpert_info()["bytes"],
                   leading_gains=[float(t) for t in theta_d[:3]])
        dev.optpert_reserve(False)
    bfs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--widths", default="8,16,32")
    a = ap.parse_args()
    fs = _cylinder()
    try:
        res = {"mesh": "cylinder O1", "n_steps": a.steps, "passes": a.passes, "widths": [probe_width(fs, int(k), a.steps, a.passes) for k in a.widths.split(",")]}
    finally:
        fs.th.release_device()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
