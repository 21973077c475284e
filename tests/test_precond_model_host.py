"""Host side of the factorisation-free preconditioner (``csrc/fc_precond.hpp``) against its numpy specification
(``tests/support/precond_model.py``) without a GPU: a C++ driver over the header (``tests/support/precond_model_dump.cpp``, compiled with
g++) dumps everything ``fc_setup_krylov`` builds for the oracle's operators on the meshes of ``precond_model.CASES`` -- once with the
identity permutation, once with the reversed one -- and every piece is compared: aggregate ids exactly, matrices to rounding.

Bounds.  A matrix of the driver may differ from the specification's by 16 x the spread between the specification's two variants (sums of
the power iteration and accumulation order of every product reversed), and never by less than 16 eps, both relative to the matrix's
largest entry.  Galerkin products, the dense inverse and K_F carry bounds derived where they are asserted.  The aggregation is exact only
because no strength ratio comes near 1 (the gap condition, asserted).  The errors of the float64 folded apply against the longdouble
unfolded one are the constants ``HOST_ERROR_*`` the GPU tests take their tolerances from; they are re-measured here."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from flowcontrol_amd.fem.mesh import Mesh
from flowcontrol_amd.fem.spaces import TaylorHood
from tests.support import krylov_model as km
from tests.support import precond_model as pm

ROOT = Path(__file__).resolve().parents[1]
EPS = np.finfo(float).eps
GAP = 1e-6
PERMS = ("identity", "reversed")


def _read(path):
    rec, buf, at = {}, Path(path).read_bytes(), 0
    while at < len(buf):
        (n,) = struct.unpack_from("<i", buf, at)
        name = buf[at + 4 : at + 4 + n].decode()
        kind, count = struct.unpack_from("<iq", buf, at + 4 + n)
        at += 16 + n
        dt = np.dtype("<f8") if kind else np.dtype("<i4")
        rec[name] = np.frombuffer(buf, dtype=dt, count=count, offset=at).copy()
        at += count * dt.itemsize
    return rec


def _mat(rec, name):
    return sp.csr_matrix((rec[name + ".v"], rec[name + ".ci"], rec[name + ".rp"]), shape=tuple(rec[name + ".shape"]))


def _operator(n, enclosed):
    from oracle import ns_oracle as O

    th = TaylorHood(Mesh.unit_square(n, n))
    dofs = pm.all_wall_dofs(th) if enclosed else km.wall_dofs(th)
    A, _ = O.apply_bc_symmetric(O.assemble_matrix(O.Disc.from_taylor_hood(th), **pm.operator_args(th.node_coords)), None, dofs, None)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return th, A


class Case:
    def __init__(self, exe, tmp, n, enclosed, perm_kind):
        th, A = _operator(n, enclosed)
        self.n, self.enclosed, self.perm_kind, self.th, self.A = n, enclosed, perm_kind, th, A
        N, self.n_vel = th.N, 2 * th.nn
        self.perm = np.arange(N) if perm_kind == "identity" else np.arange(N)[::-1].copy()
        self.pin = (pm.pin_dof(th), pm.PIN_SHIFT) if enclosed else None
        f_in, f_out = tmp / f"in_{n}_{enclosed}_{perm_kind}.bin", tmp / f"out_{n}_{enclosed}_{perm_kind}.bin"
        with open(f_in, "wb") as f:
            f.write(np.array([N, self.n_vel, A.nnz, self.pin[0] if enclosed else -1], dtype="<i4").tobytes())
            f.write(np.array([pm.PIN_SHIFT], dtype="<f8").tobytes())
            f.write(A.indptr.astype("<i4").tobytes() + A.indices.astype("<i4").tobytes() + A.data.astype("<f8").tobytes())
            f.write(self.perm.astype("<i4").tobytes())
        subprocess.run([str(exe), str(f_in), str(f_out)], check=True)
        self.rec = _read(f_out)
        self.spec = pm.Spec(A, self.perm, self.n_vel, pin=self.pin)
        self.other = pm.Spec(A, self.perm, self.n_vel, pin=self.pin, reverse=True)
        self.nl = int(self.rec["levels"][0])

    @property
    def tag(self):
        return f"unit_square({self.n}){' enclosed' if self.enclosed else ''} {self.perm_kind}"

    def driver_folded(self, sweeps, amg):
        """the driver's matrices in the form of Spec.folded"""
        r = self.rec
        omega = float(r["omega"][0]) if sweeps > 1 else 1.0
        dinv = 1.0 / r["dF"]
        return dict(vpos=r["vpos"], ppos=r["ppos"], perm=self.perm, dinv=dinv, wdinv=omega * dinv, KF=_mat(r, "KF") if sweeps > 1 else None,
                    F=_mat(r, "F"), B=_mat(r, "B"), Bt=_mat(r, "Bt"), G=[_mat(r, f"L{l}.G{amg}") for l in range(self.nl)],
                    U=[_mat(r, f"L{l}.U{amg}") for l in range(self.nl)], cinv=r["cinv"].reshape(int(r["levels"][1]), -1))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("precond_model")
    exe = tmp / "precond_model_dump"
    subprocess.run(["g++", "-O2", "-std=c++17", str(ROOT / "tests" / "support" / "precond_model_dump.cpp"), "-o", str(exe)], check=True)
    return [Case(exe, tmp, n, enc, pk) for n, enc in [(n, False) for n in pm.CASES] + [(pm.ENCLOSED, True)] for pk in PERMS]


def _close(got, a, b, what):
    """``got`` (the driver's) equals the specification's ``a`` on the same pattern, within 16 x the spread between a and its variant b"""
    got, a, b = (sp.csr_matrix(m) for m in (got, a, b))
    for m in (got, a, b):
        m.sort_indices()
    assert got.shape == a.shape and np.array_equal(got.indptr, a.indptr) and np.array_equal(got.indices, a.indices), f"{what}: another pattern"
    scale = np.abs(a.data).max()
    spread = np.abs(a.data - b.data).max() / scale
    err = np.abs(got.data - a.data).max() / scale
    assert err <= 16 * max(spread, EPS), f"{what}: {err:.2e} against a spread of {spread:.2e}"
    return err


def test_case_table_and_sizes(cases):
    for c in cases:
        if not c.enclosed and c.perm_kind == "identity":  # (the greedy aggregation follows the row order: another permutation, other counts)
            assert (c.th.N, c.spec.np, len(c.spec.levels), c.spec.Ac.shape[0]) == pm.CASES[c.n], c.tag
        assert [int(v) for v in c.rec["levels"]] == [len(c.spec.levels), c.spec.Ac.shape[0]], c.tag
        for l, V in enumerate(c.spec.levels):
            assert c.rec[f"L{l}.A.shape"][0] == V["A"].shape[0] and c.rec[f"L{l}.P.shape"][1] == V["na"]


def test_aggregates_are_the_specifications_and_no_strength_ratio_is_near_one(cases):
    worst = {}
    for c in cases:
        assert c.nl == len(c.spec.levels)
        for l, V in enumerate(c.spec.levels):
            gap = float(np.abs(pm.strength_ratios(V["A"]) - 1.0).min())
            worst[(c.tag, l)] = gap
            assert gap >= GAP, f"{c.tag} level {l}: a strength ratio {gap:.1e} from 1: rounding could move an aggregate -- take another mesh"
            assert np.array_equal(c.rec[f"L{l}.agg"], V["agg"]), f"{c.tag} level {l}: aggregates differ"
            assert np.array_equal(c.other.levels[l]["agg"], V["agg"])
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert any(c.nl == 2 for c in cases) and any(c.nl == 1 for c in cases)


def test_blocks_schur_and_hierarchy_agree_to_rounding(cases):
    for c in cases:
        r, s, o = c.rec, c.spec, c.other
        # split_blocks against scipy slicing: no arithmetic, bit for bit
        assert np.array_equal(r["vpos"], s.vpos) and np.array_equal(r["ppos"], s.ppos) and np.array_equal(r["dF"], s.dF)
        for name, M in (("F", s.F), ("B", s.B), ("Bt", s.Bt)):
            D = _mat(r, name)
            assert np.array_equal(D.indptr, M.indptr) and np.array_equal(D.indices, M.indices) and np.array_equal(D.data, M.data), f"{c.tag} {name}"
        assert abs(r["rhoF"][0] - s.rhoF) <= 16 * max(abs(s.rhoF - o.rhoF), EPS * s.rhoF), c.tag
        assert abs(r["omega"][0] - s.omega(2)) <= 1e-14 * s.omega(2) and s.omega(1) == 1.0
        _close(_mat(r, "S"), s.S, o.S, f"{c.tag} S")
        if c.enclosed:  # the pin: the shift on the diagonal of the pinned dof's compact row, nowhere else
            k = int(np.flatnonzero(c.perm[s.ppos] == c.pin[0])[0])
            free = pm.Spec(c.A, c.perm, c.n_vel).S
            d = (_mat(r, "S") - free).tocoo()
            assert np.array_equal(d.row[d.data != 0], [k]) and np.array_equal(d.col[d.data != 0], [k]) and abs(d.data[d.data != 0][0] - pm.PIN_SHIFT) < 1e-12
        for l, (V, W) in enumerate(zip(s.levels, o.levels)):
            p = f"L{l}."
            _close(_mat(r, p + "A"), V["A"], W["A"], f"{c.tag} A_{l}")
            _close(_mat(r, p + "P"), V["P"], W["P"], f"{c.tag} P_{l}")
            assert (_mat(r, p + "R") != _mat(r, p + "P").T).nnz == 0
            assert abs(r[p + "rho"][0] - V["rho"]) <= 16 * max(abs(V["rho"] - W["rho"]), EPS * V["rho"]), (c.tag, l)
            assert np.abs(r[p + "wdinv"] - V["wdinv"]).max() <= 16 * max(np.abs(V["wdinv"] - W["wdinv"]).max(), EPS * np.abs(V["wdinv"]).max())
        # the folded operators: the same patterns (the lanes of a launch follow from them), values to rounding
        for amg in pm.AMG_SWEEPS:
            fa, fb = s.folded(2, amg), o.folded(2, amg)
            for l in range(c.nl):
                _close(_mat(r, f"L{l}.G{amg}"), fa["G"][l], fb["G"][l], f"{c.tag} G_{l} V({amg},{amg})")
                _close(_mat(r, f"L{l}.U{amg}"), fa["U"][l], fb["U"][l], f"{c.tag} U_{l} V({amg},{amg})")


def test_galerkin_identity_and_coarse_inverse(cases):
    for c in cases:
        r = c.rec
        mats = [_mat(r, f"L{l}.A") for l in range(c.nl)]
        n_c = int(r["levels"][1])
        cinv = r["cinv"].reshape(n_c, n_c)
        if c.nl:  # the coarsest operator itself is not dumped: the Galerkin product of the last sparse level, or S
            P = _mat(r, f"L{c.nl - 1}.P")
            A_last = (P.T @ mats[-1] @ P).toarray()
        else:
            A_last = _mat(r, "S").toarray()
        for l in range(c.nl - 1):
            P, A = _mat(r, f"L{l}.P"), mats[l]
            want = (P.T @ A @ P).toarray()
            # every entry is a double sum of products p_ki a_kl p_lj: k terms each, k = the longest rows of P^T, A and P together
            k = int(np.diff(P.T.tocsr().indptr).max() + np.diff(A.indptr).max() + np.diff(P.indptr).max())
            bound = (k + 2) * EPS * (abs(P.T) @ abs(A) @ abs(P)).toarray()
            assert np.all(np.abs(mats[l + 1].toarray() - want) <= bound), f"{c.tag}: A_{l + 1} is not P^T A_{l} P"
        # Gauss-Jordan with partial pivoting: |X A - I| <= c n eps cond(A)
        cond = np.linalg.cond(A_last)
        res = np.linalg.norm(cinv @ A_last - np.eye(n_c), 2)
        print(f"{c.tag}: coarsest {n_c} rows, cond {cond:.2e}, |inv A - I| {res:.2e}")
        assert res <= n_c * EPS * cond, f"{c.tag}: coarse_inv A_L - I = {res:.2e}, cond {cond:.2e}"
        assert np.abs(A_last - c.spec.Ac).max() <= 16 * max(np.abs(c.spec.Ac - c.other.Ac).max(), EPS * np.abs(c.spec.Ac).max())


def test_folded_jacobi_is_two_sweeps_entry_by_entry(cases):
    for c in cases:
        r = c.rec
        F, KF = _mat(r, "F"), _mat(r, "KF")
        wd = float(r["omega"][0]) / r["dF"]
        assert np.array_equal(KF.indptr, F.indptr) and np.array_equal(KF.indices, F.indices)
        i, j = pm._rows(F), F.indices
        want = wd[i] * ((i == j) * 2.0 - F.data * wd[j])
        # three roundings on |F_ij wd_j| <= 2 (+ 2 on the diagonal), one more for wd_i
        assert np.all(np.abs(KF.data - want) <= 4 * EPS * np.abs(wd[i]) * ((i == j) * 2.0 + np.abs(F.data * wd[j]))), c.tag
        # ... and two damped sweeps from zero: u = Wd r, u += Wd (r - F u)
        x = np.cos(0.3 * np.arange(F.shape[0]))
        u = wd * x
        u = u + wd * (x - F @ u)
        assert np.linalg.norm(KF @ x - u) <= 64 * EPS * np.linalg.norm(u)


def test_folded_float64_apply_against_the_longdouble_model_measures_the_host_errors(cases):
    worst_v, worst_p, spread = [0.0, 0.0], [0.0, 0.0], [0.0] * 4
    for c in cases:
        xs = pm.inputs(c.th.N, c.n_vel, c.perm)
        for amg in pm.AMG_SWEEPS:
            for sweeps in pm.SWEEPS:
                m = c.driver_folded(sweeps, amg)
                for name, x in xs.items():
                    ref = c.spec.apply(x, sweeps, amg)
                    ev, ep = pm.part_errors(pm.apply_folded(m, x, sweeps), ref, c.n_vel)
                    assert np.isfinite(ev + ep).all(), f"{c.tag} sweeps {sweeps} V({amg},{amg}) {name}: a part the model has zero in is not zero"
                    worst_v = [max(a, b) for a, b in zip(worst_v, ev)]
                    worst_p = [max(a, b) for a, b in zip(worst_p, ep)]
                    # the variant is the same operator: its unfolded apply moves by rounding only
                    if name == "random" and sweeps == 2:
                        sv, spp = pm.part_errors(c.other.apply(x, sweeps, amg), ref, c.n_vel)
                        spread = [max(a, b) for a, b in zip(spread, sv + spp)]
    print(f"measured host errors: velocity {worst_v[0]:.3e} / {worst_v[1]:.3e}, pressure {worst_p[0]:.3e} / {worst_p[1]:.3e} (2-norm / max-norm)")
    print("spread between the model's two variants (velocity 2-norm / max-norm, pressure 2-norm / max-norm):", [f"{v:.3e}" for v in spread])
    tol = pm.tolerances()
    assert all(v <= t for v, t in zip(spread, tol[0] + tol[1])), "the model's variants part by more than the tolerance of the GPU tests"
    for worst, const in ((worst_v, pm.HOST_ERROR_VELOCITY), (worst_p, pm.HOST_ERROR_PRESSURE)):
        for w, k in zip(worst, const):
            assert w <= k <= 2 * w, f"HOST_ERROR constant {k:.3e} is stale: measured {w:.3e}"
    assert pm.MARGIN * max(pm.HOST_ERROR_VELOCITY + pm.HOST_ERROR_PRESSURE) <= 1e-12


def test_reach_table_is_complete(cases):
    """Over the cases the GPU test runs, every kernel path of REACH is exercised by some predicted launch; what is not is in UNREACHED."""
    got = set()
    for c in cases:
        if c.perm_kind != "identity":
            continue
        for amg in pm.AMG_SWEEPS:
            for sweeps in pm.SWEEPS:
                route, rows = c.spec.route(sweeps, amg)
                assert len(route) == c.spec.launches(sweeps)
                here = pm.reach(route, rows, sweeps, amg, c.nl, c.enclosed)
                got |= here
                print(f"{c.tag} sweeps {sweeps} V({amg},{amg}):", [(pm.KERNELS[k], n, ln, lv, row) for (k, n, ln, lv), row in zip(route.tolist(), rows)])
    assert not set(pm.REACH) & set(pm.UNREACHED)
    assert got - set(pm.UNREACHED) == set(pm.REACH), (sorted(set(pm.REACH) - got), sorted(got - set(pm.REACH) - set(pm.UNREACHED)))
    assert not got & set(pm.UNREACHED), f"reached after all: {sorted(got & set(pm.UNREACHED))}"
