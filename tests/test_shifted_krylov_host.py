"""The complex Givens / least-squares recurrence of the shifted solver's GMRES (``csrc/fc_cgivens.hpp``) without a GPU: the header
the kernel ``fc_cgmres_givens`` includes is compiled into a small C++ driver, restated in numpy, and both are checked against
``numpy.linalg.lstsq`` on random complex Hessenberg matrices."""
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
M = 19  # 20 x 19 Hessenberg matrices


def givens_lstsq(H, g0):
    """min |g0 e1 - H y| column by column: stored rotations onto the new column, one new rotation, the right-hand side follows
    (fc_cgivens_column), then the column-oriented back substitution (fc_cgivens_backsolve).  Returns (y, |residual|)."""
    m = H.shape[1]
    R = np.zeros((m, m), dtype=complex)
    cs, sn = np.zeros(m), np.zeros(m, dtype=complex)
    g = np.zeros(m + 1, dtype=complex)
    g[0] = g0
    for j in range(m):
        col = H[: j + 2, j].copy()
        for i in range(j):
            x, y = col[i], col[i + 1]
            col[i], col[i + 1] = cs[i] * x + sn[i] * y, cs[i] * y - np.conj(sn[i]) * x
        a, b = col[j], col[j + 1]
        na, r = abs(a), np.hypot(abs(a), abs(b))
        ph = a / na if na > 0 else 1.0
        cs[j], sn[j] = na / r, (ph * np.conj(b / r) if na > 0 else 1.0)
        col[j], col[j + 1] = (ph * r if na > 0 else b), 0.0
        g[j + 1], g[j] = -np.conj(sn[j]) * g[j], cs[j] * g[j]
        R[: j + 1, j] = col[: j + 1]
    res = abs(g[m])
    y = np.zeros(m, dtype=complex)
    g = g[:m].copy()
    for i in range(m - 1, -1, -1):
        y[i] = g[i] / R[i, i]
        g[:i] -= R[:i, i] * y[i]
    return y, res


#: numpy's lstsq (the reference) is itself accurate to about eps * cond(H) only, so the 1e-13 of the comparison means something
#: for cond(H) eps << 1e-13: the cases are drawn until cond(H) <= 50 (eps * 50 = 1.1e-14), whatever the code under test returns
COND_MAX = 50.0


def _draw(rng):
    while True:
        H = np.triu(rng.standard_normal((M + 1, M)) + 1j * rng.standard_normal((M + 1, M)), -1) / np.sqrt(M)
        H[np.arange(M), np.arange(M)] += 2.0 * np.exp(2j * np.pi * rng.random(M))
        if np.linalg.cond(H) <= COND_MAX:
            return H


def _cases():
    rng = np.random.default_rng(11)
    out = [(_draw(rng), float(rng.uniform(0.5, 2.0))) for _ in range(8)]
    # the GMRES shape: real non-negative subdiagonal; and a zero diagonal entry met by the new rotation
    while True:
        H = _draw(rng)
        H[np.arange(1, M + 1), np.arange(M)] = np.abs(H[np.arange(1, M + 1), np.arange(M)])
        H0 = H.copy()
        H0[0, 0] = 0.0
        if max(np.linalg.cond(H), np.linalg.cond(H0)) <= COND_MAX:
            break
    # one plain random Hessenberg matrix, as drawn: no boost of the diagonal, no bound on its condition number
    Hraw = np.triu(rng.standard_normal((M + 1, M)) + 1j * rng.standard_normal((M + 1, M)), -1)
    return out + [(H, 1.0), (H0, 1.0), (Hraw, 1.0)]


def test_complex_givens_recurrence_matches_lstsq(tmp_path):
    exe = tmp_path / "cgivens_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tests" / "support" / "cgivens_host_check.cpp"), "-o", str(exe)],
                   check=True)
    cases = _cases()
    lines = []
    for H, g0 in cases:
        lines.append(f"{M} {g0!r}")
        for j in range(M):
            lines.append(" ".join(f"{float(v.real)!r} {float(v.imag)!r}" for v in H[:, j]))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split()
    vals = np.array(out, dtype=float)
    per = 2 + 4 * M
    assert vals.size == per * len(cases)
    for c, (H, g0) in enumerate(cases):
        blk = vals[c * per:(c + 1) * per]
        assert int(blk[0]) == M
        y1 = blk[2:2 + 2 * M].view(complex)
        y64 = blk[2 + 2 * M:].view(complex)
        rhs = np.zeros(M + 1, dtype=complex)
        rhs[0] = g0
        yref = np.linalg.lstsq(H, rhs, rcond=None)[0]
        rref = np.linalg.norm(rhs - H @ yref)
        ynp, rnp = givens_lstsq(H, g0)
        scale = np.linalg.norm(yref)
        # the drawn cases: 1e-13.  The unfiltered one: both solutions are backward stable, each within about m cond(H) eps of the
        # exact one (m = 19 columns), so they differ by at most twice that
        tol = 1e-13 if np.linalg.cond(H) <= COND_MAX else 2 * M * np.linalg.cond(H) * np.finfo(float).eps
        for name, y in (("header, one lane", y1), ("header, 64 lanes", y64), ("numpy", ynp)):
            assert np.linalg.norm(y - yref) <= tol * scale, (c, name, np.linalg.norm(y - yref) / scale, tol)
        np.testing.assert_array_equal(y1, y64)  # disjoint rows per lane: the same sums
        assert abs(blk[1] - rref) <= tol * g0 and abs(rnp - rref) <= tol * g0, (c, blk[1], rnp, rref)
