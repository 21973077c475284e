"""numpy model of the POD and DMD of flowcontrol_amd/modal.py: the same formulas on host arrays, written independently of the product
(snapshots are ROWS of X, [m][N], as the snapshot bank hands them out; M is a symmetric positive semidefinite scipy / numpy matrix,
None = identity)."""
import numpy as np

EPS = 2.0 ** -53


def _apply(M, Xt):
    """M @ Xt for Xt [N][m]."""
    return Xt if M is None else np.asarray(M @ Xt)


def gram(L, R, M=None):
    """L M R^T for row-snapshot arrays L [ma][N], R [mb][N]."""
    return np.asarray(L) @ _apply(M, np.asarray(R).T)


def gram_longdouble(L, R, M=None):
    """The same in np.longdouble (M dense or sparse; converted once)."""
    Ll, Rl = np.asarray(L, dtype=np.longdouble), np.asarray(R, dtype=np.longdouble)
    if M is None:
        return Ll @ Rl.T
    Md = np.asarray(M.toarray() if hasattr(M, "toarray") else M, dtype=np.longdouble)
    return Ll @ (Md @ Rl.T)


def gram_bound(L, R, M=None):
    """Componentwise rounding bound of an fp64 evaluation of L M R^T in any summation order: 2 (N + m) eps |L| |M| |R|^T, m the larger
    of the two column counts (the operator pass and the product are sums of at most N + m terms each, to first order)."""
    L, R = np.abs(np.asarray(L)), np.abs(np.asarray(R))
    N, m = L.shape[1], max(L.shape[0], R.shape[0])
    return 2.0 * (N + m) * EPS * (L @ _apply(None if M is None else abs(M), R.T))


def sorted_eig(G):
    w, V = np.linalg.eigh(0.5 * (G + G.T))
    o = np.argsort(w)[::-1]
    return w[o], V[:, o]


def pod(X, M=None, r=None, center=True):
    """sigma [m], V [m][r], Phi [r][N], mean [N] of the snapshots X [m][N]: X_c^T M X_c = V S^2 V^T, Phi = V_r^T X_c / S_r."""
    X = np.asarray(X, dtype=float)
    mean = X.mean(axis=0) if center else np.zeros(X.shape[1])
    Xc = X - mean
    w, V = sorted_eig(gram(Xc, Xc, M))
    sigma = np.sqrt(np.maximum(w, 0.0))
    if r is None:
        r = int(np.count_nonzero(sigma > np.sqrt(len(sigma) * 2 * EPS) * sigma[0]))
    Phi = (V[:, :r] / sigma[:r]).T @ Xc
    return sigma, V[:, :r], Phi, mean


def bdf2_rate(mu, dt, every=1):
    mu1 = np.asarray(mu, dtype=complex) ** (1.0 / every)
    return (3 * mu1 ** 2 - 4 * mu1 + 1) / (2 * dt * mu1 ** 2)


def bdf2_amplification(lam, dt, every=1):
    """One BDF2 step of x' = lam x multiplies the physical solution by the root of (3 - 2 z) mu^2 - 4 mu + 1 = 0, z = dt lam, that
    tends to 1 with z."""
    z = dt * np.asarray(lam, dtype=complex)
    return ((2 + np.sqrt(1 + 2 * z)) / (3 - 2 * z)) ** every


def dmd(X, M=None, r=2, dt=1.0, every=1):
    """mu (by decreasing modulus), lam, lam_bdf2 of the snapshots X [m][N] projected on r POD modes of X1."""
    X = np.asarray(X, dtype=float)
    X1, X2 = X[:-1], X[1:]
    w, V = sorted_eig(gram(X1, X1, M))
    T = V[:, :r] / np.sqrt(w[:r])
    mu = np.linalg.eigvals(T.T @ gram(X1, X2, M) @ T)
    mu = mu[np.argsort(-np.abs(mu), kind="stable")]
    return mu, np.log(mu.astype(complex)) / (every * dt), bdf2_rate(mu, dt, every)


def synthetic_sequence(N, m, seed=0, nvel=None):
    """x_j = sum_k Re(c_k mu_k^j v_k), j = 0 .. m - 1, for three complex mu_k of modulus near one and orthonormal real / imaginary parts
    of the v_k: a rank-6, well-conditioned sequence whose DMD with r = 6 must return the mu_k and their conjugates.  Entries past
    nvel (the pressure part of a W-layout vector, on which the energy weight vanishes) are filled by the same recurrence."""
    rng = np.random.default_rng(seed)
    mus = np.array([0.98 * np.exp(0.21j), 1.01 * np.exp(0.55j), 0.95 * np.exp(1.3j)])
    nvel = N if nvel is None else nvel
    Q = np.zeros((N, 6))
    Q[:nvel], _ = np.linalg.qr(rng.standard_normal((nvel, 6)))
    Q[nvel:] = rng.standard_normal((N - nvel, 6)) / np.sqrt(max(nvel, 1))
    v = Q[:, 0::2] + 1j * Q[:, 1::2]
    c = np.array([1.0, 0.8 - 0.3j, 1.2 + 0.5j])
    j = np.arange(m)[:, None]
    X = np.real((c * mus ** j) @ v.T)
    return X, np.r_[mus, mus.conj()]


def match(found, known):
    """Largest distance from each known value to the nearest found one."""
    found, known = np.asarray(found), np.asarray(known)
    return max(np.min(np.abs(found - k)) for k in known)
