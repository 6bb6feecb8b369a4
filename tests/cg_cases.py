"""The yardstick of the CG tests, on the CPU: a numpy float64 restatement of the iteration of KS_KSP_CG (KSPCG, left preconditioner,
preconditioned residual norm) and the small symmetric positive definite systems it is run on, as CSR arrays with integer right-hand sides.

    y = 0; r = b; z = M^-1 r; dp0 = ||z||; tol = max(rtol dp0, 1e-50)                      (dp0 == 0: y = 0, no iteration)
    iteration i:  gamma = (r,z);  p = z (i = 0) or z + (gamma / gamma_old) p;  w = P p;  delta = (p,w);  alpha = gamma / delta
                  y += alpha p;  r -= alpha w;  z = M^-1 r;  dp = ||z||;  converged when dp <= tol

tests/test_cg_cases_host.py pins the properties the GPU tests rely on (counts that rounding cannot move), without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

KRON = [(7, 151), (13, 79), (8, 64), (9, 57)]                 # n = 1057 (odd), 1027 (odd), 512 (one tile), 513 (a tile and a scalar tail)
LAP = [(33, 31, 0.5, 5), (37, 29, 0.05, 6)]                   # n = 1023, 1073


def cg_reference(P, b, minv=None, rtol=1e-8, max_it=10000):
    """The iteration above. P: scipy matrix or ndarray; minv: callable z = M^-1 r (None: the identity). Returns y, its, hist (dp / dp0 after
    every iteration, hist[0] = 1), gap = ||M^-1 (b - P y) - z_final||, tol and reason ("converged", "its", "indefinite matrix",
    "indefinite preconditioner", "not a number")."""
    minv = minv or (lambda r: r.copy())
    b = np.asarray(b, dtype=np.float64)
    y = np.zeros_like(b); r = b.copy(); z = minv(r)
    dp0 = dp = float(np.sqrt(z @ z))
    tol = max(rtol * dp0, 1e-50)
    hist = [1.0]
    its, reason, gamma_old, p = 0, None, 0.0, None
    while True:
        gamma = float(r @ z)
        if not (np.isfinite(dp) and np.isfinite(gamma)):
            reason = "not a number"
        elif dp <= tol:
            reason = "converged"
        elif its >= max_it:
            reason = "its"
        elif gamma < 0.0:
            reason = "indefinite preconditioner"
        if reason:
            break
        p = z.copy() if its == 0 else z + (gamma / gamma_old) * p
        w = P @ p
        delta = float(p @ w)
        if not np.isfinite(delta):
            reason = "not a number"
            break
        if delta <= 0.0:
            reason = "indefinite matrix"
            break
        alpha = gamma / delta
        y = y + alpha * p
        r = r - alpha * w
        z = minv(r)
        dp = float(np.sqrt(z @ z))
        gamma_old = gamma
        its += 1
        hist.append(dp / dp0 if dp0 else 0.0)
    gap = float(np.linalg.norm(minv(b - P @ y) - z))
    return SimpleNamespace(y=y, its=its, hist=np.array(hist), gap=gap, tol=tol, dp=dp, dp0=dp0, reason=reason)


def _case(P, seed, name):
    P = sp.csr_matrix(P); P.sort_indices()
    n = P.shape[0]
    b = np.random.default_rng(seed).integers(-8, 9, n).astype(np.float64)
    return SimpleNamespace(name=name, n=n, P=P, rowptr=P.indptr.astype(np.int32), col=P.indices.astype(np.int32), val=P.data.astype(np.float64), b=b,
                           diag=P.diagonal().copy())


@functools.lru_cache(maxsize=None)
def kron(m, blocks):
    """I (x) T, T the m x m tridiagonal with diagonal 2 + 0.25 j and off-diagonals -1: the operator, with or without Jacobi, has m distinct
    eigenvalues, so CG ends at iteration m exactly."""
    T = sp.diags([-np.ones(m - 1), 2.0 + 0.25 * np.arange(m), -np.ones(m - 1)], [-1, 0, 1])
    return _case(sp.kron(sp.identity(blocks), T), 100 + m, "kron(%d,%d)" % (m, blocks))


@functools.lru_cache(maxsize=None)
def lap(nx, ny, shift, seed):
    """5-point Laplacian + shift + an integer diagonal rng.integers(0, 4, n)."""
    n = nx * ny
    Tx = sp.diags([-np.ones(nx - 1), 2.0 * np.ones(nx), -np.ones(nx - 1)], [-1, 0, 1])
    Ty = sp.diags([-np.ones(ny - 1), 2.0 * np.ones(ny), -np.ones(ny - 1)], [-1, 0, 1])
    L = sp.kron(sp.identity(ny), Tx) + sp.kron(Ty, sp.identity(nx))
    d = np.random.default_rng(seed).integers(0, 4, n).astype(np.float64)
    return _case(L + sp.diags(d + shift), seed, "lap(%d,%d,%g,%d)" % (nx, ny, shift, seed))


def shifted(case, sigma):
    """P = A - sigma I of a case, as the ST forms it."""
    return (case.P - sigma * sp.identity(case.n)).tocsr()


def jacobi(P):
    d = 1.0 / P.diagonal()
    return lambda r: d * r


def pick_k(hist, near):
    """An iteration k whose neighbours are a factor of 2 apart, h[k-1] / h[k] >= 2, with sqrt(h[k-1] h[k]) closest to `near` (in the logarithm):
    at rtol = sqrt(h[k-1] h[k]) the count is k unless rounding moves a residual norm by a factor sqrt(2). Returns (k, rtol)."""
    best = None
    for k in range(1, len(hist)):
        if hist[k] > 0 and hist[k - 1] / hist[k] >= 2.0:
            rt = float(np.sqrt(hist[k - 1] * hist[k]))
            # the count at rt is k only if no earlier iterate is already below it
            if np.all(hist[:k] > rt) and (best is None or abs(np.log(rt / near)) < abs(np.log(best[1] / near))):
                best = (k, rt)
    assert best is not None, "no iteration with a factor 2 to its predecessor"
    return best


@functools.lru_cache(maxsize=None)
def lap_reference(idx, pc, sigma, near):
    """(case, P, rtol, reference) of LAP[idx] under sinvert at sigma with `pc` in ("jacobi", "none"), the tolerance derived from the reference history
    at an iteration near `near` (pick_k). Computed once per process."""
    case = lap(*LAP[idx])
    P = shifted(case, sigma)
    minv = jacobi(P) if pc == "jacobi" else None
    long = cg_reference(P, case.b, minv, rtol=1e-15)
    k, rtol = pick_k(long.hist, near)
    ref = cg_reference(P, case.b, minv, rtol=rtol)
    return case, P, rtol, ref, k


@functools.lru_cache(maxsize=None)
def kron_reference(idx, pc):
    case = kron(*KRON[idx])
    minv = jacobi(case.P) if pc == "jacobi" else None
    return case, cg_reference(case.P, case.b, minv, rtol=1e-8)
