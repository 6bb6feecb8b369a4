"""The yardstick of the BiCGStab(l) tests, on the CPU: a numpy float64 restatement of the iteration of KS_KSP_BCGSL (Sleijpen and Fokkema's
BiCGStab(l), left preconditioner, preconditioned residual norm), operation for operation, and the small non-symmetric systems it is run on.

    y = 0; r_0 = M^-1 b; rt = r_0; u_0 = 0; rho0 = 1; alpha = 0; omega = 1; dp0 = ||r_0||; tol = max(rtol dp0, 1e-50)      (dp0 == 0: y = 0, no iteration)
    cycle:  converged when ||r_0|| <= tol; "its" when its >= max_it                                                 (both tested at the start of a cycle only)
            rho0 = -omega rho0
            for j = 0 .. l-1:  rho1 = (r_j, rt); beta = alpha (rho1 / rho0); rho0 = rho1;  u_i = r_i - beta u_i (i <= j);  u_{j+1} = A^ u_j
                               sigma = (u_{j+1}, rt); alpha = rho1 / sigma;  y += alpha u_0;  r_i -= alpha u_{i+1} (i <= j);  r_{j+1} = A^ r_j;  its++
            G = [r_0 .. r_l]^T [r_0 .. r_l];  gamma = argmin ||r_0 - sum_j gamma_j r_j||  (Cholesky of G(1:l,1:l), right-hand side G(1:l,0))
            y += sum gamma_j r_{j-1};  r_0 -= sum gamma_j r_j;  u_0 -= sum gamma_j u_j;  omega = gamma_l

Every inner product goes through one hook that sums over a permutation of the unknowns: the device sums in another order than numpy, and
tests/test_bcgsl_cases_host.py pins, without a GPU, which properties no order can move (the counts the GPU tests require)."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

# (m, blocks, pc) of the I (x) T systems: n = 1208 (pairs and tiles), 384 (one tile and a half), 632
KRON = [(8, 151, "jacobi"), (6, 64, "jacobi"), (8, 79, "none")]
# (nx, ny, c, sigma) of the convection-diffusion systems under sinvert at sigma, point Jacobi
CONVDIFF = [(45, 31, 3.0, 2.0), (45, 31, 8.0, 0.0), (24, 24, 20.0, 0.0)]


def make_dot(perm=None):
    """(a, b) summed in numpy's order, or over the permutation `perm` of the unknowns"""
    if perm is None:
        return lambda a, b: float(np.sum(a * b))
    return lambda a, b: float(np.sum((a * b)[perm]))


def bcgsl_reference(P, b, minv=None, ell=2, rtol=1e-8, max_it=10000, perm=None):
    """The iteration above. P: scipy matrix or ndarray; minv: callable z = M^-1 r (None: the identity); perm: the order of every sum. Returns y,
    its (BiCG steps), hist (||r_0|| / dp0 at the start of every cycle, hist[0] = 1), gap = ||M^-1 (b - P y) - r_0||, tol, dp, dp0, values (the
    scalars of the step that ended the solve) and reason ("converged", "its", "breakdown", "singular", "not a number")."""
    minv = minv or (lambda r: r.copy())
    dot = make_dot(perm)
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    op = lambda x: minv(P @ x)
    y = np.zeros(n)
    r = [minv(b)] + [np.zeros(n) for _ in range(ell)]
    u = [np.zeros(n) for _ in range(ell + 1)]
    rt = r[0].copy()
    rho0, alpha, omega = 1.0, 0.0, 1.0
    its, reason, hist, tol, dp0, values = 0, None, [], 0.0, 0.0, {}
    while True:
        rho1 = dot(r[0], rt)
        dp = float(np.sqrt(dot(r[0], r[0])))
        if its == 0:
            dp0 = dp
            tol = max(rtol * dp0, 1e-50)
        hist.append(dp / dp0 if dp0 else 0.0)
        rho0 = -omega * rho0
        if not (np.isfinite(dp) and np.isfinite(rho1) and np.isfinite(rho0)):
            reason = "not a number"
        elif dp <= tol:
            reason = "converged"
        elif its >= max_it:
            reason = "its"
        elif rho0 == 0.0:
            reason = "breakdown"
        if reason:
            break
        for j in range(ell):
            if j > 0:
                rho1 = dot(r[j], rt)
                if not np.isfinite(rho1):
                    reason = "not a number"
                elif rho0 == 0.0:
                    reason = "breakdown"
                if reason:
                    break
            beta = alpha * (rho1 / rho0)
            rho0 = rho1
            for i in range(j + 1):
                u[i] = r[i] - beta * u[i]
            u[j + 1] = op(u[j])
            sigma = dot(u[j + 1], rt)
            values = {"rho1": rho1, "sigma": sigma}
            if not np.isfinite(sigma):
                reason = "not a number"
            elif sigma == 0.0:
                reason = "breakdown"
            if reason:
                break
            alpha = rho1 / sigma
            y = y + alpha * u[0]
            for i in range(j + 1):
                r[i] = r[i] - alpha * u[i + 1]
            r[j + 1] = op(r[j])
            its += 1
        if reason:
            break
        G = np.array([[dot(r[a], r[c]) if a <= c else 0.0 for c in range(ell + 1)] for a in range(ell + 1)])
        G = G + np.triu(G, 1).T
        C = np.zeros((ell, ell)); gamma = np.zeros(ell)
        for j in range(ell):                                # Cholesky of G(1:l,1:l), column by column
            for i in range(j, ell):
                s = G[i + 1, j + 1]
                for k in range(j):
                    s -= C[i, k] * C[j, k]
                if i == j:
                    if not np.isfinite(s):
                        reason = reason or "not a number"
                    elif s <= 0.0:
                        reason = reason or "singular"
                    if reason:
                        values = {"pivot": s}
                        break
                    C[j, j] = np.sqrt(s)
                else:
                    C[i, j] = s / C[j, j]
            if reason:
                break
        if reason:
            break
        for i in range(ell):
            s = G[i + 1, 0]
            for k in range(i):
                s -= C[i, k] * gamma[k]
            gamma[i] = s / C[i, i]
        for i in range(ell - 1, -1, -1):
            s = gamma[i]
            for k in range(i + 1, ell):
                s -= C[k, i] * gamma[k]
            gamma[i] = s / C[i, i]
        if not np.all(np.isfinite(gamma)):
            reason = "not a number"
            break
        r0_old = r[0]
        for j in range(1, ell + 1):
            y = y + gamma[j - 1] * (r0_old if j == 1 else r[j - 1])
        r0 = r[0].copy(); u0 = u[0].copy()
        for j in range(1, ell + 1):
            r0 = r0 - gamma[j - 1] * r[j]
            u0 = u0 - gamma[j - 1] * u[j]
        r[0], u[0] = r0, u0
        omega = gamma[ell - 1]
    gap = float(np.linalg.norm(minv(b - P @ y) - r[0]))
    return SimpleNamespace(y=y, its=its, hist=np.array(hist), gap=gap, tol=tol, dp=dp, dp0=dp0, reason=reason, values=values, ell=ell)


def _case(P, seed, name):
    P = sp.csr_matrix(P); P.sort_indices()
    n = P.shape[0]
    b = np.random.default_rng(seed).integers(-8, 9, n).astype(np.float64)
    return SimpleNamespace(name=name, n=n, P=P, rowptr=P.indptr.astype(np.int32), col=P.indices.astype(np.int32), val=P.data.astype(np.float64), b=b)


@functools.lru_cache(maxsize=None)
def kron(m, blocks):
    """I (x) T, T the m x m tridiagonal with diagonal 2.1 + 0.75 j, super-diagonal 1.3 and sub-diagonal -0.9: the off-diagonal products are negative, so
    every eigenvalue of T (and of D^-1 T) is complex, and the operator has m distinct ones: BiCG ends at step m exactly."""
    T = sp.diags([-0.9 * np.ones(m - 1), 2.1 + 0.75 * np.arange(m), 1.3 * np.ones(m - 1)], [-1, 0, 1])
    return _case(sp.kron(sp.identity(blocks), T), 300 + m, "kron(%d,%d)" % (m, blocks))


@functools.lru_cache(maxsize=None)
def convdiff(nx, ny, c):
    """The 5-point convection-diffusion operator on an nx x ny grid, central differences, convection in both directions: diagonal 4, off-diagonals
    -1 - c (towards lower indices) and -1 + c."""
    def t(k):
        return sp.diags([(-1.0 - c) * np.ones(k - 1), 2.0 * np.ones(k), (-1.0 + c) * np.ones(k - 1)], [-1, 0, 1])
    A = sp.kron(sp.identity(ny), t(nx)) + sp.kron(t(ny), sp.identity(nx))
    return _case(A, 500 + nx, "convdiff(%d,%d,%g)" % (nx, ny, c))


@functools.lru_cache(maxsize=None)
def convdiff_x(nx, ny, c):
    """Convection along x only, diffusion in both directions: the eigenvalues 4 + 2 cos(theta_y) + 2 i sqrt(c^2 - 1) cos(theta_x) fill a rectangle of the
    complex plane and are well separated there, which an eigensolver needs (those of convdiff lie on the line Re = 4, and the ones nearest a real
    target are a cluster)."""
    tx = sp.diags([(-1.0 - c) * np.ones(nx - 1), 2.0 * np.ones(nx), (-1.0 + c) * np.ones(nx - 1)], [-1, 0, 1])
    ty = sp.diags([-np.ones(ny - 1), 2.0 * np.ones(ny), -np.ones(ny - 1)], [-1, 0, 1])
    return _case(sp.kron(sp.identity(ny), tx) + sp.kron(ty, sp.identity(nx)), 500 + nx, "convdiff_x(%d,%d,%g)" % (nx, ny, c))


def shifted(case, sigma):
    """P = A - sigma I of a case, as the ST forms it."""
    return (case.P - sigma * sp.identity(case.n)).tocsr()


def jacobi(P):
    d = 1.0 / P.diagonal()
    return lambda r: d * r


def perms(n, count=4):
    """summation orders: numpy's own, reversed, and seeded shuffles"""
    out = [None, np.arange(n)[::-1].copy()]
    for s in range(count - 2):
        out.append(np.random.default_rng(900 + s).permutation(n))
    return out


@functools.lru_cache(maxsize=None)
def kron_reference(idx, ell, rtol=1e-12):
    m, blocks, pc = KRON[idx]
    case = kron(m, blocks)
    minv = jacobi(case.P) if pc == "jacobi" else None
    return case, pc, bcgsl_reference(case.P, case.b, minv, ell=ell, rtol=rtol)


def kron_count(idx, ell):
    """m BiCG steps rounded up to a multiple of l"""
    m = KRON[idx][0]
    return -(-m // ell) * ell


@functools.lru_cache(maxsize=None)
def convdiff_reference(idx, ell, rtol=1e-8, max_it=4000):
    nx, ny, c, sigma = CONVDIFF[idx]
    case = convdiff(nx, ny, c)
    P = shifted(case, sigma)
    return case, P, sigma, bcgsl_reference(P, case.b, jacobi(P), ell=ell, rtol=rtol, max_it=max_it)
