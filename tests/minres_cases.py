"""The yardstick of the MINRES tests, on the CPU: a numpy float64 restatement of the iteration of KS_KSP_MINRES (Paige and Saunders, the
preconditioner applied symmetrically, the norm phibar = ||b - P y|| in the M^-1 inner product) and the small symmetric INDEFINITE systems it is run
on. The builders and the right-hand sides are those of tests/cg_cases.py.

    y = 0; r1 = r2 = b; z = M^-1 b; beta1 = sqrt((b,z)); tol = max(rtol beta1, 1e-50)          (beta1 == 0: y = 0, no iteration)
    oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0
    iteration i:  v = z / beta;  u = P v;  if i > 0: u -= (beta / oldb) r1;  alfa = (v,u);  u -= (alfa / beta) r2
                  r1 = r2; r2 = u;  z = M^-1 r2;  oldb = beta;  beta = sqrt((r2,z))
                  oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta
                  gamma = max(hypot(gbar, beta), DBL_EPSILON);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar
                  w1 = w2; w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  y += phi w;  converged when phibar <= tol

tests/test_minres_cases_host.py pins the properties the GPU tests rely on (counts that rounding cannot move), without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import cg_cases as cc

EPS = float(np.finfo(np.float64).eps)
KRON = [(7, 151), (8, 64), (9, 57)]                           # n = 1057 (odd), 512 (one tile), 513 (a tile and a scalar tail): with and without Jacobi-abs
KRON_NONE = KRON + [(13, 79)]                                 # n = 1027: without a preconditioner only (with Jacobi-abs it takes 15 iterations, not 13)
# (index into cc.LAP, sigma): 4 and 5 negative eigenvalues, and a definite one
LAP = [(0, 1.5), (1, 1.1), (0, 0.9)]
# (index into LAP, pc) whose count is exact (tests/test_minres_cases_host.py): all but LAP[1] without a preconditioner, which fails the rule there
LAP_COUNTS = [(0, "none"), (0, "jacobi-abs"), (1, "jacobi-abs"), (2, "none"), (2, "jacobi-abs")]
LAP_ALL = LAP_COUNTS + [(1, "none")]
# LAP[0] under block Jacobi with dense blocks of 8 rows: the count is exact at the widest step above this floor (tests/test_minres_cases_host.py)
BJACOBI_BLOCK, BJACOBI_FLOOR = 8, 1e-7


def minres_reference(P, b, minv=None, rtol=1e-8, max_it=10000, perm=None):
    """The iteration above. P: scipy matrix or ndarray; minv: callable z = M^-1 r (None: the identity). perm: the two dots of an iteration are summed
    over the unknowns in this order (a different rounding of every inner product, nothing else changes). Returns y, its, hist (phibar / beta1 after
    every iteration, hist[0] = 1), gap = |phibar - sqrt((r, M^-1 r))| of the final iterate with r = b - P y, tol, phibar, beta1 and reason
    ("converged", "its", "indefinite preconditioner", "not a number")."""
    minv = minv or (lambda r: r.copy())
    dot = (lambda a, c: float(a @ c)) if perm is None else (lambda a, c: float(a[perm] @ c[perm]))
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    y = np.zeros(n); r1 = b.copy(); r2 = b.copy(); z = minv(b)
    bz = dot(b, z)
    out = lambda **kw: SimpleNamespace(y=y, **kw)
    if not np.isfinite(bz):
        return out(its=0, hist=np.array([1.0]), gap=0.0, tol=0.0, phibar=float("nan"), beta1=float("nan"), reason="not a number")
    if bz < 0.0:
        return out(its=0, hist=np.array([1.0]), gap=0.0, tol=0.0, phibar=0.0, beta1=float("nan"), reason="indefinite preconditioner")
    beta1 = float(np.sqrt(bz))
    tol = max(rtol * beta1, 1e-50)
    if beta1 == 0.0:
        return out(its=0, hist=np.array([1.0]), gap=0.0, tol=tol, phibar=0.0, beta1=0.0, reason="converged")
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w = np.zeros(n); w2 = np.zeros(n)
    hist = [1.0]
    its, reason = 0, None
    while reason is None:
        v = z / beta
        u = P @ v
        if its > 0:
            u = u - (beta / oldb) * r1
        alfa = dot(v, u)
        if not np.isfinite(alfa):
            reason = "not a number"
            break
        u = u - (alfa / beta) * r2
        r1 = r2; r2 = u
        z = minv(r2)
        bz = dot(r2, z)
        if not np.isfinite(bz):
            reason = "not a number"
            break
        if bz < 0.0:
            reason = "indefinite preconditioner"
            break
        oldb = beta
        beta = float(np.sqrt(bz))
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = max(float(np.hypot(gbar, beta)), EPS)
        cs = gbar / gamma
        sn = beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        w1 = w2; w2 = w
        w = (v - oldeps * w1 - delta * w2) / gamma
        y = y + phi * w
        its += 1
        hist.append(phibar / beta1)
        if phibar <= tol:
            reason = "converged"
        elif its >= max_it:
            reason = "its"
    r = b - P @ y
    true = float(np.sqrt(max(float(r @ minv(r)), 0.0)))
    return SimpleNamespace(y=y, its=its, hist=np.array(hist), gap=abs(phibar - true), tol=tol, phibar=phibar, beta1=beta1, reason=reason, true=true)


def jacobi_abs(P):
    """Point Jacobi with PCJacobiSetUseAbs: 1 / |diag(P)|; a zero entry leaves its row unscaled."""
    d = np.abs(np.asarray(P.diagonal(), dtype=np.float64))
    d = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    return lambda r: d * r


def block_jacobi(P, bs):
    """Block Jacobi with dense blocks (KS_PC_BJACOBI): the exact inverses of the diagonal blocks of bs consecutive rows."""
    D = P.toarray()
    inv = [np.linalg.inv(D[i:i + bs, i:i + bs]) for i in range(0, D.shape[0], bs)]
    return lambda r: np.concatenate([m @ r[j * bs:j * bs + len(m)] for j, m in enumerate(inv)])


def minv_of(P, pc):
    return jacobi_abs(P) if pc == "jacobi-abs" else None


def mnorm(minv, r):
    """||r|| in the M^-1 inner product, sqrt((r, M^-1 r))."""
    z = r if minv is None else minv(r)
    return float(np.sqrt(max(float(r @ z), 0.0)))


@functools.lru_cache(maxsize=None)
def kron(m, blocks):
    """I (x) T, T the m x m tridiagonal with diagonal -2.1 + 0.75 j and off-diagonals -1: symmetric indefinite (three negative eigenvalues, negative
    diagonal entries), m distinct eigenvalues with or without Jacobi-abs, so MINRES ends at iteration m exactly."""
    T = sp.diags([-np.ones(m - 1), -2.1 + 0.75 * np.arange(m), -np.ones(m - 1)], [-1, 0, 1])
    return cc._case(sp.kron(sp.identity(blocks), T), 100 + m, "ikron(%d,%d)" % (m, blocks))


@functools.lru_cache(maxsize=None)
def kron_reference(m, blocks, pc):
    case = kron(m, blocks)
    return case, minres_reference(case.P, case.b, minv_of(case.P, pc), rtol=1e-8)


def pick_k(hist, lo=1e-10):
    """The step k with the largest ratio h[k-1] / h[k] among those with lo < h[k] < 1e-5; the tolerance is the geometric mean of the two.
    Returns (k, rtol, ratio)."""
    best = None
    for k in range(1, len(hist)):
        if lo < hist[k] < 1e-5:
            ratio = hist[k - 1] / hist[k]
            if best is None or ratio > best[2]:
                best = (k, float(np.sqrt(hist[k - 1] * hist[k])), float(ratio))
    assert best is not None, "the history does not pass through (%g, 1e-5)" % lo
    return best


@functools.lru_cache(maxsize=None)
def lap_reference(which, pc):
    """(case, P, rtol, reference, k, ratio) of LAP[which] = (index into cg_cases.LAP, sigma) under sinvert at sigma with `pc` in ("jacobi-abs", "none"),
    the tolerance derived from the restatement's history (pick_k). Computed once per process."""
    idx, sigma = LAP[which]
    case = cc.lap(*cc.LAP[idx])
    P = cc.shifted(case, sigma)
    minv = minv_of(P, pc)
    long = minres_reference(P, case.b, minv, rtol=1e-12)
    k, rtol, ratio = pick_k(long.hist)
    ref = minres_reference(P, case.b, minv, rtol=rtol)
    return case, P, rtol, ref, k, ratio
