"""A numpy restatement of the Jacobi-Davidson solver of slepc_amd/csrc/ks_jd.hip as built, for the iteration counts quoted in tests/test_gpu_jd.py.

The outer loop is the one of scripts/gd_restatement.py (the library's two solvers share Gd::solve in the same way); this file fills its correction hook
with what Jd::correction does: Q = [locked, U], Zq = B Q, Y = K^-1 Zq, M = Zq^T Y, the shift pair from `fix`, the fallbacks to the GD correction, and the
left-preconditioned BiCGStab or GMRES(30) of ks_st.hip on P K^-1 (theta1 A - theta0 B) from a zero start, where reaching max_it or breaking down
ends the solve with the iterate it has. What differs from the library is the random initial basis (numpy's generator here), so the counts are quoted
as ranges over three seeds. Runs on the CPU:  python scripts/jd_restatement.py"""
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import scenarios as sc  # noqa: E402
from gd_restatement import bjacobi, gd, jacobi  # noqa: E402

EPS = np.finfo(float).eps


def bcgs(op, rhs, rtol, max_it):
    """ks_ksp_bcgs, not strict: returns (y, iterations)"""
    y = np.zeros_like(rhs); r = rhs.copy()
    beta0 = np.linalg.norm(r)
    if beta0 == 0.0 or not np.isfinite(beta0):
        return y, 0
    tol = max(rtol * beta0, 1e-50)
    rh = r.copy(); p = np.zeros_like(r); v = np.zeros_like(r)
    rho = alpha = omega = 1.0
    its = 0
    for _ in range(max_it):
        rho_new = rh @ r
        if rho_new == 0.0 or omega == 0.0 or not np.isfinite(rho_new):
            break
        bt = (rho_new / rho) * (alpha / omega)
        p = bt * (p - omega * v) + r
        v = op(p)
        d = rh @ v
        if d == 0.0 or not np.isfinite(d):
            break
        alpha = rho_new / d
        s = r - alpha * v
        t = op(s)
        tt = t @ t
        omega = (s @ t) / tt if tt != 0.0 else 0.0
        y = y + alpha * p + omega * s
        r = s - omega * t
        rho = rho_new; its += 1
        if np.linalg.norm(r) <= tol:
            break
    return y, its


def gmres(op, rhs, rtol, max_it, restart=30):
    """ks_ksp_gmres, not strict (classical Gram-Schmidt without refinement): returns (y, iterations)"""
    n = rhs.shape[0]
    y = np.zeros(n); r = rhs.copy(); beta = np.linalg.norm(r)
    if beta == 0.0 or not np.isfinite(beta):
        return y, 0
    tol = max(rtol * beta, 1e-50)
    its = 0
    while True:
        K = np.zeros((n, restart + 1)); Hm = np.zeros((restart + 1, restart)); K[:, 0] = r / beta
        g = np.zeros(restart + 1); g[0] = beta
        jj = 0; res = beta
        for j in range(restart):
            w = op(K[:, j])
            h = K[:, :j + 1].T @ w
            w = w - K[:, :j + 1] @ h
            hn = np.linalg.norm(w)
            Hm[:j + 1, j] = h; Hm[j + 1, j] = hn
            if hn > 0:
                K[:, j + 1] = w / hn
            its += 1; jj = j + 1
            yc, *_ = np.linalg.lstsq(Hm[:jj + 1, :jj], g[:jj + 1], rcond=None)
            res = np.linalg.norm(g[:jj + 1] - Hm[:jj + 1, :jj] @ yc)
            if res <= tol or its >= max_it or hn == 0.0:
                break
        y = y + K[:, :jj] @ yc
        if res <= tol or its >= max_it:
            return y, its
        r = rhs - op(y); beta = np.linalg.norm(r)
        if beta <= tol or not np.isfinite(beta):
            return y, its


def lu_inverse(M):
    """ksd::lu_inverse: None when a pivot is at most n eps ||M||_inf"""
    k = M.shape[0]
    if k == 0:
        return M.copy()
    lu, piv = scipy.linalg.lu_factor(M, check_finite=False)
    if not np.all(np.abs(np.diag(lu)) > k * EPS * np.abs(M).sum(axis=1).max()):
        return None
    return scipy.linalg.lu_solve((lu, piv), np.eye(k))


def jd(A, B=None, which="largest_magnitude", target=0.0, pc=None, fix=0.01, const_tol=True, ksp="bcgs", rtol=1e-4, ksp_max_it=90, **kw):
    """returns (eigenvalues, outer iterations, restarts, locks, inner solves, inner iterations, GD fallbacks)"""
    Bm = (lambda x: B @ x) if B is not None else (lambda x: x)
    Kinv = pc if pc is not None else (lambda R: R)
    st = {"dyntol": 0.5, "solves": 0, "its": 0, "fallbacks": 0}
    largest = which in ("largest_magnitude", "largest_real")

    def correct(X, R, theta, locked):
        Q = np.hstack([locked, X]); nb = X.shape[1]
        Zq = Bm(Q); Yq = Kinv(Zq)
        Minv = lu_inverse(Zq.T @ Yq)
        proj = (lambda w: w - Yq @ (Minv @ (Zq.T @ w))) if Minv is not None else None
        tol = rtol if const_tol else st["dyntol"]
        D = np.zeros_like(R); solved = False
        for j in range(nb):
            rn = np.linalg.norm(R[:, j])
            if rn < fix * abs(theta[j]):
                th0, th1 = theta[j], 1.0
            elif which == "target_magnitude":
                th0, th1 = target, 1.0
            elif largest:
                th0, th1 = 1.0, 0.0
            else:
                th0, th1 = 0.0, 1.0
            fallback = proj is None or (B is None and th1 == 0.0)
            if not fallback:
                def op(x):
                    return proj(Kinv((th1 * (A @ x) - th0 * Bm(x))[:, None])[:, 0])
                rhs = -proj(Kinv(R[:, j:j + 1])[:, 0])
                t, its = (bcgs if ksp == "bcgs" else gmres)(op, rhs, tol, ksp_max_it)
                st["solves"] += 1; st["its"] += its; solved = True
                nt = np.linalg.norm(t)
                fallback = not (nt > 0.0) or not np.isfinite(nt)
            if fallback:
                t = Kinv(R[:, j:j + 1])[:, 0]
                if proj is not None:
                    t = proj(t)
                st["fallbacks"] += 1
            D[:, j] = t
        if solved:
            st["dyntol"] = max(0.5 * st["dyntol"], 10 * EPS)
        return D

    def on_lock():
        st["dyntol"] = 0.5

    out = gd(A, B, which=which, target=target, correct=correct, on_lock=on_lock, **kw)
    return out + (st["solves"], st["its"], st["fallbacks"])


def report(name, runs):
    its = [r[1] for r in runs]
    print("%-40s its %3d..%3d  restarts %d..%d  inner solves %d..%d  inner its %d..%d  fallbacks %d..%d" % (
        name, min(its), max(its), min(r[2] for r in runs), max(r[2] for r in runs), min(r[4] for r in runs), max(r[4] for r in runs),
        min(r[5] for r in runs), max(r[5] for r in runs), min(r[6] for r in runs), max(r[6] for r in runs)))
    return max(its)


def main():
    seeds = range(3)
    n = 324
    A1 = sc.laplacian2d_csr(18, 18); B1 = sp.diags(2.0 / np.log(np.arange(n) + 2.0)).tocsr()
    for bs in (1, 3):
        report("test1 bs %d" % bs, [jd(A1, B1, nev=4, tol=1e-10, conv="norm", bs=bs, pc=jacobi(B1), seed=s, max_it=1500) for s in seeds])
    G = sc.graph_laplacian_2d(10, 11)
    report("test10", [jd(G, nev=4, which="smallest_real", pc=jacobi(G), defl=np.ones((110, 1)), seed=s, max_it=500) for s in seeds])
    T = sc.tridiag_csr(18, -1.0, 2.0, -1.0)
    for ncv in (0, 19):
        report("test20 ncv %s" % (ncv or "default"), [jd(T, nev=1, which="smallest_real", tol=1e-9, ncv=ncv, pc=jacobi(T), seed=s, max_it=1500) for s in seeds])
    for (a, b) in ((10, 11), (20, 22)):
        L = sc.laplacian2d_csr(a, b)
        report("test28 %d x %d" % (a, b), [jd(L, nev=3, which="smallest_real", pc=jacobi(L), seed=s) for s in seeds])
    L8 = sc.laplacian2d_csr(20, 20)
    report("test8 bs 3 ncv 11 (largest magnitude)", [jd(L8, nev=4, bs=3, ncv=11, seed=s, max_it=40000) for s in seeds])
    LAP = sc.laplacian2d_csr(12, 9)
    for bs in (1, 4):
        for ksp in ("bcgs", "gmres"):
            report("ends smallest jacobi bs %d %s" % (bs, ksp), [jd(LAP, nev=4, which="smallest_real", bs=bs, ksp=ksp, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])
            report("ends largest none bs %d %s" % (bs, ksp), [jd(LAP, nev=4, which="largest_real", bs=bs, ksp=ksp, seed=s, max_it=2000) for s in seeds])
    K = (LAP - 1.0 * sp.identity(108)).tocsr()
    for bs in (1, 4):
        for blk in (24, 64):
            report("target 1.0 block Jacobi %d bs %d" % (blk, bs), [jd(LAP, nev=3, which="target_magnitude", target=1.0, bs=bs, pc=bjacobi(K, blk), seed=s, max_it=2000) for s in seeds])
    Bt = sp.diags([np.full(107, 0.25), np.ones(108), np.full(107, 0.25)], [-1, 0, 1], format="csr")
    for bs in (1, 4):
        for ksp in ("bcgs", "gmres"):
            report("ghep tridiagonal B bs %d %s" % (bs, ksp), [jd(LAP, Bt, nev=5, which="smallest_real", bs=bs, ksp=ksp, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])
    for fix in (1e30, 1e-30):
        report("fix %g" % fix, [jd(LAP, nev=4, which="smallest_real", fix=fix, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])
    for fix in (1e30, 1e-30):
        report("largest real, no PC, fix %g" % fix, [jd(LAP, nev=4, which="largest_real", fix=fix, seed=s, max_it=2000) for s in seeds])
    report("dynamic tolerance", [jd(LAP, nev=4, which="smallest_real", const_tol=False, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])


if __name__ == "__main__":
    main()
