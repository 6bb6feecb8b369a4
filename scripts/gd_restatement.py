"""A numpy restatement of the Generalized Davidson loop of slepc_amd/csrc/ks_gd.hip, for the iteration counts quoted in tests/test_gpu_gd.py.

Same set-up rules, same order of steps (products of the new columns, new columns of H, solve and sort, residuals of the first min(bs, m) pairs,
convergence test in order, stopping test, then lock OR restart OR expand), same restart formulas. What differs from the library is the random
initial basis (numpy's generator here), so the counts are quoted as ranges over a few seeds. Runs on the CPU:  python scripts/gd_restatement.py"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import scenarios as sc  # noqa: E402

EPS = np.finfo(float).eps


def key_of(which, target):
    return {"smallest_real": lambda x: x, "largest_real": lambda x: -x, "largest_magnitude": lambda x: -abs(x),
            "target_magnitude": lambda x: abs(x - target)}[which]


def restart_basis(Q, oldU, size_X, size_plusk):
    n = Q.shape[0]
    cols = [Q[:, c] for c in range(size_X)]
    for c in range(size_plusk):
        z = np.zeros(n); z[:oldU.shape[0]] = oldU[:, c]; cols.append(z)
    Z = []
    for z in cols:
        n0 = np.linalg.norm(z); z = z.copy()
        for _ in range(2):
            for zk in Z:
                z -= (zk @ z) * zk
        if np.linalg.norm(z) > 64 * n * EPS * n0:
            Z.append(z / np.linalg.norm(z))
    return np.stack(Z, axis=1)


def gd(A, B=None, nev=1, which="largest_magnitude", target=0.0, tol=1e-8, conv="rel", bs=1, pc=None, minv=0, plusk=1, initv=0, ncv=0, mpd=0,
       defl=None, seed=0, max_it=0, correct=None, on_lock=None):
    """returns (eigenvalues of the locked pairs, iterations, restarts, locks). correct / on_lock: the hooks of the loop that Jacobi-Davidson fills
    (scripts/jd_restatement.py): the expansion vectors of the block in place of pc(R), and a call when pairs are locked."""
    n = A.shape[0]
    if not ncv:
        ncv = mpd + nev + bs if mpd else (n + nev + bs if n < 10 else max(nev, min(n - bs, max(2 * nev, nev + 15)) + bs))
    mpd = mpd or min(n, ncv)
    minv = minv or (1 if n < 10 else min(max(bs, 6), mpd // 2))
    initv = initv or (1 if n < 10 else 6)
    max_it = max_it or max(100 * ncv, 2 * n)
    assert nev + bs <= ncv and minv + bs <= mpd and initv <= mpd and 2 <= mpd <= ncv
    key = key_of(which, target)
    nrma = abs(A).sum(axis=1).max(); nrmb = abs(B).sum(axis=1).max() if B is not None else 1.0
    Bm = (lambda x: B @ x) if B is not None else (lambda x: x)
    rng = np.random.default_rng(seed)
    Y = np.zeros((n, 0))                                  # constraints and locked vectors
    if defl is not None:
        for c in range(defl.shape[1]):
            z = defl[:, c].copy()
            for _ in range(2):
                z -= Y @ (Y.T @ Bm(z))
            Y = np.hstack([Y, (z / np.sqrt(z @ Bm(z)))[:, None]])
    nc = Y.shape[1]

    def orthonormalize(V, z):
        W = np.hstack([Y, V]); n0 = np.sqrt(z @ Bm(z))
        for _ in range(2):
            z = z - W @ (W.T @ Bm(z))
        nz = np.sqrt(max(z @ Bm(z), 0.0))
        return (z / nz) if nz > 1e-8 * n0 else None

    def random_column(V):
        while True:
            z = orthonormalize(V, rng.uniform(-1.0, 1.0, n))
            if z is not None:
                return np.hstack([V, z[:, None]])

    V = np.zeros((n, 0))
    while V.shape[1] < min(initv, mpd, ncv):
        V = random_column(V)
    AV = np.zeros((n, 0)); BV = np.zeros((n, 0)); H = np.zeros((0, 0)); oldU = None
    eig = []; its = restarts = locks = 0
    while True:
        m = V.shape[1]
        if m == 0:
            V = random_column(V); m = 1
        mp = AV.shape[1]
        if mp < m:
            AV = np.hstack([AV, A @ V[:, mp:]]); BV = np.hstack([BV, Bm(V[:, mp:])])
            Hn = np.zeros((m, m)); Hn[:mp, :mp] = H
            C = V.T @ AV[:, mp:]
            Hn[:, mp:] = C; Hn[mp:, :] = C.T
            H = Hn
        w, Q = np.linalg.eigh((H + H.T) / 2)
        order = sorted(range(m), key=lambda i: key(w[i]))
        w, Q = w[order], Q[:, order]
        nb = min(bs, m)
        X = V @ Q[:, :nb]; R = AV @ Q[:, :nb] - (BV @ Q[:, :nb]) * w[:nb]
        npre = 0
        for j in range(nb):
            res = np.linalg.norm(R[:, j]) / np.linalg.norm(X[:, j])
            est = {"rel": res / abs(w[j]) if w[j] != 0 else np.inf, "abs": res, "norm": res / (nrma + abs(w[j]) * nrmb)}[conv]
            if est < tol:
                npre += 1
            else:
                break
        nconv = len(eig)
        npre = max(min(npre, nev - nconv), 0)
        if nconv >= nev:
            return np.array(eig), its, restarts, locks
        if its >= max_it:
            raise RuntimeError("no convergence in %d iterations (%d locked)" % (its, nconv))
        if npre > 0:
            V = V @ Q; AV = AV @ Q; BV = BV @ Q
            Y = np.hstack([Y, V[:, :npre]]); eig.extend(w[:npre])
            V, AV, BV = V[:, npre:], AV[:, npre:], BV[:, npre:]
            H = np.diag(w[npre:]); oldU = None; locks += 1
            if on_lock is not None:
                on_lock()
        elif m + bs > mpd or nconv + m + bs > ncv:
            mrs = max(0, min(mpd - 1, ncv - nconv - 2))
            so = oldU.shape[0] if oldU is not None else 0
            size_X = max(1, min(min(minv, mrs - (1 if (mrs > 1 and plusk > 0 and so > 0) else 0)), m))
            size_plusk = max(0, min(plusk, so, mrs - size_X, m - size_X))
            Z = restart_basis(Q, oldU if oldU is not None else np.zeros((0, 0)), size_X, size_plusk)
            V = V @ Z; AV = AV @ Z; BV = BV @ Z; H = Z.T @ H @ Z; oldU = None; restarts += 1
        else:
            if correct is not None:
                D = correct(X=X, R=R, theta=w[:nb], locked=Y[:, nc:])
            else:
                D = pc(R) if pc is not None else R
            kept = 0
            for j in range(nb):
                z = orthonormalize(V, D[:, j])
                if z is not None:
                    V = np.hstack([V, z[:, None]]); kept += 1
            if not kept:
                V = random_column(V)
            if plusk > 0:
                oldU = Q.copy()
        its += 1


def jacobi(M):
    d = M.diagonal()
    return lambda R: R / d[:, None]


def bjacobi(M, bsz):
    M = M.toarray(); n = M.shape[0]
    inv = [np.linalg.inv(M[b:min(b + bsz, n), b:min(b + bsz, n)]) for b in range(0, n, bsz)]

    def apply(R):
        return np.vstack([inv[i] @ R[b:min(b + bsz, n)] for i, b in enumerate(range(0, n, bsz))])
    return apply


def report(name, runs):
    its = [r[1] for r in runs]
    print("%-34s its %3d..%3d  restarts %d..%d  locks %d..%d" % (name, min(its), max(its), min(r[2] for r in runs), max(r[2] for r in runs), min(r[3] for r in runs), max(r[3] for r in runs)))
    return max(its)


def main():
    seeds = range(3)
    # test1: GHEP on the 18 x 18 grid, B diagonal; largest magnitude with no shift set: M from B alone (point Jacobi)
    n = 324
    A1 = sc.laplacian2d_csr(18, 18); B1 = sp.diags(2.0 / np.log(np.arange(n) + 2.0)).tocsr()
    for bs in (1, 3):
        report("test1 bs %d" % bs, [gd(A1, B1, nev=4, tol=1e-10, conv="norm", bs=bs, pc=jacobi(B1), seed=s, max_it=1500) for s in seeds])
    G = sc.graph_laplacian_2d(10, 11)
    for bs in (1, 2):
        report("test10 bs %d" % bs, [gd(G, nev=4, which="smallest_real", bs=bs, pc=jacobi(G), defl=np.ones((110, 1)), seed=s, max_it=500) for s in seeds])
    LAP = sc.laplacian2d_csr(12, 9)
    for bs in (1, 4, 16):
        report("ends smallest jacobi bs %d" % bs, [gd(LAP, nev=6, which="smallest_real", bs=bs, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])
        report("ends largest none bs %d" % bs, [gd(LAP, nev=6, which="largest_real", bs=bs, seed=s, max_it=2000) for s in seeds])
    K = (LAP - 1.0 * sp.identity(108)).tocsr()
    for bs in (1, 3):
        report("target 1.0 bjacobi 24 bs %d" % bs, [gd(LAP, nev=3, which="target_magnitude", target=1.0, bs=bs, pc=bjacobi(K, 24), seed=s, max_it=2000) for s in seeds])
    Bt = sp.diags([np.full(107, 0.25), np.ones(108), np.full(107, 0.25)], [-1, 0, 1], format="csr")
    for bs in (1, 4):
        report("ghep tridiagonal B bs %d" % bs, [gd(LAP, Bt, nev=5, which="smallest_real", bs=bs, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])
    # largest real of the same pencil with no shift set: the infinite default shift, M = the diagonal blocks of B alone
    report("ghep largest, bjacobi 8 on B bs 2", [gd(LAP, Bt, nev=3, which="largest_real", bs=2, pc=bjacobi(Bt, 8), seed=s, max_it=2000) for s in seeds])
    for minv in (3, 6):
        for plusk in (0, 1, 2):
            report("restart minv %d plusk %d" % (minv, plusk), [gd(LAP, nev=4, which="smallest_real", bs=2, ncv=12, minv=minv, plusk=plusk, pc=jacobi(LAP), seed=s, max_it=2000) for s in seeds])


if __name__ == "__main__":
    main()
