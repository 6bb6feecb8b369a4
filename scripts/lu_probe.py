"""Probe of the sparse LU preconditioner (KS_PC_LU; not a test): the 2-D Laplacian 255 x 255 and the 3-D Laplacian 32^3, shift-and-invert at a
shift inside the spectrum. Per matrix: set-up time on the host (ordering, factorisation, layout, upload), entries, levels and launches of the
schedule, the time of a forward application (mean of 200 back-to-back PCApply between two host waits, after a warm-up, host clock around the
waits) for several values of the wide-level threshold (KSGPU_LU_WIDE, read at set-up), the time of one ks_st_apply with LU + PREONLY, and of the
same ks_st_apply with GMRES(30) + bjacobi-ilu (8192 rows) to rtol 1e-12 - the path LU is measured against.
Usage: lu_probe.py [output file] ; LU_PROBE_SMALL=1 runs reduced sizes."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import slepc_amd as ks

small = bool(os.environ.get("LU_PROBE_SMALL"))
ctx = ks.Context(0)
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else sys.stdout
WIDES = (1, 8, 16, 64, 256)          # 1: every level a launch of its own


def log(*a):
    print(*a, file=out); out.flush()


def tridiag(m):
    return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])


def laplacian2d(m):
    A = (sp.kron(sp.identity(m), tridiag(m)) + sp.kron(tridiag(m), sp.identity(m))).tocsr(); A.sort_indices()
    return A


def laplacian3d(m):
    T = tridiag(m); I = sp.identity(m)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr(); A.sort_indices()
    return A


def timed_applies(st, W, count):
    for _ in range(5):
        st.PCApplyDev(W.column_ptr(0), W.column_ptr(1))
    ctx.synchronize(); t = time.time()
    for _ in range(count):
        st.PCApplyDev(W.column_ptr(0), W.column_ptr(1))
    ctx.synchronize()
    return (time.time() - t) / count


def run(name, S, sigma):
    A = ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=True)
    n = S.shape[0]
    P = (S - sigma * sp.identity(n)).tocsr()
    log("%s: n=%d nnz=%d sigma=%g" % (name, n, S.nnz, sigma))
    x = np.random.default_rng(1).standard_normal(n)
    W = ks.BV(ctx, n, 2); W.set_column(0, x)
    for wide in WIDES:
        os.environ["KSGPU_LU_WIDE"] = str(wide)
        st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetPC("lu"); st.SetKSPType("preonly")
        t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
        info = st.PCLUGetInfo()
        assert info["wide"] == wide
        tpc = [timed_applies(st, W, 200) for _ in range(3)]
        y = st.PCApply(x)
        res = np.linalg.norm(P @ y - x) / np.linalg.norm(x)
        for _ in range(3):
            st.Apply(x)
        ctx.synchronize(); t = time.time()
        for _ in range(20):
            ks._lib.check(ctx.L.ks_st_apply(st.h, W.column_ptr(0), W.column_ptr(1)))
        ctx.synchronize(); tap = (time.time() - t) / 20
        log("  lu, wide %4d: set-up %6.2f s  entries L %d U %d  levels %d + %d  launches per application: %d wide + %d narrow  device %.1f MB\n"
            "                PCApply %8.1f us (three windows of 200: %s)  ks_st_apply (preonly) %8.1f us  ||P y - x|| / ||x|| = %.1e  negative pivots %d"
            % (wide, tset, info["nnz_l"], info["nnz_u"], info["levels_l"], info["levels_u"], info["wide_launches"], info["narrow_launches"], info["device_bytes"] / 1e6,
               1e6 * min(tpc), " ".join("%.1f" % (1e6 * v) for v in tpc), 1e6 * tap, res, st.PCLUGetInertia()[0]))
        del st
    del os.environ["KSGPU_LU_WIDE"]
    # the iterative inner solve this replaces: GMRES(30) behind ILU(0) blocks of 8192 rows, to 1e-12
    st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetPC("bjacobi-ilu", 8192); st.SetKSP(rtol=1e-12, max_it=3000)
    try:
        t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
        t = time.time(); y = st.Apply(x); tap = time.time() - t
        s = st.GetKSPStats()
        log("  gmres(30) + bjacobi-ilu(8192), rtol 1e-12: set-up %6.2f s  ks_st_apply %10.1f us  (%d iterations)  ||P y - x|| / ||x|| = %.1e"
            % (tset, 1e6 * tap, s["iterations"], np.linalg.norm(P @ y - x) / np.linalg.norm(x)))
    except ks.KsError as e:
        log("  gmres(30) + bjacobi-ilu(8192), rtol 1e-12: no answer after %.2f s: %s" % (time.time() - t, str(e)[:160]))
    del st, W, A


log("device %s" % ctx.device_info()["arch"])
m2, m3 = (63, 12) if small else (255, 32)
run("2-D Laplacian %d x %d" % (m2, m2), laplacian2d(m2), 1.03)
run("3-D Laplacian %d^3" % m3, laplacian3d(m3), 1.5)
