"""Probe of the smoothed-aggregation multigrid preconditioner (KS_PC_AMG; not a test): the 3-D Laplacian at 32^3, 64^3 and 128^3 and the 2-D Laplacian
at 1024^2, shift-and-invert at sigma = 0. Per matrix: set-up time (host planning, assembly of the level operators, upload), levels, operator
complexity, device bytes and launches per application; the time of one application (mean of 200 back-to-back PCApply between two host waits, after a
warm-up, host clock around the waits, three windows); one inner solve with GMRES(30) to rtol 1e-8 on a random right-hand side - iterations and time -
with AMG, with point Jacobi and with the ILU(0) blocks of 8192 rows; at 32^3 also the application of KS_PC_LU; and one LOBPCG solve, nev 10, smallest,
with each of the three preconditioners - time and outer iterations.
Usage: amg_probe.py [output file [case ...]] ; cases: 3d32 3d64 3d128 2d1024 (default: all); AMG_PROBE_SMALL=1 runs reduced sizes."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import slepc_amd as ks

small = bool(os.environ.get("AMG_PROBE_SMALL"))
ctx = ks.Context(0)
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else sys.stdout
PCS = (("amg", 0), ("jacobi", 0), ("bjacobi-ilu", 8192))


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


def new_st(A, pc, bs, ksp=None):
    st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A); st.SetPC(pc, bs); st.SetKSP(rtol=1e-8, max_it=3000)
    if ksp:
        st.SetKSPType(ksp)
    return st


def run(name, S, with_lu=False, eigensolve=True):
    A = ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=True)
    n = S.shape[0]
    log("%s: n=%d nnz=%d" % (name, n, S.nnz))
    x = np.random.default_rng(1).standard_normal(n)
    W = ks.BV(ctx, n, 2); W.set_column(0, x)
    st = new_st(A, "amg", 0)
    t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
    info = st.PCAMGGetInfo()
    tpc = [timed_applies(st, W, 200) for _ in range(3)]
    log("  amg: set-up %6.2f s  levels %d  rows %s  operator complexity %.3f  device %.1f MB  launches per application %d\n"
        "       PCApply %8.1f us (three windows of 200: %s)  = %.2f us per launch"
        % (tset, info["levels"], info["rows"], info["complexity"], info["device_bytes"] / 1e6, info["launches"], 1e6 * min(tpc),
           " ".join("%.1f" % (1e6 * v) for v in tpc), 1e6 * min(tpc) / info["launches"]))
    del st
    if with_lu:
        st = new_st(A, "lu", 0, "preonly")
        t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
        tlu = [timed_applies(st, W, 50) for _ in range(3)]
        log("  lu: set-up %6.2f s  PCApply %8.1f us (three windows of 50: %s)" % (tset, 1e6 * min(tlu), " ".join("%.1f" % (1e6 * v) for v in tlu)))
        del st
    for pc, bs in PCS:
        st = new_st(A, pc, bs)
        try:
            t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
            st.Apply(x)                                            # warm-up: the same solve once
            ctx.synchronize(); t = time.time(); y = st.Apply(x); ctx.synchronize(); tap = time.time() - t
            s = st.GetKSPStats()
            log("  gmres(30) + %-11s rtol 1e-8: set-up %6.2f s  one solve %10.1f us  %4d iterations  ||A y - x|| / ||x|| = %.1e"
                % (pc, tset, 1e6 * tap, s["iterations"] // s["solves"], np.linalg.norm(S @ y - x) / np.linalg.norm(x)))
        except ks.KsError as e:
            log("  gmres(30) + %-11s rtol 1e-8: no answer after %.2f s: %s" % (pc, time.time() - t, str(e)[:140]))
        del st
    if eigensolve:
        for pc, bs in PCS:
            eps = ks.EPS(ctx)
            eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetType("lobpcg"); eps.SetDimensions(10); eps.SetTolerances(1e-8, 400)
            eps.SetWhichEigenpairs("smallest_real"); eps.LOBPCGSetBlockSize(10)
            es = eps.GetST(); es.SetShift(0.0); es.SetPC(pc, bs)
            try:
                ctx.synchronize(); t = time.time(); eps.Solve(); ctx.synchronize(); tsolve = time.time() - t
                log("  lobpcg nev 10 + %-11s: %8.3f s (set-up included)  %4d outer iterations  %2d converged  smallest %.8e"
                    % (pc, tsolve, eps.GetIterationNumber(), eps.GetConverged(), eps.GetEigenvalue(0)[0] if eps.GetConverged() else float("nan")))
            except ks.KsError as e:
                log("  lobpcg nev 10 + %-11s: no answer after %.2f s: %s" % (pc, time.time() - t, str(e)[:140]))
            del eps
    del W, A


log("device %s" % ctx.device_info()["arch"])
cases = sys.argv[2:] or ["3d32", "3d64", "3d128", "2d1024"]
sizes = {"3d32": 12, "3d64": 16, "3d128": 20, "2d1024": 96} if small else {"3d32": 32, "3d64": 64, "3d128": 128, "2d1024": 1024}
for c in cases:
    m = sizes[c]
    if c.startswith("3d"):
        run("3-D Laplacian %d^3" % m, laplacian3d(m), with_lu=(c == "3d32"))
    else:
        run("2-D Laplacian %d x %d" % (m, m), laplacian2d(m))
