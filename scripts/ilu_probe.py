"""Probe of the ILU(0) block-Jacobi preconditioner (not a test): point Jacobi against bjacobi-ilu at a few block sizes on config 5's pencil and on a
3-D Laplacian, shift-and-invert. Per case and preconditioner: levels per block (what an application waits for), inner iterations per solve, time per
application of the preconditioner (mean of 200 back-to-back PCApply launches between two host waits) and of its transpose (PCApplyTranspose, a
second ST with transposed solves on), Arnoldi steps/s of a step-capped eigensolve.
Usage: ilu_probe.py [output file] ; ILU_PROBE_SMALL=1 runs reduced sizes, ILU_PROBE_PC_ONLY=1 leaves the solves out (set-up and the two
applications only: a run whose length does not depend on how the inner solves converge)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import slepc_amd as ks
from slepc_amd.workloads import config5_pencil_arrays

small = bool(os.environ.get("ILU_PROBE_SMALL"))
pc_only = bool(os.environ.get("ILU_PROBE_PC_ONLY"))
ctx = ks.Context(0)
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else sys.stdout


def log(*a):
    print(*a, file=out); out.flush()


def laplacian3d(m):
    T = sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1]); I = sp.identity(m)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr(); A.sort_indices()
    return (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)), None


def levels_per_block(arr, barr, sigma, bs):
    """L + U levels of the first few blocks, from the pattern alone (what the set-up computes on the host)."""
    rp, col, _ = arr
    n = len(rp) - 1
    tot = []
    for b0 in range(0, min(n, 4 * bs), bs):
        bl = min(bs, n - b0)
        rows = []
        for r in range(b0, b0 + bl):
            c = col[rp[r]:rp[r + 1]].astype(np.int64)
            if barr is not None and sigma != 0.0:
                c = np.concatenate([c, barr[1][barr[0][r]:barr[0][r + 1]].astype(np.int64)])
            c = np.unique(c[(c >= b0) & (c < b0 + bl)]) - b0
            rows.append(c)
        lv = np.zeros(bl, dtype=np.int64)
        for i in range(bl):
            k = rows[i][rows[i] < i]
            lv[i] = lv[k].max() + 1 if k.size else 0
        nl = lv.max() + 1
        for i in range(bl - 1, -1, -1):
            k = rows[i][rows[i] > i]
            lv[i] = lv[k].max() + 1 if k.size else 0
        tot.append(int(nl + lv.max() + 1))
    return tot


def run(name, arr, barr, sigma, nev, ncv, cap, problem, pcs):
    A = ks.Mat.from_csr(ctx, *arr, keep_csr=True)
    B = ks.Mat.from_csr(ctx, *barr, keep_csr=True) if barr is not None else None
    n = A.n
    log("%s: n=%d nnz=%d sigma=%g" % (name, n, A.nnz, sigma))
    x = np.random.default_rng(1).standard_normal(n)
    for pc, bs in pcs:
        label = pc if not bs else "%s(%d)" % (pc, bs)
        try:
            st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A, B); st.SetPC(pc, bs)
            t = time.time(); st.SetUp(); ctx.synchronize(); tset = time.time() - t
            W = ks.BV(ctx, n, 2); W.set_column(0, x)
            for _ in range(3):
                st.PCApplyDev(W.column_ptr(0), W.column_ptr(1))
            ctx.synchronize(); t = time.time()
            for _ in range(200):
                st.PCApplyDev(W.column_ptr(0), W.column_ptr(1))
            ctx.synchronize(); tpc = (time.time() - t) / 200
            # the transposed side: same factors, a second level plan (ks_st_set_transpose_solves)
            stt = ks.ST(ctx); stt.SetType("sinvert"); stt.SetShift(sigma); stt.SetMatrices(A, B); stt.SetPC(pc, bs); stt.SetTransposeSolves(True)
            t = time.time(); stt.SetUp(); ctx.synchronize(); tsett = time.time() - t
            for _ in range(3):
                stt.PCApplyTransposeDev(W.column_ptr(0), W.column_ptr(1))
            ctx.synchronize(); t = time.time()
            for _ in range(200):
                stt.PCApplyTransposeDev(W.column_ptr(0), W.column_ptr(1))
            ctx.synchronize(); tpct = (time.time() - t) / 200
            del stt
            lev = ("  levels/block %s" % levels_per_block(arr, barr, sigma, bs)) if bs else ""
            if pc_only:
                log("  %-18s set-up %6.2f s (%6.2f s with the transposed side)  PCApply %8.1f us  PCApplyTranspose %8.1f us%s" % (label, tset, tsett, 1e6 * tpc, 1e6 * tpct, lev))
                del st, W
                continue
            for _ in range(2):
                st.Apply(x)
            s = st.GetKSPStats()
            eps = ks.EPS(ctx); eps.SetOperators(A, B); eps.SetProblemType(problem); eps.SetDimensions(nev, ncv); eps.SetTarget(sigma)
            s2 = eps.GetST(); s2.SetType("sinvert"); s2.SetPC(pc, bs)
            eps.SetMaxSteps(cap)
            t = time.time(); eps.Solve(); dt = time.time() - t
            es = eps.GetStats(); k2 = s2.GetKSPStats()
            log("  %-18s set-up %6.2f s  PCApply %8.1f us  PCApplyTranspose %8.1f us  inner its/solve %7.1f (Apply) %7.1f (eigensolve)  %7.1f steps/s over %d steps%s"
                % (label, tset, 1e6 * tpc, 1e6 * tpct, s["iterations"] / max(1, s["solves"]), k2["iterations"] / max(1, k2["solves"]), es["arnoldi_steps"] / dt, es["arnoldi_steps"], lev))
            del eps, st, W
        except ks.KsError as e:
            log("  %-18s failed: %s" % (label, e))


pcs = [("jacobi", 0), ("bjacobi-ilu", 64), ("bjacobi-ilu", 512), ("bjacobi-ilu", 2048), ("bjacobi-ilu", 8192)]
n5 = 100000 if small else 1000000
a5, b5 = config5_pencil_arrays(n5)
run("config 5 pencil, target 0 (the benchmark's)", a5, b5, 0.0, 20, 60, 120, ks.EPS_GNHEP, pcs)
run("config 5 pencil, target 36 (inside the spectrum)", a5, b5, 36.0, 20, 60, 120, ks.EPS_GNHEP, pcs)
m = 24 if small else 48
aL, _ = laplacian3d(m)
run("3-D Laplacian %d^3, target 0" % m, aL, None, 0.0, 4, 24, 48, ks.EPS_NHEP, pcs)
