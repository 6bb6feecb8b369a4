"""Timings of the two block kernels of LOBPCG and of a whole solve on the MI355X. One JSON object per measurement on stdout.

  --ilu       ks_st_pc_apply_multi with 1, 2, 4, 8, 16 columns against that many ks_st_pc_apply calls (the single-vector kernel), ILU(0) blocks of
              512, 2048 and 8192 rows of the 7-point Laplacian on a --grid^3 grid (default 160: 4.1e6 rows, factors of 290 MB - past the Infinity Cache)
  --residual  k_block_residual against BVCopy + bs axpys + bs norms through the existing entry points, n = 1e6 and 1e7, bs = 8 and 16; GB/s against the
              compulsory 24 n bs bytes
  --solve     the --solve-grid^3 Laplacian (default 216), nev 10, bs 10, smallest real, tol 1e-8, with point Jacobi (and --solve-ilu: ILU blocks of 2048);
              --ks: the same ten eigenvalues through Krylov-Schur with shift-and-invert at sigma = 0 and the same preconditioner

A timed window is --inner calls (default 50) enqueued back to back between two host waits, so the host's cost per call is not charged to either
side unless the device is faster than the host can enqueue; the first window of every shape is a warm-up; the minimum of --reps windows is reported
beside the median, per call. Entries that wait for the host themselves (the block residual returns its norms) are timed per call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slepc_amd as ks  # noqa: E402


INNER = 50


def timed(ctx, fn, reps, inner=None):
    inner = inner or INNER
    fn(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        ctx.synchronize(); t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize(); ts.append((time.perf_counter() - t0) / inner)
    return min(ts), float(np.median(ts))


def lap3d_csr(g):
    import scipy.sparse as sp
    T = sp.diags([-np.ones(g - 1), 2.0 * np.ones(g), -np.ones(g - 1)], [-1, 0, 1])
    I = sp.identity(g)
    S = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    S.sort_indices()
    return S


def emit(**kw):
    print(json.dumps(kw), flush=True)


def probe_ilu(ctx, g, reps):
    S = lap3d_csr(g); n = S.shape[0]
    A = ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data, keep_csr=True)
    W = ks.BV(ctx, n, 32)
    W.SetActiveColumns(0, 16); W.SetRandom(1)
    for bs in (512, 2048, 8192):
        st = ks.ST(ctx); st.SetType("precond"); st.SetShift(-0.5); st.SetMatrices(A); st.SetPC("bjacobi-ilu", bs)
        t0 = time.perf_counter(); st.SetUp(); setup = time.perf_counter() - t0
        for nc in (1, 2, 4, 8, 16):
            multi = timed(ctx, lambda: st.PCApplyMultiDev(W.column_ptr(0), W.ld, W.column_ptr(16), W.ld, nc), reps)
            loop = timed(ctx, lambda: [st.PCApplyDev(W.column_ptr(j), W.column_ptr(16 + j)) for j in range(nc)], reps)
            emit(probe="ilu_apply", n=n, block=bs, columns=nc, multi_ms=multi[0] * 1e3, multi_median_ms=multi[1] * 1e3, loop_ms=loop[0] * 1e3,
                 loop_median_ms=loop[1] * 1e3, ratio=loop[0] / multi[0], setup_s=setup)
        st.destroy()


def probe_residual(ctx, reps):
    for n in (10 ** 6, 10 ** 7):
        for bs in (8, 16):
            R, AX, X = (ks.BV(ctx, n, bs) for _ in range(3))
            AX.SetRandom(2); X.SetRandom(3)
            theta = np.linspace(0.5, 2.0, bs)
            fused = timed(ctx, lambda: R.BlockResidual(AX, X, theta), reps, inner=1)

            def separate():
                AX.Copy(R)
                for j in range(bs):
                    R.SetActiveColumns(j, j + 1); X.SetActiveColumns(j, j + 1)
                    R.Mult(-theta[j], 1.0, X)
                R.SetActiveColumns(0, bs); X.SetActiveColumns(0, bs)
                return [R.NormColumn(j) for j in range(bs)]
            sep = timed(ctx, separate, reps, inner=1)
            emit(probe="block_residual", n=n, bs=bs, kernel_ms=fused[0] * 1e3, kernel_median_ms=fused[1] * 1e3, separate_ms=sep[0] * 1e3,
                 GBps=24.0 * n * bs / fused[0] / 1e9, ratio=sep[0] / fused[0])
            del R, AX, X


def probe_solve(ctx, g, ilu, with_ks):
    if ilu:
        S = lap3d_csr(g)
        A = ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data, keep_csr=True)
    else:
        A = ks.Mat.laplacian3d(ctx, g, g, g)
    for pc, bs in ([("jacobi", 0)] + ([("bjacobi-ilu", 2048)] if ilu else [])):
        eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetType("lobpcg")
        eps.SetDimensions(10); eps.LOBPCGSetBlockSize(10); eps.SetTolerances(1e-8, 5000); eps.GetST().SetPC(pc, bs)
        ctx.synchronize(); t0 = time.perf_counter(); eps.Solve(); ctx.synchronize(); dt = time.perf_counter() - t0
        emit(probe="lobpcg_solve", grid=g, pc=pc, block=bs, seconds=dt, its=eps.GetIterationNumber(), nconv=eps.GetConverged(), reason=eps.GetConvergedReason(),
             eig=[eps.GetEigenvalue(i)[0] for i in range(min(10, eps.GetConverged()))], **eps.LOBPCGGetStats())
        if with_ks:
            e2 = ks.EPS(ctx); e2.SetOperators(A); e2.SetProblemType(ks.EPS_HEP); e2.SetDimensions(10); e2.SetTolerances(1e-8, 0)
            e2.SetTarget(0.0); e2.SetWhichEigenpairs("target_magnitude")
            st = e2.GetST(); st.SetType("sinvert"); st.SetPC(pc, bs)
            ctx.synchronize(); t0 = time.perf_counter()
            try:
                e2.Solve(); ctx.synchronize()
                emit(probe="krylovschur_sinvert", grid=g, pc=pc, block=bs, seconds=time.perf_counter() - t0, its=e2.GetIterationNumber(), nconv=e2.GetConverged(),
                     ksp=st.GetKSPStats())
            except ks.KsError as e:
                emit(probe="krylovschur_sinvert", grid=g, pc=pc, block=bs, seconds=time.perf_counter() - t0, error=str(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ilu", action="store_true"); ap.add_argument("--residual", action="store_true"); ap.add_argument("--solve", action="store_true")
    ap.add_argument("--solve-ilu", action="store_true"); ap.add_argument("--ks", action="store_true")
    ap.add_argument("--grid", type=int, default=160); ap.add_argument("--solve-grid", type=int, default=216); ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    global INNER
    INNER = a.inner
    ctx = ks.Context(0)
    emit(probe="device", **ctx.device_info())
    if a.residual:
        probe_residual(ctx, a.reps)
    if a.ilu:
        probe_ilu(ctx, a.grid, a.reps)
    if a.solve:
        probe_solve(ctx, a.solve_grid, a.solve_ilu, a.ks)


if __name__ == "__main__":
    main()
