"""Timings of the fused Ritz-residual sweep of Generalized Davidson against the composition it replaces, and of a whole GD solve, on the MI355X
(DESIGN section 22). One JSON object per measurement on stdout.

  (no --leg)  the driver: every leg below as a fresh child process under its own time limit, one after the other; the first leg that fails, is
              killed or runs out of time ends the run (nothing more is started on the device)
  --leg kernel --n N [--generalized]
              ks_bv_ritz_residual against ks_bv_mult for x, A x (and B x), ks_bv_block_residual and ks_bv_normcolumn of every column of x, in the
              same process, alternating, m in {8, 24, 40}, ncols in {1, 4, 8, 16}; GB/s on the compulsory bytes 8 n (2 m + ncols) (3 m generalized)
  --leg solve the --solve-grid^3 Laplacian (default 100), nev 10, smallest real, point Jacobi, bs 4, at most --steps iterations (default 300): seconds
              per iteration and the device time per iteration of every kernel class, from a second, profiled run of the same solve

Both sides return their norms to the host, so a call is timed on its own: the host clock around one call, which ends in the call's own host wait.
The first call of every shape is a warm-up; minimum and median of five windows of --inner calls (default 10) are reported per call."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = (8, 24, 40)
NCOLS = (1, 4, 8, 16)
WINDOWS = 5


def emit(**kw):
    print(json.dumps(kw), flush=True)


def windows(ctx, fns, inner):
    """min and median seconds per call of every function of fns, their windows alternating"""
    for f in fns:
        f()
    ctx.synchronize()
    ts = [[] for _ in fns]
    for _ in range(WINDOWS):
        for i, f in enumerate(fns):
            ctx.synchronize(); t0 = time.perf_counter()
            for _ in range(inner):
                f()
            ctx.synchronize(); ts[i].append((time.perf_counter() - t0) / inner)
    return [(min(t), float(np.median(t))) for t in ts]


def leg_kernel(n, generalized, inner):
    import slepc_amd as ks
    ctx = ks.Context(0)
    emit(probe="device", **ctx.device_info())
    mmax = max(MS)
    V, AV = ks.BV(ctx, n, mmax), ks.BV(ctx, n, mmax)
    BV = ks.BV(ctx, n, mmax) if generalized else None
    V.SetRandom(1); AV.SetRandom(2)
    if generalized:
        BV.SetRandom(3)
    R, X, AX = ks.BV(ctx, n, 16), ks.BV(ctx, n, 16), ks.BV(ctx, n, 16)
    BX = ks.BV(ctx, n, 16) if generalized else X
    rng = np.random.default_rng(4)
    for m in MS:
        for b in (V, AV) + ((BV,) if generalized else ()):
            b.SetActiveColumns(0, m)
        for ncols in NCOLS:
            S = np.asfortranarray(rng.standard_normal((m, ncols)) / np.sqrt(m)); theta = np.linspace(0.5, 2.0, ncols)
            for b in (R, X, AX) + ((BX,) if generalized else ()):
                b.SetActiveColumns(0, ncols)
            out = {}

            def fused():
                out["fused"] = R.RitzResidual(V, AV, BV, S, theta)

            def composed():
                X.Mult(1.0, 0.0, V, S); AX.Mult(1.0, 0.0, AV, S)
                if generalized:
                    BX.Mult(1.0, 0.0, BV, S)
                rn = R.BlockResidual(AX, BX, theta)
                out["composed"] = (rn, np.array([X.NormColumn(j) for j in range(ncols)]))

            (f0, f1), (c0, c1) = windows(ctx, (fused, composed), inner)
            agree = max(np.abs(out["fused"][0] / out["composed"][0] - 1.0).max(), np.abs(out["fused"][1] / out["composed"][1] - 1.0).max())
            nbytes = 8.0 * n * ((3 if generalized else 2) * m + ncols)
            emit(probe="ritz_residual", n=n, generalized=generalized, m=m, ncols=ncols, fused_ms=f0 * 1e3, fused_median_ms=f1 * 1e3, composed_ms=c0 * 1e3,
                 composed_median_ms=c1 * 1e3, GBps=nbytes / f0 / 1e9, composed_GBps=nbytes / c0 / 1e9, ratio=c0 / f0, norms_rel_diff=agree)


def leg_solve(grid, steps):
    import slepc_amd as ks
    ctx = ks.Context(0)
    A = ks.Mat.laplacian3d(ctx, grid, grid, grid)

    def solve(profile):
        eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetType("gd")
        eps.SetDimensions(10); eps.GDSetBlockSize(4); eps.SetWhichEigenpairs("smallest_real"); eps.SetTolerances(1e-8, steps); eps.GetST().SetPC("jacobi")
        if profile:
            ctx.prof_reset(); ctx.prof_enable(True)
        ctx.synchronize(); t0 = time.perf_counter(); eps.Solve(); ctx.synchronize(); dt = time.perf_counter() - t0
        prof = ctx.prof_get() if profile else {}
        if profile:
            ctx.prof_enable(False)
        return eps, dt, prof

    solve(False)                                                         # warm-up: code objects, layouts
    eps, dt, _ = solve(False)
    its = max(eps.GetIterationNumber(), 1)
    _, dtp, prof = solve(True)
    emit(probe="gd_solve", grid=grid, n=grid ** 3, seconds=dt, its=its, ms_per_iteration=dt / its * 1e3, nconv=eps.GetConverged(), reason=eps.GetConvergedReason(),
         profiled_seconds=dtp, device_ms_per_iteration={k: v["ms"] / its for k, v in sorted(prof.items())},
         launches_per_iteration={k: v["launches"] / its for k, v in sorted(prof.items())}, **eps.GDGetStats())


def driver(a):
    legs = [(["--leg", "kernel", "--n", str(n)] + (["--generalized"] if g else []), 420) for n in (10 ** 6, 10 ** 7) for g in (False, True)]
    legs.append((["--leg", "solve", "--solve-grid", str(a.solve_grid), "--steps", str(a.steps)], 300))
    for args, limit in legs:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--inner", str(a.inner)] + args
        rc = subprocess.run(cmd).returncode
        if rc:
            emit(probe="stopped", leg=args, rc=rc)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["kernel", "solve"]); ap.add_argument("--n", type=int, default=10 ** 6); ap.add_argument("--generalized", action="store_true")
    ap.add_argument("--inner", type=int, default=10); ap.add_argument("--solve-grid", type=int, default=100); ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    if a.leg == "kernel":
        leg_kernel(a.n, a.generalized, a.inner)
    elif a.leg == "solve":
        leg_solve(a.solve_grid, a.steps)
    else:
        sys.exit(driver(a))


if __name__ == "__main__":
    main()
