"""The windowed CSR layout against the CSR kernel it replaces, on one box: KSGPU_SPMV=csr and =window built from the same arrays, both resident,
timed in alternating rounds with device events (the library's profile records), us per product and CSR-algorithmic TB/s (SURVEY 8d bytes), the spread
of the csr leg over the rounds, maxdiff between the two products, and what the automatic choice makes of the matrix.

Matrices: the ragged 27-point mesh with 3 unknowns per node (tests/window_cases.mesh27) at --grid^3 for every --keeps value, and csr_probe's banded
random matrix (n = --banded, mean 32), which the automatic choice must leave as csr.

  python scripts/window_probe.py [--grid 100] [--keeps 0.7,0.5] [--banded 1000000] [--rounds 5] [--reps 40] [--legs csr,window]
  python scripts/window_probe.py --pmc-run window --grid 100     # three products of one leg and nothing else: the body of a rocprofv3 --pmc pass"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import slepc_amd as ks
import window_cases as wc

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=100)
ap.add_argument("--keeps", default="0.7,0.5")
ap.add_argument("--banded", type=int, default=1000000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--legs", default="csr,window")
ap.add_argument("--pmc-run", default="")
args = ap.parse_args()
ctx = ks.Context(0)


def build(fmt, a):
    if fmt:
        os.environ["KSGPU_SPMV"] = fmt
    else:
        os.environ.pop("KSGPU_SPMV", None)
    return ks.Mat.from_csr(ctx, *a)


def timed(A, x, y, reps):
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    for _ in range(reps):
        A.mult_dev(x, y)
    ctx.synchronize()
    p = ctx.prof_get(); ctx.prof_enable(False)
    v = p["spmv_csr"]
    return 1e3 * v["ms"] / v["launches"], v["hbm_bytes"] / v["launches"]


def probe(name, a):
    rp, col, val = a
    n, nnz = len(rp) - 1, int(rp[-1])
    csr_bytes = 12.0 * nnz + 4.0 * (n + 1) + 16.0 * n
    if args.pmc_run:
        A = build(args.pmc_run, a)
        V = ks.BV(ctx, n, 2); V.SetRandomColumn(0)
        for _ in range(3):
            A.mult_dev(V.column_ptr(0), V.column_ptr(1))
        ctx.synchronize()
        ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset(); A.mult_dev(V.column_ptr(0), V.column_ptr(1)); ctx.synchronize()
        own = ctx.prof_get()["spmv_csr"]["hbm_bytes"]; ctx.prof_enable(False)
        print("%s n=%d nnz=%d %s layout=%s window_info=%s model bytes per product (layout_own_bytes + 16 n) %.0f, CSR algorithm %.0f"
              % (name, n, nnz, args.pmc_run, A.layout(), A.window_info(), own, csr_bytes), flush=True)
        return
    auto = build(None, a)
    print("%s n=%d nnz=%d (%.1f per row): automatic choice -> %s %s" % (name, n, nnz, nnz / n, auto.layout(), auto.window_info()), flush=True)
    auto.destroy()
    legs = args.legs.split(",")
    mats = {f: build(f, a) for f in legs}
    xs = np.random.default_rng(0).standard_normal(n)
    ys = {f: mats[f].mult(xs) for f in legs}
    V = ks.BV(ctx, n, 2); V.SetRandomColumn(0)
    x, y = V.column_ptr(0), V.column_ptr(1)
    for f in legs:                                                         # warm-up: code objects, clocks, both matrices touched
        for _ in range(10):
            mats[f].mult_dev(x, y)
    ctx.synchronize()
    us = {f: [] for f in legs}; own = {}
    for _ in range(args.rounds):                                           # alternating: csr, window, csr, window, ...
        for f in legs:
            t, b = timed(mats[f], x, y, args.reps)
            us[f].append(t); own[f] = b
    for f in legs:
        u = np.array(us[f]); med = float(np.median(u))
        print("%s %-7s layout=%-6s rounds(us) %s  median %7.1f  min %7.1f  max %7.1f  spread %4.1f %%  %.2f TB/s (CSR bytes)  own bytes %.4g  maxdiff vs %s %.1e"
              % (name, f, mats[f].layout(), " ".join("%.1f" % v for v in u), med, u.min(), u.max(), 100.0 * (u.max() - u.min()) / med, csr_bytes / med / 1e6,
                 own[f], legs[0], np.nanmax(np.abs(ys[f] - ys[legs[0]]))), flush=True)
    if "window" in mats:
        print("%s window_info %s" % (name, mats["window"].window_info()), flush=True)
    V.destroy()
    for A in mats.values():
        A.destroy()


for keep in [float(k) for k in args.keeps.split(",") if k]:
    rp, col, val, n = wc.mesh27(args.grid, 3, keep, 1)
    probe("mesh %d^3 x 3 keep %.1f" % (args.grid, keep), (rp, col, val))
    del rp, col, val
if args.banded and not args.pmc_run:
    probe("banded random n=%d mean 32" % args.banded, wc.banded_random(args.banded, 32))
