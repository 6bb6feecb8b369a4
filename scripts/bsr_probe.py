"""The block CSR layout against the CSR kernel it replaces and the windowed CSR layout, on one box: Mat.from_bsr (layout bsr), and from_bsr under
KSGPU_SPMV=csr and =window (the same arrays, expanded by the library), all resident, timed in alternating rounds with device events (the library's
profile records): us per product, the spread of the csr leg over its rounds, the model bytes of each leg (layout_own_bytes + 16 n), and the maxdiff of
every leg's y against the csr leg's, which must be 0. With --multi K the same for ks_mat_mult_multi on K columns (bsr against the CSR block kernel).

Matrices: bsr_cases.mesh_blocks(m, bs, keep), general variant; for bs = 3 m = --m3, for the other block sizes the m whose stored scalars
(27-point pattern: about 27 keep bs^2 m^3) come closest to that mesh's.

  python scripts/bsr_probe.py [--sizes 3,2,4,5,6,7,8] [--m3 100] [--keep 0.8] [--rounds 5] [--reps 40] [--legs csr,bsr,window] [--multi 8]
  python scripts/bsr_probe.py --pmc-run bsr --sizes 3 --m3 100     # three products of one leg and nothing else: the body of a rocprofv3 --pmc pass"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import slepc_amd as ks
import bsr_cases as bc

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="3,2,4,5,6,7,8")
ap.add_argument("--m3", type=int, default=100)
ap.add_argument("--keep", type=float, default=0.8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--legs", default="csr,bsr,window")
ap.add_argument("--multi", type=int, default=8)
ap.add_argument("--pmc-run", default="")
args = ap.parse_args()
ctx = ks.Context(0)


def build(fmt, a):
    if fmt == "bsr":
        os.environ.pop("KSGPU_SPMV", None)
    else:
        os.environ["KSGPU_SPMV"] = fmt
    A = ks.Mat.from_bsr(ctx, *a)
    os.environ.pop("KSGPU_SPMV", None)
    return A


def timed(fn, reps):
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    p = ctx.prof_get(); ctx.prof_enable(False)
    v = p["spmv_csr"]
    return 1e3 * v["ms"] / reps, v["hbm_bytes"] / reps      # us and model bytes per call (a call may be several launches)


def report(name, what, legs, mats, us, own, ys):
    ref = legs[0]
    for f in legs:
        u = np.array(us[f]); med = float(np.median(u))
        print("%s %-6s %-7s layout=%-6s rounds(us) %s  median %8.1f  min %8.1f  max %8.1f  spread %4.1f %%  model bytes %.4g (%.2f TB/s)  maxdiff vs %s %.1e"
              % (name, what, f, mats[f].layout(), " ".join("%.1f" % v for v in u), med, u.min(), u.max(), 100.0 * (u.max() - u.min()) / med, own[f], own[f] / med / 1e6,
                 ref, np.nanmax(np.abs(ys[f] - ys[ref]))), flush=True)
    if "bsr" in us and ref in us and ref != "bsr":
        c, b = np.array(us[ref]), float(np.median(us["bsr"]))
        print("%s %-6s verdict: bsr median %.1f us against %s median %.1f us with spread %.1f us: bsr %s" %
              (name, what, b, ref, float(np.median(c)), c.max() - c.min(), "WINS" if b < float(np.median(c)) - (c.max() - c.min()) else "does NOT beat csr by more than its spread"), flush=True)


def probe(bs, m):
    a = bc.mesh_blocks(m, bs, args.keep, symmetric=False)
    nb, nnzb = len(a[0]) - 1, int(a[0][-1])
    n, nnz = nb * bs, nnzb * bs * bs
    name = "mesh %d^3 x %d keep %.1f" % (m, bs, args.keep)
    print("%s n=%d nnz=%d (%.1f per row) blocks=%d: bsr stream %.4g bytes = %.2f per nonzero, csr stream %.4g = %.2f per nonzero"
          % (name, n, nnz, nnz / n, nnzb, bc.layout_bytes(a[0], a[2]), bc.layout_bytes(a[0], a[2]) / nnz, 12.0 * nnz + 4.0 * (n + 1), (12.0 * nnz + 4.0 * (n + 1)) / nnz), flush=True)
    V = ks.BV(ctx, n, 2 * max(1, args.multi)); V.SetRandom()
    x, y = V.column_ptr(0), V.column_ptr(max(1, args.multi))
    if args.pmc_run:
        A = build(args.pmc_run, a)
        for _ in range(3):
            A.mult_dev(x, y)
        ctx.synchronize()
        ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset(); A.mult_dev(x, y); ctx.synchronize()
        own = ctx.prof_get()["spmv_csr"]["hbm_bytes"]; ctx.prof_enable(False)
        print("%s %s layout=%s bsr_info=%s model bytes per product (layout_own_bytes + 16 n) %.0f" % (name, args.pmc_run, A.layout(), A.bsr_info(), own), flush=True)
        return
    legs = args.legs.split(",")
    mats = {f: build(f, a) for f in legs}
    print("%s bsr_info %s" % (name, mats["bsr"].bsr_info() if "bsr" in mats else None), flush=True)
    xs = np.random.default_rng(0).standard_normal(n)
    ys = {f: mats[f].mult(xs) for f in legs}
    for f in legs:                                                             # warm-up: code objects, clocks, every matrix touched
        for _ in range(10):
            mats[f].mult_dev(x, y)
    ctx.synchronize()
    us = {f: [] for f in legs}; own = {}
    for _ in range(args.rounds):                                               # alternating: csr, bsr, window, csr, ...
        for f in legs:
            t, b = timed(lambda: mats[f].mult_dev(x, y), args.reps)
            us[f].append(t); own[f] = b
    report(name, "mult", legs, mats, us, own, ys)
    if args.multi > 1:
        K = args.multi
        mlegs = [f for f in legs if f != "window"]                             # the windowed layout has no block kernel (column loop)
        Xs = np.random.default_rng(1).standard_normal((n, K))
        Ys = {f: mats[f].mult_multi(Xs) for f in mlegs}
        for f in mlegs:
            for j in range(K):
                assert np.array_equal(Ys[f][:, j], mats[f].mult(Xs[:, j])), (f, j)
        us = {f: [] for f in mlegs}; own = {}
        for f in mlegs:
            for _ in range(5):
                mats[f].mult_multi_dev(x, V.ld, y, V.ld, K)
        ctx.synchronize()
        for _ in range(args.rounds):
            for f in mlegs:
                t, b = timed(lambda: mats[f].mult_multi_dev(x, V.ld, y, V.ld, K), max(1, args.reps // 4))
                us[f].append(t); own[f] = b
        report(name, "multi%d" % K, mlegs, mats, us, own, Ys)
    V.destroy()
    for A in mats.values():
        A.destroy()


target = 27.0 * 9 * args.m3 ** 3
for bs in [int(s) for s in args.sizes.split(",") if s]:
    m = args.m3 if bs == 3 else max(4, int(round((target / (27.0 * bs * bs)) ** (1.0 / 3.0))))
    probe(bs, m)
