#!/usr/bin/env python3
"""Inner solves of the ST on a NON-SYMMETRIC system by BiCGStab(l) (l = 1, 2, 4; check intervals 1 and the default 4), GMRES(30) and the host-loop
BiCGStab: time per solve and per BiCG step.

Problem: the 7-point convection-diffusion stencil on an m^3 grid (central differences, convection along all three axes: diagonal 6, off-diagonals
-1 - c towards lower indices and -1 + c; assembled through ks_mat_create_csr), m = 100 and 216, shift-and-invert at sigma = 0 and at sigma = 2 (the
system of tests/bcgsl_cases.py in three dimensions), point Jacobi, rtol = 1e-8, a seeded random right-hand side. The method is that of
scripts/micro/cg_inner.py: each size in a process of its own under a time limit; every variant warmed up with one whole solve, then timed in
alternating rounds with HIP events on the context's stream around whole solves; the figure of a variant is the median of its rounds, the spread is
printed next to it. A solve that ends without converging (max_it, breakdown) is reported as such: its time per step stands, its time per solve is
the time to its end. GMRES and BiCGStab count one product per iteration and two per iteration; a BiCGStab(l) step has two products, like a
BiCGStab iteration. A last, untimed BiCGStab(2) solve runs with the library's profiler on and says where a step's time goes.

    python scripts/micro/bcgsl_inner.py [--sizes 100 216] [--sigmas 0 2] [--c 3] [--rounds 5] [--max-it 2000] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VARIANTS = [("gmres", 0, None), ("bcgs", 0, None), ("bcgsl", 1, 1), ("bcgsl", 1, 4), ("bcgsl", 2, 1), ("bcgsl", 2, 4), ("bcgsl", 4, 1), ("bcgsl", 4, 4)]


class Events:
    """hipEvent timing on one stream, through the HIP runtime the library itself is bound to."""

    def __init__(self, hip, stream):
        self.hip, self.stream = hip, stream
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.e0)) == 0 and hip.hipEventCreate(C.byref(self.e1)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value


def stencil(m, c):
    import numpy as np
    import scipy.sparse as sp
    t = sp.diags([(-1.0 - c) * np.ones(m - 1), 2.0 * np.ones(m), (-1.0 + c) * np.ones(m - 1)], [-1, 0, 1], format="csr")
    i = sp.identity(m, format="csr")
    A = (sp.kron(sp.kron(i, i), t) + sp.kron(sp.kron(i, t), i) + sp.kron(sp.kron(t, i), i)).tocsr()
    A.sort_indices()
    return A


def child(m, sigma, c, rounds, max_it):
    import numpy as np
    import slepc_amd as ks
    from slepc_amd import _lib
    _lib.lib()
    hip = C.CDLL(_lib.runtime_info()["hip_runtime_path"])
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx = ks.Context(0, stream=stream.value)
    ev = Events(hip, stream)
    n = m ** 3
    S = stencil(m, c)
    A = ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))
    del S
    W = ks.BV(ctx, n, 2)
    W.set_column(0, np.random.default_rng(7).standard_normal(n))
    xp, yp = C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1))
    sts = []
    for ksp, ell, chk in VARIANTS:
        st = ks.ST(ctx)
        st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetKSPType(ksp); st.SetPC("jacobi")
        st.SetKSP(rtol=1e-8, max_it=max_it)
        if ksp == "bcgsl":
            st.BCGSLSetEll(ell); st.BCGSLSetCheckInterval(chk)
        st.SetUp()
        sts.append(st)

    def solve(st):
        rc = ctx.L.ks_st_apply(st.h, xp, yp)
        if rc not in (0, 91):
            _lib.check(rc)
        return rc

    its, failed, rnorm, times = [], [], [], [[] for _ in VARIANTS]
    for st in sts:                                            # warm-up: one whole solve each (code objects, work vectors, the iteration count)
        before = st.GetKSPStats()["iterations"]
        failed.append(_lib.lib().ks_last_error_message().decode()[:90] if solve(st) == 91 else "")
        its.append(st.GetKSPStats()["iterations"] - before)
        rnorm.append(st.GetKSPStats()["last_rnorm"])
    ctx.synchronize()
    for _ in range(rounds):                                   # alternating: a drift of the machine hits every variant alike
        for i, st in enumerate(sts):
            times[i].append(ev.time(lambda: solve(st)))
    print("n = %d^3 = %d rows, convection-diffusion c = %g, sinvert sigma %g, jacobi, rtol 1e-8, max_it %d, %d rounds" % (m, n, c, sigma, max_it, rounds))
    print("%-14s %10s %12s %16s %10s %12s %s" % ("ksp", "iterations", "ms/solve", "spread", "us/it", "last_rnorm", ""))
    per = {}
    for i, (ksp, ell, chk) in enumerate(VARIANTS):
        t = statistics.median(times[i])
        name = ksp if ksp != "bcgsl" else "bcgsl(%d) c=%d" % (ell, chk)
        per[name] = 1e3 * t / max(its[i], 1)
        print("%-14s %10d %12.3f %7.1f..%-8.1f %10.2f %12.3e %s" % (name, its[i], t, min(times[i]), max(times[i]), per[name], rnorm[i], "did NOT converge: " + failed[i] if failed[i] else "(converged)"))
    print("per step: bcgsl(1) c=4 / bcgs iteration = %.3f, bcgsl(2) c=4 / bcgs = %.3f, bcgsl(2) c=4 / bcgsl(2) c=1 = %.3f, bcgsl(4) c=4 / bcgsl(4) c=1 = %.3f"
          % (per["bcgsl(1) c=4"] / per["bcgs"], per["bcgsl(2) c=4"] / per["bcgs"], per["bcgsl(2) c=4"] / per["bcgsl(2) c=1"], per["bcgsl(4) c=4"] / per["bcgsl(4) c=1"]))
    # where a BiCGStab(2) step's time goes (profiler on: its events slow the host, so this solve is not among the timed ones)
    st = sts[5]
    ctx.prof_enable(True); ctx.prof_reset()
    wall = ev.time(lambda: solve(st))
    prof = ctx.prof_get()
    ctx.prof_enable(False)
    kern = sum(v["ms"] for v in prof.values())
    for name in sorted(prof):
        p = prof[name]
        if p["launches"]:
            print("  bcgsl(2) c=4 profiled: %-12s %6d launches %9.3f ms %7.2f us each, %.2f TB/s of compulsory bytes" % (name, p["launches"], p["ms"], 1e3 * p["ms"] / p["launches"], p["hbm_bytes"] / (p["ms"] * 1e9) if p["ms"] else 0.0))
    print("  bcgsl(2) c=4 profiled: solve %.3f ms, kernels %.3f ms, between kernels %.3f ms = %.0f %% (%d steps)" % (wall, kern, wall - kern, 100.0 * (wall - kern) / wall if wall else 0.0, its[5]))
    for s in sts:
        s.destroy()
    W.destroy(); A.destroy(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 216])
    ap.add_argument("--sigmas", type=float, nargs="+", default=[0.0, 2.0])
    ap.add_argument("--c", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-it", type=int, default=2000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per size and shift")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--child-sigma", type=float, default=0.0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.child_sigma, a.c, a.rounds, a.max_it)
        return 0
    text = []
    for m in a.sizes:
        for sigma in a.sigmas:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(m), "--child-sigma", str(sigma), "--c", str(a.c), "--rounds", str(a.rounds),
                                "--max-it", str(a.max_it)], capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:                       # a run that failed ends the script: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode
            text.append(r.stdout)
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
