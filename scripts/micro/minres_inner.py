#!/usr/bin/env python3
"""Inner solves of the ST on a symmetric INDEFINITE system by MINRES (check intervals 1 and 8), GMRES(30) and BiCGStab: time per solve and per iteration.

Problem: ks_mat_create_laplacian3d at 100^3 and 216^3 rows, shift-and-invert at a sigma between the second and the third level of the spectrum (four
eigenvalues below it: the lowest and the triple one above it), point Jacobi with use_abs, rtol = 1e-8, a seeded random right-hand side. The method is
that of scripts/micro/cg_inner.py: each size in a process of its own under a time limit; every variant warmed up with one whole solve, then timed in
alternating rounds with HIP events on the context's stream around whole solves; the figure of a variant is the median of its rounds, the spread is
printed next to it. A solve that reaches max_it is reported as such: its time per iteration stands, its time per solve is the time to the cap. A
last, untimed MINRES solve runs with the library's profiler on and says where an iteration's time goes.

    python scripts/micro/minres_inner.py [--sizes 100 216] [--rounds 5] [--max-it 4000] [--out FILE]
"""
import argparse
import ctypes as C
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VARIANTS = [("gmres", None), ("bcgs", None), ("minres", 1), ("minres", 8)]


def sigma_for(m):
    """Between the levels (2,1,1) and (2,2,1) of the 7-point Laplacian on the m^3 grid: eigenvalues 4 (s_i + s_j + s_k), s_i = sin^2(i pi / (2 (m + 1)))."""
    s = lambda i: math.sin(i * math.pi / (2 * (m + 1))) ** 2
    return 0.5 * (4 * (s(2) + 2 * s(1)) + 4 * (2 * s(2) + s(1)))


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


def child(m, rounds, max_it):
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
    sigma = sigma_for(m)
    A = ks.Mat.laplacian3d(ctx, m, m, m)
    W = ks.BV(ctx, n, 2)
    W.set_column(0, np.random.default_rng(7).standard_normal(n))
    xp, yp = C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1))
    sts = []
    for ksp, c in VARIANTS:
        st = ks.ST(ctx)
        st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetKSPType(ksp); st.SetPC("jacobi"); st.PCJacobiSetUseAbs(True)
        st.SetKSP(rtol=1e-8, max_it=max_it)
        if c:
            st.MINRESSetCheckInterval(c)
        st.SetUp()
        sts.append(st)

    def solve(st):
        rc = ctx.L.ks_st_apply(st.h, xp, yp)
        if rc not in (0, 91):
            _lib.check(rc)
        return rc

    its, capped, times = [], [], [[] for _ in VARIANTS]
    for st in sts:                                            # warm-up: one whole solve each (code objects, work vectors, the iteration count)
        before = st.GetKSPStats()["iterations"]
        capped.append(solve(st) == 91)
        its.append(st.GetKSPStats()["iterations"] - before)
    ctx.synchronize()
    for _ in range(rounds):                                   # alternating: a drift of the machine hits every variant alike
        for i, st in enumerate(sts):
            times[i].append(ev.time(lambda: solve(st)))
    print("n = %d^3 = %d rows, sinvert sigma %.6g (4 eigenvalues below), jacobi-abs, rtol 1e-8, max_it %d, %d rounds" % (m, n, sigma, max_it, rounds))
    print("%-12s %10s %12s %14s %14s %s" % ("ksp", "iterations", "ms/solve", "spread", "us/iteration", ""))
    med = []
    for i, (ksp, c) in enumerate(VARIANTS):
        t = statistics.median(times[i]); med.append(t)
        name = ksp if not c else "minres c=%d" % c
        print("%-12s %10d %12.3f %6.1f..%-7.1f %14.2f %s" % (name, its[i], t, min(times[i]), max(times[i]), 1e3 * t / max(its[i], 1), "(did NOT converge: reached max_it)" if capped[i] else "(converged)"))
    per = [1e3 * med[i] / max(its[i], 1) for i in range(len(VARIANTS))]
    print("per iteration: minres c=8 / gmres = %.3f, minres c=8 / bcgs = %.3f, minres c=8 / minres c=1 = %.3f" % (per[3] / per[0], per[3] / per[1], per[3] / per[2]))
    print("MINRES converges: %s; GMRES(30) converges: %s; BiCGStab converges: %s; a MINRES iteration costs less than a GMRES(30) iteration: %s"
          % ("NO" if capped[3] else "yes", "NO" if capped[0] else "yes", "NO" if capped[1] else "yes", "yes" if per[3] < per[0] else "NO"))
    # where a MINRES iteration's time goes (profiler on: its events slow the host, so this solve is not among the timed ones)
    st = sts[3]
    ctx.prof_enable(True); ctx.prof_reset()
    wall = ev.time(lambda: solve(st))
    prof = ctx.prof_get()
    ctx.prof_enable(False)
    kern = sum(v["ms"] for v in prof.values())
    for name in sorted(prof):
        p = prof[name]
        if p["launches"]:
            print("  minres c=8 profiled: %-12s %6d launches %9.3f ms %7.2f us each, %.2f TB/s of compulsory bytes" % (name, p["launches"], p["ms"], 1e3 * p["ms"] / p["launches"], p["hbm_bytes"] / (p["ms"] * 1e9) if p["ms"] else 0.0))
    print("  minres c=8 profiled: solve %.3f ms, kernels %.3f ms, between kernels %.3f ms (%d iterations)" % (wall, kern, wall - kern, its[3]))
    for s in sts:
        s.destroy()
    W.destroy(); A.destroy(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 216])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-it", type=int, default=4000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per size")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rounds, a.max_it)
        return 0
    text = []
    for m in a.sizes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(m), "--rounds", str(a.rounds), "--max-it", str(a.max_it)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:                       # a size that failed ends the run: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode
        text.append(r.stdout)
    out = "\n".join(text)
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
