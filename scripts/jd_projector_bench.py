"""One projected operator application of the Jacobi-Davidson correction equation on the bench's 216^3 Laplacian, two ways, for
profiles/jd_projected_operator.txt:

  fused     ks_bv_oblique_project: the dot sweep that forms w = s .* (a u + b v), the one-workgroup reduce with M^-1, the update sweep with the
            partial sums of e^T w, the sum of those: no host wait before the dot arrives
  composed  what the parent commit offers for the same result: ksk_lincomb, ks_bv_dotvec (host wait), M^-1 h on the host, ks_bv_multvec, and a dot
            (a second host wait)

u = A t is one SpMV in both and is timed on its own. Device events on the context's stream around each form, warmed, the two alternating in one run;
medians. The bytes are computed from the shapes (8 n per vector pass). Usage:  python scripts/jd_projector_bench.py [side] [reps] [outfile]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import slepc_amd as ks  # noqa: E402
from slepc_amd import _lib  # noqa: E402


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    L = _lib.lib()
    hip = C.CDLL(_lib.runtime_info()["hip_runtime_path"])
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx = ks.Context(0, stream=stream.value)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    lincomb = L._Z11ksk_lincombP8ks_ctx_sxPKddS2_dS2_Pd                   # ksk_lincomb(ctx, n, s, a, u, b, v, out), the ST's own combination kernel
    lincomb.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lincomb.restype = C.c_int

    def timed(fn):
        hip.hipEventRecord(ev[0], stream); fn(); hip.hipEventRecord(ev[1], stream)
        hip.hipEventSynchronize(ev[1])
        ms = C.c_float(); hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
        return ms.value * 1e3

    A = ks.Mat.laplacian3d(ctx, side, side, side)
    n = side ** 3
    rng = np.random.default_rng(1)
    vec = ks.BV(ctx, n, 7)                    # t, u = A t, dinv, w (fused), w (composed), e, spare
    vec.set_column(0, rng.standard_normal(n)); vec.set_column(2, np.full(n, 1.0 / 6.0)); vec.set_column(5, rng.standard_normal(n))
    t, u, dinv, wf, wc, e = (vec.column_ptr(j) for j in range(6))
    E = ks.BV(ctx, n, 1); E.set_column(0, vec.column(5))
    theta = 0.37
    say("# one projected operator application w = P (dinv .* (A t - theta t)), P = I - Y Minv Z^T, and r^T w; 3-D 7-point Laplacian %d^3, n = %d" % (side, n))
    say("# device %s, %d repetitions alternating, medians (min..max) in microseconds" % (ctx.device_info()["arch"], reps))
    spmv = sorted(timed(lambda: A.mult_dev(t, u)) for _ in range(reps + 3))[: reps]
    say("SpMV u = A t (common to both forms): %.0f us" % statistics.median(spmv))
    for k in (1, 5, 11):
        Z, Y = ks.BV(ctx, n, k), ks.BV(ctx, n, k)
        for j in range(k):
            z = rng.standard_normal(n) / np.sqrt(n)
            Z.set_column(j, z); Y.set_column(j, z / 6.0 + 0.01 * rng.standard_normal(n) / np.sqrt(n))
        M = np.zeros((k, k), order="F"); Z.Dot(Y, M)           # M = Y^T Z as BVDot lays it out; transposed below: M(i,j) = z_i^T y_j
        Minv = np.asfortranarray(np.linalg.inv(M.T))
        hold = ks.BV(ctx, k * k, 1); hold.set_column(0, Minv.ravel(order="F"))
        mp = C.c_void_p(hold.column_ptr(0))
        dots = {}

        def fused():
            d = C.c_double()
            _lib.check(L.ks_bv_oblique_project(Y.h, Z.h, mp, k, 1.0, C.c_void_p(u), -theta, C.c_void_p(t), C.c_void_p(dinv), C.c_void_p(wf), C.c_void_p(e), C.byref(d)))
            dots["fused"] = d.value

        def composed():
            _lib.check(lincomb(ctx.h, n, C.c_void_p(dinv), 1.0, C.c_void_p(u), -theta, C.c_void_p(t), C.c_void_p(wc)))
            h = Z.DotVec(wc)
            Y.MultVec(-1.0, 1.0, wc, Minv @ h)
            dots["composed"] = E.DotVec(wc)[0]

        A.mult_dev(t, u)
        for _ in range(3):
            fused(); composed()
        tf, tc = [], []
        for _ in range(reps):
            tf.append(timed(fused)); tc.append(timed(composed))
        rel = abs(dots["fused"] - dots["composed"]) / max(abs(dots["composed"]), 1e-300)
        bf = 8.0 * n * ((k + 4) + (k + 3)); bc = 8.0 * n * (4 + (k + 1) + (k + 2) + 2)
        mf, mc = statistics.median(tf), statistics.median(tc)
        say("k = %2d  fused    %7.0f us (%.0f..%.0f)  %6.2f GB moved  %5.2f TB/s   host waits 1" % (k, mf, min(tf), max(tf), bf / 1e9, bf / mf / 1e6))
        say("        composed %7.0f us (%.0f..%.0f)  %6.2f GB moved  %5.2f TB/s   host waits 2   fused / composed = %.3f   r^T w agree to %.1e" % (
            mc, min(tc), max(tc), bc / 1e9, bc / mc / 1e6, mf / mc, rel))
        for b in (Z, Y, hold):
            b.destroy()
    say("# bytes: fused = dot sweep (k columns of Z, u, t, dinv read, w written) + update sweep (k columns of Y, w, r read, w written) = (2k + 7) 8n;")
    say("#        composed = lincomb 4 + dotvec (k + 1) + multvec (k + 2) + dot 2 = (2k + 9) 8n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
