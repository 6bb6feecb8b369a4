"""Fingerprints of four small eigensolves on paths of the EPS driver that bench.py does not take, for comparing two BUILDS bit for bit:
one line per solve with its, nconv, the steps / passes / restarts stats and the sha256 of the eigenvalues, error estimates and eigenvectors.
Run it once per build on the same GPU; the two outputs must be identical as text (profiles/r13_eps_driver_ab.txt).

    python scripts/eps_ab.py [--root TREE]      TREE: the checkout whose slepc_amd (and libksgpu.so) is loaded; default: this one

The solves (n <= 1600, a few seconds in all):
  nhep-harmonic   Arnoldi variant with harmonic extraction, true residuals and trackall on a dense-ish matrix with a planted interior pair
  ghep-sinvert    Lanczos variant under shift-and-invert with B, purification on
  twosided-shift  two-sided Krylov-Schur under STSHIFT (sigma = 0.5) on a 2-D convection-diffusion operator
  lobpcg-hard     LOBPCG, block size 4, restart 0.6 (hard locking with a guard of two), nev = 6"""
import argparse
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:16]


def mat(ks, ctx, S):
    S = sp.csr_matrix(S); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=True)


def lap2d(n, m):
    def T(k):
        return sp.diags([-np.ones(k - 1), 2.0 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    return sp.kron(sp.identity(m), T(n)) + sp.kron(T(m), sp.identity(n))


def planted_pair(n=400):
    rng = np.random.default_rng(4)
    D = np.zeros((n, n))
    D[:2, :2] = [[0.3, 0.8], [-0.8, 0.3]]
    D[np.arange(2, n), np.arange(2, n)] = np.r_[np.linspace(-3.0, -1.5, n // 2 - 1), np.linspace(1.6, 3.0, n - n // 2 - 1)]
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return Q @ D @ Q.T


def convection_diffusion(n, px=0.05, py=0.02):
    Tx = sp.diags([-(1 + px) * np.ones(n - 1), 2.0 * np.ones(n), -(1 - px) * np.ones(n - 1)], [-1, 0, 1])
    Ty = sp.diags([-(1 + py) * np.ones(n - 1), 2.0 * np.ones(n), -(1 - py) * np.ones(n - 1)], [-1, 0, 1])
    return sp.kron(sp.identity(n), Tx) + sp.kron(Ty, sp.identity(n))


def report(name, eps, left=False):
    n = eps.GetConverged()
    st = eps.GetStats()
    pairs = [eps.GetEigenpair(i) for i in range(n)]
    vec = [np.r_[p[2], p[3]] for p in pairs]
    if left:
        vec += [np.r_[eps.GetLeftEigenvector(i)] for i in range(n)]
    print("%-15s its %d nconv %d reason %d steps %d passes %d restarts %d eig %s errest %s vec %s" % (
        name, eps.GetIterationNumber(), n, eps.GetConvergedReason(), st["arnoldi_steps"], st["gs_passes"], st["restarts"],
        sha([p[:2] for p in pairs]), sha([eps.GetErrorEstimate(i) for i in range(n)]), sha(vec) if vec else "-"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import slepc_amd as ks
    assert os.path.abspath(ks.__file__).startswith(os.path.abspath(args.root) + os.sep), ks.__file__
    ctx = ks.Context(0)

    eps = ks.EPS(ctx)
    eps.SetOperators(mat(ks, ctx, planted_pair())); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(2, 30); eps.SetTolerances(1e-9, 300)
    eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(0.25); eps.SetExtraction("harmonic")
    eps.SetTrueResidual(True); eps.SetTrackAll(True)
    eps.Solve(); report("nhep-harmonic", eps)

    A = lap2d(40, 40)
    n = A.shape[0]
    B = sp.diags([np.full(n - 1, 1 / 6), np.full(n, 2 / 3), np.full(n - 1, 1 / 6)], [-1, 0, 1])
    eps = ks.EPS(ctx)
    eps.SetOperators(mat(ks, ctx, A), mat(ks, ctx, B)); eps.SetProblemType(ks.EPS_GHEP); eps.SetDimensions(5, 24); eps.SetPurify(True)
    st = eps.GetST(); st.SetKSP(rtol=1e-14); st.SetType("sinvert"); eps.SetTarget(-0.1)      # below the spectrum: A - sigma B stays definite for the inner solves
    eps.Solve(); report("ghep-sinvert", eps)

    eps = ks.EPS(ctx)
    eps.SetOperators(mat(ks, ctx, convection_diffusion(32))); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4)
    eps.SetWhichEigenpairs("largest_real"); eps.SetTwoSided(True)
    st = eps.GetST(); st.SetType("shift"); st.SetShift(0.5)
    eps.Solve(); report("twosided-shift", eps, left=True)

    eps = ks.EPS(ctx)
    eps.SetOperators(mat(ks, ctx, lap2d(30, 27))); eps.SetProblemType(ks.EPS_HEP); eps.SetType("lobpcg")
    eps.SetDimensions(6); eps.LOBPCGSetBlockSize(4); eps.LOBPCGSetRestart(0.6); eps.SetTolerances(1e-8, 1000)
    eps.Solve()
    ls = eps.LOBPCGGetStats()
    report("lobpcg-hard", eps)
    print("%-15s iterations %d hard_locks %d mat_columns %d pc_columns %d" % ("", ls["iterations"], ls["hard_locks"], ls["mat_columns"], ls["pc_columns"]))
    assert ls["hard_locks"] >= 1, ls
    ctx.close()


if __name__ == "__main__":
    main()
