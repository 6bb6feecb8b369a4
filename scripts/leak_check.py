"""Device-memory leak check: free memory (hipMemGetInfo through torch) before and after many create/solve/destroy cycles
covering the solver variants, ST types, constraints, wide bases and block orthogonalisation."""
import gc, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import slepc_amd as ks
import scenarios as sc
import nhep_cases as nc
from oracle import oracle as O

ctx = ks.Context(0)


def cycle(i):
    S = sc.graph_laplacian_2d(20, 17)
    A = ks.Mat.from_csr(ctx, S.indptr, S.indices, S.data)
    eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(3, 16 if i % 2 else 80)
    eps.SetWhichEigenpairs("smallest_real"); eps.SetDeflationSpace(np.ones((S.shape[0], 1))); eps.Solve()
    Ao = nc.planted_pairs(600)
    An = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    e2 = ks.EPS(ctx); e2.SetOperators(An); e2.SetProblemType(ks.EPS_NHEP); e2.SetDimensions(3, 20); e2.SetTarget(-2.0)
    st = e2.GetST(); st.SetType(["sinvert", "cayley"][i % 2]); st.SetKSP(rtol=1e-12)
    if i % 2:
        st.CayleySetAntishift(5.0)
    e2.Solve()
    Lo = O.laplacian2d(24, 17)
    L = ks.Mat.from_csr(ctx, Lo.rowptr, Lo.col, Lo.val)
    d = 1.0 + 0.5 * np.cos(np.arange(Lo.n)) ** 2
    B = ks.Mat.from_csr(ctx, np.arange(Lo.n + 1, dtype=np.int32), np.arange(Lo.n, dtype=np.int32), d)
    e3 = ks.EPS(ctx); e3.SetOperators(L, B); e3.SetProblemType(ks.EPS_GHEP); e3.SetDimensions(3, 16); e3.GetST().SetKSP(rtol=1e-13); e3.Solve()
    # the LU factors of P = L - sigma B with their transposed plan: set up, applied, set up again by a new shift and a new ordering
    Lk = ks.Mat.from_csr(ctx, Lo.rowptr, Lo.col, Lo.val, keep_csr=True)
    Bk = ks.Mat.from_csr(ctx, np.arange(Lo.n + 1, dtype=np.int32), np.arange(Lo.n, dtype=np.int32), d, keep_csr=True)
    slu = ks.ST(ctx); slu.SetType("sinvert"); slu.SetShift(1.3); slu.SetMatrices(Lk, Bk); slu.SetPC("lu"); slu.SetKSPType("preonly"); slu.SetTransposeSolves(True)
    slu.Apply(np.ones(Lo.n)); slu.SetShift(2.1 + 0.01 * i); slu.ApplyTranspose(np.ones(Lo.n)); slu.PCLUSetOrdering("natural"); slu.PCApply(np.ones(Lo.n))
    # the multigrid hierarchy of the same P: set up, applied to one and to nine vectors, set up again by a new shift and by new options
    samg = ks.ST(ctx); samg.SetType("sinvert"); samg.SetShift(-0.3); samg.SetMatrices(Lk, Bk); samg.SetPC("amg"); samg.PCAMGSetCoarse(8, 10)
    samg.Apply(np.ones(Lo.n)); samg.SetShift(-0.2 - 0.01 * i); samg.PCApplyMulti(np.ones((Lo.n, 9))); samg.PCAMGSetSmoother(3); samg.PCAMGSetProlongatorSmoothing(False); samg.PCApply(np.ones(Lo.n))
    del samg
    # MINRES on the same indefinite P with Jacobi-abs: state, pinned copy and work vectors set up, a solve, set up again by a new shift
    smr = ks.ST(ctx); smr.SetType("sinvert"); smr.SetShift(1.3); smr.SetMatrices(Lk, Bk); smr.SetKSPType("minres"); smr.SetPC("jacobi"); smr.PCJacobiSetUseAbs(True)
    smr.Apply(np.ones(Lo.n)); smr.SetShift(2.1 + 0.01 * i); smr.Apply(np.ones(Lo.n))
    assert smr.GetMINRESStats()["sweeps"] > 0
    del smr
    del slu, Lk, Bk
    V = ks.BV(ctx, 3000, 90); V.set_dense(np.random.default_rng(i).standard_normal((3000, 90)))
    V.SetOrthogBlock(["chol", "svqb", "gs", "tsqr"][i % 4])
    if i % 4 == 3:
        V.SetActiveColumns(0, 40)
    V.Orthogonalize(None)
    for o in (eps, e2, e3):
        assert o.GetConverged() >= 1
    # the binned and the XCD-sliced SpMV layouts (forced on a small random matrix), and the communicator's one-shot mailboxes
    os.environ["KSGPU_SPMV"] = ["binned", "sliced"][i % 2]
    rng = np.random.default_rng(i)
    nb = 6000; rp = np.arange(0, 8 * nb + 1, 8, dtype=np.int32)
    M = ks.Mat.from_csr(ctx, rp, rng.integers(0, nb, 8 * nb).astype(np.int32), rng.uniform(-1, 1, 8 * nb))
    del os.environ["KSGPU_SPMV"]
    assert M.layout() == ["binned", "sliced"][i % 2]
    M.mult(np.ones(nb))
    M.destroy()
    del eps, e2, e3, V, A, An, L, B, st


cycle(0); cycle(1); cycle(2); cycle(3)
gc.collect(); ctx.synchronize()
free0, total = torch.cuda.mem_get_info(0)
N = 40
for i in range(N):
    cycle(i)
gc.collect(); ctx.synchronize()
free1, _ = torch.cuda.mem_get_info(0)
print("free before %.1f MiB, after %d cycles %.1f MiB, difference %.2f MiB" % (free0 / 2**20, N, free1 / 2**20, (free0 - free1) / 2**20))
assert free0 - free1 < 8 * 2**20, "device memory leak"
print("no leak")
