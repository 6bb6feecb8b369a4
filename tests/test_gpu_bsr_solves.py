"""Solvers on block CSR input: everything above the product is the existing code, so a solve on Mat.from_bsr must be, bit for bit, the solve on
Mat.from_csr of the expansion forced to the CSR kernels (KSGPU_SPMV=csr) - eigenvalues, iteration counts, ST.Apply, the transposed product, MatAXPY.

The matrices are bsr_cases.mesh_blocks: symmetric (6, 3, 0.8), n = 648, and general (5, 4, 0.8), n = 500; and their twins (9, 3, 0.8), n = 2187, and
(8, 4, 0.8), n = 2048. The library has two forms of the CSR product and, mirroring them, two of the block CSR product: below 2048 rows lanes share a
row and combine by a butterfly (k_spmv_csr / k_spmv_bsr_vec, the block product is the column loop), from 2048 rows on a lane sums its row in entry
order (k_spmv_csr_wave / k_spmv_bsr, k_spmm_bsr). The small meshes compare the first pair, the twins the second; each pair has the same summation
order, so every comparison is np.array_equal or ==.

Sinvert with KS_PC_LU + PREONLY, with the ILU(0) blocks + GMRES in copy mode (P assembled from the kept arrays) and in the default shell mode
(P x = A x - sigma x: every iteration multiplies by A itself), mult_transpose and axpy_new."""
import functools

import numpy as np
import pytest

import bsr_cases as bc

pytestmark = pytest.mark.gpu

SYM, GEN = (6, 3, 0.8, True), (5, 4, 0.8, False)
SYM_LARGE, GEN_LARGE = (9, 3, 0.8, True), (8, 4, 0.8, False)


@functools.lru_cache(maxsize=None)
def case(m, bs, keep, symmetric):
    a = bc.mesh_blocks(m, bs, keep, symmetric=symmetric)
    e = bc.expand(*a)
    for v in a + e:
        v.setflags(write=False)
    return a, e


def pair(ctx, monkeypatch, spec, keep_csr=False):
    """(the block CSR matrix, the CSR matrix of the same arrays forced to csr)"""
    import slepc_amd as ks
    a, e = case(*spec)
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    Ab = ks.Mat.from_bsr(ctx, *a, keep_csr=keep_csr)
    monkeypatch.setenv("KSGPU_SPMV", "csr")
    Ac = ks.Mat.from_csr(ctx, *e, keep_csr=keep_csr)
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    assert Ab.layout() == "bsr" and Ac.layout() == "csr" and (Ab.n, Ab.nnz) == (Ac.n, Ac.nnz)
    return Ab, Ac


def solve(ctx, A, solver, ptype):
    import slepc_amd as ks
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ptype); eps.SetType(solver)
    if solver == "lobpcg":
        eps.SetDimensions(4); eps.LOBPCGSetBlockSize(4); eps.SetTolerances(1e-6, 400)
    else:
        eps.SetDimensions(4, 24); eps.SetTolerances(1e-8, 300)
    eps.Solve()
    k = eps.GetConverged()
    assert k >= 1
    out = ([eps.GetEigenvalue(i) for i in range(min(k, 4))], eps.GetIterationNumber(), k, A.n)
    eps.destroy()
    return out


def eigen_case(ctx, monkeypatch, spec, solver, hep):
    import slepc_amd as ks
    Ab, Ac = pair(ctx, monkeypatch, spec)
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    try:
        rb = solve(ctx, Ab, solver, ks.EPS_HEP if hep else ks.EPS_NHEP)
        ctx.synchronize()
        prof = ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)
    rc = solve(ctx, Ac, solver, ks.EPS_HEP if hep else ks.EPS_NHEP)
    variants = {k[1] for k in prof}
    assert variants <= {25, 26} and (26 in variants) == (solver == "lobpcg" and rb[3] >= 2048), variants      # the solve ran on the block CSR kernels; LOBPCG on the block product (small matrices: the column loop)
    print(spec, solver, "bsr", rb, "csr", rc)
    Ab.destroy(); Ac.destroy()
    return rb, rc


@pytest.mark.parametrize("spec,solver,hep", [(SYM, "krylovschur", True), (GEN, "krylovschur", False), (SYM, "lobpcg", True),
                                             (SYM_LARGE, "krylovschur", True), (GEN_LARGE, "krylovschur", False), (SYM_LARGE, "lobpcg", True)],
                         ids=["ks-hep-648", "ks-nhep-500", "lobpcg-648", "ks-hep-2187", "ks-nhep-2048", "lobpcg-2187"])
def test_eigensolvers_have_the_bits_of_the_csr_solve(ctx, monkeypatch, spec, solver, hep):
    rb, rc = eigen_case(ctx, monkeypatch, spec, solver, hep)
    assert rb == rc


def gmres_apply(ctx, A, x, mode):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(0.5); st.SetMatrices(A); st.SetMatMode(mode); st.SetPC("bjacobi-ilu", 64); st.SetKSPType("gmres"); st.SetKSP(rtol=1e-12)
    y = st.Apply(x)
    st.destroy()
    return y


def residual_ok(spec, y, x):
    import scipy.sparse as sp
    a, e = case(*spec)
    S = sp.csr_matrix((e[2], e[1], e[0]), shape=(len(x), len(x)))
    return np.linalg.norm((S @ y - 0.5 * y) - x) <= 1e-9 * np.linalg.norm(x)


@pytest.mark.parametrize("spec", [SYM, GEN, SYM_LARGE, GEN_LARGE], ids=["sym-648", "gen-500", "sym-2187", "gen-2048"])
def test_sinvert_gmres_on_the_operator_itself_has_the_csr_bits(ctx, monkeypatch, spec):
    """Shell mode: every GMRES iteration multiplies by A itself, block CSR on one side and the CSR kernel of the same size class on the other."""
    Ab, Ac = pair(ctx, monkeypatch, spec, keep_csr=True)
    x = np.random.default_rng(9).standard_normal(Ab.n)
    yb, yc = gmres_apply(ctx, Ab, x, "shell"), gmres_apply(ctx, Ac, x, "shell")
    assert np.array_equal(yb, yc), np.abs(yb - yc).max()
    assert residual_ok(spec, yb, x)
    Ab.destroy(); Ac.destroy()


@pytest.mark.parametrize("spec", [SYM, GEN], ids=["sym-648", "gen-500"])
def test_sinvert_applies_transpose_and_axpy_have_the_csr_bits(ctx, monkeypatch, spec):
    import slepc_amd as ks
    Ab, Ac = pair(ctx, monkeypatch, spec, keep_csr=True)
    n = Ab.n
    x = np.random.default_rng(9).standard_normal(n)
    ys = []
    for A in (Ab, Ac):
        st = ks.ST(ctx)
        st.SetType("sinvert"); st.SetShift(0.5); st.SetMatrices(A); st.SetPC("lu"); st.SetKSPType("preonly")
        ys.append(st.Apply(x))
        st.destroy()
    assert np.array_equal(ys[0], ys[1]) and residual_ok(spec, ys[0], x)
    yb, yc = gmres_apply(ctx, Ab, x, "copy"), gmres_apply(ctx, Ac, x, "copy")
    assert np.array_equal(yb, yc) and residual_ok(spec, yb, x)
    assert np.array_equal(Ab.mult_transpose(x), Ac.mult_transpose(x))
    Pb, Pc = Ab.axpy_new(-0.25), Ac.axpy_new(-0.25)
    Qb, Qc = Ab.axpy_new(2.0, Ab), Ac.axpy_new(2.0, Ac)
    assert Pb.layout() == Pc.layout() != "bsr" and Qb.layout() == Qc.layout() != "bsr"            # results go through the ordinary chooser
    assert np.array_equal(Pb.mult(x), Pc.mult(x)) and np.array_equal(Qb.mult(x), Qc.mult(x))
    assert np.array_equal(Pb.get_diagonal(), Pc.get_diagonal())
    for M in (Pb, Pc, Qb, Qc, Ab, Ac):
        M.destroy()
