"""Two-sided Krylov-Schur behind a solve and with a B matrix, and two-sided balancing behind a solve: what ks_st_set_transpose_solves on the
EPS's ST opens (ks_krylovschur.hip: the left basis is expanded with Op^T = M^T P^-T, the converged left vectors of a generalized problem go through
P^-T, the left residual is ||A^T y - conj(k) B^T y||).

References: the value columns of the reference's ex41_1.out and eps_test29_1.out, numpy's dense eigenvalues, and residuals computed on the host
from the returned vectors. Bounds: with unit vectors both residuals are at most 2 ||A - sigma B||_2 tol - ||A - sigma B||_2 tol is what the
relative test on the transformed pair (theta = 1 / (k - sigma), ||Op x - theta x|| <= tol |theta|) implies for the original residual, since
A x - k B x = -(k - sigma) P (Op x - theta x) for sinvert; the factor 2 covers the inexact inner solves and the estimate-versus-true gap.
Biorthogonality: (k_j - k_i) y_i^H B x_j = rl_i^H x_j - y_i^H rr_j, so |y_i^H B x_j| <= (||rl_i|| + ||rr_j||) / |k_i - k_j| + 64 eps ||B||_2."""
import numpy as np
import pytest
import scipy.sparse as sp

import golden_inputs as gi
import ilu_cases as ic
import nhep_cases as nc
import twosided_cases as TS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8
EPS = np.finfo(float).eps


def _pairs(eps, Sa, Sb, n):
    """(k, x, y, ||A x - k B x||, ||A^T conj(y) - k B^T conj(y)||) for the first n pairs, complex vectors (y^H A = k y^H B)"""
    out = []
    for i in range(n):
        kr, ki, xr, xi = eps.GetEigenpair(i)
        yr, yi = eps.GetLeftEigenvector(i)
        k = complex(kr, ki); x = xr + 1j * xi; y = yr + 1j * yi
        rr = np.linalg.norm(Sa @ x - k * (Sb @ x)); rl = np.linalg.norm(Sa.T @ y.conj() - k * (Sb.T @ y.conj()))
        out.append((k, x, y, rr, rl))
    return out


def _check_pairs(eps, Sa, Sb, n, cap, what):
    """unit vectors, both residuals under the cap, ComputeError = max(right, left) / |k|, B-biorthogonality within what the residuals allow"""
    P = _pairs(eps, Sa, Sb, n)
    nb = np.linalg.norm(Sb.toarray(), 2)
    for i, (k, x, y, rr, rl) in enumerate(P):
        print("%s pair %d: k = %r, right %.2e, left %.2e, cap %.2e (ratio %.3f)" % (what, i, k, rr, rl, cap, max(rr, rl) / cap))
        assert abs(np.linalg.norm(x) - 1.0) < 1e-12 and abs(np.linalg.norm(y) - 1.0) < 1e-12
        assert rr <= cap and rl <= cap
        err = eps.ComputeError(i)
        assert abs(err - max(rr, rl) / abs(k)) <= 1e-12 + 1e-6 * err, (err, rr, rl)
    for i, (ki_, _, y, _, rli) in enumerate(P):
        for j, (kj, x, _, rrj, _) in enumerate(P):
            if abs(ki_ - kj) > 1e-6 * abs(ki_):
                assert abs(np.vdot(y, Sb @ x)) <= (rli + rrj) / abs(ki_ - kj) + 64 * EPS * nb, (i, j)
    return P


# ---- ex41 -st_type sinvert -eps_target 1.1 ----------------------------------------------------------------------------------------------
def _ex41(ctx, kind, pc, bs, transpose=True):
    import slepc_amd as ks
    Ao = O.markov_matrix(15)
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)
    v0, w0 = TS.ex41_start_vectors(Ao.n)
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4); eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(1.1)
    eps.SetTwoSided(True); eps.SetInitialSpace(v0[:, None]); eps.SetLeftInitialSpace(w0[:, None])
    st = eps.GetST(); st.SetType(kind); st.SetKSP(rtol=1e-12); st.SetPC(pc, bs); st.SetTransposeSolves(transpose)
    return eps, st, A, Ao


@pytest.mark.parametrize("kind", ["sinvert", "cayley"])
@pytest.mark.parametrize("pc,bs", [("jacobi", 0), ("bjacobi-ilu", 64)])
def test_ex41_behind_sinvert_and_cayley(ctx, kind, pc, bs):
    """ex41 as the reference runs it: markov(15), nev 4, target 1.1, ex41's start vectors; ILU blocks of 64 are two blocks of 64 + 56 rows. Cayley
    (antishift = the shift) finds the same four values."""
    eps, st, A, Ao = _ex41(ctx, kind, pc, bs)
    eps.Solve()
    assert eps.GetConverged() >= 4 and eps.GetConvergedReason() == 1 and st.GetShift() == 1.1
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert all(eps.GetEigenvalue(i)[1] == 0.0 for i in range(4))
    assert np.allclose(lam, gi.table_first_column(gi.read("eps/ex41_1.out"))[:4], atol=0.6e-6)      # printed with 6 decimals
    S = Ao.to_scipy().tocsr(); I = sp.identity(Ao.n, format="csr")
    cap = 2.0 * np.linalg.norm((S - 1.1 * I).toarray(), 2) * TOL
    _check_pairs(eps, S, I, 4, cap, "ex41 %s %s" % (kind, pc))
    ksp = st.GetKSPStats()
    print("ex41 %s %s: restarts %d, inner solves %d, iterations %d (%.1f per solve)" % (kind, pc, eps.GetIterationNumber(), ksp["solves"], ksp["iterations"],
                                                                                      ksp["iterations"] / ksp["solves"]))


def test_ex41_behind_sinvert_is_refused_without_the_switch(ctx):
    import slepc_amd as ks
    eps, st, A, Ao = _ex41(ctx, "sinvert", "jacobi", 0, transpose=False)
    with pytest.raises(ks.KsError) as e:
        eps.Solve()
    assert e.value.rc == 56 and "ks_st_set_transpose_solves" in str(e.value)


# ---- test29: EPSSetTwoSided on the generalized bfw62 pencil behind sinvert ------------------------------------------------------------------
def test_test29_two_sided_generalized_golden(ctx):
    import slepc_amd as ks
    A = ks.Mat.load(ctx, gi.matrix_path("bfw62a.petsc")); B = ks.Mat.load(ctx, gi.matrix_path("bfw62b.petsc"))
    Sa = O.load_petsc_binary(gi.matrix_path("bfw62a.petsc")).to_scipy().tocsr(); Sb = O.load_petsc_binary(gi.matrix_path("bfw62b.petsc")).to_scipy().tocsr()
    sigma = -190000.0
    eps = ks.EPS(ctx)
    eps.SetOperators(A, B); eps.SetProblemType(ks.EPS_GNHEP); eps.SetDimensions(4); eps.SetTarget(sigma); eps.SetTwoSided(True)
    st = eps.GetST(); st.SetType("sinvert"); st.SetKSP(rtol=1e-14, restart=62); st.SetTransposeSolves(True)
    eps.Solve()
    assert eps.GetConverged() >= 4
    ref = gi.table_first_column(gi.read("eps/eps_test29_1.out"))
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam, ref, rtol=1e-10)
    cap = 2.0 * np.linalg.norm((Sa - sigma * Sb).toarray(), 2) * TOL
    _check_pairs(eps, Sa, Sb, 4, cap, "test29")
    # the same problem without the switch: the B matrix is refused, as before
    eps2 = ks.EPS(ctx)
    eps2.SetOperators(A, B); eps2.SetProblemType(ks.EPS_GNHEP); eps2.SetDimensions(4); eps2.SetTarget(sigma); eps2.SetTwoSided(True)
    eps2.GetST().SetType("sinvert")
    with pytest.raises(ks.KsError) as e:
        eps2.Solve()
    assert e.value.rc == 56 and "ks_st_set_transpose_solves" in str(e.value)


# ---- shift with two matrices: P = B ------------------------------------------------------------------------------------------------------
def test_shift_with_two_matrices(ctx):
    """The 16 x 20 pencil, GNHEP with the default ST: Op = B^-1 A, Op^T = A^T B^-T, converged left vectors through B^-T. The solver tolerance is
    1e-10 so that the values can be held to numpy's at 1e-8 relative; the residual cap is the same form, 2 ||B||_2 |k| tol (P = B, theta = k)."""
    import scipy.linalg as sl
    import slepc_amd as ks
    Sa, Sb = ic.line_pencil(16, 20)
    A = ks.Mat.from_csr(ctx, *ic.arrays(Sa), keep_csr=True); B = ks.Mat.from_csr(ctx, *ic.arrays(Sb), keep_csr=True)
    tol = 1e-10
    eps = ks.EPS(ctx)
    eps.SetOperators(A, B); eps.SetProblemType(ks.EPS_GNHEP); eps.SetDimensions(4, 32); eps.SetTolerances(tol); eps.SetTwoSided(True)
    st = eps.GetST(); st.SetKSP(rtol=1e-13); st.SetPC("bjacobi-ilu", 64); st.SetTransposeSolves(True)
    eps.Solve()
    assert eps.GetConverged() >= 4
    w = sl.eigvals(Sa.toarray(), Sb.toarray()); w = w[np.argsort(-np.abs(w))][:4]
    lam = np.array([complex(*eps.GetEigenvalue(i)) for i in range(4)])
    assert np.allclose(lam, w, rtol=1e-8, atol=0)
    cap = 2.0 * np.linalg.norm(Sb.toarray(), 2) * np.abs(lam).max() * tol
    _check_pairs(eps, Sa, Sb, 4, cap, "shift, two matrices")


# ---- two-sided balancing in a one-sided solve behind sinvert -----------------------------------------------------------------------------
def test_two_sided_balancing_behind_sinvert(ctx):
    """brusselator(50), target -5 (the spectrum runs from -311 to 0), GMRES with the restart at the dimension. build_balance multiplies with the
    operator's transpose, which is a solve with P^T: refused with 56 without the switch, as before."""
    import slepc_amd as ks
    Ao = nc.brusselator(50); S = Ao.to_scipy().toarray()
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)
    target = -5.0

    def new(switch):
        eps = ks.EPS(ctx)
        eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4); eps.SetTolerances(1e-10)
        eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(target); eps.SetBalance("twoside")
        st = eps.GetST(); st.SetType("sinvert"); st.SetKSP(rtol=1e-13, restart=Ao.n); st.SetTransposeSolves(switch)
        return eps
    eps = new(True)
    eps.Solve()
    assert eps.GetConverged() >= 4
    w = np.linalg.eigvals(S); w = w[np.argsort(np.abs(w - target), kind="stable")][:4]
    lam = np.array([complex(*eps.GetEigenvalue(i)) for i in range(4)])
    assert np.allclose(np.sort_complex(lam), np.sort_complex(w), rtol=1e-8, atol=0)
    errs = [eps.ComputeError(i) for i in range(4)]
    print("two-sided balancing behind sinvert: restarts %d, errors %s" % (eps.GetIterationNumber(), errs))
    assert max(errs) < 1e-7
    with pytest.raises(ks.KsError) as e:
        new(False).Solve()
    assert e.value.rc == 56
