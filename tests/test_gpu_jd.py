"""Jacobi-Davidson solves (ks_eps_set_type(KS_EPS_JD), slepc_amd/csrc/ks_jd.hip) against the reference's golden outputs and against dense numpy /
LAPACK solves done here.

Bounds, as in tests/test_gpu_gd.py. For a unit eigenvector estimate x with residual r = A x - theta x of a symmetric A some eigenvalue lies within
||r||_2 of theta; with the wanted eigenvalues separated by far more than the tolerance that is the i-th one: |theta_i - lambda_i| <= err_i + 64 eps
||A||_2, err_i the absolute residual ks_eps_compute_error returns. For A x = lambda B x the same holds in the B^-1 norm: |theta - lambda| <= ||r||_2 /
sqrt(lambda_min(B)) for a B-normalised x.

Outer iteration counts of the loop as built, from its numpy restatement scripts/jd_restatement.py (three seeds each; inner solver BiCGStab, rtol 1e-4,
at most 90 iterations unless named; the restatement applies the exact inverse of a 64-row block where the library's "bjacobi-ilu" has ILU(0)):
  test1 (max_it 1500)                  bs 1: 26-28    bs 3: 20-23
  test10 (500)                         20-22
  test20 (1500)                        6-7, both solves
  test28 (default: 100 ncv)            10 x 11: 16    20 x 22: 16-19
  test8, bs 3, ncv 11 (40000)          39-55, with 42-67 pairs corrected the GD way
  ends of the spectrum (400)           smallest real, Jacobi   bs 1: 21-22 (GMRES 23-24)   bs 4: 12-14
                                       largest real, no PC     bs 1: 24-28                 bs 4: 15-19
  target 1.0 (400)                     blocks of 24: bs 1 16-19, bs 4 9-11;  blocks of 64: bs 1 16-18, bs 4 9-13
  tridiagonal B (400)                  bs 1: 25-28    bs 4: 12-15
  smallest real: fix 1e30 / 1e-30 (400)      34-37 / 37-38;   dynamic tolerance (400)  31-33
  largest real, no PC: fix 1e30 / 1e-30 (1000)   31-43 / 112-116 (the second is the GD correction throughout)
On the MI355X (the library's own random start) the same cases took: test1 27 / 22, test10 22, test20 6 (its second solve), test28 16 and 18, test8 46 (43 pairs the
GD way); smallest real 21 (GMRES 21) / 11 (14), largest real 24 / 19; target 15 / 12 with blocks of 24 and 16 / 10 with ILU(0) blocks of 64; tridiagonal B
26 (27) / 12 (12); smallest real with the two values of fix 15 and 36, largest real 29 and 115; the dynamic tolerance 31. Every cap is at least five times
the largest count of its case; no reference program's own max_it is within a factor of two of its count, so none is left out. Every solve asserts
EPS_CONVERGED_TOL."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import golden_inputs as gi
import scenarios as sc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
EPSM = np.finfo(float).eps
SUP, OUTOFRANGE = 56, 63
CAP = 400


def _mat(ctx, S, keep=True, **kw):
    import slepc_amd as ks
    S = S.tocsr(); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep, **kw)


def _jd(ctx, A, B=None, nev=1, bs=0, tol=1e-8, max_it=CAP, which=None, ptype=None, ncv=0, mpd=0, ksp=None):
    import slepc_amd as ks
    eps = ks.EPS(ctx)
    eps.SetOperators(A, B)
    eps.SetProblemType(ptype or (ks.EPS_GHEP if B is not None else ks.EPS_HEP))
    eps.SetType("jd")
    eps.SetDimensions(nev, ncv, mpd)
    if bs:
        eps.JDSetBlockSize(bs)
    eps.SetTolerances(tol, max_it)
    if which:
        eps.SetWhichEigenpairs(which)
    if ksp:
        eps.GetST().SetKSPType(ksp)
    return eps


def _values(eps, k):
    return np.array([eps.GetEigenvalue(i)[0] for i in range(k)])


LAP = sc.laplacian2d_csr(12, 9)                       # n = 108, simple eigenvalues
LAP_EIG = np.linalg.eigvalsh(LAP.toarray())
LAP_NORM = LAP_EIG[-1]
BT = sp.diags([np.full(107, 0.25), np.ones(108), np.full(107, 0.25)], [-1, 0, 1], format="csr")


def _inner(eps):
    st = eps.JDGetStats()
    assert st["inner_solves"] > 0 and st["inner_iterations"] > 0 and st["iterations"] > 0 and st["mat_columns"] > 0 and st["locks"] > 0, st
    return st


def _check_against(eps, k, exact, normA, tol, Bd=None):
    """the bound of the module docstring for the first k pairs, the relative residuals against the tolerance, B-orthonormal locked vectors, inner solves"""
    import slepc_amd as ks
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= k and eps.GetType() == "jd"
    lam = _values(eps, k)
    err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(k)])
    bmin = np.linalg.eigvalsh(Bd)[0] if Bd is not None else 1.0
    print("its %d, |theta - lambda| %s, residuals %s, stats %s" % (eps.GetIterationNumber(), np.abs(lam - exact[:k]), err, eps.JDGetStats()))
    assert np.all(np.abs(lam - exact[:k]) <= err / np.sqrt(bmin) + 64 * EPSM * normA / bmin), (lam, exact[:k], err)
    assert np.all(err <= tol * np.abs(lam) / np.sqrt(bmin)), (err, lam)          # ||r|| / ||x||_2 < tol |theta| at the lock, ||x||_2 <= 1 / sqrt(lambda_min(B))
    X = np.stack([eps.GetEigenvector(i) for i in range(k)], axis=1)
    G = X.T @ (Bd @ X) if Bd is not None else X.T @ X
    assert np.abs(G - np.eye(k)).max() <= 1e-8
    _inner(eps)
    return lam, X


# ---- the reference's programs, with the options the reference runs them with ----------------------------------------------------------------
def _test1_pencil():
    n = 324
    return sc.laplacian2d_csr(18, 18), sp.diags(2.0 / np.log(np.arange(n) + 2.0)).tocsr()


def _test1(ctx, A, B, bs):
    eps = _jd(ctx, A, B, nev=4, bs=bs, tol=1e-10, max_it=1500)
    eps.SetConvergenceTest("norm")
    eps.Solve()
    return eps


@pytest.mark.parametrize("bs", [1, 3])
def test_reference_test1(ctx, bs):
    """test1 with -eps_type jd prints test1_1.out: GHEP, default `which` (largest magnitude: K = diag(B), the pair (1, 0) until `fix` applies)"""
    import slepc_amd as ks
    As, Bs = _test1_pencil()
    eps = _test1(ctx, _mat(ctx, As), _mat(ctx, Bs), bs)
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4 and eps.GetType() == "jd"
    ref = gi.eigenvalues_line(gi.read("eps/eps_test1_1.out"))
    assert len(ref) == 4
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.JDGetStats()))
    assert ["%.5f" % v for v in _values(eps, 4)] == ["%.5f" % v for v in ref]
    X = np.stack([eps.GetEigenvector(i) for i in range(4)], axis=1)
    assert np.abs(X.T @ (Bs @ X) - np.eye(4)).max() <= 10 * 1e-10
    st = _inner(eps)
    assert st["pc_columns"] > 0 and eps.JDGetBlockSize() == bs


def test_reference_test10(ctx):
    """test10 -eps_nev 4 -m 11: the constant null vector of the 10 x 11 mesh-graph Laplacian deflated, smallest real"""
    import slepc_amd as ks
    S = sc.graph_laplacian_2d(10, 11)
    eps = _jd(ctx, _mat(ctx, S), nev=4, max_it=500, which="smallest_real")
    eps.SetDeflationSpace(np.ones((110, 1)))
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.JDGetStats()))
    assert np.allclose(np.round(_values(eps, 4), 5), gi.eigenvalues_line(gi.read("eps/eps_test10_1.out")), atol=1.5e-5)
    X = np.stack([eps.GetEigenvector(i) for i in range(4)], axis=1)
    assert np.abs(np.ones(110) @ X).max() < 1e-10                       # the corrections are orthogonalised against the constraint with the basis
    _inner(eps)


def test_reference_test20(ctx):
    """test20 -n 18 -eps_max_it 1500: the smallest eigenvalue of the 1-D Laplacian, then again on the same solver with ncv + 2"""
    import slepc_amd as ks
    S = sc.tridiag_csr(18, -1.0, 2.0, -1.0)
    tol = max(1000 * EPSM, 1e-9)
    ref = gi.eigenvalue_lines(gi.read("eps/eps_test20_1.out"))
    eps = _jd(ctx, _mat(ctx, S), nev=1, tol=tol, max_it=1500, which="smallest_real")
    eps.Solve()
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.JDGetStats()))
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and abs(round(_values(eps, 1)[0], 5) - ref[0][0]) < 1.5e-5
    _inner(eps)
    nev, ncv, mpd = eps.GetDimensions()
    eps.SetDimensions(nev, ncv + 2)
    eps.Solve()
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.JDGetStats()))
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetDimensions()[1] == ncv + 2
    assert abs(round(_values(eps, 1)[0], 5) - ref[1][0]) < 1.5e-5
    _inner(eps)


def test_reference_test28(ctx):
    """test28 -eps_type jd: two Laplacians of different sizes solved one after the other on the same solver, nev = 3, smallest real"""
    import slepc_amd as ks
    ref = gi.eigenvalue_lines(gi.read("eps/eps_test28_1.out"))
    eps = ks.EPS(ctx)
    for k, (n, m) in enumerate(((10, 11), (20, 22))):
        S = sc.laplacian2d_csr(n, m)
        eps.SetOperators(_mat(ctx, S))
        if k == 0:
            eps.SetProblemType(ks.EPS_HEP); eps.SetType("jd"); eps.SetWhichEigenpairs("smallest_real"); eps.SetDimensions(3)
        eps.Solve()
        print("its %d, stats %s" % (eps.GetIterationNumber(), eps.JDGetStats()))
        assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 3 and eps.GetIterationNumber() <= 5 * 19
        assert np.allclose(np.round(_values(eps, 3), 5), ref[k], atol=1.5e-5)
        assert eps.GetEigenvector(0).shape == (n * m,) and eps.ComputeError(0) < 1e-7
        _inner(eps)


def test_reference_test8_takes_the_gd_correction(ctx):
    """test8 -n 20 -eps_nev 4 -eps_ncv 11 -eps_max_it 40000 -eps_type jd -eps_jd_blocksize 3 (the matrix assembled: the ST needs one). A standard
    problem and largest magnitude: the pair (1, 0) without a B - the reference's "odd situation" - so every pair takes the GD correction until its
    residual is below fix |theta|. 7.88881 is a double eigenvalue."""
    import slepc_amd as ks
    eps = _jd(ctx, _mat(ctx, sc.laplacian2d_csr(20, 20)), nev=4, bs=3, ncv=11, max_it=40000)
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4
    st = eps.JDGetStats()
    print("its %d, stats %s" % (eps.GetIterationNumber(), st))
    ref = gi.eigenvalues_line(gi.read("eps/eps_test8_1.out"))
    assert len(ref) == 4
    assert ["%.5f" % v for v in _values(eps, 4)] == ["%.5f" % v for v in ref]
    assert st["gd_fallbacks"] > 0 and st["pc_columns"] == 0
    assert eps.GetIterationNumber() <= 5 * 55


# ---- against dense solves: both ends of the spectrum, an interior target, a generalized problem; both block sizes, both inner solvers -------
@pytest.mark.parametrize("ksp", ["bcgs", "gmres"])
@pytest.mark.parametrize("bs", [1, 4])
@pytest.mark.parametrize("which", ["smallest_real", "largest_real"])
def test_ends_of_the_spectrum(ctx, bs, which, ksp):
    """smallest real with point Jacobi; largest real with no shift set: the infinite default shift, no preconditioner, the GD correction until `fix`"""
    eps = _jd(ctx, _mat(ctx, LAP), nev=4, bs=bs, which=which, ksp=ksp)
    eps.Solve()
    _check_against(eps, 4, LAP_EIG if which == "smallest_real" else LAP_EIG[::-1], LAP_NORM, 1e-8)
    st = eps.JDGetStats()
    assert (st["pc_columns"] > 0) == (which == "smallest_real")
    assert (st["gd_fallbacks"] > 0) == (which == "largest_real")


@pytest.mark.parametrize("bs", [1, 4])
@pytest.mark.parametrize("pc", [("bjacobi", 24), ("bjacobi-ilu", 64)])
def test_interior_target(ctx, bs, pc):
    """the three eigenvalues closest to 1.0 (0.96176, 1.05352, 0.88494), K = the diagonal blocks of A - 1.0 I, dense or ILU(0)"""
    eps = _jd(ctx, _mat(ctx, LAP), nev=3, bs=bs, which="target_magnitude")
    eps.SetTarget(1.0)
    eps.GetST().SetPC(*pc)
    eps.Solve()
    exact = np.array(sorted(LAP_EIG, key=lambda x: abs(x - 1.0)))
    assert np.allclose(exact[:3], [0.96176, 1.05352, 0.88494], atol=1e-5)
    _check_against(eps, 3, exact, LAP_NORM, 1e-8)
    assert eps.JDGetStats()["pc_columns"] > 0 and eps.JDGetStats()["gd_fallbacks"] == 0


@pytest.mark.parametrize("ksp", ["bcgs", "gmres"])
@pytest.mark.parametrize("bs", [1, 4])
def test_tridiagonal_b_pencil(ctx, bs, ksp):
    Bd = BT.toarray()
    exact = scipy.linalg.eigh(LAP.toarray(), Bd, eigvals_only=True)
    eps = _jd(ctx, _mat(ctx, LAP), _mat(ctx, BT), nev=5, bs=bs, which="smallest_real", ksp=ksp)
    eps.Solve()
    _check_against(eps, 5, exact, LAP_NORM, 1e-8, Bd=Bd)


# ---- the parameters JD adds --------------------------------------------------------------------------------------------------------------------
def test_fix_decides_between_the_ritz_value_and_the_target(ctx):
    """Largest real of a standard problem makes the choice visible: the target pair is (1, 0), which without a B is the GD correction. fix enormous:
    every pair takes (theta_j, 1) from the first iteration - every correction is an inner solve, none falls back; fix tiny: none ever does - no
    inner solve at all. Both converge to the same values; so do both on the smallest real, where the pairs are (theta_j, 1) and (0, 1)."""
    A = _mat(ctx, LAP)
    out = {}
    for fix in (1e30, 1e-30):
        eps = _jd(ctx, A, nev=4, which="largest_real", max_it=1000)
        eps.JDSetFix(fix)
        assert eps.JDGetFix() == fix
        eps.Solve()
        import slepc_amd as ks
        assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4
        lam = _values(eps, 4); err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(4)])
        assert np.all(np.abs(lam - LAP_EIG[::-1][:4]) <= err + 64 * EPSM * LAP_NORM)
        out[fix] = eps.JDGetStats()
        print("fix %g: its %d, stats %s" % (fix, eps.GetIterationNumber(), out[fix]))
    assert out[1e30]["gd_fallbacks"] == 0 and out[1e30]["inner_solves"] > 0
    assert out[1e-30]["inner_solves"] == 0 and out[1e-30]["gd_fallbacks"] > 0
    for fix in (1e30, 1e-30):
        eps = _jd(ctx, A, nev=4, which="smallest_real")
        eps.JDSetFix(fix)
        eps.Solve()
        _check_against(eps, 4, LAP_EIG, LAP_NORM, 1e-8)
        assert eps.JDGetStats()["gd_fallbacks"] == 0


def test_dynamic_tolerance_converges_to_the_same_values(ctx):
    A = _mat(ctx, LAP)
    lam = {}
    for const in (True, False):
        eps = _jd(ctx, A, nev=4, which="smallest_real")
        assert eps.JDGetConstCorrectionTol() is True                     # the default
        eps.JDSetConstCorrectionTol(const)
        assert eps.JDGetConstCorrectionTol() is const
        eps.Solve()
        lam[const], _ = _check_against(eps, 4, LAP_EIG, LAP_NORM, 1e-8)
        lam[const] = (lam[const], eps.JDGetStats())
    assert np.allclose(lam[True][0], lam[False][0], rtol=0, atol=2e-8 * LAP_NORM)
    # loose early solves: fewer inner iterations per solve than the constant 1e-4
    assert lam[False][1]["inner_iterations"] / lam[False][1]["inner_solves"] < lam[True][1]["inner_iterations"] / lam[True][1]["inner_solves"]


def test_the_caller_s_ksp_settings_win_and_the_st_keeps_its_own(ctx):
    """rtol and max_it set on the ST are JD's; JD's defaults (1e-4, 90) are never written into the ST, whose values a later sinvert solve uses"""
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    eps = _jd(ctx, A, nev=2, which="smallest_real")
    eps.GetST().SetKSP(rtol=1e-2, max_it=7)
    eps.Solve()
    st = _inner(eps)
    assert st["inner_iterations"] <= 7 * st["inner_solves"]
    _check_against(eps, 2, LAP_EIG, LAP_NORM, 1e-8)
    eps2 = _jd(ctx, A, nev=2, which="smallest_real")
    eps2.Solve()
    assert _inner(eps2)["inner_iterations"] > 7 * _inner(eps2)["inner_solves"]       # the default limit is 90 and these solves use more than 7
    # GD's settings are its own: JD's block size does not move them
    eps2.JDSetBlockSize(3)
    assert eps2.JDGetBlockSize() == 3 and eps2.GDGetBlockSize() == 1
    eps2.GDSetRestart(4, 2)
    assert eps2.JDGetRestart() != (4, 2)


# ---- the object: second solve, type switching, callbacks -----------------------------------------------------------------------------------
def test_second_solve_repeats_the_values(ctx):
    eps = _jd(ctx, _mat(ctx, LAP), nev=4, bs=2, which="smallest_real")
    eps.Solve()
    first = _values(eps, 4); its = eps.GetIterationNumber(); st = eps.JDGetStats()
    eps.Solve()
    assert np.array_equal(_values(eps, 4), first) and eps.GetIterationNumber() == its and eps.JDGetStats() == st
    _check_against(eps, 4, LAP_EIG, LAP_NORM, 1e-8)


def _rc(eps):
    import slepc_amd as ks
    try:
        eps.Solve()
    except ks.KsError as e:
        return e.rc
    return 0


def test_type_round_trip_restores_the_st_and_the_krylovschur_result(ctx):
    import slepc_amd as ks
    A = _mat(ctx, sc.laplacian2d_csr(13, 11))

    def ks_solve(prepare):
        eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(4, 20)
        prepare(eps)
        eps.Solve()
        return [eps.GetEigenvalue(i) for i in range(eps.GetConverged())], eps.GetIterationNumber(), eps.GetStats()

    plain = ks_solve(lambda eps: None)
    back = ks_solve(lambda eps: (eps.SetType("jd"), eps.SetType("krylovschur")))
    assert plain == back and len(plain[0]) >= 4

    def solved_as_jd_first(eps):                     # a JD solve (largest magnitude: the infinite default shift) on the same object, then back
        eps.SetType("jd"); eps.Solve(); assert eps.GetType() == "jd"
        eps.SetType("krylovschur")
    assert ks_solve(solved_as_jd_first) == plain

    def sinvert_after_jd(with_jd):                   # the ST's own KSP values survive a JD solve: the same sinvert run with and without one before it
        eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(3, 16)
        if with_jd:
            eps.SetType("jd"); eps.SetWhichEigenpairs("smallest_real"); eps.Solve(); eps.SetType("krylovschur")
        eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(1.0); eps.GetST().SetType("sinvert")
        eps.Solve()
        return [eps.GetEigenvalue(i) for i in range(3)], eps.GetIterationNumber(), eps.GetST().GetKSPStats()["iterations"] > 0
    assert sinvert_after_jd(True) == sinvert_after_jd(False)
    eps = ks.EPS(ctx); eps.SetOperators(A)
    assert ctx.L.ks_eps_set_type(eps.h, 4) == SUP and eps.GetType() == "krylovschur"      # an unknown type is refused


def test_monitor_stopping_and_initial_space(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    w, Q = np.linalg.eigh(LAP.toarray())
    seen = []
    cold = _jd(ctx, A, nev=4, bs=2, which="smallest_real"); cold.SetRandomSeed(77)
    cold.MonitorSet(lambda its, nconv, er, ei, ee: seen.append((its, nconv, len(er))))
    cold.Solve()
    _check_against(cold, 4, LAP_EIG, LAP_NORM, 1e-8)
    assert [s[0] for s in seen] == list(range(1, cold.GetIterationNumber() + 1))       # once per iteration
    assert all(b[1] >= a[1] for a, b in zip(seen, seen[1:])) and all(s[2] <= 4 for s in seen)
    warm = _jd(ctx, A, nev=4, bs=2, which="smallest_real"); warm.SetRandomSeed(77)
    warm.SetInitialSpace(Q[:, :4] + 1e-3 * np.random.default_rng(8).standard_normal((108, 4)))
    warm.Solve()
    _check_against(warm, 4, LAP_EIG, LAP_NORM, 1e-8)
    assert warm.GetIterationNumber() < cold.GetIterationNumber(), (warm.GetIterationNumber(), cold.GetIterationNumber())
    stop = _jd(ctx, A, nev=4, bs=2, which="smallest_real")
    stop.SetStoppingTestFunction(lambda its, max_it, nconv, nev: ks.EPS_CONVERGED_USER if its >= 3 else 0)
    stop.Solve()
    assert stop.GetConvergedReason() == ks.EPS_CONVERGED_USER and stop.GetIterationNumber() == 3


# ---- set-up errors: GD's list (EPSSetUp_XD, davidson.c:51-77) and fix <= 0 --------------------------------------------------------------------
def test_setup_errors(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    Bs = sp.identity(108, format="csr") * 2.0
    e = _jd(ctx, A, nev=4, ncv=3); assert _rc(e) == SUP                               # ncv < nev
    e = _jd(ctx, A, nev=4, ncv=10, mpd=11); assert _rc(e) == SUP                      # mpd > ncv
    e = _jd(ctx, A, nev=1, ncv=10, mpd=1); assert _rc(e) == SUP                       # mpd < 2
    e = _jd(ctx, A, nev=4, bs=3, ncv=6); assert _rc(e) == SUP                         # nev + bs > ncv
    e = _jd(ctx, A, nev=2); e.SetTrueResidual(True); assert _rc(e) == SUP
    e = _jd(ctx, A, nev=2); e.SetTwoSided(True); assert _rc(e) == SUP
    e = _jd(ctx, A, nev=2); e.SetExtraction("harmonic"); assert _rc(e) == SUP
    e = _jd(ctx, A, nev=2); e.SetArbitrarySelection(lambda re, im, xr, xi: (re, im)); assert _rc(e) == SUP
    e = _jd(ctx, A, nev=2, bs=4, ncv=12, mpd=8); e.JDSetRestart(5, 1); assert _rc(e) == SUP      # minv + bs > mpd
    e = _jd(ctx, A, nev=2, ncv=12, mpd=5); e.JDSetInitialSize(6); assert _rc(e) == SUP           # initial size > mpd
    e = _jd(ctx, A, nev=2, ptype=ks.EPS_NHEP); assert _rc(e) == SUP
    e = _jd(ctx, A, _mat(ctx, Bs), nev=2, ptype=ks.EPS_GNHEP); assert _rc(e) == SUP
    e = _jd(ctx, A, _mat(ctx, Bs), nev=2); e.JDSetBOrth(False); assert e.JDGetBOrth() is False and _rc(e) == SUP
    e = _jd(ctx, A, nev=2)
    for bad in (17, -1):
        with pytest.raises(ks.KsError) as ex:
            e.JDSetBlockSize(bad)
        assert ex.value.rc == OUTOFRANGE
    for bad in (0.0, -0.5):
        with pytest.raises(ks.KsError) as ex:
            e.JDSetFix(bad)
        assert ex.value.rc == OUTOFRANGE
    assert e.JDGetFix() == 0.01 and e.GetType() == "jd"
    # the defaults are GD's: ncv = max(nev, min(n - bs, max(2 nev, nev + 15)) + bs), mpd = min(n, ncv), max_it = max(100 ncv, 2 n)
    e = _jd(ctx, A, nev=2, bs=3, max_it=0, which="smallest_real"); assert _rc(e) == 0
    assert e.GetDimensions() == (2, 20, 20) and e.GetTolerances()[1] == 2000
    assert e.JDGetRestart() == (6, 1) and e.JDGetInitialSize() == 6 and e.JDGetBOrth() is True
    e = _jd(ctx, A, nev=2, ncv=12, which="smallest_real"); e.JDSetRestart(3, 2); e.JDSetInitialSize(5); assert _rc(e) == 0
    assert e.JDGetRestart() == (3, 2) and e.JDGetInitialSize() == 5 and e.GetDimensions() == (2, 12, 12)
    assert np.allclose(_values(e, 2), LAP_EIG[:2], rtol=1e-7)


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks(ctx):
    import slepc_amd as ks
    As, Bs = _test1_pencil()
    As = As.tocsr(); Bs = Bs.tocsr()
    split = [(0, 170), (170, 324)]

    def rank_fn(rank, comm):
        c = ks.Context(0)
        comm.install(c, rank)
        s0, s1 = split[rank]
        A = _mat(c, As[s0:s1], row_start=s0, n_global=324); B = _mat(c, Bs[s0:s1], row_start=s0, n_global=324)
        eps = _test1(c, A, B, 3)
        out = (["%.5f" % v for v in _values(eps, 4)], eps.GetIterationNumber(), eps.GetConverged(), eps.GetConvergedReason(), eps.JDGetStats())
        del eps
        A.destroy(); B.destroy(); c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    ref = ["%.5f" % v for v in gi.eigenvalues_line(gi.read("eps/eps_test1_1.out"))]
    assert res[0][0] == ref and res[1][0] == ref
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2] and res[0][3] == res[1][3] == ks.EPS_CONVERGED_TOL
    assert res[0][4] == res[1][4] and res[0][4]["inner_solves"] > 0
