"""Generalized Davidson solves (ks_eps_set_type(KS_EPS_GD), slepc_amd/csrc/ks_gd.hip) against the reference's golden outputs and against dense
numpy / LAPACK solves done here.

Bounds, as in tests/test_gpu_lobpcg.py. For a unit eigenvector estimate x with residual r = A x - theta x of a symmetric A some eigenvalue lies
within ||r||_2 of theta; with the wanted eigenvalues separated by far more than the tolerance that is the i-th one: |theta_i - lambda_i| <= err_i +
64 eps ||A||_2, err_i the absolute residual ks_eps_compute_error returns. For A x = lambda B x the same holds in the B^-1 norm:
|theta - lambda| <= ||r||_2 / sqrt(lambda_min(B)) for a B-normalised x.

Iteration counts of the loop as built, from its numpy restatement scripts/gd_restatement.py (three seeds each; the default restart minv 6 - 16 at
bs 16 -, plusk 1 unless named):
  test1 (max_it 1500)                 bs 1: 149-154   bs 3: 92-99
  test10 (max_it 500)                 bs 1: 154-156   bs 2: 98-102
  ends of the spectrum (2000)         smallest real, Jacobi   bs 1: 182-187  bs 4: 99-105  bs 16: 101-108
                                      largest real, no PC     bs 1: 156-161  bs 4: 83-90   bs 16: 93-95
  target 1.0, bjacobi 24 (2000)       bs 1: 204-218   bs 3: 98-111
  tridiagonal B (2000)                bs 1: 157-160   bs 4: 78-79;  largest real, block Jacobi (8) on B alone, bs 2: 49-53
  restart parameters, ncv 12 (2000)   minv 3: plusk 0 184-197, 1 147-154, 2 138-148;  minv 6: plusk 0 140-155, 1 151-158, 2 126-130
On the MI355X (the library's own random start) the same cases took 153 / 96, 156 / 98, 178 / 98 / 96 and 162 / 85 / 81, 226 / 117, 156 / 75, and 127 to 191
with the restart parameters; the B-only block preconditioner 51, and 101 once a shift of -1 is set. Every cap is at least five times the largest count of its case except test10's, which is the reference program's
(500, 3.2 times its 156); no count comes within a factor of two of its cap, so a cap cannot hide a failure. Every solve asserts EPS_CONVERGED_TOL."""
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


def _mat(ctx, S, keep=True, **kw):
    import slepc_amd as ks
    S = S.tocsr(); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep, **kw)


def _gd(ctx, A, B=None, nev=1, bs=0, tol=1e-8, max_it=2000, which=None, ptype=None, ncv=0, mpd=0):
    import slepc_amd as ks
    eps = ks.EPS(ctx)
    eps.SetOperators(A, B)
    eps.SetProblemType(ptype or (ks.EPS_GHEP if B is not None else ks.EPS_HEP))
    eps.SetType("gd")
    eps.SetDimensions(nev, ncv, mpd)
    if bs:
        eps.GDSetBlockSize(bs)
    eps.SetTolerances(tol, max_it)
    if which:
        eps.SetWhichEigenpairs(which)
    return eps


def _values(eps, k):
    return np.array([eps.GetEigenvalue(i)[0] for i in range(k)])


LAP = sc.laplacian2d_csr(12, 9)                       # n = 108, simple eigenvalues
LAP_EIG = np.linalg.eigvalsh(LAP.toarray())
LAP_NORM = LAP_EIG[-1]


def _check_against(eps, k, exact, normA, tol):
    """the bound of the module docstring for the first k pairs, the relative residuals against the tolerance, orthonormal eigenvectors"""
    import slepc_amd as ks
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= k
    lam = _values(eps, k)
    err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(k)])
    print("its %d, |theta - lambda| %s, residuals %s, stats %s" % (eps.GetIterationNumber(), np.abs(lam - exact[:k]), err, eps.GDGetStats()))
    assert np.all(np.abs(lam - exact[:k]) <= err + 64 * EPSM * normA), (lam, exact[:k], err)
    assert np.all(err <= tol * np.abs(lam)), (err, lam)
    X = np.stack([eps.GetEigenvector(i) for i in range(k)], axis=1)
    assert np.abs(X.T @ X - np.eye(k)).max() <= 1e-8
    return lam, X


# ---- the reference's programs --------------------------------------------------------------------------------------------------------------
def _test1_pencil():
    n = 324
    return sc.laplacian2d_csr(18, 18), sp.diags(2.0 / np.log(np.arange(n) + 2.0)).tocsr()


def _test1(ctx, A, B, bs):
    eps = _gd(ctx, A, B, nev=4, bs=bs, tol=1e-10, max_it=1500)
    eps.SetConvergenceTest("norm")
    eps.Solve()
    return eps


@pytest.mark.parametrize("bs", [1, 3])
def test_reference_test1(ctx, bs):
    """test1 with -eps_type gd prints test1_1.out: GHEP, default `which` (largest magnitude: the infinite default shift, M = diag(B)^-1)"""
    import slepc_amd as ks
    As, Bs = _test1_pencil()
    eps = _test1(ctx, _mat(ctx, As), _mat(ctx, Bs), bs)
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4 and eps.GetType() == "gd"
    ref = gi.eigenvalues_line(gi.read("eps/eps_test1_1.out"))
    assert len(ref) == 4
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.GDGetStats()))
    assert ["%.5f" % v for v in _values(eps, 4)] == ["%.5f" % v for v in ref]
    X = np.stack([eps.GetEigenvector(i) for i in range(4)], axis=1)
    assert np.abs(X.T @ (Bs @ X) - np.eye(4)).max() <= 10 * 1e-10
    st = eps.GDGetStats()
    assert st["fused_residuals"] > 0 and st["mat_columns"] > 0 and st["pc_columns"] > 0 and st["locks"] > 0 and st["iterations"] > 0
    assert eps.GDGetBlockSize() == bs


@pytest.mark.parametrize("bs", [1, 2])
def test_reference_test10(ctx, bs):
    """test10 -eps_nev 4 -m 11: the constant null vector of the 10 x 11 mesh-graph Laplacian deflated, smallest real"""
    import slepc_amd as ks
    S = sc.graph_laplacian_2d(10, 11)
    eps = _gd(ctx, _mat(ctx, S), nev=4, bs=bs, max_it=500, which="smallest_real")
    eps.SetDeflationSpace(np.ones((110, 1)))
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 4
    print("its %d, stats %s" % (eps.GetIterationNumber(), eps.GDGetStats()))
    assert np.allclose(np.round(_values(eps, 4), 5), gi.eigenvalues_line(gi.read("eps/eps_test10_1.out")), atol=1.5e-5)


# ---- both ends of the spectrum, a target, a generalized problem ---------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 4, 16])
@pytest.mark.parametrize("which", ["smallest_real", "largest_real"])
def test_ends_of_the_spectrum(ctx, bs, which):
    """smallest real with point Jacobi; largest real with no shift set: the infinite default shift, no preconditioning of a standard problem"""
    eps = _gd(ctx, _mat(ctx, LAP), nev=6, bs=bs, which=which)
    eps.Solve()
    _check_against(eps, 6, LAP_EIG if which == "smallest_real" else LAP_EIG[::-1], LAP_NORM, 1e-8)
    st = eps.GDGetStats()
    assert (st["pc_columns"] > 0) == (which == "smallest_real")
    assert st["fused_residuals"] > 0 and st["mat_columns"] > 0 and st["locks"] > 0


@pytest.mark.parametrize("bs", [1, 3])
def test_target(ctx, bs):
    """the three eigenvalues closest to 1.0 (0.96176, 1.05352, 0.88494; the next one is 0.0024 further), block Jacobi on A - 1.0 I"""
    eps = _gd(ctx, _mat(ctx, LAP), nev=3, bs=bs, which="target_magnitude")
    eps.SetTarget(1.0)
    eps.GetST().SetPC("bjacobi", 24)
    eps.Solve()
    exact = np.array(sorted(LAP_EIG, key=lambda x: abs(x - 1.0)))
    assert np.allclose(exact[:3], [0.96176, 1.05352, 0.88494], atol=1e-5)
    _check_against(eps, 3, exact, LAP_NORM, 1e-8)
    assert eps.GDGetStats()["pc_columns"] > 0


@pytest.mark.parametrize("bs", [1, 4])
def test_generalized(ctx, bs):
    import slepc_amd as ks
    n = LAP.shape[0]
    Bs = sp.diags([np.full(n - 1, 0.25), np.ones(n), np.full(n - 1, 0.25)], [-1, 0, 1], format="csr")
    Bd = Bs.toarray()
    exact = scipy.linalg.eigh(LAP.toarray(), Bd, eigvals_only=True)
    bmin = np.linalg.eigvalsh(Bd)[0]
    eps = _gd(ctx, _mat(ctx, LAP), _mat(ctx, Bs), nev=5, bs=bs, which="smallest_real")
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 5
    lam = _values(eps, 5)
    err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(5)])
    print("its %d, |theta - lambda| %s, bound %s" % (eps.GetIterationNumber(), np.abs(lam - exact[:5]), err / np.sqrt(bmin)))
    assert np.all(np.abs(lam - exact[:5]) <= err / np.sqrt(bmin) + 64 * EPSM * LAP_NORM / bmin)
    X = np.stack([eps.GetEigenvector(i) for i in range(5)], axis=1)
    assert np.abs(X.T @ Bd @ X - np.eye(5)).max() <= 1e-8


def test_infinite_default_shift_builds_the_block_preconditioner_on_b(ctx):
    """largest real of the same pencil with no shift set: M = the diagonal blocks (8 rows) of B alone; a shift the caller sets wins over that default"""
    import slepc_amd as ks
    n = LAP.shape[0]
    Bs = sp.diags([np.full(n - 1, 0.25), np.ones(n), np.full(n - 1, 0.25)], [-1, 0, 1], format="csr")
    Bd = Bs.toarray()
    exact = scipy.linalg.eigh(LAP.toarray(), Bd, eigvals_only=True)[::-1]
    bmin = np.linalg.eigvalsh(Bd)[0]
    A, B = _mat(ctx, LAP), _mat(ctx, Bs)
    its = []
    for shift in (None, -1.0):
        eps = _gd(ctx, A, B, nev=3, bs=2, which="largest_real")
        eps.GetST().SetPC("bjacobi", 8)
        if shift is not None:
            eps.GetST().SetShift(shift)
        eps.Solve()
        assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 3
        lam = _values(eps, 3)
        err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(3)])
        assert np.all(np.abs(lam - exact[:3]) <= err / np.sqrt(bmin) + 64 * EPSM * LAP_NORM / bmin)
        assert eps.GDGetStats()["pc_columns"] > 0
        its.append(eps.GetIterationNumber())
    print("its with M from B alone %d, with M from A + B %d" % tuple(its))


@pytest.mark.parametrize("minv", [3, 6])
@pytest.mark.parametrize("plusk", [0, 1, 2])
def test_restart_parameters(ctx, minv, plusk):
    eps = _gd(ctx, _mat(ctx, LAP), nev=4, bs=2, which="smallest_real", ncv=12)
    eps.GDSetRestart(minv, plusk)
    eps.GDSetInitialSize(6)
    eps.Solve()
    _check_against(eps, 4, LAP_EIG, LAP_NORM, 1e-8)
    assert eps.GDGetStats()["restarts"] >= 1
    assert eps.GDGetRestart() == (minv, plusk) and eps.GDGetInitialSize() == 6 and eps.GDGetBlockSize() == 2 and eps.GDGetBOrth() is True
    assert eps.GetDimensions() == (4, 12, 12)


# ---- the object: second solve, type switching, callbacks -----------------------------------------------------------------------------------
def test_second_solve_repeats_the_values(ctx):
    eps = _gd(ctx, _mat(ctx, LAP), nev=4, bs=2, which="smallest_real")
    eps.Solve()
    first = _values(eps, 4); its = eps.GetIterationNumber()
    eps.Solve()
    assert np.array_equal(_values(eps, 4), first) and eps.GetIterationNumber() == its
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
    back = ks_solve(lambda eps: (eps.SetType("gd"), eps.SetType("krylovschur")))
    assert plain == back and len(plain[0]) >= 4

    def solved_as_gd_first(eps):                     # a GD solve (largest magnitude: the infinite default shift) on the same object, then back
        eps.SetType("gd"); eps.Solve(); assert eps.GetType() == "gd"
        eps.SetType("krylovschur")
    assert ks_solve(solved_as_gd_first) == plain
    eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(2)
    eps.GetST().SetType("precond")
    assert _rc(eps) == SUP                                                  # a Krylov-Schur solve with KS_ST_PRECOND is still refused
    assert eps.GetType() == "krylovschur"


def test_monitor_stopping_and_initial_space(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    w, Q = np.linalg.eigh(LAP.toarray())
    seen = []
    cold = _gd(ctx, A, nev=4, bs=2, which="smallest_real"); cold.SetRandomSeed(77)
    cold.MonitorSet(lambda its, nconv, er, ei, ee: seen.append((its, nconv, len(er))))
    cold.Solve()
    _check_against(cold, 4, LAP_EIG, LAP_NORM, 1e-8)
    assert [s[0] for s in seen] == list(range(1, cold.GetIterationNumber() + 1))       # once per iteration
    assert all(b[1] >= a[1] for a, b in zip(seen, seen[1:])) and all(s[2] <= 4 for s in seen)
    warm = _gd(ctx, A, nev=4, bs=2, which="smallest_real"); warm.SetRandomSeed(77)
    warm.SetInitialSpace(Q[:, :4] + 1e-3 * np.random.default_rng(8).standard_normal((108, 4)))
    warm.Solve()
    _check_against(warm, 4, LAP_EIG, LAP_NORM, 1e-8)
    assert warm.GetIterationNumber() < cold.GetIterationNumber(), (warm.GetIterationNumber(), cold.GetIterationNumber())
    stop = _gd(ctx, A, nev=4, bs=2, which="smallest_real")
    stop.SetStoppingTestFunction(lambda its, max_it, nconv, nev: ks.EPS_CONVERGED_USER if its >= 3 else 0)
    stop.Solve()
    assert stop.GetConvergedReason() == ks.EPS_CONVERGED_USER and stop.GetIterationNumber() == 3


# ---- set-up errors (EPSSetUp_XD, davidson.c:51-77) -----------------------------------------------------------------------------------------
def test_setup_errors(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    Bs = sp.identity(108, format="csr") * 2.0
    e = _gd(ctx, A, nev=4, ncv=3); assert _rc(e) == SUP                               # ncv < nev
    e = _gd(ctx, A, nev=4, ncv=10, mpd=11); assert _rc(e) == SUP                      # mpd > ncv
    e = _gd(ctx, A, nev=1, ncv=10, mpd=1); assert _rc(e) == SUP                       # mpd < 2
    e = _gd(ctx, A, nev=4, bs=3, ncv=6); assert _rc(e) == SUP                         # nev + bs > ncv
    e = _gd(ctx, A, nev=2); e.SetTrueResidual(True); assert _rc(e) == SUP
    e = _gd(ctx, A, nev=2); e.SetTwoSided(True); assert _rc(e) == SUP
    e = _gd(ctx, A, nev=2); e.SetExtraction("harmonic"); assert _rc(e) == SUP
    e = _gd(ctx, A, nev=2); e.SetArbitrarySelection(lambda re, im, xr, xi: (re, im)); assert _rc(e) == SUP
    e = _gd(ctx, A, nev=2, bs=4, ncv=12, mpd=8); e.GDSetRestart(5, 1); assert _rc(e) == SUP      # minv + bs > mpd
    e = _gd(ctx, A, nev=2, ncv=12, mpd=5); e.GDSetInitialSize(6); assert _rc(e) == SUP           # initial size > mpd
    e = _gd(ctx, A, nev=2, ptype=ks.EPS_NHEP); assert _rc(e) == SUP
    e = _gd(ctx, A, _mat(ctx, Bs), nev=2, ptype=ks.EPS_GNHEP); assert _rc(e) == SUP
    e = _gd(ctx, A, _mat(ctx, Bs), nev=2); e.GDSetBOrth(False); assert e.GDGetBOrth() is False and _rc(e) == SUP
    e = _gd(ctx, A, nev=2)
    for bad in (17, -1):
        with pytest.raises(ks.KsError) as ex:
            e.GDSetBlockSize(bad)
        assert ex.value.rc == OUTOFRANGE
    assert e.GetType() == "gd"
    # the defaults: ncv = max(nev, min(n - bs, max(2 nev, nev + 15)) + bs), mpd = min(n, ncv), max_it = max(100 ncv, 2 n); balancing is ignored
    e = _gd(ctx, A, nev=2, bs=3, max_it=0, which="smallest_real"); e.SetBalance("oneside"); assert _rc(e) == 0
    assert e.GetDimensions() == (2, 20, 20) and e.GetTolerances()[1] == 2000
    assert e.GDGetRestart() == (6, 1) and e.GDGetInitialSize() == 6
    e = _gd(ctx, A, nev=2, mpd=9, which="smallest_real"); assert _rc(e) == 0 and e.GetDimensions() == (2, 12, 9)      # mpd given: ncv = mpd + nev + bs
    assert e.GDGetRestart() == (4, 1)                                                  # min(max(bs, 6), mpd / 2)
    small = _mat(ctx, sc.tridiag_csr(8, -1.0, 2.0, -1.0))
    e = _gd(ctx, small, nev=2, which="smallest_real"); assert _rc(e) == 0             # n < 10: ncv = n + nev + bs, minv = initial size = 1
    assert e.GetDimensions() == (2, 11, 8) and e.GDGetRestart() == (1, 1) and e.GDGetInitialSize() == 1
    assert np.allclose(_values(e, 2), 2.0 - 2.0 * np.cos(np.pi * np.arange(1, 3) / 9.0), rtol=1e-7)


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
        out = (["%.5f" % v for v in _values(eps, 4)], eps.GetIterationNumber(), eps.GetConverged(), eps.GetConvergedReason())
        del eps
        A.destroy(); B.destroy(); c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    ref = ["%.5f" % v for v in gi.eigenvalues_line(gi.read("eps/eps_test1_1.out"))]
    assert res[0][0] == ref and res[1][0] == ref
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2] and res[0][3] == res[1][3] == ks.EPS_CONVERGED_TOL
