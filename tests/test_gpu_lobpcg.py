"""LOBPCG solves (ks_eps_set_type(KS_EPS_LOBPCG), slepc_amd/csrc/ks_lobpcg.hip) against the reference's golden outputs and against dense
numpy / LAPACK solves done here.

Bounds. For a unit eigenvector estimate x with residual r = A x - theta x of a symmetric A some eigenvalue lies within ||r||_2 of theta; with the
eigenvalues of the wanted end of the spectrum separated by far more than the tolerance that is the i-th one. So |theta_i - lambda_i| <= err_i +
64 eps ||A||_2, err_i the absolute residual ks_eps_compute_error returns and the second term the rounding of the reference and of the residual.
For A x = lambda B x the same holds in the B^-1 norm: |theta - lambda| <= ||r||_2 / sqrt(lambda_min(B)) for a B-normalised x.

Every shape below converged in 29 to 176 iterations in a numpy restatement of the reference's loop, so max_it = 1000 (1200, 2000 where the
reference's program or the issue sets it) cannot hide a failure, and every test asserts EPS_CONVERGED_TOL."""
import numpy as np
import pytest
import scipy.sparse as sp

import golden_inputs as gi
import scenarios as sc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
EPSM = np.finfo(float).eps
SUP, USER_INPUT, OUTOFRANGE = 56, 95, 63


def _mat(ctx, S, keep=True, **kw):
    import slepc_amd as ks
    S = S.tocsr(); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep, **kw)


def _lobpcg(ctx, A, B=None, nev=1, bs=0, tol=1e-8, max_it=1000, which=None, ptype=None):
    import slepc_amd as ks
    eps = ks.EPS(ctx)
    eps.SetOperators(A, B)
    eps.SetProblemType(ptype or (ks.EPS_GHEP if B is not None else ks.EPS_HEP))
    eps.SetType("lobpcg")
    eps.SetDimensions(nev)
    if bs:
        eps.LOBPCGSetBlockSize(bs)
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
    print("its %d, |theta - lambda| %s, residuals %s" % (eps.GetIterationNumber(), np.abs(lam - exact[:k]), err))
    assert np.all(np.abs(lam - exact[:k]) <= err + 64 * EPSM * normA), (lam, exact[:k], err)
    assert np.all(err <= tol * np.abs(lam)), (err, lam)
    X = np.stack([eps.GetEigenvector(i) for i in range(k)], axis=1)
    assert np.abs(X.T @ X - np.eye(k)).max() <= 1e-8
    return lam, X


# ---- 1, 2: the reference's programs ------------------------------------------------------------------------------------------------------
def _test24(ctx, A, rows=slice(None), n=30):
    import slepc_amd as ks
    eps = _lobpcg(ctx, A, nev=4, bs=4, tol=1e-8, max_it=1200)
    eps.SetConvergenceTest("abs")
    eps.LOBPCGSetRestart(0.7)
    alpha = np.pi / (n + 1); beta = np.sqrt(2.0 / (n + 1))
    Cm = np.stack([np.sin(alpha * (np.arange(n) + 1) * (i + 1)) * beta for i in range(2)], axis=1)      # the two lowest eigenvectors, test24.c:73-83
    eps.SetDeflationSpace(Cm[rows])
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL
    assert (eps.LOBPCGGetBlockSize(), eps.LOBPCGGetRestart(), eps.LOBPCGGetLocking(), eps.GetType()) == (4, 0.7, True, "lobpcg")
    return eps


def test_reference_test24(ctx):
    eps = _test24(ctx, _mat(ctx, sc.tridiag_csr(30, -1.0, 2.0, -1.0)))
    ref = gi.eigenvalues_line(gi.read("eps/eps_test24_1.out"))
    assert len(ref) == 4 and eps.GetConverged() >= 4
    assert ["%.5f" % v for v in _values(eps, 4)] == ["%.5f" % v for v in ref]
    st = eps.LOBPCGGetStats()
    assert st["iterations"] > 0 and st["mat_columns"] > 0 and st["pc_columns"] > 0


def test_reference_ex19(ctx):
    import slepc_amd as ks
    eps = _lobpcg(ctx, ks.Mat.laplacian3d(ctx, 10, 10, 10), nev=8, tol=1e-7)
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL
    ref = gi.eigenvalues_line(gi.read("eps/ex19_1.out"))
    assert len(ref) == 8
    assert ["%.5f" % v for v in _values(eps, 8)] == ["%.5f" % v for v in ref]


# ---- 3: hard locking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lock", [True, False])
@pytest.mark.parametrize("restart,guard", [(0.9, 0), (0.6, 2)])
def test_hard_locking(ctx, lock, restart, guard):
    assert min(int((1.0 - restart) * 4 + 0.45), 3) == guard              # lobpcg.c:75
    eps = _lobpcg(ctx, _mat(ctx, LAP), nev=6, bs=4, tol=1e-8)
    eps.LOBPCGSetRestart(restart); eps.LOBPCGSetLocking(lock)
    eps.Solve()
    _check_against(eps, 6, LAP_EIG, LAP_NORM, 1e-8)
    assert eps.LOBPCGGetStats()["hard_locks"] >= 1
    assert eps.LOBPCGGetLocking() == lock


# ---- 4, 5 ----------------------------------------------------------------------------------------------------------------------------------
def test_block_size_one(ctx):
    eps = _lobpcg(ctx, _mat(ctx, LAP), nev=3, bs=1, tol=1e-8, max_it=2000)
    eps.Solve()
    _check_against(eps, 3, LAP_EIG, LAP_NORM, 1e-8)
    assert eps.LOBPCGGetStats()["hard_locks"] >= 2


def test_largest_real(ctx):
    eps = _lobpcg(ctx, _mat(ctx, LAP), nev=5, bs=3, tol=1e-8, which="largest_real")
    eps.Solve()
    _check_against(eps, 5, LAP_EIG[::-1], LAP_NORM, 1e-8)


# ---- 6: generalized ----------------------------------------------------------------------------------------------------------------------
def test_generalized(ctx):
    import slepc_amd as ks
    n = LAP.shape[0]
    u = np.random.default_rng(5).uniform(0.0, 1.0, n)
    Bs = sp.diags([np.full(n - 1, 0.3), 2.0 + u, np.full(n - 1, 0.3)], [-1, 0, 1], format="csr")
    Bd = Bs.toarray()
    Lc = np.linalg.cholesky(Bd)
    Cm = np.linalg.solve(Lc, np.linalg.solve(Lc, LAP.toarray()).T).T
    exact = np.linalg.eigvalsh((Cm + Cm.T) / 2)
    bmin = np.linalg.eigvalsh(Bd)[0]
    eps = _lobpcg(ctx, _mat(ctx, LAP), _mat(ctx, Bs), nev=6, bs=4, tol=1e-8)
    eps.GetST().SetPC("jacobi")
    eps.Solve()
    assert eps.GetConvergedReason() == ks.EPS_CONVERGED_TOL and eps.GetConverged() >= 6
    lam = _values(eps, 6)
    err = np.array([eps.ComputeError(i, ks.EPS_ERROR_ABSOLUTE) for i in range(6)])
    print("its %d, |theta - lambda| %s, bound %s" % (eps.GetIterationNumber(), np.abs(lam - exact[:6]), err / np.sqrt(bmin)))
    assert np.all(np.abs(lam - exact[:6]) <= err / np.sqrt(bmin))
    X = np.stack([eps.GetEigenvector(i) for i in range(6)], axis=1)
    assert np.abs(X.T @ Bd @ X - np.eye(6)).max() <= 1e-8


# ---- 7: preconditioners ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,bs", [("none", 0), ("jacobi", 0), ("bjacobi-ilu", 64)])
def test_preconditioners(ctx, pc, bs):
    eps = _lobpcg(ctx, _mat(ctx, LAP), nev=6, bs=4, tol=1e-8)
    eps.GetST().SetPC(pc, bs)
    eps.Solve()
    _check_against(eps, 6, LAP_EIG, LAP_NORM, 1e-8)
    st = eps.LOBPCGGetStats()
    assert (st["pc_columns"] > 0) == (pc != "none")


# ---- 8: initial space and callbacks ------------------------------------------------------------------------------------------------------
def test_initial_space_monitor_and_stopping(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    w, Q = np.linalg.eigh(LAP.toarray())
    seen = []
    cold = _lobpcg(ctx, A, nev=6, bs=4, tol=1e-8); cold.SetRandomSeed(77)
    cold.MonitorSet(lambda its, nconv, er, ei, ee: seen.append((its, nconv, len(er))))
    cold.Solve()
    _check_against(cold, 6, LAP_EIG, LAP_NORM, 1e-8)
    its = [s[0] for s in seen]
    st = cold.LOBPCGGetStats()
    assert its == sorted(its)
    assert len(its) == st["iterations"] - (st["hard_locks"] + 1)      # every pass of the loop but the first of each block (`if (its)`, lobpcg.c:205); a hard lock repeats a number (its - 1, :215)
    assert all(b[1] >= a[1] for a, b in zip(seen, seen[1:]))                          # nconv never goes down
    warm = _lobpcg(ctx, A, nev=6, bs=4, tol=1e-8); warm.SetRandomSeed(77)
    warm.SetInitialSpace(Q[:, :6] + 1e-3 * np.random.default_rng(8).standard_normal((108, 6)))
    warm.Solve()
    _check_against(warm, 6, LAP_EIG, LAP_NORM, 1e-8)
    assert warm.GetIterationNumber() < cold.GetIterationNumber(), (warm.GetIterationNumber(), cold.GetIterationNumber())
    stop = _lobpcg(ctx, A, nev=6, bs=4, tol=1e-8)
    stop.SetStoppingTestFunction(lambda its, max_it, nconv, nev: ks.EPS_CONVERGED_USER if its >= 3 else 0)
    stop.Solve()
    assert stop.GetConvergedReason() == ks.EPS_CONVERGED_USER and stop.GetIterationNumber() == 3


# ---- 9: errors ----------------------------------------------------------------------------------------------------------------------------
def _rc(eps):
    import slepc_amd as ks
    try:
        eps.Solve()
    except ks.KsError as e:
        return e.rc
    return 0


def test_setup_errors(ctx):
    import slepc_amd as ks
    A = _mat(ctx, LAP)
    e = _lobpcg(ctx, A, nev=2, ptype=ks.EPS_NHEP); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=2, which="largest_magnitude"); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=2, which="target_real"); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=2); e.SetArbitrarySelection(lambda re, im, xr, xi: (re, im)); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=2); e.SetExtraction("harmonic"); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=2); e.SetTwoSided(True); assert _rc(e) == SUP
    small = _mat(ctx, sc.tridiag_csr(19, -1.0, 2.0, -1.0))
    e = _lobpcg(ctx, small, nev=4, bs=4); assert _rc(e) == SUP                        # 19 < 5 * 4
    e = _lobpcg(ctx, _mat(ctx, sc.tridiag_csr(21, -1.0, 2.0, -1.0)), nev=4, bs=4)     # 21 - 2 constraints < 20
    e.SetDeflationSpace(np.eye(21)[:, :2]); assert _rc(e) == SUP
    e = _lobpcg(ctx, A, nev=6, bs=4); e.SetDimensions(6, 15); assert _rc(e) == USER_INPUT      # max(12, (5 // 4 + 3) * 4) = 16
    e = _lobpcg(ctx, A, nev=6, bs=4); e.SetDimensions(6, 16); assert _rc(e) == 0
    e = _lobpcg(ctx, A, nev=6, bs=4); e.SetDimensions(6, 0, 11); assert _rc(e) == USER_INPUT
    e = _lobpcg(ctx, A, nev=6, bs=4); e.SetDimensions(6, 0, 12); assert _rc(e) == 0
    e = _lobpcg(ctx, A, nev=2)
    with pytest.raises(ks.KsError) as ex:
        e.LOBPCGSetBlockSize(17)
    assert ex.value.rc == OUTOFRANGE
    with pytest.raises(ks.KsError) as ex:
        e.LOBPCGSetRestart(0.05)
    assert ex.value.rc == OUTOFRANGE
    e = _lobpcg(ctx, A, nev=2, max_it=0); e.SetBalance("oneside"); assert _rc(e) == 0           # balancing is ignored; max_it left to the default
    assert e.GetTolerances()[1] == max(100, 2 * 108 // 6)                             # nev 2: bs 2, ncv 6


def test_krylovschur_refuses_precond_and_is_unchanged_by_a_type_round_trip(ctx):
    import slepc_amd as ks
    S = sc.laplacian2d_csr(13, 11)
    A = _mat(ctx, S)

    def ks_solve(prepare):
        eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(4, 20)
        prepare(eps)
        eps.Solve()
        return [eps.GetEigenvalue(i) for i in range(eps.GetConverged())], eps.GetIterationNumber(), eps.GetStats()

    plain = ks_solve(lambda eps: None)
    back = ks_solve(lambda eps: (eps.SetType("lobpcg"), eps.SetType("krylovschur")))
    assert plain == back and len(plain[0]) >= 4
    eps = ks.EPS(ctx); eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(2)
    eps.GetST().SetType("precond")
    assert _rc(eps) == SUP
    assert eps.GetType() == "krylovschur"


# ---- 10: two ranks -----------------------------------------------------------------------------------------------------------------------
def test_two_ranks(ctx):
    import slepc_amd as ks
    S = sc.tridiag_csr(30, -1.0, 2.0, -1.0)
    split = [(0, 16), (16, 30)]

    def rank_fn(rank, comm):
        c = ks.Context(0)
        comm.install(c, rank)
        s0, s1 = split[rank]
        A = _mat(c, S[s0:s1], row_start=s0, n_global=30)
        eps = _test24(c, A, rows=slice(s0, s1))
        out = (["%.5f" % v for v in _values(eps, 4)], eps.GetIterationNumber(), eps.GetConverged())
        del eps
        A.destroy(); c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    ref = ["%.5f" % v for v in gi.eigenvalues_line(gi.read("eps/eps_test24_1.out"))]
    assert res[0][0] == ref and res[1][0] == ref
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
