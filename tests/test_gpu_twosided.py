"""Two-sided Krylov-Schur on the GPU (EPSSetTwoSided: right and left eigenvectors of non-symmetric problems) and the transposed operator view it
expands the left basis with.

References: the reference's golden outputs for -eps_two_sided runs (ex5_1, ex9_1, test9_7_real, the value column of ex41_1), exact eigenvalues
(convection-diffusion), the CPU restatement of tests/twosided_cases.py for integer control flow, and residuals computed on the host with scipy
from the returned vectors. Bounds: relative residuals below the solver tolerance 1e-8; |y_i^T x_j| <= (||r_i|| + ||r_j||) / |k_i - k_j| (from
y_i^T A x_j evaluated on both sides, unit vectors) plus 64 eps for the rounding of the product itself; |k - exact| <= 10 ||r|| / |y^T x|, the
first-order perturbation bound with a factor 10 for the second-order term."""
import numpy as np
import pytest

import golden_inputs as gi
import nhep_cases as nc
import twosided_cases as TS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-8
EPS = np.finfo(float).eps


def _solve(ctx, Ao, nev=4, which="largest_real", lock=True, v0=None, w0=None, sigma=None, keep_csr=True, twosided=True):
    import slepc_amd as ks
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=keep_csr)
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(nev)
    if which is not None:
        eps.SetWhichEigenpairs(which)
    eps.KrylovSchurSetLocking(lock); eps.SetTwoSided(twosided)
    if v0 is not None:
        eps.SetInitialSpace(v0[:, None])
    if w0 is not None:
        eps.SetLeftInitialSpace(w0[:, None])
    if sigma is not None:
        st = eps.GetST(); st.SetType("shift"); st.SetShift(sigma)
    eps.Solve()
    return eps, A


def _pairs(eps, S, n):
    """(k, x, y, right residual, left residual) for the first n pairs, complex vectors; the residuals by ex41's formulas (TS.residuals)"""
    out = []
    for i in range(n):
        kr, ki, xr, xi = eps.GetEigenpair(i)
        yr, yi = eps.GetLeftEigenvector(i)
        rr = TS.residuals(S, kr, ki, xr, xi); rl = TS.residuals(S, kr, ki, yr, yi, left=True)
        out.append((complex(kr, ki), xr + 1j * xi, yr + 1j * yi, rr, rl))
    return out


def _check_pairs(eps, S, n, record):
    """both residuals below tol (relative), ComputeError their maximum, unit vectors, biorthogonality within what the residuals allow"""
    P = _pairs(eps, S, n)
    for i, (k, x, y, rr, rl) in enumerate(P):
        record.append((rr / abs(k), rl / abs(k)))
        print("pair %d: k = %r, right %.2e, left %.2e (relative)" % (i, k, rr / abs(k), rl / abs(k)))
        assert rr / abs(k) < TOL and rl / abs(k) < TOL
        assert abs(np.linalg.norm(x) - 1.0) < 1e-12 and abs(np.linalg.norm(y) - 1.0) < 1e-12
        err = eps.ComputeError(i)
        assert abs(err - max(rr, rl) / abs(k)) <= 1e-12 + 1e-6 * err, (err, rr, rl)
    for i, (ki_, _, y, _, rli) in enumerate(P):
        for j, (kj, x, _, rrj, _) in enumerate(P):
            if abs(ki_ - kj) > 1e-6:                               # (a pair's own second member has the same k: that is y^H x, not an off-diagonal term)
                assert abs(np.vdot(y, x)) <= (rli + rrj) / abs(ki_ - kj) + 64 * EPS, (i, j)
    return P


@pytest.mark.parametrize("lock", [1, 0])
def test_markov_largest_real_both_sides(ctx, lock):
    """ex5 -eps_two_sided 1 (ex5.c's test block loops over {{0 1}}, one output file)"""
    Ao = O.markov_matrix(15); S = Ao.to_scipy()
    eps, _ = _solve(ctx, Ao, lock=bool(lock))
    assert eps.GetTwoSided() and eps.GetConverged() >= 4 and eps.GetConvergedReason() == 1
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.array_equal(np.round(lam, 5), gi.eigenvalues_line(gi.read("eps/ex5_1.out")))
    rec = []
    _check_pairs(eps, S, 4, rec)
    print("markov largest_real lock=%d: restarts %d, steps %d, max residual %.2e" % (lock, eps.GetIterationNumber(), eps.GetStats()["arnoldi_steps"], np.max(rec)))


def test_brusselator_conjugate_pairs(ctx):
    """ex9 -eps_two_sided 1: both members of each pair, (yr, yi) with y^H A = k y^H"""
    Ao = nc.brusselator(50); S = Ao.to_scipy()
    eps, _ = _solve(ctx, Ao)
    assert eps.GetConverged() >= 4
    lam = np.array([complex(*eps.GetEigenvalue(i)) for i in range(4)])
    gold = gi.complex_eigenvalue_lines(gi.read("eps/ex9_1.out"))[0]
    assert np.allclose(np.round(lam, 5), gold, atol=1.5e-5)
    assert lam[0].imag > 0 and lam[1] == lam[0].conjugate() and lam[3] == lam[2].conjugate()
    rec = []
    P = _check_pairs(eps, S, 4, rec)
    assert np.array_equal(P[1][2], P[0][2].conjugate()) and np.array_equal(P[1][1], P[0][1].conjugate())     # second member: (xr, -xi), (yr, -yi)
    print("brusselator: restarts %d, steps %d, max residual %.2e" % (eps.GetIterationNumber(), eps.GetStats()["arnoldi_steps"], np.max(rec)))


def test_markov_largest_magnitude_permutes_the_left_half(ctx):
    """test9 -eps_two_sided (default which): 1 / -1 and 0.97137 / -0.97137 tie in modulus, so the two projected halves come out of their sorts in
    different orders and DS NHEPTS has to permute the second one"""
    Ao = O.markov_matrix(15); S = Ao.to_scipy()
    eps, _ = _solve(ctx, Ao, which=None)
    assert eps.GetConverged() >= 4
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    gold = gi.eigenvalues_line(gi.read("eps/eps_test9_7_real.out"))          # 1, -1, 0.97137, -0.97137: which of two values of equal modulus comes first is rounding
    assert np.array_equal(np.sort(np.round(lam, 5)), np.sort(gold)) and np.array_equal(np.abs(np.round(lam, 5)), np.abs(gold))
    rec = []
    _check_pairs(eps, S, 4, rec)
    perms = eps.GetTwoSidedStats()["ds_permutations"]
    print("markov largest magnitude: restarts %d, permuted sorts %d, max residual %.2e" % (eps.GetIterationNumber(), perms, np.max(rec)))
    assert perms >= 1


@pytest.mark.parametrize("sigma", [None, 0.3])
def test_fixed_start_vectors_follow_the_restatement(ctx, sigma):
    """ex41's start vectors (v0 = e0 + e1 + e2, w0 = 2 e0 + 0.5 e2); with sigma the expansion runs through the ST's shell operator and its
    transposed view. Restarts, converged pairs and steps are the restatement's (its estimates stay clear of tol: test_ds_twosided_host.py)"""
    Ao = O.markov_matrix(15); S = Ao.to_scipy()
    v0, w0 = TS.ex41_start_vectors(Ao.n)
    r = TS.eps_krylovschur_twosided(Ao, 4, which="largest_real", v0=v0, w0=w0, sigma=sigma or 0.0)
    eps, _ = _solve(ctx, Ao, v0=v0, w0=w0, sigma=sigma)
    st = eps.GetStats()
    print("ex41 start vectors, sigma %s: restarts %d (restatement %d), nconv %d (%d), steps %d (%d), passes %d (%d)"
          % (sigma, eps.GetIterationNumber(), r.its, eps.GetConverged(), r.nconv, st["arnoldi_steps"], r.steps, st["gs_passes"], r.passes))
    assert (eps.GetIterationNumber(), eps.GetConverged(), st["arnoldi_steps"]) == (r.its, r.nconv, r.steps)
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(r.nconv)])
    assert np.abs(lam - r.eigr[r.perm]).max() <= 1e-10 * np.abs(lam).max()
    assert np.allclose(lam[:4], gi.table_first_column(gi.read("eps/ex41_1.out"))[:4], atol=0.6e-6)      # printed with 6 decimals
    _check_pairs(eps, S, 4, [])


def test_convection_diffusion_first_order_bound(ctx, monkeypatch):
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    Ao, exact = TS.convection_diffusion(32); S = Ao.to_scipy()
    eps, A = _solve(ctx, Ao)
    assert A.layout() == "dict" and A.transpose_view().layout() == "dict"
    assert eps.GetConverged() >= 4
    rec = []
    P = _check_pairs(eps, S, 4, rec)
    for i, (k, x, y, rr, rl) in enumerate(P):
        assert k.imag == 0.0
        s = abs(np.vdot(y, x))
        print("convection-diffusion %d: |k - exact| %.2e, bound %.2e, |y^T x| %.3f" % (i, abs(k.real - exact[i]), 10 * max(rr, rl) / s, s))
        assert abs(k.real - exact[i]) <= 10 * max(rr, rl) / s
    print("convection-diffusion: restarts %d, max residual %.2e" % (eps.GetIterationNumber(), np.max(rec)))


@pytest.mark.parametrize("case", ["markov", "ragged"])
def test_transposed_view_is_the_transposed_product_bit_for_bit(ctx, case, monkeypatch):
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    Ao = O.markov_matrix(15) if case == "markov" else TS.ragged_nonsymmetric()
    n = Ao.n
    if case == "ragged":
        assert np.diff(Ao.rowptr).max() > 16 and np.diff(Ao.rowptr).min() < 4
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)
    At = A.transpose_view()
    x = np.random.default_rng(3).standard_normal(n)
    St = Ao.to_scipy().T.tocsr(); St.sort_indices()
    y = At.mult(x)
    assert np.array_equal(y, A.mult_transpose(x))
    assert np.linalg.norm(y - St @ x) <= 64 * EPS * np.linalg.norm(St @ x) * np.sqrt(40)
    assert np.array_equal(At.mult_transpose(x), A.mult(x))                     # and the view's transposed product is the matrix itself
    assert np.array_equal(At.transpose_view().mult(x), A.mult(x))
    # the same Arnoldi run on the view and on a matrix assembled from S^T: same layout, same kernels, same bits
    B = ks.Mat.from_csr(ctx, St.indptr.astype(np.int32), St.indices.astype(np.int32), St.data)
    assert B.layout() == At.layout()
    m = 12
    H = []
    for M in (At, B):
        V = ks.BV(ctx, n, m + 1)
        V.set_column(0, x / np.linalg.norm(x))
        Hm = np.zeros((m + 1, m), order="F")
        mm, beta, brk = V.MatArnoldi(M, Hm, 0, m)
        assert mm == m and not brk
        H.append((Hm, beta, V.dense()))
    assert np.array_equal(H[0][0], H[1][0]) and H[0][1] == H[1][1] and np.array_equal(H[0][2], H[1][2])
    # a shell matrix: the view is a shell over the transposed callback
    Sh = ks.Mat.shell(ctx, n, lambda xp, yp: A.mult_dev(xp, yp))
    with pytest.raises(ks.KsError) as e:
        Sh.transpose_view()
    assert e.value.rc == 56
    Sh.shell_set_mult_transpose(lambda xp, yp: A.mult_transpose_dev(xp, yp))
    Tv = Sh.transpose_view()
    assert Tv.layout() == "shell" and np.array_equal(Tv.mult(x), y) and np.array_equal(Tv.mult_transpose(x), A.mult(x))
    # without the kept CSR arrays there is nothing to transpose
    with pytest.raises(ks.KsError) as e:
        ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val).transpose_view()
    assert e.value.rc == 58


def _refused(eps):
    import slepc_amd as ks
    with pytest.raises(ks.KsError) as e:
        eps.Solve()
    return e.value.rc


def test_refusals_and_trivial_left_vectors(ctx):
    import slepc_amd as ks
    Ao = O.markov_matrix(15)
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)

    def new(M=A, B=None, ptype=ks.EPS_NHEP):
        eps = ks.EPS(ctx); eps.SetOperators(M, B); eps.SetProblemType(ptype); eps.SetDimensions(4); eps.SetWhichEigenpairs("largest_real"); eps.SetTwoSided(True)
        return eps
    Lo = O.laplacian2d(8)
    Lm = ks.Mat.from_csr(ctx, Lo.rowptr, Lo.col, Lo.val, keep_csr=True)
    assert _refused(new(Lm, ptype=ks.EPS_HEP)) == 56                           # Hermitian problem
    Bo = O.laplacian1d(Ao.n)
    Bm = ks.Mat.from_csr(ctx, Bo.rowptr, Bo.col, Bo.val, keep_csr=True)
    assert _refused(new(A, Bm, ks.EPS_GNHEP)) == 56                            # a B matrix
    assert _refused(new(Lm, Lm, ks.EPS_GHEP)) == 56
    for kind in ("sinvert", "cayley"):                                          # an ST with a solve
        eps = new(); eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(1.1)
        st = eps.GetST(); st.SetType(kind); st.SetShift(1.1)
        assert _refused(eps) == 56
    eps = new(); eps.SetBalance("oneside"); assert _refused(eps) == 56
    eps = new(); eps.SetExtraction("harmonic"); assert _refused(eps) == 56
    eps = new(); eps.SetTrueResidual(True); assert _refused(eps) == 56
    eps = new(); eps.SetDeflationSpace(np.ones((Ao.n, 1))); assert _refused(eps) == 56
    # an operator without a transposed product fails at set-up, with the code of the missing piece
    assert _refused(new(ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val))) == 58
    assert _refused(new(ks.Mat.shell(ctx, Ao.n, lambda xp, yp: A.mult_dev(xp, yp)))) == 56
    # without the flag: a non-symmetric solve has no left vectors, a symmetric one returns the right ones
    eps = new(); eps.SetTwoSided(False); eps.Solve()
    with pytest.raises(ks.KsError) as e:
        eps.GetLeftEigenvector(0)
    assert e.value.rc == 73
    eps = ks.EPS(ctx); eps.SetOperators(Lm); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(3); eps.Solve()
    for i in range(3):
        yr, yi = eps.GetLeftEigenvector(i)
        assert np.array_equal(yr, eps.GetEigenvector(i)) and not yi.any()


def test_more_than_one_rank_is_refused():
    import slepc_amd as ks
    from thread_comm import ThreadComm, run_ranks

    def body(rank, comm):
        c = ks.Context(0)
        try:
            comm.install(c, rank)
            A = ks.Mat.laplacian3d(c, 4, 4, 4, z0=2 * rank, nz_local=2)
            eps = ks.EPS(c); eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(2); eps.SetTwoSided(True)
            rc = _refused(eps)
            eps.destroy(); A.destroy()
            return rc
        finally:
            c.close()
    assert run_ranks(ThreadComm(2), body) == [56, 56]
