"""KS_KSP_CG, the conjugate-gradient inner solver of the ST, on one rank against the numpy restatement of tests/cg_cases.py.

The iteration counts are exact: on the kron systems CG ends at iteration m whatever the rounding (the residual falls from above 1.6e-6 to below
3.1e-17 there), on the lap systems the tolerance sits in the middle of a factor-of-two step of the reference history (cg_cases.pick_k). The true
preconditioned residual of the returned iterate may exceed the tolerance by the distance between the recursive and the true residual; the bound is
tol + 8 g with g that distance as the restatement measured it on the same case (the "8 times the CPU-measured distance" of test_gpu_bv_ranks.py)."""
import math

import numpy as np
import pytest

import cg_cases as cc
import golden_inputs as gi
import scenarios as sc
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _mat(ctx, S, keep=True):
    import slepc_amd as ks
    S = S.tocsr(); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep)


def _csr(S):
    S = S.tocsr(); S.sort_indices()
    return O.CSR(S.shape[0], S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))


def _sinvert(ctx, case, sigma, pc, mode="shell", rtol=1e-8, block=0, check=None):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(_mat(ctx, case.P)); st.SetMatMode(mode)
    st.SetKSPType("cg"); st.SetPC(pc, block); st.SetKSP(rtol=rtol)
    if check is not None:
        st.CGSetCheckInterval(check)
    return st


def _check_solve(st, P, b, ref, minv):
    y = st.Apply(b)
    stats = st.GetKSPStats()
    res = float(np.linalg.norm(minv(b - P @ y)))
    print("its %d (reference %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e" % (stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, ref.gap))
    assert stats["solves"] == 1 and stats["iterations"] == ref.its
    assert stats["last_rnorm"] <= ref.tol
    assert res <= ref.tol + 8 * ref.gap
    return y


# ---- 1: counts and solutions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shell", "copy"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("idx", range(len(cc.KRON)))
def test_kron_counts_and_solutions(ctx, idx, pc, mode):
    """m distinct eigenvalues: the count is m; n = 1057, 1027 and 513 have the scalar tail, n = 512 is one tile exactly."""
    case, ref = cc.kron_reference(idx, pc)
    st = _sinvert(ctx, case, 0.0, pc, mode)
    minv = cc.jacobi(case.P) if pc == "jacobi" else (lambda r: r)
    y = _check_solve(st, case.P, case.b, ref, minv)
    dense = case.P.toarray()
    assert np.linalg.cond(dense) < 30
    assert np.linalg.norm(y - np.linalg.solve(dense, case.b)) <= 1e-12 * np.linalg.norm(y)


@pytest.mark.parametrize("near", [1e-8, 1e-12])
@pytest.mark.parametrize("mode", ["shell", "copy"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("sigma", [0.0, -0.5])
@pytest.mark.parametrize("idx", range(len(cc.LAP)))
def test_lap_counts_and_solutions(ctx, idx, sigma, pc, mode, near):
    """Several batches of the default check interval; sigma = -0.5 in shell mode forms w = A p + 0.5 p inside the (p,w) sweep."""
    case, P, rtol, ref, k = cc.lap_reference(idx, pc, sigma, near)
    st = _sinvert(ctx, case, sigma, pc, mode, rtol=rtol)
    _check_solve(st, P, case.b, ref, cc.jacobi(P) if pc == "jacobi" else (lambda r: r))


# ---- 2: gating ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kron", "lap"])
def test_check_interval_changes_no_bit(ctx, which):
    if which == "kron":
        case, ref = cc.kron_reference(1, "jacobi"); P, rtol, sigma = case.P, 1e-8, 0.0
    else:
        case, P, rtol, ref, _ = cc.lap_reference(0, "jacobi", -0.5, 1e-8); sigma = -0.5
    out = {}
    for c in (1, 3, 8, 64):
        st = _sinvert(ctx, case, sigma, "jacobi", rtol=rtol, check=c)
        assert st.CGGetCheckInterval() == c
        y = st.Apply(case.b)
        ksp, cg = st.GetKSPStats(), st.GetCGStats()
        print("c %d: its %d, %s" % (c, ksp["iterations"], cg))
        assert ksp["iterations"] == ref.its
        assert cg["host_waits"] <= math.ceil(ref.its / c) + 2
        assert cg["sweeps"] >= 3 * ref.its
        y2 = st.Apply(case.b)                                    # the same solve again: the same bits
        ksp2, cg2 = st.GetKSPStats(), st.GetCGStats()
        assert np.array_equal(y, y2) and ksp2["iterations"] == 2 * ref.its and ksp2["last_rnorm"] == ksp["last_rnorm"]
        assert cg2["host_waits"] - cg["host_waits"] <= math.ceil(ref.its / c) + 2
        out[c] = (y, ksp["iterations"], ksp["last_rnorm"], cg)
    for c in (3, 8, 64):
        assert np.array_equal(out[c][0], out[1][0]) and out[c][1] == out[1][1] and out[c][2] == out[1][2]
    assert out[64][3]["gated_iterations"] > 0
    assert out[1][3]["gated_iterations"] == 0


def test_default_check_interval(ctx):
    import slepc_amd as ks
    assert ks.ST(ctx).CGGetCheckInterval() == 8


# ---- 3: the preconditioners with kernels of their own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,block", [("bjacobi", 8), ("bjacobi-ilu", 64), ("lu", 0), ("amg", 0)])
def test_block_preconditioners(ctx, pc, block):
    """The update sweep stops after r, the preconditioner's own application makes z, a two-dot sweep follows. M^-1 of the restatement and of the
    residual is ST.PCApply (existing code, not under test here)."""
    case = cc.lap(*cc.LAP[0])
    st = _sinvert(ctx, case, 0.0, pc, block=block)
    st.SetUp()
    ref = cc.cg_reference(case.P, case.b, st.PCApply, rtol=1e-8)
    assert ref.reason == "converged"
    y = st.Apply(case.b)
    stats = st.GetKSPStats()
    res = float(np.linalg.norm(st.PCApply(case.b - case.P @ y)))
    print("%s: its %d (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e" % (pc, stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, ref.gap))
    assert stats["solves"] == 1 and stats["last_rnorm"] <= ref.tol
    assert res <= ref.tol + 8 * ref.gap
    if pc == "lu":
        assert stats["iterations"] == 1
    if pc == "amg":
        assert stats["iterations"] <= cc.cg_reference(case.P, case.b, cc.jacobi(case.P), rtol=1e-8).its


# ---- 3b: a misaligned solution vector ---------------------------------------------------------------------------------------------------------------
def _apply_unaligned(ctx, st, b):
    """st.Apply(b) with y eight bytes past a 16-byte boundary, in a BV of n + 1 rows; the row in front of y is checked untouched"""
    import ctypes as C
    import slepc_amd as ks
    n = len(b)
    W = ks.BV(ctx, n + 1, 2)
    W.set_column(0, np.concatenate([b, [0.0]])); W.set_column(1, np.full(n + 1, 7.0))
    assert W.column_ptr(1) % 16 == 0
    ks._lib.check(ctx.L.ks_st_apply(st.h, C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1) + 8)))
    full = W.column(1)
    assert full[0] == 7.0
    return full[1:]


UNALIGNED = [("kron", pc, mode) for pc in ("jacobi", "none") for mode in ("shell", "copy")] + [("lap", "jacobi", "shell"), ("lap", "bjacobi", "shell")]


@pytest.mark.parametrize("which,pc,mode", UNALIGNED)
def test_unaligned_solution_vector_takes_the_one_row_sweeps(ctx, which, pc, mode):
    """y eight bytes past a 16-byte boundary: every sweep runs its one-row-per-lane form. Counts and bounds of the aligned tests. kron: n = 513, two
    tiles of the one-row form and a row; lap with Jacobi at sigma = -0.5 in shell mode: the combining (p,w) sweep; lap with blocks of 8: the update
    that ends after r and the dot sweep. M^-1 of that restatement and of the residual is ST.PCApply, as in test_block_preconditioners; its count of
    17 is exact too: the history passes 1e-8 between 2.89e-8 and 9.59e-9, 4 % below the tolerance, where the pair form and the one-row form of the
    device differ in the thirteenth digit."""
    if pc == "bjacobi":
        case = cc.lap(*cc.LAP[0]); P = case.P
        st = _sinvert(ctx, case, 0.0, pc, block=8)
        st.SetUp()
        minv = st.PCApply
        ref = cc.cg_reference(P, case.b, minv, rtol=1e-8)
        assert ref.reason == "converged" and ref.its == 17 and ref.hist[16] > 2e-8 and ref.hist[17] < 0.97e-8
    elif which == "lap":
        case, P, rtol, ref, _ = cc.lap_reference(0, pc, -0.5, 1e-8)
        st = _sinvert(ctx, case, -0.5, pc, mode, rtol=rtol)
        minv = cc.jacobi(P)
    else:
        case, ref = cc.kron_reference(3, pc); P = case.P
        assert case.n == 513
        st = _sinvert(ctx, case, 0.0, pc, mode)
        minv = cc.jacobi(P) if pc == "jacobi" else (lambda r: r)
    y = _apply_unaligned(ctx, st, case.b)
    stats = st.GetKSPStats()
    res = float(np.linalg.norm(minv(case.b - P @ y)))
    print("its %d (reference %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e" % (stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, ref.gap))
    assert stats["solves"] == 1 and stats["iterations"] == ref.its
    assert stats["last_rnorm"] <= ref.tol
    assert res <= ref.tol + 8 * ref.gap


# ---- 4: the other transformations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sigma", [("shift", 0.3), ("cayley", -0.7)])
@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_shift_and_cayley_match_the_oracle(ctx, kind, sigma, mode):
    """B^-1 solves of a shift with two matrices, and Cayley with the shift below the spectrum (A - sigma B positive definite; in shell mode the (p,w)
    sweep forms w = A p - sigma B p): the bound and inner tolerance of test_bicgstab_inner_solver_matches_oracle."""
    import slepc_amd as ks
    A, B = sc.test32_pencil(18)
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType("cg"); st.SetKSP(rtol=1e-14)
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    y = st.Apply(x); y0 = O.ST(_csr(A), _csr(B), kind, sigma).apply(x)
    print("%s %s: %.3e" % (kind, mode, np.linalg.norm(y - y0) / np.linalg.norm(y0)))
    assert np.linalg.norm(y - y0) <= 1e-10 * np.linalg.norm(y0)
    assert st.GetKSPStats()["solves"] == 1 and st.GetKSPStats()["iterations"] > 0


@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_transposed_solve_is_the_forward_solve(ctx, mode):
    import slepc_amd as ks
    A, B = sc.test32_pencil(18)
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(-0.7); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType("cg"); st.SetKSP(rtol=1e-14)
    st.SetTransposeSolves(True)
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    yt = st.MatSolveTranspose(b)
    y0 = np.linalg.solve((A + 0.7 * B).toarray(), b)
    assert np.linalg.norm(yt - y0) <= 1e-10 * np.linalg.norm(y0)
    st1 = ks.ST(ctx)
    st1.SetType("sinvert"); st1.SetShift(-0.7); st1.SetMatrices(_mat(ctx, A)); st1.SetMatMode(mode); st1.SetKSPType("cg"); st1.SetKSP(rtol=1e-14)
    st1.SetTransposeSolves(True)
    yf = st1.Apply(b)                                  # one matrix: STApply is the forward solve itself
    assert np.linalg.norm(st1.MatSolveTranspose(b) - yf) <= 1e-10 * np.linalg.norm(yf)


# ---- 5: errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_way_back_to_gmres(ctx):
    import slepc_amd as ks
    from slepc_amd import _lib
    case = cc.lap(*cc.LAP[0])
    lam = np.linalg.eigvalsh(case.P.toarray())
    st = _sinvert(ctx, case, 0.5 * (lam[3] + lam[4]), "none")              # the shift inside the spectrum: A - sigma I is indefinite
    with pytest.raises(ks.KsError) as e:
        st.Apply(case.b)
    assert e.value.rc == 91 and "indefinite" in str(e.value) and "indefinite" in _lib.lib().ks_last_error_message().decode()
    st = _sinvert(ctx, case, 0.0, "jacobi")
    st.SetKSP(max_it=2)
    with pytest.raises(ks.KsError) as e:
        st.Apply(case.b)
    assert e.value.rc == 91 and "reached 2 iterations" in str(e.value)
    assert st.GetKSPStats()["iterations"] == 2
    assert ctx.L.ks_st_set_ksp_type(st.h, 3) == 56 and ctx.L.ks_st_set_ksp_type(st.h, 5) == 56 and ctx.L.ks_st_set_ksp_type(st.h, -1) == 56      # KS_KSP_CG is 4; 3 names nothing
    before = st.CGGetCheckInterval()
    assert ctx.L.ks_st_cg_set_check_interval(st.h, 0) == 63 and ctx.L.ks_st_cg_set_check_interval(st.h, 1025) == 63
    assert st.CGGetCheckInterval() == before == 8                                 # a refused value leaves the interval alone
    assert ctx.L.ks_st_cg_set_check_interval(st.h, 1) == 0 and st.CGGetCheckInterval() == 1
    assert ctx.L.ks_st_cg_set_check_interval(st.h, 1024) == 0 and st.CGGetCheckInterval() == 1024
    # a zero right-hand side: y = 0 and no iteration
    st = _sinvert(ctx, case, 0.0, "jacobi")
    y = st.Apply(np.zeros(case.n))
    assert not y.any() and st.GetKSPStats() == {"solves": 1, "iterations": 0, "last_rnorm": 0.0}
    # GMRES before and after a CG solve on the same ST: the same bits
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(_mat(ctx, case.P))
    g1 = st.Apply(case.b)
    st.SetKSPType("cg")
    c1 = st.Apply(case.b)
    st.SetKSPType("gmres")
    g2 = st.Apply(case.b)
    assert np.array_equal(g1, g2)
    assert np.linalg.norm(c1 - g1) <= 1e-6 * np.linalg.norm(g1) and st.GetCGStats()["sweeps"] > 0


def test_jacobi_davidson_refuses_cg(ctx):
    import slepc_amd as ks
    case = cc.lap(*cc.LAP[0])
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, case.P)); eps.SetProblemType(ks.EPS_HEP); eps.SetType("jd"); eps.SetDimensions(2)
    eps.GetST().SetKSPType("cg")
    with pytest.raises(ks.KsError) as e:
        eps.Solve()
    assert e.value.rc == 56 and "KSPCG" in str(e.value)


# ---- 6: whole solves ------------------------------------------------------------------------------------------------------------------------------
def test_eps_ex11_suffix_2_golden(ctx):
    """ex11 -eps_nev 4 -eps_ncv 20 -eps_target 0 -st_type sinvert -st_ksp_type cg -st_pc_type jacobi: the Fiedler vector problem of
    test_eps_ex11_fiedler_restart_parameter_golden with its deflation space, the inner solves by CG. The graph Laplacian is singular; the
    right-hand sides are orthogonal to its null space, the constant vector, which is deflated."""
    import slepc_amd as ks
    S = sc.graph_laplacian_2d(10, 10)
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, S)); eps.SetProblemType(ks.EPS_HEP); eps.SetWhichEigenpairs("smallest_real"); eps.SetDimensions(4, 20)
    eps.SetDeflationSpace(np.ones((100, 1))); eps.SetTarget(0.0); eps.SetWhichEigenpairs("target_magnitude")      # what -eps_target selects
    st = eps.GetST(); st.SetType("sinvert"); st.SetKSPType("cg"); st.SetPC("jacobi")
    eps.Solve()
    assert eps.GetConverged() >= 4
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    print(lam, st.GetKSPStats(), st.GetCGStats())
    assert np.allclose(np.round(lam[:4], 5), gi.eigenvalue_lines(gi.read("eps/ex11_1.out"))[0], atol=1.5e-5)
    assert st.GetKSPStats()["solves"] > 0 and st.GetCGStats()["sweeps"] > 0


def test_ghep_shift_with_cg_matches_gmres(ctx):
    """test32's pencil (B symmetric positive definite, not diagonal) under KS_ST_SHIFT: the B^-1 solves by CG give the eigenvalues of the GMRES run to
    the bound of test_config5_with_bicgstab."""
    import slepc_amd as ks
    A, B = sc.test32_pencil(18)
    lam = {}
    for ksp in ("gmres", "cg"):
        eps = ks.EPS(ctx)
        eps.SetOperators(_mat(ctx, A), _mat(ctx, B)); eps.SetProblemType(ks.EPS_GHEP); eps.SetDimensions(4, 24)
        st = eps.GetST(); st.SetKSPType(ksp); st.SetKSP(rtol=1e-13)
        eps.Solve()
        assert eps.GetConverged() >= 4
        lam[ksp] = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam["cg"], lam["gmres"], rtol=1e-9)
