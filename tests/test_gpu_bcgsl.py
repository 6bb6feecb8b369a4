"""KS_KSP_BCGSL, the BiCGStab(l) inner solver of the ST, on one rank against the numpy restatement of tests/bcgsl_cases.py.

The counts on the I (x) T systems are exact: BiCG ends at step m, BiCGStab(l) at m rounded up to a multiple of l, whatever the rounding
(tests/test_bcgsl_cases_host.py: the residual falls from above 100 tol to below tol / 100 there in every summation order). On the convection-diffusion
systems the count moves with the summation order and is not pinned: convergence within twice the restatement's count is. The true preconditioned
residual of the returned iterate may exceed the tolerance by the distance between the recursive and the true residual; the bound is tol + 8 g with g that
distance as the restatement measured it on the same case (the rule of tests/test_gpu_cg.py).

A solve that converges after k cycles is found converged by the first sweep of cycle k + 1, so k + 1 cycles run: the host reads the state
ceil((k + 1) / c) times and c ceil((k + 1) / c) - (k + 1) enqueued cycles find the solve ended."""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import bcgsl_cases as bc
import cg_cases as cc

pytestmark = pytest.mark.gpu


def _mat(ctx, S, keep=True):
    import slepc_amd as ks
    S = sp.csr_matrix(S); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep)


def _sinvert(ctx, A, sigma, pc, ell, mode="shell", rtol=1e-8, block=0, check=None, max_it=None):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A)); st.SetMatMode(mode)
    st.SetKSPType("bcgsl"); st.BCGSLSetEll(ell); st.SetPC(pc, block); st.SetKSP(rtol=rtol)
    if max_it:
        st.SetKSP(max_it=max_it)
    if check is not None:
        st.BCGSLSetCheckInterval(check)
    return st


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


def _bounds(st, y, P, b, ref, minv, its=None):
    stats = st.GetKSPStats()
    res = float(np.linalg.norm(minv(b - P @ y)))
    dist = float(np.linalg.norm(minv(P @ (y - ref.y))))
    print("its %d (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, M^-1 P (y - y_ref) %.3e, gap %.2e, %s"
          % (stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, dist, ref.gap, st.GetBCGSLStats()))
    assert stats["solves"] == 1 and stats["last_rnorm"] <= ref.tol
    if its is not None:
        assert stats["iterations"] == its
    assert res <= ref.tol + 8 * ref.gap
    return stats, dist


# ---- 1: pinned counts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shell", "copy"])
@pytest.mark.parametrize("ell", [1, 2, 3, 4])
@pytest.mark.parametrize("idx", range(len(bc.KRON)))
def test_kron_counts_and_solutions(ctx, idx, ell, mode):
    case, pc, ref = bc.kron_reference(idx, ell)
    assert ref.reason == "converged" and ref.its == bc.kron_count(idx, ell)
    st = _sinvert(ctx, case.P, 0.0, pc, ell, mode, rtol=1e-12)
    assert st.BCGSLGetEll() == ell
    minv = bc.jacobi(case.P) if pc == "jacobi" else (lambda r: r)
    y = st.Apply(case.b)
    _, dist = _bounds(st, y, case.P, case.b, ref, minv, its=ref.its)
    assert dist <= ref.tol + 8 * ref.gap
    k = ref.its // ell
    bl = st.GetBCGSLStats()
    assert bl["host_waits"] == math.ceil((k + 1) / 4) and bl["gated_iterations"] == 4 * math.ceil((k + 1) / 4) - (k + 1)      # the default interval


# ---- 2: gating ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kron", "convdiff"])
def test_check_interval_changes_no_bit(ctx, which):
    ell = 2
    if which == "kron":
        case, pc, ref = bc.kron_reference(0, ell); P, sigma, rtol = case.P, 0.0, 1e-12
    else:
        case, P, sigma, ref = bc.convdiff_reference(1, ell); rtol = 1e-8
    out = {}
    for c in (1, 3, 8, 64):
        st = _sinvert(ctx, case.P, sigma, "jacobi", ell, rtol=rtol, check=c)
        assert st.BCGSLGetCheckInterval() == c
        y = st.Apply(case.b)
        ksp, bl = st.GetKSPStats(), st.GetBCGSLStats()
        print("c %d: its %d, %s" % (c, ksp["iterations"], bl))
        assert ksp["iterations"] % ell == 0
        k = ksp["iterations"] // ell
        assert bl["host_waits"] == math.ceil((k + 1) / c) and bl["gated_iterations"] == c * math.ceil((k + 1) / c) - (k + 1)
        y2 = st.Apply(case.b)                                    # the same solve again: the same bits
        ksp2 = st.GetKSPStats()
        assert np.array_equal(y, y2) and ksp2["iterations"] == 2 * ksp["iterations"] and ksp2["last_rnorm"] == ksp["last_rnorm"]
        out[c] = (y, ksp["iterations"], ksp["last_rnorm"])
    for c in (3, 8, 64):
        assert np.array_equal(out[c][0], out[1][0]) and out[c][1] == out[1][1] and out[c][2] == out[1][2]
    if which == "kron":
        assert out[1][1] == ref.its


# ---- 3: both widths of every sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_unaligned_solution_vector_takes_the_one_row_sweeps(ctx, ell, mode):
    """y eight bytes past a 16-byte boundary: every sweep runs its one-row-per-lane form; the pinned count of the aligned test. (The combining
    apply sweep of shell mode at a non-zero shift runs in both widths in test_convdiff_converges_with_l2.)"""
    case, pc, ref = bc.kron_reference(0, ell)
    st = _sinvert(ctx, case.P, 0.0, pc, ell, mode, rtol=1e-12)
    y = _apply_unaligned(ctx, st, case.b)
    _, dist = _bounds(st, y, case.P, case.b, ref, bc.jacobi(case.P), its=ref.its)
    assert dist <= ref.tol + 8 * ref.gap


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("idx", range(len(bc.CONVDIFF)))
def test_convdiff_converges_with_l2(ctx, idx, aligned):
    """45 x 31 (n = 1395, odd: the pair form ends with a single row) at c = 3, sigma = 2 - the target inside the spectrum, shell mode forms A x - 2 x in
    the apply sweep - and at c = 8; 24 x 24 at c = 20. Convergence within twice the restatement's count; the count itself is not pinned."""
    case, P, sigma, ref = bc.convdiff_reference(idx, 2)
    assert ref.reason == "converged"
    st = _sinvert(ctx, case.P, sigma, "jacobi", 2, rtol=1e-8, max_it=2 * ref.its)
    y = st.Apply(case.b) if aligned else _apply_unaligned(ctx, st, case.b)
    stats, _ = _bounds(st, y, P, case.b, ref, bc.jacobi(P))
    assert 0 < stats["iterations"] <= 2 * ref.its + 1


# ---- 4: every ending ------------------------------------------------------------------------------------------------------------------------------
def test_every_ending(ctx):
    import slepc_amd as ks
    from slepc_amd import _lib
    case = bc.kron(8, 151)
    # a zero right-hand side: y = 0 and no iteration
    st = _sinvert(ctx, case.P, 0.0, "jacobi", 2)
    y = st.Apply(np.zeros(case.n))
    assert not y.any() and st.GetKSPStats() == {"solves": 1, "iterations": 0, "last_rnorm": 0.0}
    # max_it is tested at the start of a cycle: 3 with l = 2 ends after 4 steps
    st = _sinvert(ctx, case.P, 0.0, "jacobi", 2, rtol=1e-12, max_it=3)
    with pytest.raises(ks.KsError) as e:
        st.Apply(case.b)
    assert e.value.rc == 91 and "reached 4 iterations" in str(e.value) and "reached 4 iterations" in _lib.lib().ks_last_error_message().decode()
    assert st.GetKSPStats()["iterations"] == 4
    # not a number
    bn = case.b.copy(); bn[5] = np.nan
    st = _sinvert(ctx, case.P, 0.0, "jacobi", 2)
    with pytest.raises(ks.KsError) as e:
        st.Apply(bn)
    assert e.value.rc == 91 and "not a number" in str(e.value)
    # breakdown: P skew-symmetric and an integer right-hand side, sigma = (P r_0, r_0) = 0 exactly in any order (tests/test_bcgsl_cases_host.py)
    n = 600
    b = np.random.default_rng(7).integers(-8, 9, n).astype(np.float64)
    S = sp.kron(sp.identity(n // 2), np.array([[0.0, 1.0], [-1.0, 0.0]])).tocsr()
    for ell in (1, 2):
        st = _sinvert(ctx, S, 0.0, "none", ell)
        with pytest.raises(ks.KsError) as e:
            st.Apply(b)
        assert e.value.rc == 91 and "breakdown" in str(e.value) and st.GetKSPStats()["iterations"] == 0
    # a singular minimum-residual step: P = 2 I, alpha = 1/2 and r_0 = 0 exactly after the first step, A^ r_0 = 0, the Gram matrix of l = 1 is zero
    st = _sinvert(ctx, 2.0 * sp.identity(n), 0.0, "none", 1)
    with pytest.raises(ks.KsError) as e:
        st.Apply(b)
    assert e.value.rc == 91 and "singular minimum-residual step" in str(e.value) and st.GetKSPStats()["iterations"] == 1


# ---- 5: the preconditioners with kernels of their own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,block,ell", [("bjacobi", 8, 2), ("bjacobi-ilu", 64, 2), ("lu", 0, 1), ("amg", 0, 2), ("none", 0, 4)])
def test_every_pc_type(ctx, pc, block, ell):
    """The product goes to the scratch column, the preconditioner's own application makes the vector, a one-dot sweep follows. M^-1 of the restatement
    and of the residual is ST.PCApply (existing code, not under test here). The system is a diagonally dominant convection-diffusion operator on
    33 x 31 (c = 0.5). With LU the operator is the identity up to rounding and the second BiCG step of a cycle would divide rounding noise by
    rounding noise: l = 1 there, one cycle."""
    case = bc.convdiff(33, 31, 0.5)
    st = _sinvert(ctx, case.P, 0.0, pc, ell, block=block)
    st.SetUp()
    minv = st.PCApply if pc != "none" else (lambda r: r.copy())
    ref = bc.bcgsl_reference(case.P, case.b, minv, ell=ell, rtol=1e-8)
    assert ref.reason == "converged"
    y = st.Apply(case.b)
    stats, _ = _bounds(st, y, case.P, case.b, ref, minv)
    assert 0 < stats["iterations"] <= 2 * ref.its
    if pc == "lu":
        assert stats["iterations"] == 1


# ---- 6: the other transformations, the transposed side --------------------------------------------------------------------------------------------
def _pencil():
    A = bc.convdiff(12, 11, 1.0).P
    n = A.shape[0]
    B = sp.diags([0.1 * np.ones(n - 1), 1.0 + 0.01 * np.arange(n) / n, 0.1 * np.ones(n - 1)], [-1, 0, 1]).tocsr()
    return A, B


@pytest.mark.parametrize("kind,sigma", [("shift", 0.3), ("cayley", -0.7), ("sinvert", 0.3)])
@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_transformations_match_lu_preonly(ctx, kind, sigma, mode):
    """Shift with two matrices (B^-1 solves), Cayley and a two-matrix shift-and-invert (in shell mode the apply sweep forms w = A x - sigma B x)
    against the same ST with KS_PC_LU and KS_KSP_PREONLY. Both answers solve a system whose condition number is below 100 (asserted) to a
    relative residual of 1e-13 or better: their distance is below 1e-10."""
    import slepc_amd as ks
    A, B = _pencil()
    Pd = (B if kind == "shift" else A - sigma * B).toarray()
    assert np.linalg.cond(Pd) < 100
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    ys = {}
    for ksp, pc in (("bcgsl", "jacobi"), ("preonly", "lu")):
        st = ks.ST(ctx)
        st.SetType(kind); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType(ksp); st.SetPC(pc); st.SetKSP(rtol=1e-13)
        ys[ksp] = st.Apply(x)
        if ksp == "bcgsl":
            assert st.GetKSPStats()["solves"] == 1 and st.GetKSPStats()["iterations"] > 0 and st.GetBCGSLStats()["sweeps"] > 0
    d = np.linalg.norm(ys["bcgsl"] - ys["preonly"]) / np.linalg.norm(ys["preonly"])
    print("%s %s: %.3e" % (kind, mode, d))
    assert d <= 1e-10


@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_transposed_solve_is_the_solve_with_the_transposed_matrix(ctx, mode):
    import slepc_amd as ks
    A, B = _pencil()
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(0.3); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType("bcgsl"); st.SetKSP(rtol=1e-13)
    st.SetTransposeSolves(True)
    yt = st.MatSolveTranspose(b)
    y0 = np.linalg.solve((A - 0.3 * B).toarray().T, b)
    assert np.linalg.norm(yt - y0) <= 1e-10 * np.linalg.norm(y0)
    # one matrix: STApply is the solve itself; the transposed side of A against the forward solve with A^T
    st1 = ks.ST(ctx)
    st1.SetType("sinvert"); st1.SetShift(0.3); st1.SetMatrices(_mat(ctx, A)); st1.SetMatMode(mode); st1.SetKSPType("bcgsl"); st1.SetKSP(rtol=1e-13)
    st1.SetTransposeSolves(True)
    stt = ks.ST(ctx)
    stt.SetType("sinvert"); stt.SetShift(0.3); stt.SetMatrices(_mat(ctx, A.T)); stt.SetMatMode(mode); stt.SetKSPType("bcgsl"); stt.SetKSP(rtol=1e-13)
    x = stt.Apply(b)
    assert np.linalg.norm(st1.MatSolveTranspose(b) - x) <= 1e-10 * np.linalg.norm(x)


# ---- 7: the interface -----------------------------------------------------------------------------------------------------------------------------
def test_setters_defaults_and_the_header(ctx):
    import slepc_amd as ks
    st = ks.ST(ctx)
    assert st.BCGSLGetEll() == 2 and st.BCGSLGetCheckInterval() == 4
    assert st.CGGetCheckInterval() == 8 and st.MINRESGetCheckInterval() == 8
    for bad in (0, 5, -1):
        assert ctx.L.ks_st_bcgsl_set_ell(st.h, bad) == 63
    assert st.BCGSLGetEll() == 2
    for ell in (1, 2, 3, 4):
        st.BCGSLSetEll(ell); assert st.BCGSLGetEll() == ell
    assert ctx.L.ks_st_bcgsl_set_check_interval(st.h, 0) == 63 and ctx.L.ks_st_bcgsl_set_check_interval(st.h, 1025) == 63
    assert st.BCGSLGetCheckInterval() == 4
    st.BCGSLSetCheckInterval(1); assert st.BCGSLGetCheckInterval() == 1
    st.BCGSLSetCheckInterval(1024); assert st.BCGSLGetCheckInterval() == 1024
    assert st.CGGetCheckInterval() == 8 and st.MINRESGetCheckInterval() == 8               # a setting apart from CG's and MINRES's
    assert ctx.L.ks_st_set_ksp_type(st.h, 8) == 0
    for t in (3, 5, 7, 9, -1):
        assert ctx.L.ks_st_set_ksp_type(st.h, t) == 56
    assert "KSPBCGSL" in ks._lib.lib().ks_last_error_message().decode()
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ksgpu.h")).read()
    assert "KS_KSP_BCGSL = 8" in text and "KS_KSP_MINRES = 6" in text
    assert st.GetBCGSLStats() == {"sweeps": 0, "host_waits": 0, "gated_iterations": 0}


def test_changing_l_rebuilds_the_work_vectors(ctx):
    """l = 4 after l = 1 on one ST: the setter clears the set-up, the BV of 2 l + 4 columns is made anew; and back."""
    case, pc, _ = bc.kron_reference(0, 1)
    st = _sinvert(ctx, case.P, 0.0, pc, 1, rtol=1e-12)
    ys = {}
    for ell in (1, 4, 2, 4):
        st.BCGSLSetEll(ell)
        before = st.GetKSPStats()["iterations"]
        y = st.Apply(case.b)
        assert st.GetKSPStats()["iterations"] - before == bc.kron_count(0, ell)
        if ell in ys:
            assert np.array_equal(ys[ell], y)
        ys[ell] = y


def test_jacobi_davidson_refuses_bcgsl(ctx):
    import slepc_amd as ks
    case = cc.lap(*cc.LAP[0])
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, case.P)); eps.SetProblemType(ks.EPS_HEP); eps.SetType("jd"); eps.SetDimensions(2)
    eps.GetST().SetKSPType("bcgsl")
    with pytest.raises(ks.KsError) as e:
        eps.Solve()
    assert e.value.rc == 56 and "KSPBCGSL" in str(e.value)


def test_gmres_before_and_after_on_one_st(ctx):
    import slepc_amd as ks
    case, pc, ref = bc.kron_reference(0, 2)
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(_mat(ctx, case.P)); st.SetKSP(rtol=1e-12)
    g1 = st.Apply(case.b)
    st.SetKSPType("bcgsl")
    b1 = st.Apply(case.b)
    st.SetKSPType("gmres")
    g2 = st.Apply(case.b)
    assert np.array_equal(g1, g2)
    assert np.linalg.norm(b1 - g1) <= 1e-10 * np.linalg.norm(g1) and st.GetBCGSLStats()["sweeps"] > 0
    assert st.GetKSPStats()["solves"] == 3


# ---- 8: a whole eigensolve ------------------------------------------------------------------------------------------------------------------------
def test_krylovschur_sinvert_matches_lu(ctx):
    """Krylov-Schur on the 45 x 31 convection-diffusion operator with convection along x (c = 3, complex eigenvalues in the rectangle 2 < Re < 6,
    |Im| < 5.66) under shift-and-invert at the target 0.5: the inner solves by BiCGStab(2) with point Jacobi at rtol 1e-12 (80 to 120 steps at 1e-10 in the
    restatement on the right-hand sides of an Arnoldi process; at the targets 1 and 1.5 single solves need up to 1000 and break down on the device) give the eigenvalues of the run with LU + PREONLY. Both runs converge to a relative residual of 1e-10. The four eigenvalues nearest
    the target (2.0096, 2.0384 and the pair 2.0096 +- 0.3860 i) are simple but ill-conditioned, the operator being far from normal: at the EPS
    default of 1e-8 the run with LU is 5.4e-6 off the exact 2.00963055, a factor 540. At 1e-10 that is 5e-8, and the bound 1e-6 leaves a factor 20.
    The target lies in the disc of the spectrum, left of its real parts, not among them: with a real target among them P = A - t I has eigenvalues
    around the origin, and BiCGStab(l) with point Jacobi does not converge there (restatement: 6000 steps at t = 2.5 for l = 2 and l = 4); with
    convection in both directions (bcgsl_cases.convdiff) every eigenvalue has the real part 4, the ones nearest a real target are a cluster, and the
    run with LU + PREONLY itself converges to none of them."""
    import slepc_amd as ks
    case = bc.convdiff_x(45, 31, 3.0)
    lam = {}
    for ksp, pc in (("preonly", "lu"), ("bcgsl", "jacobi")):
        eps = ks.EPS(ctx)
        eps.SetOperators(_mat(ctx, case.P)); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4, 24)
        eps.SetTarget(0.5); eps.SetWhichEigenpairs("target_magnitude")
        st = eps.GetST(); st.SetType("sinvert"); st.SetKSPType(ksp); st.SetPC(pc); st.SetKSP(rtol=1e-12, max_it=4000)
        eps.SetTolerances(tol=1e-10)
        eps.Solve()
        lam[ksp] = np.array([complex(*eps.GetEigenvalue(i)) for i in range(min(4, eps.GetConverged()))])
        print(ksp, eps.GetConverged(), lam[ksp], st.GetKSPStats(), st.GetBCGSLStats())
        assert eps.GetConverged() >= 4
        if ksp == "bcgsl":
            assert st.GetBCGSLStats()["sweeps"] > 0 and st.BCGSLGetEll() == 2

    def key(z):
        return sorted(z, key=lambda v: (round(abs(v - 0.5), 6), round(v.imag, 6)))
    a, b = np.array(key(lam["preonly"])), np.array(key(lam["bcgsl"]))
    assert np.all(np.abs(a - b) <= 1e-6 * np.abs(a))
    assert np.all(np.abs(a - np.array([2.00963055, 2.03842944, 2.00963055 - 0.38603739j, 2.00963055 + 0.38603739j])) <= 1e-6)
