"""KS_KSP_MINRES, the MINRES inner solver of the ST, on one rank against the numpy restatement of tests/minres_cases.py.

The iteration counts are exact where tests/test_minres_cases_host.py pins them: on the I (x) T systems MINRES ends at iteration m whatever the
rounding (the residual falls from above 0.17 to below 3e-11 there), on the shifted Laplacians the tolerance sits in the middle of the widest step
of the restatement's history. The true residual of the returned iterate in the M^-1 norm may exceed the tolerance by the distance between the
recurred phibar and the true norm; the bound is tol + 8 g with g that distance as the restatement measured it on the same case. The solution is
compared with the restatement's through the same bound: ||P (y - y_ref)|| in the M^-1 norm, the distance of the two residuals, <= tol + 8 g."""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cg_cases as cc
import minres_cases as mc
import scenarios as sc

pytestmark = pytest.mark.gpu
KRON_CASES = [(m, b, pc) for (m, b) in mc.KRON for pc in ("jacobi-abs", "none")] + [(13, 79, "none")]


def _mat(ctx, S, keep=True):
    import slepc_amd as ks
    S = sp.csr_matrix(S); S.sort_indices()
    return ks.Mat.from_csr(ctx, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), keep_csr=keep)


def _set_pc(st, pc, block=0):
    if pc == "jacobi-abs":
        st.SetPC("jacobi"); st.PCJacobiSetUseAbs(True)
    else:
        st.SetPC(pc, block)


def _sinvert(ctx, A, sigma, pc, mode="shell", rtol=1e-8, block=0, check=None, ksp="minres"):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A)); st.SetMatMode(mode)
    st.SetKSPType(ksp); _set_pc(st, pc, block); st.SetKSP(rtol=rtol)
    if check is not None:
        st.MINRESSetCheckInterval(check)
    return st


def _check_solve(st, P, b, ref, minv, count=True):
    y = st.Apply(b)
    stats = st.GetKSPStats()
    res = mc.mnorm(minv, b - P @ y)
    diff = mc.mnorm(minv, P @ (y - ref.y))
    print("its %d (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, P (y - y_ref) %.3e, gap %.2e" % (stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, diff, ref.gap))
    assert stats["solves"] == 1
    if count:
        assert stats["iterations"] == ref.its
    assert stats["last_rnorm"] <= ref.tol
    assert res <= ref.tol + 8 * ref.gap
    assert diff <= ref.tol + 8 * ref.gap
    return y


# ---- 1: counts and solutions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shell", "copy"])
@pytest.mark.parametrize("m,blocks,pc", KRON_CASES)
def test_kron_counts_and_solutions(ctx, m, blocks, pc, mode):
    """Three negative eigenvalues and negative diagonal entries; the count is m. n = 1057, 1027 and 513 have the scalar tail, n = 512 is one tile."""
    case, ref = mc.kron_reference(m, blocks, pc)
    st = _sinvert(ctx, case.P, 0.0, pc, mode)
    y = _check_solve(st, case.P, case.b, ref, mc.minv_of(case.P, pc))
    x = np.linalg.solve(case.P.toarray(), case.b)
    assert np.linalg.norm(y - x) <= 1e-9 * np.linalg.norm(x)                      # cond(P) < 100 and h[m] <= 3e-11


@pytest.mark.parametrize("mode", ["shell", "copy"])
@pytest.mark.parametrize("which,pc", mc.LAP_ALL)
def test_lap_counts_and_solutions(ctx, which, pc, mode):
    """Sinvert at a shift inside the spectrum (4 and 5 negative eigenvalues; LAP[2] is definite), many batches of the default check interval. In shell
    mode the alfa sweep forms u = A v - sigma v. LAP[1] without a preconditioner fails the rule of the host tests and is run for the residual only."""
    idx, sigma = mc.LAP[which]
    case, P, rtol, ref, k, _ = mc.lap_reference(which, pc)
    st = _sinvert(ctx, case.P, sigma, pc, mode, rtol=rtol)
    _check_solve(st, P, case.b, ref, mc.minv_of(P, pc), count=(which, pc) in mc.LAP_COUNTS)


# ---- 2: gating ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kron", "lap"])
def test_check_interval_changes_no_bit(ctx, which):
    if which == "kron":
        case, ref = mc.kron_reference(7, 151, "jacobi-abs"); A, rtol, sigma = case.P, 1e-8, 0.0
    else:
        case, _, rtol, ref, _, _ = mc.lap_reference(0, "jacobi-abs"); A, sigma = case.P, mc.LAP[0][1]
    out = {}
    for c in (1, 3, 8, 64):
        st = _sinvert(ctx, A, sigma, "jacobi-abs", rtol=rtol, check=c)
        assert st.MINRESGetCheckInterval() == c and st.CGGetCheckInterval() == 8
        y = st.Apply(case.b)
        ksp, mr = st.GetKSPStats(), st.GetMINRESStats()
        print("c %d: its %d, %s" % (c, ksp["iterations"], mr))
        batches = math.ceil(ref.its / c)
        assert ksp["iterations"] == ref.its
        assert mr["host_waits"] == batches and mr["gated_iterations"] == batches * c - ref.its
        assert mr["sweeps"] >= 3 * ref.its
        y2 = st.Apply(case.b)                                    # the same solve again: the same bits
        ksp2, mr2 = st.GetKSPStats(), st.GetMINRESStats()
        assert np.array_equal(y, y2) and ksp2["iterations"] == 2 * ref.its and ksp2["last_rnorm"] == ksp["last_rnorm"]
        assert mr2["host_waits"] == 2 * batches and mr2["gated_iterations"] == 2 * (batches * c - ref.its)
        assert st.GetCGStats() == {"sweeps": 0, "host_waits": 0, "gated_iterations": 0}
        out[c] = (y, ksp["iterations"], ksp["last_rnorm"])
    for c in (3, 8, 64):
        assert np.array_equal(out[c][0], out[1][0]) and out[c][1] == out[1][1] and out[c][2] == out[1][2]


def test_interval_defaults_and_range_checks(ctx):
    import slepc_amd as ks
    st = ks.ST(ctx)
    assert st.MINRESGetCheckInterval() == 8 and st.PCJacobiGetUseAbs() is False
    assert ctx.L.ks_st_minres_set_check_interval(st.h, 0) == 63 and ctx.L.ks_st_minres_set_check_interval(st.h, 1025) == 63
    assert ctx.L.ks_st_minres_set_check_interval(st.h, -1) == 63
    assert st.MINRESGetCheckInterval() == 8                                          # a refused value leaves the interval alone
    assert ctx.L.ks_st_minres_set_check_interval(st.h, 1) == 0 and st.MINRESGetCheckInterval() == 1
    assert ctx.L.ks_st_minres_set_check_interval(st.h, 1024) == 0 and st.MINRESGetCheckInterval() == 1024
    assert st.CGGetCheckInterval() == 8                                              # CG's interval is a setting of its own
    st.CGSetCheckInterval(5)
    assert st.MINRESGetCheckInterval() == 1024
    assert ctx.L.ks_st_set_ksp_type(st.h, 6) == 0 and ctx.L.ks_st_set_ksp_type(st.h, 7) == 56
    hdr = open(os.path.join(os.path.dirname(ks.__file__), "..", "include", "ksgpu.h")).read()
    assert "KS_KSP_MINRES = 6" in hdr
    st.PCJacobiSetUseAbs(True)
    assert st.PCJacobiGetUseAbs() is True


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


def test_unaligned_solution_vector_takes_the_one_row_sweeps(ctx):
    """y eight bytes past a 16-byte boundary: every sweep runs its one-row-per-lane form. Counts and bounds of the aligned runs. Jacobi-abs: lanczos with
    the diagonal; none (n = 513: two tiles of the one-row form and a row): lanczos on the residual itself; LAP[0] at its shift in shell mode: the
    combining alfa sweep; blocks of 8: lanczos ends after the residual, the dot sweep follows. M^-1 of that restatement is ST.PCApply, as in the
    aligned test; at its rtol of 1e-8 rounding moves the count (101 to 106 with permuted dots), so the tolerance sits in the widest step of the history above 1e-7,
    k = 87, which tests/test_minres_cases_host.py pins."""
    case, ref = mc.kron_reference(7, 151, "jacobi-abs")
    for mode in ("shell", "copy"):
        st = _sinvert(ctx, case.P, 0.0, "jacobi-abs", mode)
        y = _apply_unaligned(ctx, st, case.b)
        stats = st.GetKSPStats()
        minv = mc.minv_of(case.P, "jacobi-abs")
        assert stats["iterations"] == ref.its and stats["last_rnorm"] <= ref.tol
        assert mc.mnorm(minv, case.b - case.P @ y) <= ref.tol + 8 * ref.gap
        assert mc.mnorm(minv, case.P @ (y - ref.y)) <= ref.tol + 8 * ref.gap
    case, ref = mc.kron_reference(9, 57, "none")
    lcase, lP, lrtol, lref, _, _ = mc.lap_reference(0, "jacobi-abs")
    for A, sigma, P, b, pc, rtol, r in [(case.P, 0.0, case.P, case.b, "none", 1e-8, ref), (lcase.P, mc.LAP[0][1], lP, lcase.b, "jacobi-abs", lrtol, lref)]:
        st = _sinvert(ctx, A, sigma, pc, "shell", rtol=rtol)
        y = _apply_unaligned(ctx, st, b)
        stats = st.GetKSPStats()
        minv = mc.minv_of(P, pc)
        print("%s n %d: its %d (restatement %d), last_rnorm %.3e, tol %.3e" % (pc, len(b), stats["iterations"], r.its, stats["last_rnorm"], r.tol))
        assert stats["iterations"] == r.its and stats["last_rnorm"] <= r.tol
        assert mc.mnorm(minv, b - P @ y) <= r.tol + 8 * r.gap
        assert mc.mnorm(minv, P @ (y - r.y)) <= r.tol + 8 * r.gap
    st = _sinvert(ctx, lcase.P, mc.LAP[0][1], "bjacobi", block=mc.BJACOBI_BLOCK)
    st.SetUp()
    k, brtol, ratio = mc.pick_k(mc.minres_reference(lP, lcase.b, st.PCApply, rtol=1e-12).hist, mc.BJACOBI_FLOOR)
    bref = mc.minres_reference(lP, lcase.b, st.PCApply, rtol=brtol)
    assert bref.reason == "converged" and bref.its == k == 87 and ratio >= 1.4
    st.SetKSP(rtol=brtol)
    y = _apply_unaligned(ctx, st, lcase.b)
    stats = st.GetKSPStats()
    res, diff = mc.mnorm(st.PCApply, lcase.b - lP @ y), mc.mnorm(st.PCApply, lP @ (y - bref.y))
    print("bjacobi: its %d (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, P (y - y_ref) %.3e, gap %.2e" % (stats["iterations"], bref.its, stats["last_rnorm"], bref.tol, res, diff, bref.gap))
    assert stats["solves"] == 1 and stats["iterations"] == bref.its and stats["last_rnorm"] <= bref.tol
    assert res <= bref.tol + 8 * bref.gap
    assert diff <= bref.tol + 8 * bref.gap


# ---- 3: endings -----------------------------------------------------------------------------------------------------------------------------------
def test_zero_right_hand_side(ctx):
    case = mc.kron(7, 151)
    st = _sinvert(ctx, case.P, 0.0, "jacobi-abs")
    y = st.Apply(np.zeros(case.n))
    assert not y.any() and st.GetKSPStats() == {"solves": 1, "iterations": 0, "last_rnorm": 0.0}
    assert st.GetMINRESStats()["host_waits"] == 1


def test_plain_jacobi_is_indefinite_and_use_abs_converges(ctx):
    import slepc_amd as ks
    from slepc_amd import _lib
    case, ref = mc.kron_reference(7, 151, "jacobi-abs")
    st = _sinvert(ctx, case.P, 0.0, "jacobi")
    with pytest.raises(ks.KsError) as e:
        st.Apply(case.b)
    assert e.value.rc == 91 and "indefinite preconditioner" in str(e.value) and "indefinite preconditioner" in _lib.lib().ks_last_error_message().decode()
    refused = st.GetKSPStats()["iterations"]                                         # iterations completed before (r2, z) < 0
    st.PCJacobiSetUseAbs(True)                                                       # the setter clears the set-up: the same ST now converges
    y = st.Apply(case.b)
    assert st.GetKSPStats()["iterations"] - refused == ref.its
    assert mc.mnorm(mc.jacobi_abs(case.P), case.b - case.P @ y) <= ref.tol + 8 * ref.gap
    d = st.PCApply(np.ones(case.n))
    assert np.array_equal(d, 1.0 / np.abs(case.diag))
    st.PCJacobiSetUseAbs(False)
    assert np.array_equal(st.PCApply(np.ones(case.n)), 1.0 / case.diag)


def test_negative_diagonal_matrix_is_refused_at_the_start(ctx):
    """(b, z) < 0 before the first iteration: a diagonal matrix with negative entries under plain Jacobi, M^-1 = P^-1 negative definite."""
    import slepc_amd as ks
    n = 600
    D = sp.diags(-1.0 - (np.arange(n) % 7))
    b = np.random.default_rng(5).integers(1, 9, n).astype(np.float64)
    st = _sinvert(ctx, D, 0.0, "jacobi")
    with pytest.raises(ks.KsError) as e:
        st.Apply(b)
    assert e.value.rc == 91 and "indefinite preconditioner" in str(e.value)
    assert st.GetKSPStats()["iterations"] == 0
    st.PCJacobiSetUseAbs(True)                                                       # M^-1 P = -I: one iteration
    y = st.Apply(b)
    assert st.GetKSPStats()["iterations"] == 1
    assert np.linalg.norm(D @ y - b) <= 1e-13 * np.linalg.norm(b)


def test_nan_and_max_it(ctx):
    import slepc_amd as ks
    case = mc.kron(7, 151)
    st = _sinvert(ctx, case.P, 0.0, "jacobi-abs")
    b = case.b.copy(); b[17] = np.nan
    with pytest.raises(ks.KsError) as e:
        st.Apply(b)
    assert e.value.rc == 91 and "not a number" in str(e.value)
    st = _sinvert(ctx, case.P, 0.0, "jacobi-abs")
    st.SetKSP(max_it=2)
    with pytest.raises(ks.KsError) as e:
        st.Apply(case.b)
    assert e.value.rc == 91 and "reached 2 iterations" in str(e.value)
    assert st.GetKSPStats()["iterations"] == 2
    ref = mc.minres_reference(case.P, case.b, mc.jacobi_abs(case.P), max_it=2)
    assert ref.reason == "its" and abs(st.GetKSPStats()["last_rnorm"] - ref.phibar) <= 1e-12 * ref.phibar


def test_jacobi_davidson_refuses_minres(ctx):
    import slepc_amd as ks
    case = cc.lap(*cc.LAP[0])
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, case.P)); eps.SetProblemType(ks.EPS_HEP); eps.SetType("jd"); eps.SetDimensions(2)
    eps.GetST().SetKSPType("minres")
    with pytest.raises(ks.KsError) as e:
        eps.Solve()
    assert e.value.rc == 56 and "KSPMINRES" in str(e.value)


# ---- 4: what must not move ------------------------------------------------------------------------------------------------------------------------
def test_use_abs_off_keeps_the_bits_of_jacobi_and_gmres(ctx):
    case = mc.kron(7, 151)                                       # negative diagonal entries: abs would change the diagonal
    P = cc.shifted(case, 0.3)
    plain = _sinvert(ctx, case.P, 0.3, "jacobi", ksp="gmres")
    d0 = plain.PCApply(np.ones(case.n)); y0 = plain.Apply(case.b)
    st = _sinvert(ctx, case.P, 0.3, "jacobi", ksp="gmres")
    st.PCJacobiSetUseAbs(True)
    d_abs = st.PCApply(np.ones(case.n))
    st.PCJacobiSetUseAbs(False)
    d1 = st.PCApply(np.ones(case.n)); y1 = st.Apply(case.b)
    assert np.array_equal(d0, 1.0 / P.diagonal()) and (d0 < 0).any()
    assert np.array_equal(d1, d0) and np.array_equal(y1, y0)
    assert np.array_equal(d_abs, np.abs(d0))
    assert st.GetKSPStats()["iterations"] == plain.GetKSPStats()["iterations"]
    # no effect on another PC type
    a = _sinvert(ctx, case.P, 0.3, "bjacobi", block=7, ksp="gmres"); b = _sinvert(ctx, case.P, 0.3, "bjacobi", block=7, ksp="gmres")
    b.PCJacobiSetUseAbs(True)
    assert np.array_equal(a.PCApply(case.b), b.PCApply(case.b))


def test_gmres_before_and_after_minres_on_one_st(ctx):
    import slepc_amd as ks
    case = cc.lap(*cc.LAP[0])
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(_mat(ctx, case.P))
    g1 = st.Apply(case.b)
    st.SetKSPType("minres")
    m1 = st.Apply(case.b)
    st.SetKSPType("gmres")
    g2 = st.Apply(case.b)
    assert np.array_equal(g1, g2)
    assert np.linalg.norm(m1 - g1) <= 1e-6 * np.linalg.norm(g1) and st.GetMINRESStats()["sweeps"] > 0


# ---- 5: matrix modes, transformations, the transposed side, a block preconditioner ---------------------------------------------------------------
def test_shell_mode_against_copy_mode(ctx):
    """The same system with P applied term by term (u = A v - sigma v formed in the alfa sweep) and assembled: the same count, and solutions as close as
    two runs of the restatement's bound allow."""
    idx, sigma = mc.LAP[0]
    case, P, rtol, ref, k, _ = mc.lap_reference(0, "jacobi-abs")
    minv = mc.minv_of(P, "jacobi-abs")
    y = {}
    for mode in ("shell", "copy"):
        st = _sinvert(ctx, case.P, sigma, "jacobi-abs", mode, rtol=rtol)
        y[mode] = st.Apply(case.b)
        assert st.GetKSPStats()["iterations"] == k
    assert mc.mnorm(minv, P @ (y["shell"] - y["copy"])) <= ref.tol + 8 * ref.gap


def _lu_oracle(ctx, kind, sigma, A, B, x, transpose=False):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode("copy"); st.SetKSPType("preonly"); st.SetPC("lu")
    if transpose:
        st.SetTransposeSolves(True)
        return st.MatSolveTranspose(x)
    return st.Apply(x)


@pytest.mark.parametrize("kind,sigma", [("shift", 0.3), ("cayley", 2.9)])
@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_shift_and_cayley_match_the_lu_solve(ctx, kind, sigma, mode):
    """The B^-1 solves of a shift with two matrices (P = B, definite) and Cayley at a shift inside the spectrum of the pencil (P = A - sigma B,
    indefinite; in shell mode the alfa sweep forms u = A v - sigma B v), against KS_PC_LU + PREONLY on the same ST settings. The bound: the true
    residual is within tol + 8 g of zero (g: the restatement's gap on this system), so the error is at most that over the smallest |eigenvalue| of
    P, plus the LU solve's own 64 eps cond(P)."""
    import slepc_amd as ks
    A, B = sc.test32_pencil(18)
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    P = (B if kind == "shift" else A - sigma * B).toarray()
    rhs = (A - sigma * B) @ x if kind == "shift" else (A + sigma * B) @ x      # cayley: the antishift defaults to the shift
    lam = np.linalg.eigvalsh(P)
    assert (lam < 0).any() == (kind == "cayley")
    ref = mc.minres_reference(P, rhs, None, rtol=1e-10)
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType("minres"); st.SetPC("none"); st.SetKSP(rtol=1e-10)
    y = st.Apply(x); y0 = _lu_oracle(ctx, kind, sigma, A, B, x)
    bound = (ref.tol + 8 * ref.gap) / np.abs(lam).min() + 64 * np.finfo(float).eps * np.linalg.cond(P) * np.linalg.norm(y0)
    print("%s %s: its %d (restatement %d), error %.3e, bound %.3e" % (kind, mode, st.GetKSPStats()["iterations"], ref.its, np.linalg.norm(y - y0), bound))
    assert ref.reason == "converged" and st.GetKSPStats()["solves"] == 1 and st.GetKSPStats()["iterations"] > 0
    assert np.linalg.norm(y - y0) <= bound


@pytest.mark.parametrize("mode", ["shell", "copy"])
def test_transposed_side(ctx, mode):
    """P is symmetric: the transposed solve runs the same iteration on the transposed views and gives the forward solution."""
    import slepc_amd as ks
    A, B = sc.test32_pencil(18)
    sigma = 2.9
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    P = (A - sigma * B).toarray()
    lam = np.linalg.eigvalsh(P)
    ref = mc.minres_reference(P, b, None, rtol=1e-10)
    st = ks.ST(ctx)
    st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(_mat(ctx, A), _mat(ctx, B)); st.SetMatMode(mode); st.SetKSPType("minres"); st.SetPC("none"); st.SetKSP(rtol=1e-10)
    st.SetTransposeSolves(True)
    yt = st.MatSolveTranspose(b)
    y0 = _lu_oracle(ctx, "sinvert", sigma, A, B, b, transpose=True)
    bound = (ref.tol + 8 * ref.gap) / np.abs(lam).min() + 64 * np.finfo(float).eps * np.linalg.cond(P) * np.linalg.norm(y0)
    assert (lam < 0).any() and st.GetKSPStats()["iterations"] > 0
    assert np.linalg.norm(yt - y0) <= bound


def test_block_jacobi_with_definite_blocks(ctx):
    """LAP[0] at sigma 1.5 is indefinite, its diagonal blocks of 8 rows are not (diagonally dominant: diagonal >= 3, at most two off-diagonal
    entries of -1): the lanczos sweep stops after the residual, the block application makes z, a dot sweep follows. M^-1 of the restatement and of
    the residual is ST.PCApply (existing code, not under test here)."""
    idx, sigma = mc.LAP[0]
    case = cc.lap(*cc.LAP[idx])
    P = cc.shifted(case, sigma)
    st = _sinvert(ctx, case.P, sigma, "bjacobi", block=8)
    st.SetUp()
    ref = mc.minres_reference(P, case.b, st.PCApply, rtol=1e-8)
    assert ref.reason == "converged"
    y = st.Apply(case.b)
    stats = st.GetKSPStats()
    res = mc.mnorm(st.PCApply, case.b - P @ y)
    print("bjacobi: its %d (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e" % (stats["iterations"], ref.its, stats["last_rnorm"], ref.tol, res, ref.gap))
    assert stats["solves"] == 1 and stats["last_rnorm"] <= ref.tol
    assert res <= ref.tol + 8 * ref.gap


# ---- 6: a whole solve -----------------------------------------------------------------------------------------------------------------------------
def test_krylov_schur_at_a_target_inside_the_spectrum(ctx):
    """Krylov-Schur with sinvert at 1.5, inside the spectrum of LAP[0] (four eigenvalues below): the inner solves by MINRES with Jacobi-abs give
    the eigenvalues of the LU + PREONLY run within the EPS tolerance."""
    import slepc_amd as ks
    case = cc.lap(*cc.LAP[0])
    tol = 1e-8
    lam = {}
    for ksp in ("lu", "minres"):
        eps = ks.EPS(ctx)
        eps.SetOperators(_mat(ctx, case.P)); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(4, 20); eps.SetTolerances(tol)
        eps.SetTarget(1.5); eps.SetWhichEigenpairs("target_magnitude")
        st = eps.GetST(); st.SetType("sinvert")
        if ksp == "lu":
            st.SetMatMode("copy"); st.SetKSPType("preonly"); st.SetPC("lu")
        else:
            st.SetKSPType("minres"); st.SetPC("jacobi"); st.PCJacobiSetUseAbs(True); st.SetKSP(rtol=1e-12)
        eps.Solve()
        assert eps.GetConverged() >= 4
        lam[ksp] = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
        if ksp == "minres":
            print(lam, st.GetKSPStats(), st.GetMINRESStats())
            assert st.GetKSPStats()["solves"] > 0 and st.GetMINRESStats()["sweeps"] > 0
    exact = np.linalg.eigvalsh(case.P.toarray())
    nearest = exact[np.argsort(np.abs(exact - 1.5))[:4]]
    assert np.allclose(np.sort(lam["minres"]), np.sort(lam["lu"]), rtol=tol, atol=0)
    assert np.allclose(np.sort(lam["minres"]), np.sort(nearest), rtol=tol, atol=0)
