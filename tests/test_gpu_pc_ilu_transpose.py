"""PCApplyTranspose on the ST's KSP (ks_st_pc_apply_transpose, behind ks_st_set_transpose_solves): the transposed block triangular solve of the
ILU(0) blocks (k_bjacobi_ilu_apply_t, slepc_amd/csrc/ks_pc.hip), the dense blocks walked by columns, point Jacobi.

The ILU kernel is checked against the reference factors of tests/ilu_cases.py, M = L U of every block, with the componentwise bound of
tests/ilu_transpose_cases.py:  |M^T y - x| <= 8 (k + 1) 2^-53 (|U^T||L^T||y|),  k the larger of the block's longest row and longest column - no
tuned tolerance. Unless a test says otherwise: sinvert with one matrix, a shift that makes P = A - sigma I strictly diagonally dominant, shell mode."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import ilu_cases as ic
import ilu_transpose_cases as itc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu


def _mat(ctx, S, keep=True, **kw):
    import slepc_amd as ks
    rp, col, val = S if isinstance(S, tuple) else ic.arrays(S)
    return ks.Mat.from_csr(ctx, rp, col, val, keep_csr=keep, **kw)


def _st(ctx, A, bs, sigma=ic.SIGMA, B=None, kind="sinvert", mode="shell", pc="bjacobi-ilu", transpose=True):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(A, B); st.SetMatMode(mode); st.SetPC(pc, bs); st.SetTransposeSolves(transpose)
    return st


def _x(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _case(ctx, S, bs, seed, what):
    st = _st(ctx, _mat(ctx, S), bs)
    x = _x(S.shape[0], seed)
    y = st.PCApplyTranspose(x)
    ref = ic.Reference.of(ic.shifted(S, ic.SIGMA), bs)
    itc.check_t(ref, x, y, what)
    return st, ref, x, y


# ---- the kernel cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64 * 3 + 1, 63])
def test_partial_blocks(ctx, n):
    """Three full blocks and a last block of one row; a single block shorter than the block size."""
    _case(ctx, ic.random_sparse(n, 6, n), 64, 1, "partial n=%d" % n)


@pytest.mark.parametrize("bs", [8192, 64])
@pytest.mark.parametrize("kind", ["diagonal", "bidiagonal"])
def test_one_wide_level_and_the_chain_in_the_second_phase(ctx, kind, bs):
    """A diagonal P is one level of bs rows per phase (more rows than lanes at 8192). A lower-bidiagonal P has its chain of bs levels of one row
    in the SECOND phase now (L^T, upper bidiagonal) and a first phase of one level (U^T is the diagonal). Two blocks, the second one short."""
    n = bs + bs // 2 + 3
    S = ic.diagonal(n) if kind == "diagonal" else ic.bidiagonal(n)
    _case(ctx, S, bs, 2, "%s bs=%d" % (kind, bs))


def test_dense_row_and_dense_column_swap_roles(ctx):
    """A block of 8192 rows whose last row is dense to the left and whose first row is dense to the right: in the transposed triangles the dense
    row of U is a dense column of U^T - a level of 8191 rows that all read code 0 - and the dense row of L a level of 8191 rows reading code 8191.
    The forward result misses the transposed bound: the test tells the two kernels apart."""
    st, ref, x, y = _case(ctx, ic.arrow(8192), 8192, 3, "arrow")
    r = max(itc.ratios_t(ref, x, st.PCApply(x)))
    print("arrow: the forward result sits at %.3g of the transposed bound" % r)
    assert r > 1.0


@pytest.mark.parametrize("lines", [4, 2.5])
def test_mixed_level_widths_on_the_convection_pencil(ctx, lines):
    nx, ny = 32, 11
    A, _ = ic.line_pencil(nx, ny)
    st, ref, x, y = _case(ctx, A, int(lines * nx), 4, "pencil, %g lines" % lines)
    r = max(itc.ratios_t(ref, x, st.PCApply(x)))
    print("pencil: the forward result sits at %.3g of the transposed bound" % r)
    assert r > 1.0


def test_unsorted_and_repeated_input(ctx):
    raw, S = ic.scrambled(200)
    x = _x(200, 5)
    y_raw = _st(ctx, _mat(ctx, raw), 64).PCApplyTranspose(x)
    y_sorted = _st(ctx, _mat(ctx, S), 64).PCApplyTranspose(x)
    assert np.array_equal(y_raw, y_sorted)
    itc.check_t(ic.Reference.of(ic.shifted(S, ic.SIGMA), 64), x, y_raw, "scrambled")


def test_setup_independence_repeatability_and_the_forward_side(ctx):
    """Shell and copy mode: identical bits. Two applications: identical bits. A new shift: new factors on both sides. PCApply returns the same
    bits with the switch on as with it off. Jacobi is its own transpose, bit for bit; dense blocks of 4 against the forward test's bound."""
    S = ic.random_sparse(300, 8, 6)
    A = _mat(ctx, S)
    x = _x(300, 6)
    y_off = _st(ctx, A, 128, transpose=False).PCApply(x)
    yt, yf = {}, {}
    for mode in ("shell", "copy"):
        st = _st(ctx, A, 128, mode=mode)
        assert st.GetTransposeSolves()
        yt[mode] = st.PCApplyTranspose(x); yf[mode] = st.PCApply(x)
        assert np.array_equal(st.PCApplyTranspose(x), yt[mode]), mode
        assert np.array_equal(yf[mode], y_off), mode
    assert np.array_equal(yt["shell"], yt["copy"])
    ref = ic.Reference.of(ic.shifted(S, ic.SIGMA), 128)
    itc.check_t(ref, x, yt["shell"], "sigma")
    assert max(itc.ratios_t(ref, x, y_off)) > 1.0                              # a non-symmetric block: M^-1 x is not M^-T x
    st.SetShift(-4.0)
    ref2 = ic.Reference.of(ic.shifted(S, -4.0), 128)
    y2 = st.PCApplyTranspose(x)
    itc.check_t(ref2, x, y2, "new sigma")
    ref2.check(x, st.PCApply(x), "new sigma, forward")
    assert not np.array_equal(y2, yt["copy"])
    st.SetShift(ic.SIGMA)
    assert np.array_equal(st.PCApplyTranspose(x), yt["copy"]) and np.array_equal(st.PCApply(x), y_off)
    st.SetPC("jacobi")
    assert np.array_equal(st.PCApplyTranspose(x), st.PCApply(x))
    st.SetPC("bjacobi", 4)
    y4 = st.PCApplyTranspose(x)
    P = ic.shifted(S, ic.SIGMA)
    D = sp.block_diag([P[i:i + 4, i:i + 4] for i in range(0, 300, 4)]).tocsr()
    assert abs(D - D.T).max() > 0.1                                             # the random matrix: D is not its transpose
    assert np.linalg.norm(D.T @ y4 - x) <= 1e-13 * np.linalg.norm(x)
    assert np.linalg.norm(D.T @ st.PCApply(x) - x) > 1e-3 * np.linalg.norm(x)
    # a last block shorter than 4 rows
    S2 = ic.random_sparse(302, 8, 7); P2 = ic.shifted(S2, ic.SIGMA); x2 = _x(302, 8)
    s2 = _st(ctx, _mat(ctx, S2), 4, pc="bjacobi")
    D2 = sp.block_diag([P2[i:i + 4, i:i + 4] for i in range(0, 302, 4)]).tocsr()
    assert np.linalg.norm(D2.T @ s2.PCApplyTranspose(x2) - x2) <= 1e-13 * np.linalg.norm(x2)


def test_two_matrices(ctx):
    n = 200
    Sa = ic.random_sparse(n, 5, 7); Sb = ic.random_sparse(n, 4, 8)
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    x = _x(n, 7)
    itc.check_t(ic.Reference.of(ic.shifted(Sa, ic.SIGMA, Sb), 64), x, _st(ctx, A, 64, B=B).PCApplyTranspose(x), "A - sigma B")
    itc.check_t(ic.Reference.of(Sb, 64), x, _st(ctx, A, 64, sigma=0.3, B=B, kind="shift").PCApplyTranspose(x), "P = B")
    itc.check_t(ic.Reference.of(ic.shifted(Sa, ic.SIGMA, Sb), 64), x, _st(ctx, A, 64, B=B, kind="cayley", mode="copy").PCApplyTranspose(x), "cayley")


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import slepc_amd as ks
    S = ic.random_sparse(100, 5, 8)
    A = _mat(ctx, S)
    x = np.ones(100)
    off = _st(ctx, A, 64, transpose=False)
    assert not off.GetTransposeSolves()
    for call in (off.PCApplyTranspose, off.MatSolveTranspose):
        with pytest.raises(ks.KsError) as e:
            call(x)
        assert e.value.rc == 56 and "ks_st_set_transpose_solves" in str(e.value)     # PETSC_ERR_SUP, the message names the switch
    on = _st(ctx, A, 64)
    W = ks.BV(ctx, 100, 2)
    with pytest.raises(ks.KsError) as e:
        on.PCApplyTransposeDev(W.column_ptr(0), W.column_ptr(0))
    assert e.value.rc == 61                                        # PETSC_ERR_ARG_IDN
    assert ctx.L.ks_st_matsolve_transpose(on.h, C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(0))) == 61
    s5 = ks.ST(ctx); s5.SetType("shift"); s5.SetShift(0.5); s5.SetMatrices(A); s5.SetTransposeSolves(True)
    for call in (s5.PCApplyTranspose, s5.MatSolveTranspose):
        with pytest.raises(ks.KsError) as e:
            call(x)
        assert e.value.rc == 58                                    # PETSC_ERR_ORDER: no linear solve
    # matrices that did not keep their CSR arrays: nothing to transpose, whatever the preconditioner
    for pc, bs in (("jacobi", 0), ("bjacobi-ilu", 64)):
        s2 = _st(ctx, _mat(ctx, S, keep=False), bs, pc=pc)
        with pytest.raises(ks.KsError) as e:
            s2.SetUp()
        assert e.value.rc == 58
    s3 = _st(ctx, A, 0, sigma=0.3, B=_mat(ctx, ic.random_sparse(100, 4, 9), keep=False), pc="jacobi")
    with pytest.raises(ks.KsError) as e:
        s3.SetUp()
    assert e.value.rc == 58


def test_two_ranks_are_refused():
    """The transpose of a row-sharded matrix is a redistribution: set-up with the switch on returns 56 on every rank."""
    N = 330
    S = ic.random_sparse(N, 8, 10)

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            r0, r1 = [(0, 200), (200, N)][rank]
            L = S[r0:r1].tocsr()
            A = ks.Mat.from_csr(ctx, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data, row_start=r0, n_global=N, keep_csr=True)
            st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(ic.SIGMA); st.SetMatrices(A); st.SetPC("bjacobi-ilu", 64); st.SetTransposeSolves(True)
            try:
                st.SetUp()
            except ks.KsError as e:
                return e.rc
            return 0
        finally:
            ctx.close()

    assert run_ranks(ThreadComm(2, pairwise=True, timeout=60), fn, join_timeout=120) == [56, 56]
