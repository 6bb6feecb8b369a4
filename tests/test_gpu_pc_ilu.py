"""Block Jacobi with ILU(0) blocks on the ST's KSP (KS_PC_BJACOBI_ILU, ks_st_pc_apply; k_bjacobi_ilu_apply in slepc_amd/csrc/ks_pc.hip).

The kernel is checked on its own through PCApply against a numpy ILU(0) of every block (tests/ilu_cases.py: same pattern rule, same IKJ order)
with the componentwise bound  |M y - x| <= 8 (k + 1) 2^-53 (|L||U||y|),  M = L U of that reference, k the block's longest row - no tuned tolerance.
Unless a test says otherwise: sinvert with one matrix, a shift that makes P = A - sigma I strictly diagonally dominant, shell mode."""

import numpy as np
import pytest
import scipy.sparse as sp

import ilu_cases as ic
from oracle import oracle as O
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu


def _line_pencil(nx, ny):
    """The pencil of tests/test_gpu_st.py: a 2-D 5-point Laplacian with a convective term (non-symmetric) and a diagonal mass matrix."""
    return ic.line_pencil(nx, ny)


def _mat(ctx, S, keep=True, **kw):
    import slepc_amd as ks
    rp, col, val = S if isinstance(S, tuple) else ic.arrays(S)
    return ks.Mat.from_csr(ctx, rp, col, val, keep_csr=keep, **kw)


def _ocsr(S):
    return O.CSR(S.shape[0], *ic.arrays(S))


def _st(ctx, A, bs, sigma=ic.SIGMA, B=None, kind="sinvert", mode="shell", pc="bjacobi-ilu"):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(A, B); st.SetMatMode(mode); st.SetPC(pc, bs)
    return st


def _x(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _pcapply_case(ctx, S, bs, seed, what):
    st = _st(ctx, _mat(ctx, S), bs)
    x = _x(S.shape[0], seed)
    y = st.PCApply(x)
    ic.Reference.of(ic.shifted(S, ic.SIGMA), bs).check(x, y, what)
    return st, x, y


# ---- the kernel cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64 * 3 + 1, 63])
def test_partial_blocks(ctx, n):
    """Three full blocks and a last block of one row; a single block shorter than the block size."""
    _pcapply_case(ctx, ic.random_sparse(n, 6, n), 64, 1, "partial n=%d" % n)


@pytest.mark.parametrize("bs", [8192, 64])
@pytest.mark.parametrize("kind", ["diagonal", "bidiagonal"])
def test_one_wide_level_and_the_longest_chain_of_levels(ctx, kind, bs):
    """A diagonal P is one level of bs rows (more rows than lanes at 8192: the level is strided over); a lower-bidiagonal P is bs levels of one
    row in the L solve - the longest chain of barriers. Two blocks, the second one short."""
    n = bs + bs // 2 + 3
    S = ic.diagonal(n) if kind == "diagonal" else ic.bidiagonal(n)
    _pcapply_case(ctx, S, bs, 2, "%s bs=%d" % (kind, bs))


def test_largest_column_code_and_longest_rows(ctx):
    """A block of 8192 rows whose last row is dense to the left and whose first row is dense to the right: rows of 8192 entries, levels of one
    row with 8191 slots beside a level of 8191 rows, column code 8191."""
    _pcapply_case(ctx, ic.arrow(8192), 8192, 3, "arrow")


@pytest.mark.parametrize("lines", [4, 2.5])
def test_mixed_level_widths_on_the_convection_pencil(ctx, lines):
    """Blocks of 4 and of 2.5 grid lines of the 2-D pencil: the levels are the diagonal wavefronts of the grid, of every width from 1 up, and the
    blocks cut through the couplings to the neighbouring lines (and, at 2.5, through a line), which are dropped."""
    nx, ny = 32, 11
    A, _ = _line_pencil(nx, ny)
    _pcapply_case(ctx, A, int(lines * nx), 4, "pencil, %g lines" % lines)


def test_unsorted_and_repeated_input(ctx):
    """Kept CSR arrays with unsorted columns and repeated entries (the diagonal three times): the result of the summed, sorted matrix, bit for bit."""
    raw, S = ic.scrambled(200)
    x = _x(200, 5)
    y_raw = _st(ctx, _mat(ctx, raw), 64).PCApply(x)
    y_sorted = _st(ctx, _mat(ctx, S), 64).PCApply(x)
    assert np.array_equal(y_raw, y_sorted)
    ic.Reference.of(ic.shifted(S, ic.SIGMA), 64).check(x, y_raw, "scrambled")


def test_setup_independence_and_repeatability(ctx):
    """Shell and copy mode take the blocks from the same kept arrays: identical bits. Two applications: identical bits. A new shift: new factors."""
    S = ic.random_sparse(300, 8, 6)
    A = _mat(ctx, S)
    x = _x(300, 6)
    ys = {}
    for mode in ("shell", "copy"):
        st = _st(ctx, A, 128, mode=mode)
        ys[mode] = st.PCApply(x)
        assert np.array_equal(st.PCApply(x), ys[mode]), mode
    assert np.array_equal(ys["shell"], ys["copy"])
    ic.Reference.of(ic.shifted(S, ic.SIGMA), 128).check(x, ys["shell"], "sigma")
    st.SetShift(-4.0)
    y2 = st.PCApply(x)
    ic.Reference.of(ic.shifted(S, -4.0), 128).check(x, y2, "new sigma")
    assert not np.array_equal(y2, ys["copy"])
    st.SetShift(ic.SIGMA)
    assert np.array_equal(st.PCApply(x), ys["copy"])
    # the other two preconditioners through the same entry
    st.SetPC("jacobi")
    P = ic.shifted(S, ic.SIGMA)
    assert np.allclose(st.PCApply(x), x / P.diagonal(), rtol=4 * 2.0 ** -52, atol=0)       # x * (1 / d) against x / d
    st.SetPC("bjacobi", 4)
    y4 = st.PCApply(x)
    D = sp.block_diag([P[i:i + 4, i:i + 4] for i in range(0, 300, 4)]).tocsr()
    assert np.linalg.norm(D @ y4 - x) <= 1e-13 * np.linalg.norm(x)


def test_two_matrices(ctx):
    """sinvert: P = A - sigma B, entry by entry a_ij + (-sigma b_ij) on the union of the patterns; shift with two matrices: P = B."""
    n = 200
    Sa = ic.random_sparse(n, 5, 7); Sb = ic.random_sparse(n, 4, 8)
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    x = _x(n, 7)
    y = _st(ctx, A, 64, B=B).PCApply(x)
    ic.Reference.of(ic.shifted(Sa, ic.SIGMA, Sb), 64).check(x, y, "A - sigma B")
    y = _st(ctx, A, 64, sigma=0.3, B=B, kind="shift").PCApply(x)
    ic.Reference.of(Sb, 64).check(x, y, "P = B")
    y = _st(ctx, A, 64, B=B, kind="cayley", mode="copy").PCApply(x)
    ic.Reference.of(ic.shifted(Sa, ic.SIGMA, Sb), 64).check(x, y, "cayley")


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import slepc_amd as ks
    S = ic.random_sparse(100, 5, 8)
    A = _mat(ctx, S)
    st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(ic.SIGMA); st.SetMatrices(A)
    for bad in (63, 8193):
        with pytest.raises(ks.KsError) as e:
            st.SetPC("bjacobi-ilu", bad)
        assert e.value.rc == 63                                    # PETSC_ERR_ARG_OUTOFRANGE
    with pytest.raises(ks.KsError) as e:
        st.SetPC("bjacobi", 33)                                     # the dense blocks keep their limits
    assert e.value.rc == 63
    with pytest.raises(ks.KsError) as e:
        st.SetPC(3, 64)
    assert e.value.rc == 56
    # matrices that did not keep their CSR arrays
    s2 = _st(ctx, _mat(ctx, S, keep=False), 64)
    with pytest.raises(ks.KsError) as e:
        s2.SetUp()
    assert e.value.rc == 58                                        # PETSC_ERR_ORDER
    # a row of a block without a stored diagonal entry (P = B of a two-matrix shift: with one matrix the shift itself stores every diagonal entry)
    T = sp.lil_matrix(ic.shifted(S, ic.SIGMA)); T[70, 70] = 0.0; T = T.tocsr(); T.eliminate_zeros()
    s3 = _st(ctx, A, 64, sigma=0.1, B=_mat(ctx, T), kind="shift")
    with pytest.raises(ks.KsError) as e:
        s3.SetUp()
    assert e.value.rc == 73 and "diagonal" in str(e.value) and "70" in str(e.value)      # PETSC_ERR_ARG_WRONGSTATE
    # ILU(0) meets an exact zero pivot: a leading 2 x 2 block [[1, 1], [1, 1]] (P = B of a two-matrix shift, so that no shift touches it)
    Z = sp.lil_matrix(ic.shifted(S, ic.SIGMA)); Z[0, :] = 0.0; Z[1, :] = 0.0; Z[0, 0] = Z[0, 1] = Z[1, 0] = Z[1, 1] = 1.0
    s4 = _st(ctx, A, 64, sigma=0.1, B=_mat(ctx, Z.tocsr()), kind="shift")
    with pytest.raises(ks.KsError) as e:
        s4.SetUp()
    assert e.value.rc == 71 and "row 1" in str(e.value)           # PETSC_ERR_MAT_LU_ZRPVT
    # PCApply: x == y; a transformation without a solve
    st.SetPC("bjacobi-ilu", 64)
    W = ks.BV(ctx, 100, 2)
    with pytest.raises(ks.KsError) as e:
        st.PCApplyDev(W.column_ptr(0), W.column_ptr(0))
    assert e.value.rc == 61                                        # PETSC_ERR_ARG_IDN
    s5 = ks.ST(ctx); s5.SetType("shift"); s5.SetShift(0.5); s5.SetMatrices(A)
    with pytest.raises(ks.KsError) as e:
        s5.PCApply(np.ones(100))
    assert e.value.rc == 58


# ---- solves -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pencil():
    nx, ny, sigma = 24, 30, -0.5
    Sa, Sb = _line_pencil(nx, ny)
    x = _x(nx * ny, 21)
    Ao, Bo = _ocsr(Sa), _ocsr(Sb)
    ref = {"sinvert": O.ST(Ao, Bo, "sinvert", sigma).apply(x), "cayley": O.ST(Ao, Bo, "cayley", sigma, nu=2.0).apply(x)}
    return nx, ny, sigma, Sa, Sb, x, ref


@pytest.mark.parametrize("kind", ["sinvert", "cayley"])
@pytest.mark.parametrize("ksp", ["gmres", "bcgs"])
def test_solves_agree_with_the_lu_oracle(ctx, pencil, ksp, kind):
    nx, ny, sigma, Sa, Sb, x, ref = pencil
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    for bs, mode in ((4 * nx, "shell"), (64, "copy")):
        st = _st(ctx, A, bs, sigma=sigma, B=B, kind=kind, mode=mode)
        if kind == "cayley":
            st.CayleySetAntishift(2.0)
        st.SetKSP(rtol=1e-12); st.SetKSPType(ksp)
        y = st.Apply(x)
        assert np.linalg.norm(y - ref[kind]) <= 1e-9 * np.linalg.norm(ref[kind]), (bs, mode)


def _cpu_gmres_iterations(P, minv, b, rtol, restart=30):
    """The library's inner solve restated with scipy: GMRES(30) on M^-1 P y = M^-1 b, zero guess, relative tolerance on the preconditioned residual."""
    import scipy.sparse.linalg as spl
    n = P.shape[0]
    its = [0]

    def count(_):
        its[0] += 1
    _, info = spl.gmres(spl.LinearOperator((n, n), matvec=lambda v: minv(P @ v)), minv(b), rtol=rtol, atol=0.0, restart=restart, maxiter=1000,
                        callback=count, callback_type="pr_norm")
    assert info == 0
    return its[0]


def test_ilu_blocks_take_fewer_iterations_than_point_jacobi(ctx, pencil):
    """The 24 x 30 pencil at sigma = -0.5, blocks of 4 grid lines (96 rows), GMRES(30) to 1e-12: restated on the CPU with scipy's gmres, point
    Jacobi takes 26 iterations and the ILU(0) blocks 10 - a gap of 2.6, far above the 1.5 below which the comparison would not be asserted."""
    nx, ny, sigma, Sa, Sb, x, ref = pencil
    P = ic.shifted(Sa, sigma, Sb)
    d = P.diagonal()
    cpu = {"jacobi": _cpu_gmres_iterations(P, lambda v: v / d, x, 1e-12), "ilu": _cpu_gmres_iterations(P, ic.Reference.of(P, 4 * nx).solve, x, 1e-12)}
    print("CPU restatement:", cpu)
    assert cpu["jacobi"] >= 1.5 * cpu["ilu"], cpu
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    its = {}
    for label, pc, bs in (("jacobi", "jacobi", 0), ("ilu", "bjacobi-ilu", 4 * nx)):
        st = _st(ctx, A, bs, sigma=sigma, B=B, pc=pc); st.SetKSP(rtol=1e-12)
        y = st.Apply(x)
        assert np.linalg.norm(y - ref["sinvert"]) <= 1e-9 * np.linalg.norm(ref["sinvert"])
        its[label] = st.GetKSPStats()["iterations"]
    print("GPU:", its)
    assert its["ilu"] < its["jacobi"], (its, cpu)


def test_a_whole_eigensolve_through_the_ilu_preconditioned_solves(ctx):
    """The eigensolve of test_block_jacobi_errors_and_a_whole_solve (tests/test_gpu_st.py) with ILU(0) blocks of 64 rows."""
    import slepc_amd as ks
    Sa, Sb = _line_pencil(16, 20)
    Ao, Bo = _ocsr(Sa), _ocsr(Sb)
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    sigma = -0.5
    eps = ks.EPS(ctx); eps.SetOperators(A, B); eps.SetProblemType(ks.EPS_GNHEP); eps.SetDimensions(4, 16); eps.SetTarget(sigma)
    s3 = eps.GetST(); s3.SetType("sinvert"); s3.SetKSP(rtol=1e-12); s3.SetPC("bjacobi-ilu", 64)
    eps.Solve()
    r = O.eps_krylovschur_nhep(Ao, 4, ncv=16, which=O.which_target_magnitude(sigma), st=O.ST(Ao, Bo, "sinvert", sigma))
    assert eps.GetConverged() >= 4 and eps.GetIterationNumber() == r.its
    lam = np.array([complex(*eps.GetEigenvalue(i)) for i in range(4)])
    assert np.allclose(lam, (r.eigr + 1j * r.eigi)[r.perm][:4], rtol=1e-9, atol=0)


# ---- ranks --------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_one_of_them_without_rows():
    """Two ranks as threads of this process, each with its own blocks: a rank's blocks are cut from ITS rows (the first one starts at its first
    row) and the columns other ranks own are dropped, so PCApply on a rank equals the reference built from that rank's rows and columns alone.
    Rows 0..199 | 200..329 (four blocks, the last of 8 rows | three blocks, the last of 2), then every row on rank 0 and none on rank 1."""
    N = 330
    S = ic.random_sparse(N, 8, 10)
    P = ic.shifted(S, ic.SIGMA)
    xg = _x(N, 10)

    def body(split):
        def fn(rank, comm):
            import slepc_amd as ks
            ctx = ks.Context(0)
            try:
                comm.install(ctx, rank)
                r0, r1 = split[rank]
                L = S[r0:r1].tocsr()
                A = ks.Mat.from_csr(ctx, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data, row_start=r0, n_global=N, keep_csr=True)
                st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(ic.SIGMA); st.SetMatrices(A); st.SetPC("bjacobi-ilu", 64)
                W = ks.BV(ctx, r1 - r0, 2, N=N)
                W.set_column(0, xg[r0:r1])
                st.PCApplyDev(W.column_ptr(0), W.column_ptr(1))
                return W.column(1)
            finally:
                ctx.close()
        return fn

    for split in ([(0, 200), (200, N)], [(0, N), (N, N)]):
        out = run_ranks(ThreadComm(2, pairwise=True, timeout=60), body(split), join_timeout=120)
        for rank, (r0, r1) in enumerate(split):
            assert out[rank].shape == (r1 - r0,)
            if r1 > r0:
                ic.Reference.of(P[r0:r1, r0:r1], 64).check(xg[r0:r1], out[rank], "rank %d of %s" % (rank, split))
