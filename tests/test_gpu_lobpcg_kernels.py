"""The two block kernels of LOBPCG and the ST entries around them.

k_block_residual (ks_bv_block_residual): integer-valued data small enough that every product and every sum is exact in double, so R must equal
numpy's bit for bit whatever the order of operations, and the squared norms are exact integers: the norm is within 2 ulp of their square root.
Every active width 1..16 in the three compiled forms - one row per lane, 16-byte plain loads, 16-byte nontemporal loads (a few rows with the large leading
dimension of tests/stream_cases.py) - and a second tile per workgroup; each call asserts the load form the library reports (Context.basis_load_counts).

ks_st_pc_apply_multi: every column against ks_st_pc_apply of that column, bit for bit, for every PC type; the ILU(0) blocks on the matrices of
tests/ilu_cases.py at the sizes where the passes of k_bjacobi_ilu_apply_multi change (ncols against the columns of a pass, the LDS budget at
block size 8192, short last blocks). ks_st_apply_mat under sinvert against the column loop."""
import ctypes as C

import numpy as np
import pytest

import ilu_cases as ic
import stream_cases as sc

pytestmark = pytest.mark.gpu

ARG_SIZ, ARG_WRONG = 60, 62


# ---- block residual ---------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _block_residual_case(ctx, n, bs, l, generalized, ld, form, nan=False):
    """One call on integer data (the bounds of test_block_residual_exact) against numpy, bit for bit; `form`: the load form the library must report
    for it, "plain" or "streaming". nan: the storage beyond row n holds NaN bytes."""
    import slepc_amd as ks
    rng = np.random.default_rng(1000 * (n % 100003) + 10 * bs + l)
    Rb, AXb, Xb = (ks.BV(ctx, n, bs, ld=ld) for _ in range(3))
    BXb = ks.BV(ctx, n, bs, ld=ld) if generalized else Xb
    assert Rb.ld > n
    if nan:
        sc.fill_nan(ctx, Rb, AXb, Xb, BXb)
    theta = _ints(rng, bs - l, -32, 32); theta[0] = 0.0
    if bs - l > 1:
        theta[1] = -3.0
    # one column at a time on the host: a panel of 16 columns and a million rows is 134 MB
    cols = []
    for j in range(bs):
        ax = _ints(rng, n, -1024, 1024); x = _ints(rng, n, -64, 64); bx = _ints(rng, n, -64, 64) if generalized else x
        r0 = _ints(rng, n, -7, 7)
        Rb.set_column(j, r0); AXb.set_column(j, ax); Xb.set_column(j, x)
        if generalized:
            BXb.set_column(j, bx)
        cols.append((ax, x, bx, r0))
    Rb.SetActiveColumns(l, bs)
    nrm, counts = sc.counted(ctx, lambda: Rb.BlockResidual(AXb, BXb, theta))
    assert counts == ((1, 0) if form == "plain" else (0, 1)), (form, counts)
    for j, (ax, x, bx, r0) in enumerate(cols):
        got = Rb.column(j)
        assert np.array_equal(Xb.column(j), x) and np.array_equal(AXb.column(j), ax)
        if generalized:
            assert np.array_equal(BXb.column(j), bx)
        if j < l:
            assert np.array_equal(got, r0), j
            continue
        ref = ax - bx * theta[j - l]
        assert np.abs(ref).max() < 2.0 ** 12
        assert np.array_equal(got, ref), (j, np.argwhere(got != ref)[:4])
        exact = np.sqrt((ref * ref).sum())
        assert abs(nrm[j - l] - exact) <= 2 * np.spacing(exact), (j, nrm[j - l], exact)
    for b in {Rb, AXb, Xb, BXb}:
        b.destroy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("bs,l", [(1, 0), (3, 0), (16, 0), (16, 2), (5, 2)])
@pytest.mark.parametrize("generalized", [True, False])
def test_block_residual_exact(ctx, n, bs, l, generalized):
    """|ax| <= 2^10, |bx| <= 2^6, |theta| <= 2^5: |r| < 2^12, the sum of n <= 4099 squares < 2^37 - all exact. ld > n (odd for the small sizes: the
    scalar path; the default even ld: the 16-byte path). Active range from column l: the columns before it keep their bits. theta holds 0 and a
    negative value. generalized = False: BX is the BV of X itself. Three blocks of a few thousand rows: the library reports plain loads."""
    _block_residual_case(ctx, n, bs, l, generalized, n + 3 if n < 257 else 0, "plain")


# the active widths test_block_residual_exact leaves out (it reaches 1, 3, 14 and 16): with them every k_block_residual<KT, VEC, true> is launched
@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("width", [2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15])
@pytest.mark.parametrize("generalized", [True, False])
def test_block_residual_exact_every_other_width(ctx, n, width, generalized):
    """n = 65 with ld = 67: the scalar path; n = 4099 with the default ld: the 16-byte path. Odd widths start at column 2 of a wider BV."""
    l = 2 if width % 2 else 0
    _block_residual_case(ctx, n, width + l, l, generalized, n + 2 if n == 65 else 0, "plain")


@pytest.mark.parametrize("n", [1, 511, 513, 4099])
@pytest.mark.parametrize("generalized", [True, False])
def test_block_residual_streaming_loads_exact(ctx, n, generalized):
    """k_block_residual<KT, 2, false> for every width: the same data and bounds on a few rows of BVs whose leading dimension puts three blocks of
    the active width above the size at which the library streams the basis (asked from the library: stream_cases.streaming_ld). The rows
    n .. ld - 1 hold NaN bytes. The odd widths from 3 start at column 1 of the BV (an even ld keeps the columns 16-byte aligned)."""
    for width in range(1, 17):
        l = 1 if width % 2 and width > 1 else 0
        _block_residual_case(ctx, n, width + l, l, generalized, sc.streaming_ld(ctx, n, 3 * width), "streaming", nan=True)


@pytest.mark.parametrize("width,form", [(1, "plain"), (2, "plain"), (16, "streaming")])
@pytest.mark.parametrize("generalized", [True, False])
def test_block_residual_second_tile_of_a_workgroup(ctx, width, form, generalized):
    """n = 8 num_cu 512 + 513 rows: more tiles than the largest grid ksl_block_residual can choose (the occupancy result, at most 8 workgroups per
    CU), so every workgroup walks its first tile, some a second one, and the last tile is a single row; with 8 per CU the partial sums of more than
    512 workgroups go through the general form of reduce_partials_to_lds. |r| < 2^12: the sum of n < 2^21 squares stays below 2^45, exact as
    before. Three blocks of 1 and 2 columns stay resident (plain loads), of 16 columns they stream."""
    num_cu = ctx.device_info()["num_cu"]
    n = sc.two_round_n(sc.BLOCK_RESIDUAL_PER_CU, num_cu)
    ntiles, grid = sc.walk(n, sc.BLOCK_RESIDUAL_PER_CU, num_cu)
    assert ntiles > grid and ntiles < 2 * grid and n % sc.TILE == 1 and n < 2 ** 21, (n, ntiles, grid)
    ld = sc.streaming_ld(ctx, n, 3 * width) if form == "streaming" else sc.even_ld(n)
    _block_residual_case(ctx, n, width, 0, generalized, ld, form)


def test_block_residual_arguments(ctx):
    import slepc_amd as ks
    R = ks.BV(ctx, 10, 17); AX = ks.BV(ctx, 10, 17); X = ks.BV(ctx, 10, 17)
    th = np.zeros(17); out = np.zeros(17)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert ctx.L.ks_bv_block_residual(R.h, AX.h, X.h, p(th), p(out)) == 63           # 17 active columns
    R.SetActiveColumns(0, 4)
    assert ctx.L.ks_bv_block_residual(R.h, R.h, X.h, p(th), p(out)) == ARG_WRONG
    assert ctx.L.ks_bv_block_residual(R.h, AX.h, ks.BV(ctx, 11, 17).h, p(th), p(out)) == 75
    assert ctx.L.ks_bv_block_residual(R.h, AX.h, X.h, p(th), p(out)) == 0


# ---- ks_st_pc_apply_multi -----------------------------------------------------------------------------------------------------------------
def _mat(ctx, S):
    import slepc_amd as ks
    return ks.Mat.from_csr(ctx, *ic.arrays(S), keep_csr=True)


def _st(ctx, A, pc, bs=0, kind="precond", B=None):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(ic.SIGMA); st.SetMatrices(A, B); st.SetPC(pc, bs)
    return st


def _multi_against_columns(ctx, st, n, ncols, seed, ldx=0, ldy=0):
    """the block through ks_st_pc_apply_multi with the given leading dimensions against ks_st_pc_apply column by column; Y starts as a pattern
    that must survive between the columns (rows n .. ldy - 1)"""
    import slepc_amd as ks
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, ncols))
    Xb = ks.BV(ctx, n, ncols, ld=ldx); Yb = ks.BV(ctx, n, ncols, ld=ldy)
    Xb.set_dense(X)
    st.PCApplyMultiDev(Xb.column_ptr(0), Xb.ld, Yb.column_ptr(0), Yb.ld, ncols)
    Y = Yb.dense()
    for j in range(ncols):
        yj = st.PCApply(X[:, j])
        assert np.array_equal(Y[:, j], yj), (j, np.abs(Y[:, j] - yj).max())
    assert np.all(np.isfinite(Y))
    return X, Y


@pytest.mark.parametrize("pc,bs", [("none", 0), ("jacobi", 0), ("bjacobi", 2), ("bjacobi", 32)])
@pytest.mark.parametrize("ncols", [1, 5, 16])
def test_pointwise_and_dense_block_preconditioners(ctx, pc, bs, ncols):
    S = ic.random_sparse(203, 6, 11)
    st = _st(ctx, _mat(ctx, S), pc, bs)
    X, Y = _multi_against_columns(ctx, st, 203, ncols, 12, ldx=203 + 5, ldy=203 + 9)
    if pc == "none":
        assert np.array_equal(X, Y)
    if pc == "jacobi":
        assert np.allclose(Y, X / (S.diagonal() - ic.SIGMA)[:, None], rtol=1e-15)


@pytest.mark.parametrize("ncols", [1, 2, 7, 8, 9, 16])
def test_ilu_blocks_of_64(ctx, ncols):
    """n = 200: three full blocks and one of 8 rows; 9 columns cross a pass of 8; ldx != ldy, both > n"""
    S = ic.random_sparse(200, 6, 21)
    st = _st(ctx, _mat(ctx, S), "bjacobi-ilu", 64)
    assert st.PCMultiColumns() == 8                     # the multi-column kernel runs here
    X, Y = _multi_against_columns(ctx, st, 200, ncols, 22, ldx=200 + 6, ldy=200 + 10)
    ref = ic.Reference.of(ic.shifted(S, ic.SIGMA), 64)
    ref.check(X[:, ncols - 1], Y[:, ncols - 1], "ilu 64, last of %d columns" % ncols)


def test_ilu_blocks_of_8192_two_columns_per_pass(ctx):
    """n = 8197: a block of 8192 rows and one of 5 rows, three columns"""
    S = ic.random_sparse(8197, 6, 31)
    st = _st(ctx, _mat(ctx, S), "bjacobi-ilu", 8192)
    assert st.PCMultiColumns() == 1                     # measured slower than the column loop at this block size: dispatched to the loop
    _multi_against_columns(ctx, st, 8197, 3, 32)


def test_ilu_blocks_of_512_the_largest_on_the_multi_column_kernel(ctx):
    """n = 1029: two blocks of 512 rows and one of 5; 9 columns = a pass of eight (32 KB of LDS) and a single one"""
    S = ic.random_sparse(1029, 6, 45)
    st = _st(ctx, _mat(ctx, S), "bjacobi-ilu", 512)
    assert st.PCMultiColumns() == 8
    _multi_against_columns(ctx, st, 1029, 9, 46)
    st513 = _st(ctx, _mat(ctx, S), "bjacobi-ilu", 513)
    assert st513.PCMultiColumns() == 1


def test_ilu_blocks_of_2048_eight_columns(ctx):
    S = ic.random_sparse(2049, 6, 41)
    st = _st(ctx, _mat(ctx, S), "bjacobi-ilu", 2048)
    assert st.PCMultiColumns() == 1
    _multi_against_columns(ctx, st, 2049, 8, 42)


def test_ilu_on_the_convection_pencil_under_sinvert(ctx):
    """the existing transformation keeps its preconditioner entry: sinvert with B, blocks of 2.5 grid lines"""
    A, B = ic.line_pencil(32, 11)
    st = _st(ctx, _mat(ctx, A), "bjacobi-ilu", 80, kind="sinvert", B=_mat(ctx, B))
    _multi_against_columns(ctx, st, 352, 5, 51)


def test_argument_errors(ctx):
    import slepc_amd as ks
    n = 100
    st = _st(ctx, _mat(ctx, ic.random_sparse(n, 5, 61)), "jacobi")
    W = ks.BV(ctx, n, 6)
    L = ctx.L
    x, y = C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(3))
    for f in (L.ks_st_pc_apply_multi, L.ks_st_apply_mat):
        assert f(st.h, 2, x, n - 1, y, W.ld) == ARG_SIZ
        assert f(st.h, 2, x, W.ld, y, n - 1) == ARG_SIZ
        assert f(st.h, 2, x, W.ld, x, W.ld) == ARG_WRONG
        assert f(st.h, 4, x, W.ld, y, W.ld) == ARG_WRONG                           # columns 0..3 overlap columns 3..6
        before = W.dense()
        assert f(st.h, 0, x, W.ld, y, W.ld) == 0
        assert np.array_equal(W.dense(), before)
        assert f(st.h, 3, x, W.ld, y, W.ld) == 0
    with pytest.raises(ks.KsError):
        st.SetPC(7)


def test_precond_apply_is_the_preconditioner(ctx):
    """KS_ST_PRECOND: STApply and STApplyMat are PCApply; the default PC is point Jacobi on A - sigma B with sigma the shift"""
    import slepc_amd as ks
    A, B = ic.line_pencil(16, 7)
    st = ks.ST(ctx); st.SetType("precond"); st.SetShift(-0.5); st.SetMatrices(_mat(ctx, A), _mat(ctx, B))
    x = np.random.default_rng(71).standard_normal(112)
    y = st.Apply(x)
    assert np.array_equal(y, st.PCApply(x))
    assert np.allclose(y, x / (A.diagonal() + 0.5 * B.diagonal()), rtol=1e-15)
    X = np.random.default_rng(72).standard_normal((112, 3))
    Y = st.ApplyMat(X)
    for j in range(3):
        assert np.array_equal(Y[:, j], st.PCApply(X[:, j]))


def test_apply_mat_under_sinvert_is_the_column_loop(ctx):
    A, B = ic.line_pencil(16, 7)
    st = _st(ctx, _mat(ctx, A), "jacobi", kind="sinvert", B=_mat(ctx, B))
    X = np.random.default_rng(81).standard_normal((112, 3))
    Y = st.ApplyMat(X)
    for j in range(3):
        assert np.array_equal(Y[:, j], st.Apply(X[:, j])), j
