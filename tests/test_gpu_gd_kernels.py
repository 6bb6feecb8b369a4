"""The fused Ritz-residual sweep of Generalized Davidson (ks_bv_ritz_residual, slepc_amd/csrc/ks_gd.hip: k_ritz_residual).

Exact test. Integer-valued data with |V| <= 2^4, |AV| <= 2^6, |BV| <= 2^4, |S| <= 2^3, |theta| <= 2^3, m <= 40, n <= 4099: |x| <= 40 2^7 < 2^13,
|ax| < 2^15, |theta bx| < 2^16, so |r| < 2^17 and both sums of squares stay below 4099 2^34 < 2^47 - every product and every sum is exact in double
whatever the order. R must equal numpy's bit for bit, the norms must be within 2 ulp of the square roots of the exact integers.

The same exact test in the forms the sweep takes at workload size (tests/stream_cases.py): nontemporal loads of the panels, reached on a few rows with a
large leading dimension, and a second tile per workgroup at 2 num_cu 512 + 513 rows with narrower ranges (their bounds are in that test's docstring).
Every exact call also asserts the load form the library reports for it (Context.basis_load_counts).

Random doubles. Against a numpy.longdouble evaluation, entrywise |R - ref| <= (m + 2) eps (|AV||S| + |theta| |BV||S|): the bound of an m-term fma
chain (each term one rounding, gamma_m <= (m + 1) eps at these m) plus the final fma. rnorm against numpy.linalg.norm of the device R at relative
n eps (a sum of n squares, each rounded once). xnorm, whose vector is never stored, against the longdouble x: n eps ||x|| for the sum plus
(m + 1) eps || |V||S| ||_2 for the chain behind each entry."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
ARG_SIZ, ARG_WRONG, ARG_OUTOFRANGE, ARG_INCOMP, ARG_NULL = 60, 62, 63, 75, 85
MS = [1, 2, 7, 8, 9, 33, 40]
NCOLS = [1, 3, 8, 9, 16]
# every pass width the dispatch compiles (JT 1, 2, 4, 8 and, without B, 16) and, with B, second passes of 1, 2, 4 and 8 columns behind a first one of 8
NCOLS_EVERY_PASS = [1, 2, 3, 4, 5, 8, 9, 10, 12, 16]
WV, WR = 42, 19                      # columns of V / AV / BV (l <= 2, m <= 40) and of R (lR <= 3, ncols <= 16)


def _ints(rng, shape, bound):
    return rng.integers(-bound, bound + 1, size=shape).astype(np.float64)


def _odd_ld(n):
    return n + 3 if (n + 3) % 2 else n + 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("generalized", [False, True])
@pytest.mark.parametrize("odd_ld", [True, False])
def test_ritz_residual_exact(ctx, n, generalized, odd_ld):
    """Every (m, ncols) pair of MS x NCOLS on one set of panels, the active ranges cycling through l in {0, 2} and lR in {0, 3} (all four
    combinations with every m and every ncols over the two ld kinds), lds > m on every third call. Odd ld: the scalar path; the default ld: the
    16-byte path. Columns of R outside [lR, lR + ncols) and the three inputs keep their bits. At n = 65 and n = 4099 the result widths are those of
    NCOLS_EVERY_PASS. Panels of a few thousand rows: every call reports plain loads."""
    import slepc_amd as ks
    widths = NCOLS_EVERY_PASS if n in (65, 4099) else NCOLS
    rng = np.random.default_rng(7000 * n + 10 * generalized + odd_ld)
    ld = _odd_ld(n) if odd_ld else 0
    Vb, AVb, Rb = ks.BV(ctx, n, WV, ld=ld), ks.BV(ctx, n, WV, ld=ld), ks.BV(ctx, n, WR, ld=ld)
    BVb = ks.BV(ctx, n, WV, ld=ld) if generalized else None
    assert (Rb.ld % 2 == 1) == odd_ld
    V, AV, BV = _ints(rng, (n, WV), 16), _ints(rng, (n, WV), 64), _ints(rng, (n, WV), 16)
    Rm = _ints(rng, (n, WR), 7)
    Vb.set_dense(V); AVb.set_dense(AV); Rb.set_dense(Rm)
    if generalized:
        BVb.set_dense(BV)
    idx = int(odd_ld)
    for m in MS:
        idx += (len(widths) + 1) % 2 if m != MS[0] else 0                  # an odd stride from one m to the next: every width meets both l
        for ncols in widths:
            l = (0, 2)[idx % 2]; lR = (0, 3)[(idx // 2) % 2]; lds = m + (2 if idx % 3 == 0 else 0)
            idx += 1
            S = np.zeros((lds, ncols), order="F"); S[:m] = _ints(rng, (m, ncols), 8)
            S[m:] = 99.0                                                   # rows past m are not read
            theta = _ints(rng, ncols, 8); theta[0] = 0.0
            if ncols > 1:
                theta[1] = -3.0
            for b in (Vb, AVb) + ((BVb,) if generalized else ()):
                b.SetActiveColumns(l, l + m)
            Rb.SetActiveColumns(lR, WR)
            (rn, xn), counts = sc.counted(ctx, lambda: Rb.RitzResidual(Vb, AVb, BVb, S.ravel(order="F"), theta, ncols=ncols, lds=lds))
            assert counts == (1, 0), (m, ncols, counts)
            x = V[:, l:l + m] @ S[:m]; ax = AV[:, l:l + m] @ S[:m]; bx = BV[:, l:l + m] @ S[:m] if generalized else x
            ref = ax - bx * theta
            assert np.abs(ref).max() < 2.0 ** 17
            Rm[:, lR:lR + ncols] = ref
            R = Rb.dense()
            assert np.array_equal(R, Rm), (m, ncols, l, lR, np.argwhere(R != Rm)[:4])
            for got, vec in ((rn, ref), (xn, x)):
                exact = np.sqrt((vec * vec).sum(axis=0))
                assert np.all(np.abs(got - exact) <= 2 * np.spacing(exact)), (m, ncols, got, exact)
    assert np.array_equal(Vb.dense(), V) and np.array_equal(AVb.dense(), AV)
    if generalized:
        assert np.array_equal(BVb.dense(), BV)


# |V|, |AV|, |BV|, |S|, |theta| and the bound on |r| that follows: the ranges of test_ritz_residual_exact, and narrower ones for 2^18 rows and more
RANGES = (16, 64, 16, 8, 8, 2.0 ** 17)
RANGES_MANY_ROWS = (4, 16, 4, 4, 4, 2.0 ** 13)


def _ritz_case(ctx, rng, n, m, ncols, generalized, ld, form, l=0, lR=0, outs="", ranges=RANGES, nan=False):
    """ks_bv_ritz_residual on BVs only as wide as the case needs (V, AV, BV: l + m columns, R: lR + ncols), then, with outs ("x", "b" or "xb"),
    ks_bv_ritz_residual_vectors on the same inputs with X, BX or both: R, X and BX against numpy bit for bit, the norms within 2 ulp of the square
    roots of the exact integers, the same bits of R and of the norms from both calls, the inputs and the columns of R before lR unchanged. `form`:
    the load form the library must report for each call. nan: the storage beyond row n holds NaN bytes."""
    import slepc_amd as ks
    bV, bAV, bBV, bS, bT, rmax = ranges
    assert n * rmax * rmax < 2.0 ** 53 and n * (m * bV * bS) ** 2 < 2.0 ** 53          # both sums of squares are exact
    Vb, AVb, Rb = ks.BV(ctx, n, l + m, ld=ld), ks.BV(ctx, n, l + m, ld=ld), ks.BV(ctx, n, lR + ncols, ld=ld)
    BVb = ks.BV(ctx, n, l + m, ld=ld) if generalized else None
    Xb = ks.BV(ctx, n, ncols, ld=ld) if "x" in outs else None
    BXb = ks.BV(ctx, n, ncols, ld=ld) if "b" in outs else None
    every = [b for b in (Vb, AVb, BVb, Rb, Xb, BXb) if b is not None]
    if nan:
        sc.fill_nan(ctx, *every)
    V, AV, BV = _ints(rng, (n, l + m), bV), _ints(rng, (n, l + m), bAV), _ints(rng, (n, l + m), bBV)
    R0 = _ints(rng, (n, lR + ncols), 7)
    Vb.set_dense(V); AVb.set_dense(AV); Rb.set_dense(R0)
    if generalized:
        BVb.set_dense(BV)
    S = np.asfortranarray(_ints(rng, (m, ncols), bS))
    theta = _ints(rng, ncols, bT); theta[0] = 0.0
    if ncols > 1:
        theta[1] = -3.0
    for b in (Vb, AVb) + ((BVb,) if generalized else ()):
        b.SetActiveColumns(l, l + m)
    Rb.SetActiveColumns(lR, lR + ncols)
    x = V[:, l:] @ S; ax = AV[:, l:] @ S; bx = BV[:, l:] @ S if generalized else x
    ref = ax - bx * theta
    assert np.abs(ref).max() < rmax
    want = (1, 0) if form == "plain" else (0, 1)

    def check(rn, xn):
        for j in range(lR + ncols):
            got = Rb.column(j); exp = R0[:, j] if j < lR else ref[:, j - lR]
            assert np.array_equal(got, exp), (m, ncols, j, np.argwhere(got != exp)[:4])
        for got, vec in ((rn, ref), (xn, x)):
            exact = np.sqrt((vec * vec).sum(axis=0))
            assert np.all(np.abs(got - exact) <= 2 * np.spacing(exact)), (m, ncols, got, exact)

    (rn, xn), counts = sc.counted(ctx, lambda: Rb.RitzResidual(Vb, AVb, BVb, S, theta))
    assert counts == want, (form, counts)
    check(rn, xn)
    if outs:
        for j in range(ncols):
            Rb.set_column(lR + j, R0[:, lR + j])                                        # the second call has to write them again
        (rn2, xn2), counts = sc.counted(ctx, lambda: Rb.RitzResidualVectors(Vb, AVb, BVb, S, theta, X=Xb, BX=BXb))
        assert counts == want, (form, counts)
        check(rn2, xn2)
        assert np.array_equal(rn, rn2) and np.array_equal(xn, xn2)
        for out, vec in ((Xb, x), (BXb, bx)):
            for j in range(ncols if out is not None else 0):
                assert np.array_equal(out.column(j), vec[:, j]), (m, ncols, j)
    for b, M in ((Vb, V), (AVb, AV)) + (((BVb, BV),) if generalized else ()):
        b.SetActiveColumns(0, l + m)
        for j in range(l + m):
            assert np.array_equal(b.column(j), M[:, j])
    for b in every:
        b.destroy()


@pytest.mark.parametrize("n", [1, 511, 513, 4099])
@pytest.mark.parametrize("generalized", [False, True])
def test_ritz_residual_streaming_loads_exact(ctx, n, generalized):
    """k_ritz_residual<JT, 2, false, GEN, OUT> for every pass width, with and without the stored vectors: the data and the bounds of
    test_ritz_residual_exact on a few rows of BVs whose leading dimension puts 2 m + ncols columns (3 m + ncols with B) above the size at which the
    library streams the basis (stream_cases.streaming_ld asks the library). Every width of NCOLS_EVERY_PASS with three of the m of MS each; the
    rows n .. ld - 1 hold NaN bytes."""
    rng = np.random.default_rng(8000 * n + generalized)
    for i, ncols in enumerate(NCOLS_EVERY_PASS):
        for q, m in enumerate((MS[i % 7], MS[(i + 2) % 7], MS[(i + 5) % 7])):
            wide = m >= 7
            outs = ("x", "b", "xb" if m >= 33 else "x")[(i + q) % 3]
            ld = sc.streaming_ld(ctx, n, (3 if generalized else 2) * m + ncols)
            _ritz_case(ctx, rng, n, m, ncols, generalized, ld, "streaming", l=2 if wide else 0, lR=3 if wide and (i + q) % 2 else 0, outs=outs, nan=True)


@pytest.mark.parametrize("m,ncols,generalized,form", [(9, 3, False, "plain"), (40, 16, False, "streaming"), (33, 9, True, "streaming")])
def test_ritz_residual_second_tile_of_a_workgroup(ctx, m, ncols, generalized, form):
    """n = 2 num_cu 512 + 513 rows: more tiles than the two workgroups per CU of ks_ritz_residual, so every workgroup walks its first tile, some a
    second one (the sums of squares carried across, x / ax / bx started again), and the last tile is a single row. Ranges for this n:
    |V|, |BV|, |S|, |theta| <= 4, |AV| <= 16, m <= 40: |x| <= 640, |ax| <= 2560, |theta bx| <= 2560, |r| < 2^13; the sums of n < 2^21 squares stay
    below 2^47 and are exact. Narrow panels (m = 9, 3 result columns) stay resident: plain loads; the two wider ones stream."""
    num_cu = ctx.device_info()["num_cu"]
    n = sc.two_round_n(sc.RITZ_PER_CU, num_cu)
    ntiles, grid = sc.walk(n, sc.RITZ_PER_CU, num_cu)
    assert ntiles > grid and ntiles < 2 * grid and n % sc.TILE == 1 and n < 2 ** 21, (n, ntiles, grid)
    columns = (3 if generalized else 2) * m + ncols
    ld = sc.streaming_ld(ctx, n, columns) if form == "streaming" else sc.even_ld(n)
    rng = np.random.default_rng(31 * m + ncols)
    _ritz_case(ctx, rng, n, m, ncols, generalized, ld, form, outs="xb", ranges=RANGES_MANY_ROWS)


def _random_case(rng, n, m, ncols, generalized):
    V, AV = rng.standard_normal((n, m)), 4.0 * rng.standard_normal((n, m))
    BV = rng.standard_normal((n, m)) if generalized else None
    S = np.asfortranarray(rng.standard_normal((m, ncols))); theta = rng.standard_normal(ncols) * 3.0
    return V, AV, BV, S, theta


def _run(ctx, V, AV, BV, S, theta, ld=0, N=None, want_xnorm=True):
    import slepc_amd as ks
    n, m = V.shape; ncols = S.shape[1]
    Vb, AVb, Rb = ks.BV(ctx, n, m, ld=ld, N=N), ks.BV(ctx, n, m, ld=ld, N=N), ks.BV(ctx, n, ncols, ld=ld, N=N)
    BVb = ks.BV(ctx, n, m, ld=ld, N=N) if BV is not None else None
    if n:
        Vb.set_dense(V); AVb.set_dense(AV)
    if n and BV is not None:
        BVb.set_dense(BV)
    rn, xn = Rb.RitzResidual(Vb, AVb, BVb, S, theta, want_xnorm=want_xnorm)
    R = Rb.dense() if n else np.zeros((0, ncols))
    for b in (Vb, AVb, Rb, BVb):
        if b is not None:
            b.destroy()
    return R, rn, xn


@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("m,ncols", [(7, 3), (33, 9), (40, 16)])
@pytest.mark.parametrize("generalized", [False, True])
def test_ritz_residual_random_doubles(ctx, n, m, ncols, generalized):
    rng = np.random.default_rng(31 * n + 7 * m + ncols + generalized)
    V, AV, BV, S, theta = _random_case(rng, n, m, ncols, generalized)
    R, rn, xn = _run(ctx, V, AV, BV, S, theta)
    ld_ = np.longdouble
    x = V.astype(ld_) @ S.astype(ld_); ax = AV.astype(ld_) @ S.astype(ld_); bx = BV.astype(ld_) @ S.astype(ld_) if generalized else x
    ref = ax - bx * theta.astype(ld_)
    absx = np.abs(V) @ np.abs(S)
    bound = (m + 2) * EPS * (np.abs(AV) @ np.abs(S) + np.abs(theta) * (np.abs(BV) @ np.abs(S) if generalized else absx))
    err = np.abs(R.astype(ld_) - ref).astype(np.float64)
    print("n=%d m=%d ncols=%d gen=%d  max err / bound %.3f" % (n, m, ncols, generalized, (err / bound).max()))
    assert np.all(err <= bound)
    dn = np.linalg.norm(R, axis=0)
    assert np.all(np.abs(rn - dn) <= n * EPS * dn), (rn, dn)
    xr = np.sqrt((x * x).sum(axis=0)).astype(np.float64)
    assert np.all(np.abs(xn - xr) <= n * EPS * xr + (m + 1) * EPS * np.linalg.norm(absx, axis=0)), (xn, xr)
    # the same data on the scalar path (odd ld): identical bits of R; xnorm may be NULL
    R1, rn1, xn1 = _run(ctx, V, AV, BV, S, theta, ld=_odd_ld(n), want_xnorm=False)
    assert np.array_equal(R1, R) and xn1 is None
    assert np.all(np.abs(rn1 - dn) <= n * EPS * dn)


@pytest.mark.parametrize("generalized", [False, True])
def test_two_thread_ranks_give_the_bits_of_one_rank(ctx, generalized):
    """rows 0..2050 on rank 0 and the other 2048 on rank 1 (an odd and an even local size): row for row the bits of the one-rank R, the norms of
    all rows on both ranks"""
    import slepc_amd as ks
    n, m, ncols = 4099, 9, 9
    rng = np.random.default_rng(515 + generalized)
    V, AV, BV, S, theta = _random_case(rng, n, m, ncols, generalized)
    R, rn, xn = _run(ctx, V, AV, BV, S, theta)
    split = [(0, 2051), (2051, n)]

    def rank_fn(rank, comm):
        c = ks.Context(0)
        comm.install(c, rank)
        s0, s1 = split[rank]
        out = _run(c, V[s0:s1], AV[s0:s1], BV[s0:s1] if generalized else None, S, theta, N=n)
        c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    for rank, (s0, s1) in enumerate(split):
        Rr, rnr, xnr = res[rank]
        assert np.array_equal(Rr, R[s0:s1])
        assert np.all(np.abs(rnr - rn) <= n * EPS * rn) and np.all(np.abs(xnr - xn) <= n * EPS * xn)
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_no_local_rows_is_legal(ctx):
    rng = np.random.default_rng(3)
    V, AV, BV, S, theta = _random_case(rng, 0, 4, 2, True)
    R, rn, xn = _run(ctx, V, AV, BV, S, theta, N=8)
    assert np.array_equal(rn, np.zeros(2)) and np.array_equal(xn, np.zeros(2))


def test_ritz_residual_arguments(ctx):
    """every row of the error table of include/ksgpu.h"""
    import slepc_amd as ks
    n = 10
    R, V, AV, BV = ks.BV(ctx, n, 20), ks.BV(ctx, n, 8), ks.BV(ctx, n, 8), ks.BV(ctx, n, 8)
    S = np.zeros(8 * 17); th = np.zeros(17); rn = np.zeros(17); xn = np.zeros(17)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    f = ctx.L.ks_bv_ritz_residual
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn)) == 0
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 0, p(th), p(rn), p(xn)) == ARG_OUTOFRANGE
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 17, p(th), p(rn), p(xn)) == ARG_OUTOFRANGE
    assert f(R.h, V.h, AV.h, BV.h, p(S), 7, 4, p(th), p(rn), p(xn)) == ARG_SIZ              # lds < m
    V.SetActiveColumns(2, 6)
    assert f(R.h, V.h, AV.h, BV.h, p(S), 4, 4, p(th), p(rn), p(xn)) == 0                    # m = 4 now
    narrow = ks.BV(ctx, n, 5); longer = ks.BV(ctx, n + 1, 8); longer_r = ks.BV(ctx, n + 1, 20)
    assert f(R.h, V.h, narrow.h, BV.h, p(S), 4, 4, p(th), p(rn), p(xn)) == ARG_SIZ          # AV with fewer than k = 6 columns
    assert f(R.h, V.h, AV.h, narrow.h, p(S), 4, 4, p(th), p(rn), p(xn)) == ARG_SIZ          # BV likewise
    for same in ((R.h, R.h, AV.h, BV.h), (R.h, V.h, R.h, BV.h), (R.h, V.h, AV.h, R.h)):
        assert f(*same, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_WRONG
    for other in ((R.h, longer.h, AV.h, BV.h), (R.h, V.h, longer.h, BV.h), (R.h, V.h, AV.h, longer.h), (longer_r.h, V.h, AV.h, BV.h)):
        assert f(*other, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_INCOMP
    assert f(None, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_NULL
    assert f(R.h, None, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_NULL
    assert f(R.h, V.h, None, BV.h, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_NULL
    assert f(R.h, V.h, AV.h, BV.h, None, 8, 4, p(th), p(rn), p(xn)) == ARG_NULL
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, None, p(rn), p(xn)) == ARG_NULL
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), None, p(xn)) == ARG_NULL
    assert f(R.h, V.h, AV.h, None, p(S), 8, 4, p(th), p(rn), None) == 0                     # BV and xnorm may be NULL
    R.SetActiveColumns(17, 20)
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn)) == ARG_SIZ              # R has 3 columns from its first active one
