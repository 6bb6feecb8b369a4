"""The transposed product of a row-sharded matrix (KS_MAT_SHARDED_TRANSPOSE: Mat.from_csr(..., sharded_transpose=True)) and what is built on it:
the transposed view, the block product on the view, two-sided Krylov-Schur and two-sided balancing across ranks, and the refusals that stay.

Products run on the matrices of tests/sharded_cases.py: integer (or k / 1024) values and integer vectors, so A^T x is exact in binary64 in ANY
summation order - the transposed diagonal block in whatever layout it took, the sums of the ghost rows, the accumulation of the other ranks'
contributions - and is compared with the integer reference c.int_matrix().T @ x by np.array_equal. Checked on the CPU below: |A^T x| scale < 2^53
for every case and vector used. One case (normal values) has a derived bound.

Ranks are threads (tests/thread_comm.py, pairwise exchange: a rank without peers never enters an exchange), each with its own Context."""
import functools

import numpy as np
import pytest

import golden_inputs as gi
import layout_cases as lc
import nhep_cases as nc
import sharded_cases as sc
import twosided_cases as TS
from oracle import oracle as O
from thread_comm import ThreadComm, run_ranks

KS_ERR_SUP, KS_ERR_ARG_INCOMP = 56, 75          # include/ksgpu.h
NVEC = 3
TOL = 1e-8
EPS = np.finfo(float).eps
PRODUCT_CASES = [("far", 4), ("far", 8), ("islands", 4), ("bighalo", 2), ("bighalo", 4)]


@functools.lru_cache(maxsize=None)
def case(name, world=4):
    if name == "far":
        return sc.far(world)
    if name == "far_even":
        return sc.far(4, seed=9, counts=sc.FAR_EVEN)
    if name == "float":
        return sc.far(world, values="normal")
    if name == "islands":
        return sc.islands()
    if name == "bighalo":
        return sc.bighalo(world)
    if name == "layouts-int":
        return sc.layouts("int")
    if name == "layouts-dyadic":
        return sc.layouts("dyadic")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def vectors(name, world=4):
    """(x, exact A^T x, exact A x) for NVEC integer vectors: computed once per case, shared by every test, never written to."""
    c = case(name, world)
    xs = sc.int_vectors(c.N, NVEC, seed=100 + c.N % 97)
    At = c.int_matrix().T.tocsr()
    yt = np.stack([(At @ x.astype(np.int64)) / float(c.scale) for x in xs])
    yf = np.stack([c.reference(x) for x in xs])
    for a in (xs, yt, yf):
        a.setflags(write=False)
    return xs, yt, yf


def transposed_diagonal_block(c, rank):
    """(rowptr, col, val) of the transposed diagonal block of a rank as the plan builds it: entries of a column by ascending row, stable."""
    r0, r1 = c.range(rank)
    rp, col, val = c.block(rank)
    n = r1 - r0
    rows = np.repeat(np.arange(n), np.diff(rp))
    loc = (col >= r0) & (col < r1)
    key = col[loc] - r0
    order = np.argsort(key, kind="stable")
    trp = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))]).astype(np.int32)
    return trp, rows[loc][order].astype(np.int32), val[loc][order]


# forced layout -> (case, layout the VIEW must report on every rank); None: the chooser's own pick. The dictionary and SELL rows are predicted on
# the CPU from the transposed diagonal blocks (layout_cases.predict_layout, test_cases_deliver_what_the_gpu_tests_rely_on); the three CSR forms
# are CSR for any matrix (choose_layout returns before any builder); binned and sliced take any block of at least 4096 rows with entries.
LAYOUT_CASES = {
    "csr": [("layouts-int", "csr"), ("far_even", "csr")],
    "csrvec": [("layouts-int", "csr"), ("far_even", "csr")],
    "csrregs": [("layouts-int", "csr"), ("far_even", "csr")],
    "sell": [("layouts-int", "sell"), ("layouts-dyadic", "sell"), ("far_even", "sell")],
    "dict": [("layouts-int", "dict"), ("layouts-dyadic", "odict"), ("far_even", "csr")],
    "odict": [("layouts-int", "odict"), ("layouts-dyadic", "odict"), ("far_even", "csr")],
    "binned": [("layouts-int", "binned"), ("far_even", "binned")],
    "sliced": [("layouts-int", "sliced"), ("far_even", "sliced")],
    None: [("layouts-int", "dict"), ("layouts-dyadic", "odict"), ("far_even", "csr")],
}


# ---- what the GPU tests rely on, on the CPU ------------------------------------------------------------------------------------------------
def test_cases_deliver_what_the_gpu_tests_rely_on():
    for name, world in PRODUCT_CASES + [("layouts-int", 4), ("layouts-dyadic", 4), ("far_even", 4)]:
        c = case(name, world)
        xs, yt, yf = vectors(name, world)
        assert np.abs(xs).max() <= 64 and np.array_equal(xs, np.rint(xs))
        assert np.abs(yt).max() * c.scale < 2.0 ** 53 and np.abs(yf).max() * c.scale < 2.0 ** 53
        col_sums = np.bincount(c.col, weights=np.abs(c.ival).astype(np.float64), minlength=c.N)
        assert col_sums.max() * 64 < 2.0 ** 53                      # every partial sum of every column, in any order
    c = case("islands")
    assert c.N - len(np.unique(c.col)) == 3                          # three columns without entries: their y is +0.0
    for fmt, rows in LAYOUT_CASES.items():
        if fmt in ("csr", "csrvec", "csrregs", "binned"):
            continue
        for name, want in rows:
            c = case(name)
            for rank in range(4):
                got = lc.predict_layout(*transposed_diagonal_block(c, rank), force=fmt)
                assert got[0] == want and (fmt is not None or name != "layouts-int" or got[1] == 8), (fmt, name, rank, got)
    for name in ("layouts-int", "far_even"):                         # binned / sliced: at least 4096 rows and entries on every rank
        c = case(name)
        for rank in range(4):
            trp = transposed_diagonal_block(c, rank)[0]
            assert len(trp) - 1 >= 4096 and trp[-1] > 0


# ---- rank bodies ----------------------------------------------------------------------------------------------------------------------------
def _open(rank, comm):
    import slepc_amd as ks
    ctx = ks.Context(0)
    comm.install(ctx, rank)
    return ks, ctx


def _mat(ks, ctx, c, rank, keep_csr=True, sharded_transpose=True):
    rp, col, val = c.block(rank)
    return ks.Mat.from_csr(ctx, rp, col, val, row_start=c.range(rank)[0], n_global=c.N, keep_csr=keep_csr, sharded_transpose=sharded_transpose)


def _threads(world, fn, timeout=120):
    return run_ranks(ThreadComm(world, pairwise=True, timeout=timeout), fn, join_timeout=2 * timeout)


def _assert_exact(y, yref, what):
    bad = np.flatnonzero(y != yref)
    assert bad.size == 0, "%s: %d of %d rows differ from the exact product, first at local row %d: %r instead of %r" % (what, bad.size, y.size, bad[0], y[bad[0]], yref[bad[0]])


def _product_rank(c, xs):
    """A^T x0, then A x1, then A^T x1 through the view - enqueued one behind the other, read back afterwards - and the view's transposed product."""
    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            B = ks.BV(ctx, A.n, 6, N=A.N)
            B.set_column(0, xs[0][r0:r1]); B.set_column(1, xs[1][r0:r1])
            A.mult_transpose_dev(B.column_ptr(0), B.column_ptr(2))
            A.mult_dev(B.column_ptr(1), B.column_ptr(3))
            At = A.transpose_view()
            At.mult_dev(B.column_ptr(1), B.column_ptr(4))
            At.mult_transpose_dev(B.column_ptr(0), B.column_ptr(5))
            res = {"t0": B.column(2), "f1": B.column(3), "t1": B.column(4), "tt0": B.column(5), "layout": At.layout(), "sizes": (At.n, At.N)}
            B.destroy(); At.destroy(); A.destroy()
            return res
        finally:
            ctx.close()
    return fn


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,world", PRODUCT_CASES)
def test_sharded_transpose_exact(name, world):
    """mult_transpose and the view's mult equal the integer A^T x bit for bit on every rank, two of them with a forward product in between; the
    view's transposed product is A x; columns without entries give +0.0; ranks with no rows, with no peers, that only send or only receive
    complete every call."""
    c = case(name, world)
    xs, yt, yf = vectors(name, world)
    out = _threads(world, _product_rank(c, xs))
    empty = np.bincount(c.col, minlength=c.N) == 0
    for rank in range(world):
        r0, r1 = c.range(rank)
        o = out[rank]
        what = "%s rank %d of %d" % (name, rank, world)
        assert o["sizes"] == (r1 - r0, c.N)
        _assert_exact(o["t0"], yt[0][r0:r1], what + ", A^T x0")
        _assert_exact(o["f1"], yf[1][r0:r1], what + ", A x1 between two transposed products")
        _assert_exact(o["t1"], yt[1][r0:r1], what + ", view x1")
        _assert_exact(o["tt0"], yf[0][r0:r1], what + ", the view's transposed product")
        for y in (o["t0"], o["t1"]):
            assert not y[empty[r0:r1]].any() and not np.signbit(y[empty[r0:r1]]).any()
    if name == "islands":
        assert empty.sum() == 3


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", ["csr", "csrvec", "csrregs", "sell", "dict", "odict", "binned", "sliced", None], ids=lambda f: f or "auto")
def test_sharded_transpose_every_layout(fmt, monkeypatch):
    """The transposed diagonal block in every layout, under the reverse exchange: the view reports the layout on EVERY rank and the product is exact."""
    if fmt is None:
        monkeypatch.delenv("KSGPU_SPMV", raising=False)
    else:
        monkeypatch.setenv("KSGPU_SPMV", fmt)
    for name, want in LAYOUT_CASES[fmt]:
        c = case(name)
        xs, yt, yf = vectors(name)
        out = _threads(4, _product_rank(c, xs))
        for rank in range(4):
            r0, r1 = c.range(rank)
            what = "%s as %s, rank %d" % (name, fmt or "auto", rank)
            assert out[rank]["layout"] == want, (fmt, name, rank, out[rank]["layout"])
            _assert_exact(out[rank]["t0"], yt[0][r0:r1], what)
            _assert_exact(out[rank]["t1"], yt[1][r0:r1], what)
            _assert_exact(out[rank]["f1"], yf[1][r0:r1], what)


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_transpose_float_bound_and_same_bits():
    """Normal values and vectors. Two runs in fresh contexts give identical bits (no atomics, fixed order). |y_i - ref_i| <= 1.01 m_i 2^-53
    (|A|^T |x|)_i with m_i = entries of column i + ranks that contribute to it + 1: the first-order bound gamma_m of ANY summation tree over
    the column's products (one rounding per product and per addition: at most entries + additions <= m roundings touch any term - the entries'
    sums inside the ranks, one addition per contributing rank), 1.01 for the higher-order terms. ref: the long-double sum per column."""
    c = case("float")
    x = np.random.default_rng(6).standard_normal(c.N)
    ref = np.zeros(c.N, np.longdouble); mag = np.zeros(c.N, np.longdouble)
    prod = c.val.astype(np.longdouble) * x.astype(np.longdouble)[c.row]
    np.add.at(ref, c.col, prod); np.add.at(mag, c.col, np.abs(prod))
    entries = np.bincount(c.col, minlength=c.N)
    pairs = np.unique(np.stack([c.col.astype(np.int64), c.owner_of_row[c.row]], axis=1), axis=0)
    ranks = np.bincount(pairs[:, 0], minlength=c.N)
    m = (entries + ranks + 1).astype(np.longdouble)

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            y = A.mult_transpose(x[r0:r1])
            A.destroy()
            return y
        finally:
            ctx.close()
    y1 = np.concatenate(_threads(4, fn))
    y2 = np.concatenate(_threads(4, fn))
    assert np.array_equal(y1, y2)
    err = np.abs(y1.astype(np.longdouble) - ref)
    bound = np.longdouble(1.01) * m * np.longdouble(2.0) ** -53 * mag
    worst = int(np.argmax(err - bound))
    print("float case: max error / bound = %.3g" % float(np.max(err[mag > 0] / bound[mag > 0])))
    assert np.all(err <= bound), (worst, float(err[worst]), float(bound[worst]))
    assert not y1[entries == 0].any()


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_transpose_block_product_on_the_view():
    """ks_mat_mult_multi with 3 columns on the view: column by column, each the bits of ks_mat_mult on the view (and exact); MatGetDiagonal of the view."""
    for name in ("far", "layouts-int"):
        c = case(name)
        xs, yt, _ = vectors(name)

        def fn(rank, comm):
            ks, ctx = _open(rank, comm)
            try:
                A = _mat(ks, ctx, c, rank)
                At = A.transpose_view()
                r0, r1 = c.range(rank)
                n = r1 - r0
                X = ks.BV(ctx, n, 3, N=c.N); Y = ks.BV(ctx, n, 3, N=c.N); Z = ks.BV(ctx, n, 3, N=c.N)
                for j in range(3):
                    X.set_column(j, xs[j][r0:r1])
                    At.mult_dev(X.column_ptr(j), Y.column_ptr(j))
                At.mult_multi_dev(X.column_ptr(0), X.ld, Z.column_ptr(0), Z.ld, 3)
                res = {"single": [Y.column(j) for j in range(3)], "multi": [Z.column(j) for j in range(3)], "diag": At.get_diagonal()}
                X.destroy(); Y.destroy(); Z.destroy(); At.destroy(); A.destroy()
                return res
            finally:
                ctx.close()
        out = _threads(4, fn)
        for rank in range(4):
            r0, r1 = c.range(rank)
            for j in range(3):
                _assert_exact(out[rank]["single"][j], yt[j][r0:r1], "%s rank %d column %d" % (name, rank, j))
                assert np.array_equal(out[rank]["multi"][j], out[rank]["single"][j]), (name, rank, j)
            assert np.array_equal(out[rank]["diag"], c.diagonal()[r0:r1]), (name, rank)      # the view answers with its matrix's diagonal


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------------
def _csr_block(Ao, r0, r1):
    p0, p1 = int(Ao.rowptr[r0]), int(Ao.rowptr[r1])
    return (Ao.rowptr[r0:r1 + 1] - p0).astype(np.int32), Ao.col[p0:p1], Ao.val[p0:p1]


def _solve_ranks(Ao, counts, npairs=4, which="largest_real", v0=None, w0=None, sigma=None, twosided=True, balance=None, st_type=None,
                 sharded_transpose=True, tsolves=False):
    """One solve with the rows of Ao cut as `counts` says; per rank: what the solver reports and its local parts of the first npairs vectors.
    A refusal is reported as {"rc": code, "msg": message}."""
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(int)

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            r0, r1 = int(starts[rank]), int(starts[rank + 1])
            rp, col, val = _csr_block(Ao, r0, r1)
            A = ks.Mat.from_csr(ctx, rp, col, val, row_start=r0, n_global=Ao.n, keep_csr=True, sharded_transpose=sharded_transpose)
            eps = ks.EPS(ctx)
            eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4); eps.SetWhichEigenpairs(which)
            eps.SetTwoSided(twosided)
            if balance:
                eps.SetBalance(balance)
            if v0 is not None:
                eps.SetInitialSpace(v0[r0:r1, None])
            if w0 is not None:
                eps.SetLeftInitialSpace(w0[r0:r1, None])
            if sigma is not None or st_type:
                st = eps.GetST(); st.SetType(st_type or "shift"); st.SetShift(sigma)
                if tsolves:
                    st.SetTransposeSolves(True)
            try:
                eps.Solve()
            except ks.KsError as e:
                return {"rc": e.rc, "msg": str(e)}
            stt = eps.GetStats()
            res = {"its": eps.GetIterationNumber(), "nconv": eps.GetConverged(), "steps": stt["arnoldi_steps"], "reason": eps.GetConvergedReason(),
                   "lam": [eps.GetEigenvalue(i) for i in range(eps.GetConverged())], "pairs": [], "err": []}
            for i in range(npairs):
                kr, ki, xr, xi = eps.GetEigenpair(i)
                yr, yi = eps.GetLeftEigenvector(i) if twosided else (np.zeros(r1 - r0), np.zeros(r1 - r0))
                res["pairs"].append((kr, ki, xr, xi, yr, yi))
                res["err"].append(eps.ComputeError(i))
            eps.destroy(); A.destroy()
            return res
        finally:
            ctx.close()
    return _threads(len(counts), fn, timeout=180)


def _gather(out, npairs=4):
    """Every rank reports the same restarts, nconv, steps and eigenvalue bits; the vectors are put together from the ranks' parts."""
    o0 = out[0]
    for o in out[1:]:
        assert (o["its"], o["nconv"], o["steps"], o["reason"]) == (o0["its"], o0["nconv"], o0["steps"], o0["reason"])
        assert o["lam"] == o0["lam"] and o["err"] == o0["err"]
    P = []
    for i in range(npairs):
        kr, ki = o0["pairs"][i][0], o0["pairs"][i][1]
        xr, xi, yr, yi = (np.concatenate([o["pairs"][i][j] for o in out]) for j in (2, 3, 4, 5))
        P.append((kr, ki, xr, xi, yr, yi))
    return P


def _check_pairs(P, errs, S, record):
    """tests/test_gpu_twosided.py's _check_pairs on gathered vectors: both residuals below tol (relative), ComputeError their maximum, unit vectors,
    |y_i^H x_j| <= (||r_i|| + ||r_j||) / |k_i - k_j| + 64 eps"""
    Q = []
    for i, (kr, ki, xr, xi, yr, yi) in enumerate(P):
        k = complex(kr, ki)
        rr = TS.residuals(S, kr, ki, xr, xi); rl = TS.residuals(S, kr, ki, yr, yi, left=True)
        record.append((rr / abs(k), rl / abs(k)))
        print("pair %d: k = %r, right %.2e, left %.2e (relative)" % (i, k, rr / abs(k), rl / abs(k)))
        assert rr / abs(k) < TOL and rl / abs(k) < TOL
        x, y = xr + 1j * xi, yr + 1j * yi
        assert abs(np.linalg.norm(x) - 1.0) < 1e-12 and abs(np.linalg.norm(y) - 1.0) < 1e-12
        assert abs(errs[i] - max(rr, rl) / abs(k)) <= 1e-12 + 1e-6 * errs[i], (errs[i], rr, rl)
        Q.append((k, x, y, rr, rl))
    for i, (ki_, _, y, _, rli) in enumerate(Q):
        for j, (kj, x, _, rrj, _) in enumerate(Q):
            if abs(ki_ - kj) > 1e-6:
                assert abs(np.vdot(y, x)) <= (rli + rrj) / abs(ki_ - kj) + 64 * EPS, (i, j)
    return Q


SPLITS = {120: [[70, 50], [50, 0, 30, 40]], 100: [[60, 40], [30, 0, 45, 25]]}      # world 2 and world 4, uneven, one rank without rows


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("split", [0, 1], ids=["world2", "world4"])
def test_twosided_markov_across_ranks(split):
    """ex5 -eps_two_sided 1 with the rows cut into slabs: eps/ex5_1.out"""
    Ao = O.markov_matrix(15); S = Ao.to_scipy()
    out = _solve_ranks(Ao, SPLITS[Ao.n][split])
    assert "rc" not in out[0], out[0]
    P = _gather(out)
    assert out[0]["nconv"] >= 4 and out[0]["reason"] == 1
    lam = np.array([k[0] for k in out[0]["lam"][:4]])
    assert np.array_equal(np.round(lam, 5), gi.eigenvalues_line(gi.read("eps/ex5_1.out")))
    rec = []
    _check_pairs(P, out[0]["err"], S, rec)
    print("markov across %d ranks: restarts %d, steps %d, max residual %.2e" % (len(out), out[0]["its"], out[0]["steps"], np.max(rec)))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("split", [0, 1], ids=["world2", "world4"])
def test_twosided_brusselator_across_ranks(split):
    """ex9 -eps_two_sided 1 across ranks: conjugate pairs, eps/ex9_1.out"""
    Ao = nc.brusselator(50); S = Ao.to_scipy()
    out = _solve_ranks(Ao, SPLITS[Ao.n][split])
    assert "rc" not in out[0], out[0]
    P = _gather(out)
    assert out[0]["nconv"] >= 4
    lam = np.array([complex(*k) for k in out[0]["lam"][:4]])
    gold = gi.complex_eigenvalue_lines(gi.read("eps/ex9_1.out"))[0]
    assert np.allclose(np.round(lam, 5), gold, atol=1.5e-5)
    assert lam[0].imag > 0 and lam[1] == lam[0].conjugate() and lam[3] == lam[2].conjugate()
    rec = []
    Q = _check_pairs(P, out[0]["err"], S, rec)
    assert np.array_equal(Q[1][2], Q[0][2].conjugate()) and np.array_equal(Q[1][1], Q[0][1].conjugate())
    print("brusselator across %d ranks: restarts %d, steps %d, max residual %.2e" % (len(out), out[0]["its"], out[0]["steps"], np.max(rec)))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("split", [0, 1], ids=["world2", "world4"])
def test_twosided_shift_across_ranks_follows_the_restatement(split):
    """ex41's start vectors and sigma = 0.3: the expansion runs through the ST's shell operator and its transposed callback (A - sigma I)^T over
    the sharded transposed product. Restarts, converged pairs and steps are the restatement's: its estimates stay clear of tol by the margin
    tests/test_ds_twosided_host.py states, far more than the rounding differences of sums taken rank by rank."""
    Ao = O.markov_matrix(15); S = Ao.to_scipy()
    v0, w0 = TS.ex41_start_vectors(Ao.n)
    r = TS.eps_krylovschur_twosided(Ao, 4, which="largest_real", v0=v0, w0=w0, sigma=0.3)
    out = _solve_ranks(Ao, SPLITS[Ao.n][split], v0=v0, w0=w0, sigma=0.3)
    assert "rc" not in out[0], out[0]
    P = _gather(out)
    print("sigma 0.3 across %d ranks: restarts %d (restatement %d), nconv %d (%d), steps %d (%d)"
          % (len(out), out[0]["its"], r.its, out[0]["nconv"], r.nconv, out[0]["steps"], r.steps))
    assert (out[0]["its"], out[0]["nconv"], out[0]["steps"]) == (r.its, r.nconv, r.steps)
    lam = np.array([k[0] for k in out[0]["lam"]])
    assert np.abs(lam - r.eigr[r.perm]).max() <= 1e-10 * np.abs(lam).max()
    assert np.allclose(lam[:4], gi.table_first_column(gi.read("eps/ex41_1.out"))[:4], atol=0.6e-6)
    _check_pairs(P, out[0]["err"], S, [])


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_twoside_balance_across_ranks():
    """ex9 suffix 3 (-eps_balance twoside, eps/ex9_1.out) in a one-sided solve on 4 ranks: EPSBuildBalance_Krylov takes A^T x of the sharded matrix.
    Residuals from the gathered vectors, below the 1e-7 the one-rank test of tests/test_gpu_nhep.py asks of ComputeError."""
    Ao = nc.brusselator(50); S = Ao.to_scipy()
    out = _solve_ranks(Ao, [30, 20, 27, 23], twosided=False, balance="twoside")
    assert "rc" not in out[0], out[0]
    P = _gather(out)
    assert out[0]["nconv"] >= 4
    lam = np.array([complex(*k) for k in out[0]["lam"][:4]])
    assert np.allclose(np.round(lam, 5), gi.complex_eigenvalue_lines(gi.read("eps/ex9_1.out"))[0], atol=1.5e-5)
    for i, (kr, ki, xr, xi, _, _) in enumerate(P):
        rr = TS.residuals(S, kr, ki, xr, xi) / abs(complex(kr, ki))
        print("pair %d: relative residual %.2e, ComputeError %.2e" % (i, rr, out[0]["err"][i]))
        assert rr < 1e-7 and out[0]["err"][i] < 1e-7
        assert abs(out[0]["err"][i] - rr) <= 1e-12 + 1e-6 * rr


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_refusals_on_every_rank():
    """Each refusal comes on every rank, with its message, and nobody is left in a collective (a rank left behind would run into the time limit of
    the communicator and fail the run): without the flag the transposed product and the two-sided set-up are KS_ERR_SUP; the flag without the
    kept arrays is KS_ERR_ARG_INCOMP; two-sided with sinvert on 2 ranks, and the infinity norm of a sharded view, are KS_ERR_SUP."""
    c = case("islands")

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            res = {}
            rp, col, val = c.block(rank)
            try:
                ks.Mat.from_csr(ctx, rp, col, val, row_start=c.range(rank)[0], n_global=c.N, keep_csr=False, sharded_transpose=True)
                res["flag"] = None
            except ks.KsError as e:
                res["flag"] = (e.rc, str(e))
            A = _mat(ks, ctx, c, rank, sharded_transpose=False)
            W = ks.BV(ctx, A.n, 2, N=A.N)
            for key, call in (("mult_transpose", lambda: A.mult_transpose_dev(W.column_ptr(0), W.column_ptr(1))), ("view", A.transpose_view)):
                try:
                    call(); res[key] = None
                except ks.KsError as e:
                    res[key] = (e.rc, str(e))
            F = _mat(ks, ctx, c, rank)
            try:
                F.transpose_view().norm_inf(); res["norm"] = None
            except ks.KsError as e:
                res["norm"] = (e.rc, str(e))
            res["norm_of_matrix"] = F.norm_inf()
            W.destroy(); F.destroy(); A.destroy()
            return res
        finally:
            ctx.close()
    out = _threads(4, fn, timeout=60)
    for o in out:
        assert o["flag"][0] == KS_ERR_ARG_INCOMP and "KS_MAT_KEEP_CSR" in o["flag"][1]
        assert o["mult_transpose"][0] == KS_ERR_SUP and o["view"][0] == KS_ERR_SUP and "redistribution" in o["mult_transpose"][1]
        assert o["norm"][0] == KS_ERR_SUP and "1-norm" in o["norm"][1]
        assert o["norm_of_matrix"] == c.abs_row_sums().max()
    Ao = O.markov_matrix(15)
    out = _solve_ranks(Ao, [70, 50], sharded_transpose=False)
    assert [o["rc"] for o in out] == [KS_ERR_SUP] * 2 and all("KS_MAT_SHARDED_TRANSPOSE" in o["msg"] for o in out)
    out = _solve_ranks(Ao, [70, 50], which="target_magnitude", st_type="sinvert", sigma=1.1, tsolves=True)
    assert [o["rc"] for o in out] == [KS_ERR_SUP] * 2 and all("more than one rank" in o["msg"] for o in out)


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_flag_travels_through_axpy_and_changes_nothing_on_one_rank():
    """P = A + alpha B of two flagged matrices has the transposed product (exact (A + alpha B)^T x: multiples of 1/8 far below 2^53); with an
    unflagged B it is refused like any unflagged matrix. On one rank the flag changes nothing: the same bits as without it, the same layout."""
    a, b = case("far"), sc.far(4, seed=8)
    xs, yta, _ = vectors("far")
    ytb = (b.int_matrix().T.tocsr() @ xs[0].astype(np.int64)) / float(b.scale)
    alpha = -0.375

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A, B, U = _mat(ks, ctx, a, rank), _mat(ks, ctx, b, rank), _mat(ks, ctx, b, rank, sharded_transpose=False)
            r0, r1 = a.range(rank)
            P = A.axpy_new(alpha, B)
            res = {"y": P.mult_transpose(xs[0][r0:r1])}
            Q = A.axpy_new(alpha, U)
            try:
                Q.mult_transpose(xs[0][r0:r1]); res["unflagged"] = None
            except ks.KsError as e:
                res["unflagged"] = e.rc
            for M in (P, Q, A, B, U):
                M.destroy()
            return res
        finally:
            ctx.close()
    out = _threads(4, fn)
    for rank in range(4):
        r0, r1 = a.range(rank)
        _assert_exact(out[rank]["y"], (yta[0] + alpha * ytb)[r0:r1], "(A + alpha B)^T x, rank %d" % rank)
        assert out[rank]["unflagged"] == KS_ERR_SUP
    import slepc_amd as ks
    ctx = ks.Context(0)
    try:
        c = case("layouts-int")
        x = vectors("layouts-int")[0][1]
        M0 = ks.Mat.from_csr(ctx, c.rowptr, c.col, c.val, keep_csr=True)
        M1 = ks.Mat.from_csr(ctx, c.rowptr, c.col, c.val, keep_csr=True, sharded_transpose=True)
        assert M0.transpose_view().layout() == M1.transpose_view().layout()
        assert np.array_equal(M0.mult_transpose(x), M1.mult_transpose(x)) and np.array_equal(M0.mult(x), M1.mult(x))
        with pytest.raises(ks.KsError) as e:
            ks.Mat.from_csr(ctx, c.rowptr, c.col, c.val, sharded_transpose=True)
        assert e.value.rc == KS_ERR_ARG_INCOMP
        M0.destroy(); M1.destroy()
    finally:
        ctx.close()
