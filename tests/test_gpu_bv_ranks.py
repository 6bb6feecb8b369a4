"""Block orthogonalisation, panel contractions with active windows and the B-inner product on ROW-SHARDED bases.

Ranks are threads of one process (tests/thread_comm.py), each with a context of its own that it closes; at most four at a time. The row splits,
the exact integer data and the longdouble references are those of tests/bv_rank_cases.py:

  even2     [500, 500]              the plain case
  ragged3   [64, 129, 807]          one 64-row tile exactly; two tiles and one row
  ragged4   [0, 5, 63, 932]         rank 0 empty - its all-zero R is the seed of TSQR's combine across ranks and the head of the stack whose
                                    orthogonal factor forms Q; 5 rows < k (the zero-padded first tile); the zero-row branches of the contractions
  ragged4b  [65, 0, 934, 1]         an empty rank in the middle, a last rank of one row
  big2      [T + 101, 70]           T = 64 * 2 * num_cu: the first size at which the blocks of k_tsqr_local / k_tsqr_formq walk more than one tile

What is exact is compared with np.array_equal against int64 arithmetic; every replicated result (M, dots, norms, R) must be the same bits on all
ranks. The R of a block method is compared with a longdouble Householder QR under the freedom of the method (bv_rank_cases.compare_R); the bound is
8 times the largest distance, measured on the CPU, between numpy's float64 QR and that reference over these cases: measured 2.28e-16 relative to
max|R|, bound R_TOL = 1.83e-15. SVQB is compared through its Gram factor R^T R and has its bound measured in that measure: 4.18e-16, bound 3.34e-15."""
import functools

import numpy as np
import pytest

import bv_rank_cases as bc
from oracle import oracle as O
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
KS_ERR_SUP = 56                   # include/ksgpu.h
BLOCKS = ["gs", "chol", "tsqr", "tsqrchol", "svqb"]


@functools.lru_cache(maxsize=None)
def _num_cu():
    import slepc_amd as ks
    c = ks.Context(0)
    try:
        return c.device_info()["num_cu"]
    finally:
        c.close()


def _split(name):
    return bc.split(name, _num_cu() if name == "big2" else 256)


def _run(counts, body, pairwise=False, no_mfma=False):
    """body(ks, ctx, rank, r0, r1, own) on one thread per rank; own(obj) hands an object over to be destroyed before the rank's context closes."""
    rg = bc.ranges(counts)

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        objs = []

        def own(o):
            objs.append(o)
            return o
        try:
            comm.install(ctx, rank)
            if no_mfma:
                ctx.set_debug("no_mfma")
            return body(ks, ctx, rank, rg[rank][0], rg[rank][1], own)
        finally:
            for o in reversed(objs):
                o.destroy()
            ctx.close()
    return run_ranks(ThreadComm(len(counts), pairwise=pairwise, timeout=60), fn, join_timeout=120)


def _sharded(ks, ctx, own, arrays, r0, r1, N):
    from slepc_amd import partition as P
    rowptr, col, val = arrays
    return own(ks.Mat.from_csr(ctx, *P.local_block(rowptr, col, val, r0, r1), row_start=r0, n_global=N))


def _basis(ks, ctx, own, X0, r0, r1):
    V = own(ks.BV(ctx, r1 - r0, X0.shape[1], N=X0.shape[0], row_start=r0))
    V.set_dense(X0[r0:r1])
    return V


def _same_on_all_ranks(out, keys):
    for rank in range(1, len(out)):
        for key in keys:
            assert np.array_equal(np.asarray(out[rank][key]), np.asarray(out[0][key])), "%r differs between rank 0 and rank %d" % (key, rank)


def _rows(out, key):
    return np.concatenate([o[key] for o in out], axis=0)


# ---- 1: panel contractions, exact -----------------------------------------------------------------------------------------------------------
ALPHA_BETA = [(0.5, 0.5), (0.5, -2.0), (-2.0, 0.5), (-2.0, -2.0)]
PANEL_CASES = ([(s, 9, True) for s in bc.ALL_SPLITS] + [(s, 9, False) for s in bc.SMALL_SPLITS]
               + [("ragged4", 70, True), ("ragged4", 70, False), ("ragged4", 100, True), ("ragged4", 100, False)])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,mx,mfma", PANEL_CASES, ids=["%s-%d-%s" % (s, m, "mfma" if f else "valu") for s, m, f in PANEL_CASES])
def test_exact_panel_ops(name, mx, mfma):
    """BVDot, BVMult, BVMultInPlace (both forms), BVDotVec, BVMultVec, BVMatProject (with B and without) and the norms over active windows
    (2, kx) of X and (1, 5) of Y on integer data: ksb_dot_range (from 65 columns of X on in 64-column blocks), ksb_mult_range's kernels and
    their guards on ranks without rows, on the matrix cores and on the vector ALUs. mx = 9 has the windows of test_matproject_and_normalize."""
    N, counts = _split(name)
    my, ly, ky, lx = 6, 1, 5, 2
    kx = 8 if mx == 9 else mx - 1
    s, e = lx + 1, kx - 1
    X0, Y0 = bc.int_basis(N, mx, 11), bc.int_basis(N, my, 12)
    Q, QQ, q = bc.int_coeffs((mx, my), 13), bc.int_coeffs((mx, mx), 14), bc.int_coeffs((mx,), 15)
    b_arrays = bc.b_csr(N)

    def body(ks, ctx, rank, r0, r1, own):
        B = _sharded(ks, ctx, own, b_arrays, r0, r1, N)
        X, Y = _basis(ks, ctx, own, X0, r0, r1), _basis(ks, ctx, own, Y0, r0, r1)
        X.SetActiveColumns(lx, kx); Y.SetActiveColumns(ly, ky)
        res = {}
        M = np.full((my, mx), 7.0, order="F"); X.Dot(Y, M); res["dot"] = M
        M = np.full((mx, mx), 7.0, order="F"); X.Dot(X, M); res["dot_xx"] = M
        M = np.full((my, mx), 7.0, order="F"); X.MatProject(B, Y, M); res["project_b"] = M
        M = np.full((my, mx), 7.0, order="F"); X.MatProject(None, Y, M); res["project"] = M
        res["dotvec"] = X.DotVec(Y.column_ptr(0))
        for i, (alpha, beta) in enumerate(ALPHA_BETA):
            Y.set_dense(Y0[r0:r1])
            Y.Mult(alpha, beta, X, Q)
            res["mult%d" % i] = Y.dense()
            X.MultVec(alpha, beta, Y.column_ptr(0), q[lx:kx])
            res["multvec%d" % i] = Y.column(0)
        X.SetActiveColumns(2, 8)
        res["norm1"], res["norminf"], res["normf"] = X.Norm(ks.NORM_1), X.Norm(ks.NORM_INFINITY), X.Norm(ks.NORM_FROBENIUS)
        res["norm2"] = np.array([X.NormColumn(j) for j in (0, 4, mx - 1)])
        X.SetActiveColumns(lx, kx)
        X.MultInPlace(QQ, s, e); res["mip"] = X.dense()
        X.MultInPlace(QQ, lx, kx, trans=True); res["mip_t"] = X.dense()
        return res
    out = _run(counts, body, pairwise=True, no_mfma=not mfma)
    replicated = ["dot", "dot_xx", "project_b", "project", "dotvec", "norm1", "norminf", "normf", "norm2"]
    _same_on_all_ranks(out, replicated)
    o = out[0]

    def block(rows, cols, value, shape):
        M = np.full(shape, 7.0)                                       # outside the active block the fill value stays
        M[rows[0]:rows[1], cols[0]:cols[1]] = value
        return M
    Xa, Ya = X0[:, lx:kx], Y0[:, ly:ky]
    assert np.array_equal(o["dot"], block((ly, ky), (lx, kx), bc.exact_gram(Ya, Xa), (my, mx)))
    assert np.array_equal(o["dot_xx"], block((lx, kx), (lx, kx), bc.exact_gram(Xa, Xa), (mx, mx)))
    assert np.array_equal(o["project_b"], block((ly, ky), (lx, kx), bc.exact_gram(Ya, Xa, with_b=True), (my, mx)))
    assert np.array_equal(o["project"], o["dot"])
    assert np.array_equal(o["dotvec"], bc.exact_gram(Xa, Y0[:, :1])[:, 0])
    for i, (alpha, beta) in enumerate(ALPHA_BETA):
        want = Y0.copy()
        want[:, ly:ky] = bc.exact_mult(alpha, beta, Ya, Xa, Q[lx:kx, ly:ky])
        got = _rows(out, "mult%d" % i)
        assert np.array_equal(got, want), "Mult(%g, %g)" % (alpha, beta)
        y0 = want[:, :1]                                              # column 0 of Y is outside its window: still Y0's
        assert np.array_equal(y0, Y0[:, :1])
        assert np.array_equal(_rows(out, "multvec%d" % i), bc.exact_mult(alpha, beta, y0, Xa, q[lx:kx, None])[:, 0]), "MultVec(%g, %g)" % (alpha, beta)
    W = X0[:, 2:8]
    assert o["norm1"] == bc.exact_norm1(W) and o["norminf"] == bc.exact_norm_inf(W)
    assert bc.ulps(o["normf"], np.sqrt(float(bc.exact_sumsq(W)))) <= 2
    for got, j in zip(o["norm2"], (0, 4, mx - 1)):
        assert bc.ulps(got, np.sqrt(float(bc.exact_sumsq(X0[:, j])))) <= 2, j
    X1 = X0.copy(); X1[:, s:e] = bc.exact_matmat(Xa, QQ[lx:kx, s:e])
    assert np.array_equal(_rows(out, "mip"), X1)
    X2 = X1.copy(); X2[:, lx:kx] = bc.exact_matmat(X1[:, lx:kx], QQ[lx:kx, lx:kx].T.copy())
    assert np.array_equal(_rows(out, "mip_t"), X2)


# ---- 2: block orthogonalisation ---------------------------------------------------------------------------------------------------------------
def _check_qr(block, X0, l, Q, R, Rref, failures, tag, level=None, resid=None):
    k = X0.shape[1]
    where = "%s %s l=%d" % (tag, block, l)
    level = 200 * EPS * np.sqrt(k) if level is None else level
    resid = 1e3 * EPS * np.abs(X0).max() * np.sqrt(k) if resid is None else resid

    def check(ok, what, figure):
        print("%-28s %-22s %.3e" % (where, what, figure))
        if not ok:
            failures.append("%s: %s = %.3e" % (where, what, figure))
    if not np.array_equal(Q[:, :l], X0[:, :l]):
        failures.append("%s: the leading columns changed" % where)
    lvl = np.abs(Q.T @ Q - np.eye(k)).max()
    check(lvl < level, "|Q^T Q - I|", lvl)
    Rfull = R.copy(); Rfull[:l, :l] = np.eye(l)                        # the leading block of R is not referenced
    res = np.abs(X0[:, l:] - Q @ Rfull[:, l:]).max()
    check(res < resid, "|X - Q R|", res)
    if block != "svqb" and not np.all(np.tril(R, -1)[:, l:] == 0):
        failures.append("%s: R is not upper triangular" % where)
    if block in ("gs", "chol") and not np.all(np.diag(R)[l:] > 0):
        failures.append("%s: diag(R) is not positive" % where)
    if Rref is not None:
        d = bc.compare_R(block, R, Rref, l)
        check(d < bc.r_tolerance(block), "R against longdouble", d)


ORTHOG_CASES = ([(s, 12, tuple(BLOCKS)) for s in bc.SMALL_SPLITS] + [("ragged4", 64, tuple(BLOCKS)), ("ragged3", 64, tuple(BLOCKS)),
                ("ragged4", 100, ("tsqr", "tsqrchol")), ("big2", 12, ("tsqr", "tsqrchol", "chol"))])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,k,blocks", ORTHOG_CASES, ids=["%s-%d" % (s, k) for s, k, _ in ORTHOG_CASES])
def test_block_orthogonalize_across_ranks(name, k, blocks):
    """BVOrthogonalize with every block method, windows l = 0 and l = 3: the rank level of TSQR (tsqr_r's combine in rank order, tsqr_q's stack
    and this rank's slice of its orthogonal factor), ranks with fewer rows than columns or none, the multi-tile blocks of big2, the panel-by-panel
    path at k = 100, and the Gram matrices / V inv(R) / block Gram-Schmidt of the other methods on sharded rows."""
    N, counts = _split(name)
    windows = (0, 3)

    def body(ks, ctx, rank, r0, r1, own):
        res = {}
        V = own(ks.BV(ctx, r1 - r0, k, N=N, row_start=r0))
        for block in blocks:
            for l in windows:
                V.SetActiveColumns(0, k)
                V.set_dense(bc.normal_basis(N, k, l)[r0:r1])
                V.SetActiveColumns(l, k); V.SetOrthogBlock(block)
                R = np.zeros((k, k), order="F")
                V.Orthogonalize(R)
                res["Q", block, l] = V.dense(); res["R", block, l] = R
        return res
    out = _run(counts, body)
    _same_on_all_ranks(out, [("R", b, l) for b in blocks for l in windows])
    failures = []
    for block in blocks:
        for l in windows:
            _check_qr(block, bc.normal_basis(N, k, l), l, _rows(out, ("Q", block, l)), out[0]["R", block, l], bc.normal_basis_R(N, k, l), failures, "%s k=%d" % (name, k))
    assert not failures, "\n".join(failures)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["ragged4", "big2"])
def test_tsqr_ill_conditioned_across_ranks(name):
    """cond(V) = 1e12, the construction of test_tsqr_accumulates_its_reflectors and its bounds: Q = V inv(R) is not orthogonal here, so the
    reflectors of every rank and the orthogonal factor of the combine across ranks are what formed Q - also where the first rank has no rows and
    the second fewer than columns (ragged4: |Q^T Q - I| was 5.4e-12 while the zero rows of such factors were pivot rows of the rank-level stack)."""
    N, counts = _split(name)
    k = 12
    X0 = bc.ill_conditioned_basis(N, k)

    def body(ks, ctx, rank, r0, r1, own):
        V = _basis(ks, ctx, own, X0, r0, r1)
        V.SetOrthogBlock("tsqr")
        R = np.zeros((k, k), order="F")
        V.Orthogonalize(R)
        return {"Q": V.dense(), "R": R}
    out = _run(counts, body)
    _same_on_all_ranks(out, ["R"])
    failures = []
    _check_qr("tsqr", X0, 0, _rows(out, "Q"), out[0]["R"], None, failures, name + " cond=1e12", level=1e-13, resid=1e-13)
    assert not failures, "\n".join(failures)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("p", [0.0, 1e-14, 1e-13, 1e-12, 1e-10, 1e-8, 1e-4])
def test_nearly_orthonormal_block_across_ranks(p):
    """A second pass: V = Q (I + p S) on ragged4, every block method. The scaled Gram matrix is I + O(p), so SVQB's eigenvalues cluster with gaps of
    about p; Q^T Q and V = Q R must hold to the bounds of test_orthogonalize_properties however small p is."""
    N, counts = _split("ragged4")
    k = 12
    X0 = bc.nearly_orthonormal_basis(N, k, p)

    def body(ks, ctx, rank, r0, r1, own):
        res = {}
        V = own(ks.BV(ctx, r1 - r0, k, N=N, row_start=r0))
        for block in BLOCKS:
            V.set_dense(X0[r0:r1]); V.SetOrthogBlock(block)
            R = np.zeros((k, k), order="F")
            V.Orthogonalize(R)
            res["Q", block] = V.dense(); res["R", block] = R
        return res
    out = _run(counts, body)
    _same_on_all_ranks(out, [("R", b) for b in BLOCKS])
    failures = []
    for block in BLOCKS:
        _check_qr(block, X0, 0, _rows(out, ("Q", block)), out[0]["R", block], None, failures, "ragged4 p=%g" % p)
    assert not failures, "\n".join(failures)


@pytest.mark.timeout(300)
def test_tsqr_rank_deficient_panel_across_ranks():
    """Five rows in all ([0, 5, 0, 0]) for twelve columns: the stack of the ranks' factors keeps fewer non-zero rows than it has columns. No
    orthonormal Q exists; what holds is X = Q R to rounding, an upper triangular R that is the same on every rank, and orthonormal ROWS of Q."""
    counts, k = bc.TINY4, 12
    N = sum(counts)
    X0 = np.random.default_rng(5).standard_normal((N, k))

    def body(ks, ctx, rank, r0, r1, own):
        V = _basis(ks, ctx, own, X0, r0, r1)
        V.SetOrthogBlock("tsqr")
        R = np.zeros((k, k), order="F")
        V.Orthogonalize(R)
        return {"Q": V.dense(), "R": R}
    out = _run(counts, body)
    _same_on_all_ranks(out, ["R"])
    Q, R = _rows(out, "Q"), out[0]["R"]
    assert np.all(np.tril(R, -1) == 0) and np.all(np.isfinite(Q)) and np.all(np.isfinite(R))
    assert np.abs(X0 - Q @ R).max() < 1e3 * EPS * np.abs(X0).max() * np.sqrt(k)
    assert np.abs(Q @ Q.T - np.eye(N)).max() < 200 * EPS * np.sqrt(k)


# ---- 3: the B-inner product -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["even2", "ragged4", "ragged4b"])
def test_b_inner_product_across_ranks(name):
    """BVSetMatrix with a row-sharded B: the matrix branch of ksb_dot_range (a sharded block product in front of the Gram sweep), ksb_norm_b,
    Gram-Schmidt with B v recomputed by a sharded product before every pass (bmat in ks_gs.hip), block GS / CHOL / SVQB in the B-inner
    product, TSQR's refusal on every rank, and Lanczos in the B-inner product against the single-rank oracle."""
    N, counts = _split(name)
    k, steps = 12, 20
    X0, Y0 = bc.int_basis(N, 9, 21), bc.int_basis(N, 6, 22)
    Z0, W0 = bc.normal_basis(N, 8, 0), bc.normal_basis(N, k, 0)
    b_arrays = bc.b_csr(N)
    Ao = O.laplacian2d(40, 25)
    assert Ao.n == N

    def body(ks, ctx, rank, r0, r1, own):
        B = _sharded(ks, ctx, own, b_arrays, r0, r1, N)
        A = _sharded(ks, ctx, own, (Ao.rowptr, Ao.col, Ao.val), r0, r1, N)
        res = {}
        X, Y = _basis(ks, ctx, own, X0, r0, r1), _basis(ks, ctx, own, Y0, r0, r1)
        X.SetMatrix(B); Y.SetMatrix(B)
        M = np.zeros((6, 9), order="F"); X.Dot(Y, M); res["dot"] = M
        res["bnorm"] = np.array([X.NormColumn(j) for j in range(9)])
        Z = _basis(ks, ctx, own, Z0, r0, r1)
        Z.SetMatrix(B)
        for j in range(8):
            _, nrm, _ = Z.OrthogonalizeColumn(j)
            Z.ScaleColumn(j, 1.0 / nrm)
        res["gs_columns"] = Z.dense()
        W = own(ks.BV(ctx, r1 - r0, k, N=N, row_start=r0))
        W.SetMatrix(B)
        for block in ("gs", "chol", "svqb"):
            W.set_dense(W0[r0:r1]); W.SetOrthogBlock(block)
            R = np.zeros((k, k), order="F")
            W.Orthogonalize(R)
            res["Q", block] = W.dense(); res["R", block] = R
        for block in ("tsqr", "tsqrchol"):
            W.set_dense(W0[r0:r1]); W.SetOrthogBlock(block)
            try:
                W.Orthogonalize(None)
                res["refused", block] = 0
            except ks.KsError as err:
                res["refused", block] = err.rc
            res["kept", block] = bool(np.array_equal(W.dense(), W0[r0:r1]))
        V = own(ks.BV(ctx, r1 - r0, steps + 1, N=N, row_start=r0))
        V.SetMatrix(B)
        V.SetRandomColumn(0)
        _, nrm, _ = V.OrthogonalizeColumn(0); V.ScaleColumn(0, 1.0 / nrm)
        T = np.zeros((steps + 1, 3), order="F")
        p0 = V.gs_passes()[0]
        res["lanczos"] = V.MatLanczos(A, T, 0, steps)
        res["T"] = T; res["passes"] = V.gs_passes()[0] - p0; res["V"] = V.dense()
        return res
    out = _run(counts, body, pairwise=True)
    _same_on_all_ranks(out, ["dot", "bnorm", "T", "passes", "lanczos"] + [("R", b) for b in ("gs", "chol", "svqb")])
    o = out[0]
    Bd = bc.b_dense(N)
    assert np.array_equal(o["dot"], bc.exact_gram(Y0, X0, with_b=True))                    # exactly Y^T B X
    xbx = np.diag(bc.exact_gram(X0, X0, with_b=True))
    for j in range(9):
        assert bc.ulps(o["bnorm"][j], np.sqrt(xbx[j])) <= 1, (j, o["bnorm"][j], np.sqrt(xbx[j]))
    Q = _rows(out, "gs_columns")
    assert np.abs(Q.T @ Bd @ Q - np.eye(8)).max() < 1e-12
    for block in ("gs", "chol", "svqb"):
        Q, R = _rows(out, ("Q", block)), o["R", block]
        lvl = np.abs(Q.T @ Bd @ Q - np.eye(k)).max()
        print("%-10s %-8s |Q^T B Q - I| = %.3e" % (name, block, lvl))
        assert lvl < 200 * EPS * np.sqrt(k) * bc.COND_B, (block, lvl)
        assert np.abs(W0 - Q @ R).max() < 1e3 * EPS * np.abs(W0).max() * np.sqrt(k) * bc.COND_B, block
    for rank in range(len(counts)):                                                         # every rank is told, none is left at a barrier
        for block in ("tsqr", "tsqrchol"):
            assert out[rank]["refused", block] == KS_ERR_SUP and out[rank]["kept", block], (rank, block)
    # Lanczos in the B-inner product: the single-rank oracle on the same start vector (its values depend on the global row only)
    Bo = O.CSR(N, *b_arrays)
    Vo = O.BV(N, steps + 1)
    Vo.SetMatrix(Bo)
    Vo.SetRandomColumn(0)
    _, nrm, _ = Vo.OrthogonalizeColumn(0); Vo.ScaleColumn(0, 1.0 / nrm)
    To = np.zeros((steps + 1, 3), order="F")
    p0 = Vo.passes_total()
    ro = Vo.MatLanczos(Ao, To, 0, steps)
    assert o["lanczos"][0] == ro[0] == steps and not o["lanczos"][2]
    assert o["passes"] == Vo.passes_total() - p0
    assert np.abs(o["T"] - To).max() < 1e-9 and abs(o["lanczos"][1] - ro[1]) < 1e-9
    Vd = _rows(out, "V")
    assert np.abs(Vd.T @ Bd @ Vd - np.eye(steps + 1)).max() < 1e-11


# ---- 4: a generalized symmetric solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("like", ["even2", "ragged4"])
def test_ghep_solve_across_ranks(like):
    """The GHEP of test_eps_test1_ghep_golden (the 18 x 18 grid Laplacian against a diagonal B, 324 rows: the smallest problem for which
    test_gpu_ghep.py holds iterations, converged pairs and eigenvalues against the oracle) on two even ranks and on [0, 5, 63, 256]: Lanczos
    in the B-inner product, purification and B-normalisation on sharded rows, with that test's settings and tolerances."""
    (arp, acol, aval), (brp, bcol, bval) = bc.ghep_test1_pencil(18)
    Ao, Bo = O.CSR(len(arp) - 1, arp, acol, aval), O.CSR(len(brp) - 1, brp, bcol, bval)
    N = Ao.n
    counts = bc.split_like(like, N)

    def body(ks, ctx, rank, r0, r1, own):
        A = _sharded(ks, ctx, own, (Ao.rowptr, Ao.col, Ao.val), r0, r1, N)
        B = _sharded(ks, ctx, own, (Bo.rowptr, Bo.col, Bo.val), r0, r1, N)
        eps = own(ks.EPS(ctx))
        eps.SetOperators(A, B); eps.SetProblemType(ks.EPS_GHEP); eps.SetDimensions(4, 0); eps.SetTolerances(0.0, 1500)
        eps.SetConvergenceTest("norm")
        eps.GetST().SetKSP(rtol=1e-14)
        eps.Solve()
        nconv = eps.GetConverged()
        return {"nconv": nconv, "its": eps.GetIterationNumber(), "lam": np.array([eps.GetEigenvalue(i)[0] for i in range(nconv)]),
                "err": np.array([eps.ComputeError(i) for i in range(nconv)]),
                "X": np.stack([eps.GetEigenvector(i) for i in range(nconv)], axis=1) if nconv else np.zeros((r1 - r0, 0))}
    out = _run(counts, body, pairwise=True)
    _same_on_all_ranks(out, ["nconv", "its", "lam", "err"])
    r = O.eps_krylovschur_hep(Ao, 4, max_it=1500, st=O.ST(Ao, Bo, "shift", 0.0), B=Bo, conv="norm")
    o = out[0]
    assert o["nconv"] == r.nconv and o["its"] == r.its, (o["nconv"], r.nconv, o["its"], r.its)
    assert np.allclose(o["lam"], r.eigr[r.perm], rtol=1e-10)
    assert o["err"].max() < 1e-6
    X = _rows(out, "X")
    assert X.shape == (N, r.nconv) and np.abs(X.T @ (Bo.to_scipy() @ X) - np.eye(r.nconv)).max() < 1e-8
