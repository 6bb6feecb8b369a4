"""The row-sharded product (ks_mat_mult_internal with comm.size > 1) on GENERAL matrices: every layout of the diagonal block, both halos.

The slab tests (test_gpu_multirank.py, test_gpu_slabs8.py, test_gpu_spmm.py, test_gpu_dict_patterns.py) give the multi-rank path its easiest
inputs: one or two adjacent peers, one contiguous run of ghosts per peer, sorted columns, a dictionary diagonal block. Here the host diag/off-diag
split, the halo plan, compact_offdiag_rows, k_pack + the provider exchange or k_halo_pack / k_halo_unpack, and the accumulating pass over the
ghosts run on the matrices of tests/sharded_cases.py: ragged unsorted rows with duplicates, ghosts owned by every other rank, ranks with no rows,
with no peers, that only send or only receive, halos of several workgroups with three peers of unequal counts.

Values and vectors are small integers (or k / 1024), so that every sum is exact in binary64 in any order: results are compared with the integer
reference by np.array_equal, for every layout's summation order and the separate ghost pass alike. One case (normal values) has a derived bound.

Thread tests run one Python thread per rank (tests/thread_comm.py, pairwise exchange), each with its own Context; the peer halo runs between
processes only: with the few hardware queues of one process a spinning unpack kernel of one rank can sit in front of the pack it waits for."""
import functools
import os
import sys
import time

import numpy as np
import pytest

import sharded_cases as sc
from thread_comm import ThreadComm, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS_ERR_SUP, KS_ERR_ARG_WRONG = 56, 62          # include/ksgpu.h
NVEC = 16


@functools.lru_cache(maxsize=None)
def case(name, world=4):
    if name == "far":
        return sc.far(world)
    if name == "far2":                          # a second matrix under far's ownership (the B of A + alpha B)
        return sc.far(world, seed=8)
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
    """(x, exact A x) for NVEC integer vectors: computed once per case, shared by every test, never written to."""
    c = case(name, world)
    xs = sc.int_vectors(c.N, NVEC, seed=100 + c.N % 97)
    ys = np.stack([c.reference(x) for x in xs])
    xs.setflags(write=False); ys.setflags(write=False)
    return xs, ys


# ---- the generators deliver what the GPU tests rely on (no GPU) -----------------------------------------------------------------------------
def test_case_generators_deliver_their_properties():
    for world in (4, 8):
        c = case("far", world)
        counts = np.asarray(c.counts)
        assert 0 in c.counts and 65 in c.counts
        if world == 8:
            assert {0, 1, 63, 64, 65} <= set(c.counts)
        needs, nghost, nsend = sc.halo_plan(c)
        nonempty = set(np.flatnonzero(counts > 0).tolist())
        for p in range(world):
            if counts[p] == 0:
                assert not needs[p] and nsend[p] == 0
            else:                                                  # every other non-empty rank is a peer, in both directions
                assert set(needs[p]) == nonempty - {p}
        nloc, ngho, dup_loc, dup_gho = c.row_stats()
        N = c.N
        assert 0.03 * N < np.count_nonzero(nloc + ngho == 0) < 0.07 * N             # empty rows
        assert 0.05 * N < np.count_nonzero((nloc == 0) & (ngho > 0)) < 0.20 * N      # rows whose entries are all ghosts (the 5 % made so, and short rows by chance)
        assert 0.04 * N < np.count_nonzero((nloc > 0) & (ngho == 0)) < 0.20 * N      # rows without ghosts
        assert 0.03 * N < np.count_nonzero(dup_loc & dup_gho) < 0.07 * N             # a repeated column in the local AND in the ghost part
        assert (nloc + ngho).max() <= 40
        p0 = int(c.rowptr[0]); cols = c.col[p0:int(c.rowptr[c.counts[0]])]
        assert np.any(np.diff(cols[:200]) < 0)                                        # unsorted
        dup_diag = np.bincount(c.row[c.col == c.row], minlength=N)
        assert np.count_nonzero(dup_diag >= 2) > 0.03 * N                             # duplicates ON the diagonal
        sums = c.abs_row_sums()
        assert np.argmax(sums) == c.planted and ngho[c.planted] >= 10                 # the largest row sum is in the planted row ...
        loc = c.entry_is_local()
        local_part = np.bincount(c.row, weights=np.abs(c.ival) * loc, minlength=N) / c.scale
        assert local_part.max() < 0.05 * sums[c.planted]                              # ... and no diagonal block comes anywhere near it
    c = case("far_even")
    assert c.counts == [4608] * 4 and all(len(n) == 3 for n in sc.halo_plan(c)[0])
    c = case("islands")
    needs, nghost, nsend = sc.halo_plan(c)
    assert [set(n) for n in needs] == [{3}, set(), set(), {2}]                        # 0 <- 3 (not adjacent) and 3 <- 2, each one way
    assert nghost[1] == 0 and nsend[1] == 0                                           # the isolated rank
    assert nghost[2] == 0 and nsend[2] > 0 and nghost[0] > 0 and nsend[0] == 0        # send only, receive only
    assert nghost[3] > 0 and nsend[3] > 0
    for world in (2, 4):
        c = case("bighalo", world)
        needs, nghost, nsend = sc.halo_plan(c)
        for p in range(world):
            assert min(nsend[p], nghost[p]) > 3 * 2048, (world, p, nsend[p], nghost[p])
            assert len(needs[p]) == world - 1
            if world == 4:
                assert len(set(needs[p].values())) == 3                              # three peers of unequal counts
    for v in ("int", "dyadic"):
        c = case("layouts-" + v)
        needs, nghost, nsend = sc.halo_plan(c)
        nloc, ngho, _, _ = c.row_stats()
        assert (nloc + ngho).max() <= 13 and c.counts == [sc.LAYOUTS_NLOCAL] * 4
        assert [set(n) for n in needs] == [{1, 2}, {0, 2, 3}, {0, 1, 3}, {1, 2}]          # the neighbours and the rank two further on
        r0, r1 = c.range(1)
        loc = c.entry_is_local()
        distinct = len(np.unique(c.ival[loc]))
        assert distinct == 8 if v == "int" else distinct > 2000
        assert np.argmax(c.abs_row_sums()) == c.planted
    for name, world in (("far", 4), ("far", 8), ("far2", 4), ("far_even", 4), ("islands", 4), ("bighalo", 2), ("bighalo", 4), ("layouts-int", 4), ("layouts-dyadic", 4)):
        xs, ys = vectors(name, world)
        c = case(name, world)
        assert np.abs(xs).max() <= 64 and np.array_equal(xs, np.rint(xs))
        assert np.abs(ys).max() * c.scale < 2.0 ** 53 and np.abs(c.abs_row_sums()).max() * 64 * c.scale < 2.0 ** 53
    f = case("float")
    g = case("far")                                                                   # far's pattern (the order inside a row apart), normal values
    assert f.counts == g.counts and np.array_equal(f.rowptr, g.rowptr)
    assert np.array_equal(f.col[np.lexsort((f.col, f.row))], g.col[np.lexsort((g.col, g.row))]) and f.ival is None


# ---- rank bodies ----------------------------------------------------------------------------------------------------------------------------
def _open(rank, comm):
    import slepc_amd as ks
    ctx = ks.Context(0)
    comm.install(ctx, rank)
    return ks, ctx


def _mat(ks, ctx, c, rank, keep_csr=False):
    rp, col, val = c.block(rank)
    return ks.Mat.from_csr(ctx, rp, col, val, row_start=c.range(rank)[0], n_global=c.N, keep_csr=keep_csr)


def _products(ks, ctx, A, xs_local):
    """A x for every x, all enqueued back to back with NO host wait in between (the vectors are uploaded first), then read back."""
    k = len(xs_local)
    B = ks.BV(ctx, A.n, 2 * k, N=A.N)
    for j, x in enumerate(xs_local):
        B.set_column(j, x)
    for j in range(k):
        A.mult_dev(B.column_ptr(j), B.column_ptr(k + j))
    ys = [B.column(k + j) for j in range(k)]
    B.destroy()
    return ys


def _threads(world, fn, timeout=120):
    return run_ranks(ThreadComm(world, pairwise=True, timeout=timeout), fn, join_timeout=2 * timeout)


def _assert_exact(y, yref, what):
    bad = np.flatnonzero(y != yref)
    assert bad.size == 0, "%s: %d of %d rows differ from the exact product, first at local row %d: %r instead of %r" % (what, bad.size, y.size, bad[0], y[bad[0]], yref[bad[0]])


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,world", [("far", 4), ("far", 8), ("islands", 4), ("bighalo", 2), ("bighalo", 4)])
def test_sharded_product_exact(name, world):
    """Every rank's product equals the integer reference bit for bit; empty rows are +0.0; a rank without rows completes every call."""
    c = case(name, world)
    xs, ys = vectors(name, world)

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            ctx.comm_check()
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            res = {"sizes": (A.n, A.N, A.nnz), "y": _products(ks, ctx, A, [xs[0][r0:r1], xs[1][r0:r1]])}
            res["diag"] = A.get_diagonal()
            res["norm"] = A.norm_inf()
            A.destroy()
            return res
        finally:
            ctx.close()
    out = _threads(world, fn)
    nloc, ngho, _, _ = c.row_stats()
    for rank in range(world):
        r0, r1 = c.range(rank)
        o = out[rank]
        assert o["sizes"] == (r1 - r0, c.N, int(c.rowptr[r1] - c.rowptr[r0]))
        for j in range(2):
            assert o["y"][j].shape == (r1 - r0,)
            _assert_exact(o["y"][j], ys[j][r0:r1], "%s rank %d of %d" % (name, rank, world))
            empty = (nloc + ngho)[r0:r1] == 0
            assert not np.signbit(o["y"][j][empty]).any() and not o["y"][j][empty].any()
        assert np.array_equal(o["diag"], c.diagonal()[r0:r1])
        assert o["norm"] == c.abs_row_sums().max()


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------
# layout asked for -> (case, layout the matrix must report); None: no KSGPU_SPMV, the chooser's own pick
LAYOUT_CASES = {
    "csr": [("layouts-int", "csr"), ("layouts-dyadic", "csr")],
    "csrvec": [("layouts-int", "csr"), ("layouts-dyadic", "csr")],
    "csrregs": [("layouts-int", "csr"), ("layouts-dyadic", "csr")],
    "sell": [("layouts-int", "sell"), ("layouts-dyadic", "sell")],
    "dict": [("layouts-int", "dict")],
    "odict": [("layouts-dyadic", "odict"), ("layouts-int", "odict")],
    "binned": [("far_even", "binned"), ("layouts-int", "binned")],
    "sliced": [("far_even", "sliced"), ("layouts-int", "sliced")],
    None: [("layouts-int", "dict"), ("layouts-dyadic", "odict"), ("far_even", "csr")],
}


def _layout_rank(c, xs, nprod=2):
    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            res = {"layout": A.layout(), "y": _products(ks, ctx, A, [x[r0:r1] for x in xs[:nprod]])}
            res["diag"] = A.get_diagonal()
            res["norm"] = A.norm_inf()
            A.destroy()
            return res
        finally:
            ctx.close()
    return fn


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", ["csr", "csrvec", "csrregs", "sell", "dict", "odict", "binned", "sliced", None], ids=lambda f: f or "auto")
def test_sharded_product_every_layout(fmt, monkeypatch):
    """Every layout of the diagonal block under a halo, on a matrix that qualifies for it: the layout is the one asked for on EVERY rank (a silent
    fall-through to SELL or CSR would leave its kernel untested) and the product is exact - so all layouts give one another's bits."""
    if fmt is None:
        monkeypatch.delenv("KSGPU_SPMV", raising=False)
    else:
        monkeypatch.setenv("KSGPU_SPMV", fmt)
    for name, want in LAYOUT_CASES[fmt]:
        c = case(name)
        xs, ys = vectors(name)
        out = _threads(4, _layout_rank(c, xs))
        for rank in range(4):
            r0, r1 = c.range(rank)
            assert out[rank]["layout"] == want, (fmt, name, rank, out[rank]["layout"])
            for j in range(2):
                _assert_exact(out[rank]["y"][j], ys[j][r0:r1], "%s as %s, rank %d" % (name, fmt or "auto", rank))


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_product_back_to_back_and_orderings():
    """Sixteen products of sixteen different vectors enqueued with no host wait in between: send_buf and ghost are not overwritten while an earlier
    product still reads them. The same with the halo on the main stream (halo_overlap = 0) instead of under the diagonal-block product."""
    for name in ("far", "bighalo"):
        c = case(name)
        xs, ys = vectors(name)

        def fn(rank, comm):
            ks, ctx = _open(rank, comm)
            try:
                A = _mat(ks, ctx, c, rank)
                r0, r1 = c.range(rank)
                xl = [x[r0:r1] for x in xs]
                res = {"overlap": _products(ks, ctx, A, xl)}
                ctx.set_debug("halo_overlap", 0)
                res["inorder"] = _products(ks, ctx, A, xl)
                ctx.synchronize()
                A.destroy()
                return res
            finally:
                ctx.close()
        out = _threads(4, fn)
        for rank in range(4):
            r0, r1 = c.range(rank)
            for j in range(NVEC):
                _assert_exact(out[rank]["overlap"][j], ys[j][r0:r1], "%s rank %d product %d" % (name, rank, j))
                assert np.array_equal(out[rank]["inorder"][j], out[rank]["overlap"][j]), (name, rank, j)


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_nonfinite_stays_in_its_rows():
    """An inf owned by rank 2 and a nan owned by rank 0: exactly the rows that reference those columns - on any rank, rows that hold nothing but
    ghosts included - are non-finite (nan where the reference is nan); every other row is finite and exact."""
    c = case("far")
    xs, ys = vectors("far")
    x = xs[2].copy()
    nloc, ngho, _, _ = c.row_stats()
    owner = c.owner_of_row
    # the inf: the column of rank 2 that the first rows of the other ranks read. The nan: the first column of rank 0 that rows of all three
    # non-empty ranks read, one of them a row with nothing but ghosts
    j_inf = c.range(2)[0] + c.counts[2] // 2
    sel = c.col < c.range(0)[1]
    pairs = np.unique(np.stack([c.col[sel], owner[c.row[sel]]], axis=1), axis=0)
    seen_by = np.bincount(pairs[:, 0], minlength=c.counts[0])
    ghost_only = np.zeros(c.counts[0], bool); ghost_only[c.col[sel][nloc[c.row[sel]] == 0]] = True
    j_nan = int(np.flatnonzero((seen_by == 3) & ghost_only)[0])
    x[j_inf], x[j_nan] = np.inf, np.nan
    touched = np.zeros(c.N, bool)
    touched[c.rows_referencing(j_inf)] = True; touched[c.rows_referencing(j_nan)] = True
    with np.errstate(invalid="ignore"):
        yref = sc.sp.csr_matrix((c.val, c.col, c.rowptr), shape=(c.N, c.N)) @ x      # every finite partial sum is exact; inf and nan do not depend on the order
    assert np.array_equal(~np.isfinite(yref), touched) and np.isnan(yref).any() and np.isinf(yref).any()
    assert (touched & (nloc == 0)).any()                                              # a ghost-only row is among them
    assert len(set(owner[np.isnan(yref)])) == 3 and len(set(owner[np.isinf(yref)]) - {2}) >= 1      # the nan on every non-empty rank, the inf beyond its owner

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            y = _products(ks, ctx, A, [x[r0:r1]])[0]
            A.destroy()
            return y
        finally:
            ctx.close()
    out = _threads(4, fn)
    y = np.concatenate(out)
    assert np.array_equal(np.isnan(y), np.isnan(yref))
    assert np.array_equal(np.isfinite(y), ~touched)
    assert np.array_equal(y, yref, equal_nan=True)                                    # finite rows exact, infinite rows with the reference's sign
    _assert_exact(y[~touched], ys[2][~touched], "rows that reference neither column")


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_block_product_and_bv_matmult():
    """ks_mat_mult_multi with 1, 8 and 11 columns and padded leading dimensions, and BVMatMult under both methods, on sharded matrices: the bits of
    the column-by-column product and the exact reference."""
    for name in ("far", "layouts-int"):
        c = case(name)
        xs, ys = vectors(name)

        def fn(rank, comm):
            ks, ctx = _open(rank, comm)
            try:
                A = _mat(ks, ctx, c, rank)
                r0, r1 = c.range(rank)
                n = r1 - r0
                res = {"single": _products(ks, ctx, A, [x[r0:r1] for x in xs[:11]])}
                ld = (n + 31) // 32 * 32
                X = ks.BV(ctx, n, 11, ld=ld + 32, N=c.N); Y = ks.BV(ctx, n, 11, ld=ld + 96, N=c.N)
                for j in range(11):
                    X.set_column(j, xs[j][r0:r1])
                for k in (1, 8, 11):
                    for j in range(11):
                        Y.set_column(j, np.full(n, -7.0))
                    A.mult_multi_dev(X.column_ptr(0), X.ld, Y.column_ptr(0), Y.ld, k)
                    res["multi%d" % k] = [Y.column(j) for j in range(11)]
                for method in ("vecs", "mat"):
                    W = ks.BV(ctx, n, 11, N=c.N)
                    X.SetMatMultMethod(ks.MATMULT[method])
                    X.MatMult(A, W)
                    res[method] = [W.column(j) for j in range(11)]
                    W.destroy()
                res["ld"] = (X.ld, Y.ld)
                X.destroy(); Y.destroy(); A.destroy()
                return res
            finally:
                ctx.close()
        out = _threads(4, fn)
        for rank in range(4):
            r0, r1 = c.range(rank)
            o = out[rank]
            assert o["ld"][0] >= r1 - r0 + 32 and o["ld"][1] >= r1 - r0 + 96
            for j in range(11):
                _assert_exact(o["single"][j], ys[j][r0:r1], "%s rank %d column %d" % (name, rank, j))
            for k in (1, 8, 11):
                for j in range(11):
                    want = o["single"][j] if j < k else np.full(r1 - r0, -7.0)       # columns beyond ncols are not touched
                    assert np.array_equal(o["multi%d" % k][j], want), (name, rank, k, j)
            for method in ("vecs", "mat"):
                for j in range(11):
                    assert np.array_equal(o[method][j], o["single"][j]), (name, rank, method, j)


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_diagonal_norm_and_axpy(monkeypatch):
    """MatGetDiagonal (duplicates on the diagonal summed) and MatNorm(NORM_INFINITY) of sharded matrices, also where the layout released the CSR arrays
    and serves both from what it cached per rank; the largest row sum sits in ghost entries, so a norm without the off-diagonal block fails.
    A + alpha B of two sharded matrices multiplies to the exact (A + alpha B) x; MatMultTranspose of a sharded matrix is KS_ERR_SUP on every rank."""
    for name, fmt in (("far", None), ("layouts-int", "dict"), ("layouts-int", "binned"), ("layouts-int", "sliced")):
        if fmt is None:
            monkeypatch.delenv("KSGPU_SPMV", raising=False)
        else:
            monkeypatch.setenv("KSGPU_SPMV", fmt)
        c = case(name)
        xs, ys = vectors(name)
        out = _threads(4, _layout_rank(c, xs, nprod=1))
        nloc, ngho, _, _ = c.row_stats()
        assert ngho[c.planted] > 0
        for rank in range(4):
            r0, r1 = c.range(rank)
            assert fmt is None or out[rank]["layout"] == fmt                          # (far: whatever the chooser picks per rank)
            assert np.array_equal(out[rank]["diag"], c.diagonal()[r0:r1]), (name, fmt, rank)
            assert out[rank]["norm"] == c.abs_row_sums().max() == c.abs_row_sums()[c.planted], (name, fmt, rank, out[rank]["norm"])
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    a, b = case("far"), case("far2")
    xs, ya = vectors("far")
    _, yb = vectors("far2")
    assert np.array_equal(vectors("far2")[0], xs)
    alpha = -0.375

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A, B = _mat(ks, ctx, a, rank, keep_csr=True), _mat(ks, ctx, b, rank, keep_csr=True)
            P = A.axpy_new(alpha, B)
            r0, r1 = a.range(rank)
            res = {"y": _products(ks, ctx, P, [xs[3][r0:r1]])[0], "diag": P.get_diagonal(), "norm": P.norm_inf()}
            W = ks.BV(ctx, A.n, 2, N=A.N)
            try:
                A.mult_transpose_dev(W.column_ptr(0), W.column_ptr(1))
                res["transpose"] = None
            except ks.KsError as e:
                res["transpose"] = e.rc
            W.destroy(); P.destroy(); A.destroy(); B.destroy()
            return res
        finally:
            ctx.close()
    out = _threads(4, fn)
    da, db = a.diagonal(), b.diagonal()
    for rank in range(4):
        r0, r1 = a.range(rank)
        _assert_exact(out[rank]["y"], (ya[3] + alpha * yb[3])[r0:r1], "A + alpha B, rank %d" % rank)      # multiples of 1/8 far below 2^53: exact
        assert np.array_equal(out[rank]["diag"], (da + alpha * db)[r0:r1])
        assert out[rank]["transpose"] == KS_ERR_SUP
    # one norm on all ranks; its value depends on how the sum keeps duplicate entries apart, but ||P x||_inf <= ||P||_inf ||x||_inf holds for any of them
    assert len({o["norm"] for o in out}) == 1 and out[0]["norm"] * 64 >= np.abs(ya[3] + alpha * yb[3]).max()


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_sharded_creation_rejects_unordered_row_blocks():
    """Row blocks given in descending rank order: every rank refuses with KS_ERR_ARG_WRONG right after the allgather of the starts - none of them
    goes on into a collective the others have left."""
    c = sc.Case("two", [300, 200], np.arange(501), np.arange(500), np.ones(500, np.int64))
    timeout = 40

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            other = 1 - rank
            rp, col, val = c.block(other)                           # rank 0 brings the rows [300, 500), rank 1 the rows [0, 300)
            t0 = time.perf_counter()
            try:
                ks.Mat.from_csr(ctx, rp, col, val, row_start=c.range(other)[0], n_global=c.N)
                return None, 0.0
            except ks.KsError as e:
                return e.rc, time.perf_counter() - t0
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(2, pairwise=True, timeout=timeout), fn, join_timeout=2 * timeout)
    for rank in range(2):
        assert out[rank][0] == KS_ERR_ARG_WRONG, out[rank]
        assert out[rank][1] < timeout / 4                           # nobody ran into a time limit


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------------
def _peer_worker(rank, world, port, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import slepc_amd as ks
        from slepc_amd import gloo_provider
        ctx = ks.Context(0)
        gloo_provider.install(ctx, dist, torch, rank, world)
        res = {}
        for name in (("bighalo",) if world == 2 else ("bighalo", "far", "islands")):
            c = case(name, world)
            xs, ys = vectors(name, world)
            r0, r1 = c.range(rank)
            xl = [x[r0:r1] for x in xs]
            yl = [y[r0:r1] for y in ys]
            A = _mat(ks, ctx, c, rank)
            prov = _products(ks, ctx, A, xl)
            o = {"active": A.set_halo("peer")}
            peer = _products(ks, ctx, A, xl)                        # sixteen products back to back, no host wait: parities, acknowledgements, tickets
            o["back"] = A.set_halo("provider")
            again = _products(ks, ctx, A, xl[:1])[0]
            ctx.synchronize()                                       # raises if a bounded wait of the peer halo gave up
            o["prov_exact"] = all(np.array_equal(p, y) for p, y in zip(prov, yl))
            o["peer_bits"] = [bool(np.array_equal(p, v)) for p, v in zip(peer, prov)]
            o["peer_exact"] = [int(np.count_nonzero(p != y)) for p, y in zip(peer, yl)]
            o["again_bits"] = bool(np.array_equal(again, prov[0]))
            A.destroy()
            res[name] = o
        dist.barrier()
        ctx.close()
        q.put((rank, res))
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_product_peer_halo(world):
    """The peer-mapped halo (k_halo_pack / k_halo_unpack) on general matrices, between processes: halos of four and more workgroups, so that the
    ticket hand-over decides which workgroup stamps the flags; three peers of unequal counts (the pack's peer search); a rank with no peers, one
    that only sends and one that only receives. Same bits as the provider's exchange and the exact reference, sixteen products back to back."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_peer_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(_collect(q, procs, world))
    for r in range(world):
        assert "error" not in out[r], out[r].get("error")
    for r in range(world):
        for name, o in out[r].items():
            assert o["active"] == "peer" and o["back"] == "provider", (name, r, o)      # the isolated rank of `islands` included
            assert o["prov_exact"], (name, r)
            assert o["peer_exact"] == [0] * NVEC and all(o["peer_bits"]), (name, r, o["peer_exact"], o["peer_bits"])
            assert o["again_bits"], (name, r)
    assert set(out[0]) == ({"bighalo"} if world == 2 else {"bighalo", "far", "islands"})


# ---- 9 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sharded_product_float_bound():
    """Normal values and vectors: |y_i - yhat_i| <= (k_i + 2) 2^-52 sum_j |a_ij| |x_j| per row, yhat the long-double product and k_i the row's stored
    entries (local plus ghost). That is the forward bound gamma_k of a k-term fma/add accumulation (k_i rounding errors of u = 2^-53 each, first
    order), one more addition where the ghost pass adds its sum to the diagonal block's, doubled: derived, not measured."""
    c = case("float")
    x = np.random.default_rng(5).standard_normal(c.N)
    al, xl = c.val.astype(np.longdouble), x.astype(np.longdouble)
    prod = al * xl[c.col]
    idx = c.rowptr[:-1][np.diff(c.rowptr) > 0]
    yhat = np.zeros(c.N, np.longdouble); mag = np.zeros(c.N, np.longdouble)
    nz = np.diff(c.rowptr) > 0
    yhat[nz] = np.add.reduceat(prod, idx); mag[nz] = np.add.reduceat(np.abs(prod), idx)
    k = np.diff(c.rowptr).astype(np.longdouble)

    def fn(rank, comm):
        ks, ctx = _open(rank, comm)
        try:
            A = _mat(ks, ctx, c, rank)
            r0, r1 = c.range(rank)
            y = _products(ks, ctx, A, [x[r0:r1]])[0]
            A.destroy()
            return y
        finally:
            ctx.close()
    y = np.concatenate(_threads(4, fn))
    err = np.abs(y.astype(np.longdouble) - yhat)
    bound = (k + 2) * np.longdouble(2.0) ** -52 * mag
    worst = int(np.argmax(err - bound))
    print("float case: max error / bound = %.3g" % float(np.max(err[mag > 0] / bound[mag > 0])))
    assert np.all(err <= bound), (worst, float(err[worst]), float(bound[worst]))
    assert not y[~nz].any()
