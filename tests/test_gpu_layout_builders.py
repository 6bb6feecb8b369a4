"""The assembly code of ks_mat.hip at its limits: build_dict and k_dict_encode, build_sell, exclusive_scan_int, choose_layout.

What decides which kernel a matrix gets and which tables that kernel reads is pinned here ON its boundaries (tests/layout_cases.py): 255 / 256
values and 255 / 256 / 257 offsets (code value 255 is the padding mark), row lengths 8 / 9, 16 / 17, 32 / 33 where the code width switches, both
sides of the two admission inequalities, dictionaries that take many rounds to discover, keys that are NaN, infinities, denormals and signed
zeros, and item counts of the prefix sum on and beside its 2048-item tiles.

Every layout is compared with layout_cases.predict_layout, a restatement of the choice that calls nothing, and every product on integer data with
the exact integer reference by np.array_equal; non-integer data is compared bit for bit with the SELL-64 build of the same arrays."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import layout_cases as lc
from test_gpu_dict_patterns import pattern_count
from thread_comm import ThreadComm, run_ranks

gpu = pytest.mark.gpu

DICT_LIMITS = [(255, 256), (255, 257), (256, 255), (256, 256), (1, 1), (254, 255)]       # (values, offsets)
LIMIT_LAYOUTS = {(255, 256): "dict", (255, 257): None, (256, 255): "odict", (256, 256): None, (1, 1): "dict", (254, 255): "dict"}      # None: no dictionary form
WIDTHS = {8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 0}                                   # longest row -> code width, 0: no dictionary form
N_DIAGONAL = 960 + 37          # a diagonal matrix passes the padding rule 8 n <= 4 nnz + 4096 only up to about a thousand rows
LAYERED = [(12, "values"), (40, "values"), (20, "offsets")]
SCAN_SELL_SLICES = [2046, 2047, 2048, 4096]                                             # slices + 1 = items of build_sell's scan: 2047, 2048, 2049, 4097
SCAN_SELL_SMALL = [1, 63, 64, 65]
SCAN_SLICED_N = [4095, 4096, 6144]                                                      # n + 1 = 4096, 4097, 6145


@functools.lru_cache(maxsize=None)
def case(kind, *args):
    """CSR arrays of a case, built once, shared by every test and never written to."""
    if kind == "limit":
        nval, noff = args
        a = lc.dict_boundary(nval, noff, 1, N_DIAGONAL) if (nval, noff) == (1, 1) else lc.dict_boundary(nval, noff, 8)
    elif kind == "width":
        a = lc.dict_boundary(7, 41, args[0])
    elif kind == "symmetric":
        a = lc.symmetric_boundary(255, 256, {8: 43, 16: 21}[args[0]])
    elif kind == "padding":
        a = lc.padding_rule(lc.N_DICT, *args)
    elif kind == "sell":
        a = lc.sell_rule(lc.N_DICT, *args)
    elif kind == "layered":
        a = lc.layered(*args)
    elif kind == "ragged":
        a = lc.ragged(args[0], seed=args[0] % 1000)
    elif kind == "two_rank":
        a = lc.two_rank_ghosts()
    else:
        raise KeyError(kind)
    for x in a:
        x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(kind, *args):
    """(x, exact A x, X of 8 columns, exact A X, exact diagonal, exact infinity norm) of a case; the scan cases take the single product only."""
    a = case(kind, *args)
    n = len(a[0]) - 1
    x, X = lc.int_vector(n, 3), lc.int_vector(n, 4, cols=8)
    Y = None if kind in ("ragged", "two_rank") else lc.exact_product(*a, X)
    out = (x, lc.exact_product(*a, x), X, Y, lc.exact_diagonal(*a), lc.exact_norm_inf(*a))
    for o in out[:5]:
        if o is not None:
            o.setflags(write=False)
    return out


# ---- the cases stand where the GPU tests need them (no GPU) -------------------------------------------------------------------------------
def test_layout_case_generators_deliver_their_properties():
    for nval, noff in DICT_LIMITS:
        rp, col, val = a = case("limit", nval, noff)
        n, maxlen = len(rp) - 1, (1 if (nval, noff) == (1, 1) else 8)
        lens = np.diff(rp)
        assert lc.distinct_values(val) == nval and lc.distinct_offsets(rp, col) == noff and lc.max_row_length(rp) == maxlen
        assert set(lens.tolist()) == set(range(maxlen + 1)) and n % 64 and lens[5] == 0 and lens[n - 3] == 0
        assert np.abs(val).max() <= 255 and np.array_equal(val, np.rint(val))
        lhs, rhs = lc.padding_sides(rp, 8)
        assert lhs <= rhs, (nval, noff, lhs, rhs)                                          # not "mostly padding": the dictionary limits decide
        rows = np.repeat(np.arange(n), lens)
        vi, oi = lc.codes(*a)
        off = col - rows
        for sel, fits in ((rows < 64, off[off >= 0]), (rows >= n - 64, off[off <= 0])):
            assert len(np.unique(vi[sel])) == nval and set(np.unique(fits).tolist()) <= set(off[sel].tolist())
        assert np.any((vi == nval - 1) & (oi == noff - 1))                                 # the last slot of both tables, in one entry
        want = LIMIT_LAYOUTS[(nval, noff)]
        got = lc.predict_layout(*a)
        assert (got == (want, 8 if want == "dict" else 0)) if want else got[0] in ("sell", "csr"), (nval, noff, got)
        assert lc.predict_layout(*a, force="dict") == got                                   # forced dict is the automatic attempt
        forced = lc.predict_layout(*a, force="odict")                                      # forced odict: the offsets alone decide
        assert forced == ("odict", 0) if noff <= 255 else forced[0] in ("sell", "csr"), (nval, noff, forced)
    vi, oi = lc.codes(*case("limit", 255, 256))
    assert ((vi << 8) | oi).max() == 0xfeff
    vi, oi = lc.codes(*case("limit", 256, 255))
    assert oi.max() == 254
    assert pattern_count(*case("limit", 255, 256)) <= 256 and pattern_count(*case("limit", 1, 1)) <= 256      # these take the row-pattern form
    for maxlen, w in WIDTHS.items():
        rp, col, val = a = case("width", maxlen)
        assert lc.max_row_length(rp) == maxlen and set(np.diff(rp).tolist()) == set(range(maxlen + 1))
        assert lc.distinct_values(val) == 7 and lc.distinct_offsets(rp, col) == 41
        got = lc.predict_layout(*a)
        assert got == ("dict", w) if w else got[0] in ("sell", "csr"), (maxlen, got)
    for w in (8, 16):
        rp, col, val = a = case("symmetric", w)
        n = len(rp) - 1
        assert lc.distinct_values(val) == 255 and lc.distinct_offsets(rp, col) == 256 and lc.predict_layout(*a) == ("dict", w)
        assert (w // 2 < lc.max_row_length(rp) <= w) if w == 16 else lc.max_row_length(rp) <= 8
        S = sp.csr_matrix((val, col, rp), shape=(n, n))
        assert (S != S.T).nnz == 0 and S.diagonal().max() == 0 == S.diagonal().min()
        vi, oi = lc.codes(*a)
        assert ((vi << 8) | oi).max() == 0xfeff
    for W in (8, 16, 32):
        for delta in (0, -1):
            rp, col, val = a = case("padding", W, delta)
            lhs, rhs = lc.padding_sides(rp, W)
            assert lc.max_row_length(rp) == W and lhs - rhs == -4 * delta and (np.diff(rp) == 0).sum() > 10
            assert lc.distinct_values(val) == 3 and W <= lc.distinct_offsets(rp, col) <= 2 * W - 1
            got = lc.predict_layout(*a)
            assert got == ("dict", W) if delta == 0 else got == ("sell", 0), (W, delta, got)
    for delta in (0, 64):
        rp, col, val = a = case("sell", delta)
        lhs, rhs = lc.sell_sides(rp)
        assert lhs - rhs == 8 * delta and int(rp[-1]) % 8 == 0
        assert lc.distinct_values(val) == 400 and lc.distinct_offsets(rp, col) > 256 and 8 < lc.max_row_length(rp) <= 32
        assert (lc.slice_widths(rp) == 0).sum() >= 4
        assert lc.predict_layout(*a) == (("sell", 0) if delta == 0 else ("csr", 0))
    for layers, vary in LAYERED:
        rp, col, val = a = case("layered", layers, vary)
        n = len(rp) - 1
        rows = np.repeat(np.arange(n), np.diff(rp))
        block = np.minimum(rows // lc.LAYER_ROWS, layers - 1)
        assert np.bincount(block).min() > 4096 and lc.max_row_length(rp) == 7
        key = val if vary == "values" else (col - rows)[col != rows]
        blk = block if vary == "values" else block[col != rows]
        owners = {}
        for k, b in zip(key.tolist(), blk.tolist()):
            owners.setdefault(k, set()).add(b)
        assert all(len(s) == 1 for s in owners.values())                                   # no block shares a value (an off-diagonal offset) with another
        assert (lc.distinct_values(val), lc.distinct_offsets(rp, col)) == ((2 * layers, 7) if vary == "values" else (4, 6 * layers + 1))
        assert lc.predict_layout(*a) == ("dict", 8)
    rp, col, val, line = lc.special_values()
    assert lc.distinct_values(val) == 12 == len(lc.SPECIAL_KEYS) and lc.distinct_offsets(rp, col) == 13 and lc.max_row_length(rp) == 13
    assert lc.predict_layout(rp, col, val) == ("dict", 16) and pattern_count(rp, col, val) <= 256
    x = lc.special_x(len(rp) - 1)
    assert np.all(np.isfinite(x)) and np.all(np.abs(x) > 0.5) and np.all(np.abs(x) < 1.0)
    for m in SCAN_SELL_SLICES:
        n = 64 * m - 27
        assert (n + 63) // 64 + 1 == m + 1
    assert [m + 1 for m in SCAN_SELL_SLICES] == [2047, 2048, 2049, 4097] and [n + 1 for n in SCAN_SLICED_N] == [4096, 4097, 6145]
    for n in SCAN_SELL_SMALL + SCAN_SLICED_N + [64 * m - 27 for m in SCAN_SELL_SLICES]:
        rp, col, val = case("ragged", n)
        assert len(rp) - 1 == n and rp[1] > 0 and lc.max_row_length(rp) <= 64 and (n < 63 or (np.diff(rp) == 0).sum() > n // 8)
    rp, col, val = case("two_rank")
    rows = np.repeat(np.arange(4096), np.diff(rp))
    ghost = (col // 2048) != (rows // 2048)
    assert np.array_equal(np.unique(rows[ghost]), np.arange(0, 4096, 3)) and np.bincount(rows[ghost]).max() == 1


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _layout(A):
    return A.layout(), A.dict_info()["w"]


def _assert_exact(y, yref, what):
    bad = np.flatnonzero(y != yref)
    assert bad.size == 0, "%s: %d of %d rows differ from the exact product, first at row %d: %r instead of %r" % (what, bad.size, y.size, bad[0], y[bad[0]], yref[bad[0]])


def _check_products(A, ref, what, block=True):
    x, y, X, Y, diag, nrm = ref
    _assert_exact(A.mult(x), y, what)
    if block:
        for k in (3, 8):
            Yk = A.mult_multi(X[:, :k])
            for j in range(k):
                _assert_exact(Yk[:, j], Y[:, j], "%s, column %d of %d" % (what, j, k))
    assert np.array_equal(A.get_diagonal(), diag), what
    assert A.norm_inf() == nrm, what


def _check_case(ks, ctx, debug, monkeypatch, key):
    """The automatic build against the predictor and the exact reference; for a dictionary matrix also the other storage form; the SELL-64
    build; forced dict and odict against what the predictor says they end in."""
    arrays, ref = case(*key), reference(*key)
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    pred = lc.predict_layout(*arrays)
    A = ks.Mat.from_csr(ctx, *arrays)
    assert _layout(A) == pred, (key, _layout(A), pred)
    _check_products(A, ref, "%s as %s" % (key, pred[0]))
    if pred[0] == "dict":
        info = A.dict_info()
        assert info["patterns"] == (pattern_count(*arrays) <= 256), (key, info)
        debug("no_dict_patterns")
        B = ks.Mat.from_csr(ctx, *arrays)
        debug("no_dict_patterns", 0)
        assert _layout(B) == pred and not B.dict_info()["patterns"]
        _check_products(B, ref, "%s as codes" % (key,))
        B.destroy()
    A.destroy()
    for force in ("sell", "dict", "odict"):
        monkeypatch.setenv("KSGPU_SPMV", force)
        F = ks.Mat.from_csr(ctx, *arrays)
        want = lc.predict_layout(*arrays, force=force)
        assert _layout(F) == want, (key, force, _layout(F), want)
        _check_products(F, ref, "%s forced %s, built as %s" % (key, force, want[0]), block=False)
        F.destroy()
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    return pred


# ---- dictionary limits and code widths ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nval,noff", DICT_LIMITS)
def test_dictionary_limits(ctx, debug, monkeypatch, nval, noff):
    """255 values and 256 offsets fill both tables (code 0xfeff is an entry, 0xff00 is padding); one offset more, or 256 values with 256 offsets,
    is no dictionary matrix; 256 values with 255 offsets keep their values in full (offset code 254 is an entry, 255 is padding)."""
    import slepc_amd as ks
    pred = _check_case(ks, ctx, debug, monkeypatch, ("limit", nval, noff))
    want = LIMIT_LAYOUTS[(nval, noff)]
    assert pred[0] == want if want else pred[0] in ("sell", "csr")


@gpu
@pytest.mark.parametrize("maxlen", list(WIDTHS))
def test_code_width_switches(ctx, debug, monkeypatch, maxlen):
    """The longest row decides the code width: 8 up to 8 entries, 16 up to 16, 32 up to 32, and no dictionary form beyond."""
    import slepc_amd as ks
    pred = _check_case(ks, ctx, debug, monkeypatch, ("width", maxlen))
    assert pred[1] == WIDTHS[maxlen] and (pred[0] == "dict") == (WIDTHS[maxlen] > 0)


@gpu
@pytest.mark.parametrize("w", [8, 16])
def test_fused_product_with_full_tables(ctx, debug, monkeypatch, w):
    """k_dot_spmv_dict with 255 values and 256 offsets in LDS: a Lanczos run on a symmetric matrix with and without the no_spmv_dot hook gives the
    same coefficients and the same basis, bit for bit."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    arrays = case("symmetric", w)
    n, m = len(arrays[0]) - 1, 24
    outs = {}
    for fused in (True, False):
        debug("no_spmv_dot", 0 if fused else 1)
        A = ks.Mat.from_csr(ctx, *arrays)
        assert _layout(A) == ("dict", w)
        V = ks.BV(ctx, n, m + 1)
        V.SetRandomColumn(0)
        _, nrm, _ = V.OrthogonalizeColumn(0); V.ScaleColumn(0, 1.0 / nrm)
        T = np.zeros((m + 1, 3), order="F")
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            r = V.MatLanczos(A, T, 0, m)
            ctx.synchronize()
            prof = ctx.prof_get(by_variant=True)
        finally:
            ctx.prof_enable(False)
        nf = sum(d["launches"] for (c, v), d in prof.items() if c == "spmv_dot_fused")
        assert (nf >= 1) if fused else (nf == 0), (fused, nf)
        outs[fused] = (T.copy(), V.dense(), r)
        V.destroy(); A.destroy()
    assert outs[False][2][0] == m and not outs[False][2][2]
    assert np.array_equal(outs[True][0], outs[False][0]) and np.array_equal(outs[True][1], outs[False][1]) and outs[True][2] == outs[False][2]
    A = ks.Mat.from_csr(ctx, *arrays)
    _check_products(A, reference("symmetric", w), "symmetric, W = %d" % w)
    A.destroy()


# ---- admission rules ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("W,delta", [(W, d) for W in (8, 16, 32) for d in (0, -1)])
def test_padding_rule_both_sides(ctx, debug, monkeypatch, W, delta):
    """W n = 4 nnz + 4096 is still a dictionary matrix; one entry fewer is mostly padding and goes to SELL-64."""
    import slepc_amd as ks
    pred = _check_case(ks, ctx, debug, monkeypatch, ("padding", W, delta))
    assert pred == (("dict", W) if delta == 0 else ("sell", 0))


@gpu
@pytest.mark.parametrize("delta", [0, 64])
def test_sell_rule_both_sides(ctx, debug, monkeypatch, delta):
    """64 sum width = 1.125 nnz + 4096 is the last matrix SELL-64 admits; one slice one entry wider stays CSR. Four slices hold only empty rows."""
    import slepc_amd as ks
    pred = _check_case(ks, ctx, debug, monkeypatch, ("sell", delta))
    assert pred == (("sell", 0) if delta == 0 else ("csr", 0))


# ---- discovery ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layers,vary", LAYERED)
def test_discovery_does_not_depend_on_order(ctx, monkeypatch, layers, vary):
    """Dictionaries whose entries lie in long runs of rows: a round of discovery records 4096 misses, all of them from the blocks that run
    first, so the dictionaries grow by a block or two per round. However many rounds that takes, three builds give the dictionary layout."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    arrays, ref = case("layered", layers, vary), reference("layered", layers, vary)
    pred = lc.predict_layout(*arrays)
    assert pred == ("dict", 8)
    seen = []
    for _ in range(3):
        A = ks.Mat.from_csr(ctx, *arrays)
        seen.append((A.layout(), A.dict_info()))
        _check_products(A, ref, "layered %d %s" % (layers, vary), block=False)
        A.destroy()
    assert all(s[0] == "dict" and s[1]["w"] == 8 for s in seen) and seen[0] == seen[1] == seen[2], seen
    assert seen[0][1]["patterns"] == (pattern_count(*arrays) <= 256)


# ---- keys by bit pattern ------------------------------------------------------------------------------------------------------------------
@gpu
def test_special_values_are_keys_by_bit_pattern(ctx, debug, monkeypatch):
    """0.0 and -0.0, two NaNs, both infinities, both smallest denormals, 1.0 and its neighbour, -1.0 and 1e308 are twelve dictionary keys.

    The product has the bits of the SELL-64 build (NaN where it has NaN); rows without a NaN or infinite entry are finite; the diagonal has the
    bits of the SELL-64 build's. Rows of line 0 hold only zeros, denormals and +-1, and 0.5 < |x| < 1: a product by +-1 is exact, a product by
    a denormal is one denormal unit whether it is rounded before the addition or inside an fma, and a product by a zero is a zero added to a
    sum that starts at +0.0 - so the kernels' fma chain and the oracle's multiply-then-add loop over the entries in order agree bit for bit."""
    import slepc_amd as ks
    from oracle import oracle as O
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    rp, col, val, line = lc.special_values()
    n = len(rp) - 1
    x = lc.special_x(n)
    ys, ds = {}, {}
    for form in ("patterns", "codes", "sell"):
        debug("no_dict_patterns", 1 if form == "codes" else 0)
        if form == "sell":
            monkeypatch.setenv("KSGPU_SPMV", "sell")
        A = ks.Mat.from_csr(ctx, rp, col, val)
        if form == "sell":
            assert A.layout() == "sell"
        else:
            assert _layout(A) == ("dict", 16) and A.dict_info()["patterns"] == (form == "patterns"), (form, A.layout(), A.dict_info())
        ys[form], ds[form] = A.mult(x), A.get_diagonal()
        Y = A.mult_multi(np.stack([x, -x, x[::-1]], axis=1))
        assert np.array_equal(Y[:, 0].view(np.int64), ys[form].view(np.int64)), form
        A.destroy()
    for form in ("patterns", "codes"):
        assert np.array_equal(ys[form], ys["sell"], equal_nan=True), form
        assert np.array_equal(ds[form].view(np.int64), ds["sell"].view(np.int64)), form
    y = ys["patterns"]
    rows = np.repeat(np.arange(n), np.diff(rp))
    has_nan = np.bincount(rows, weights=np.isnan(val), minlength=n) > 0                # (the band loses entries at the matrix edge: taken from the arrays)
    has_inf = np.bincount(rows, weights=np.isinf(val), minlength=n) > 0
    assert has_nan.sum() > n // 4 and has_inf.sum() > n // 4 and not (has_nan & has_inf).any() and not (has_nan | has_inf)[line <= 1].any()
    assert np.array_equal(np.isnan(y), has_nan) and np.array_equal(np.isinf(y), has_inf)      # every other row is finite
    with np.errstate(all="ignore"):
        yo = O.CSR(n, rp, col, val).mult(x)
    tame = line == 0
    assert tame.sum() > n // 7 and np.array_equal(y[tame].view(np.int64), yo[tame].view(np.int64))


# ---- the prefix sum on and beside its tiles -----------------------------------------------------------------------------------------------
def _forced(ks, ctx, monkeypatch, force, n):
    arrays, ref = case("ragged", n), reference("ragged", n)
    monkeypatch.setenv("KSGPU_SPMV", force)
    A = ks.Mat.from_csr(ctx, *arrays)
    want = lc.predict_layout(*arrays, force=force)
    assert _layout(A) == want, (force, n, _layout(A), want)
    _check_products(A, ref, "ragged n = %d forced %s" % (n, force), block=False)
    A.destroy()
    return want


@gpu
@pytest.mark.parametrize("n", SCAN_SELL_SMALL + [64 * m - 27 for m in SCAN_SELL_SLICES])
def test_scan_edges_sell(ctx, monkeypatch, n):
    """build_sell scans slices + 1 widths: 2047, 2048, 2049 and 4097 items (one below, on and one above a 2048-item tile, two tiles plus one),
    and the one or two slices of 1, 63, 64 and 65 rows."""
    import slepc_amd as ks
    assert _forced(ks, ctx, monkeypatch, "sell", n) == ("sell", 0)


@gpu
@pytest.mark.parametrize("n", SCAN_SLICED_N)
def test_scan_edges_sliced(ctx, monkeypatch, n):
    """build_sliced scans n + 1 counts per slice: 4097 and 6145 items (whole tiles plus one). The layout is built from 4096 rows on; at 4095 rows
    (4096 items) the forced choice ends where the predictor says and the product is exact all the same."""
    import slepc_amd as ks
    got = _forced(ks, ctx, monkeypatch, "sliced", n)[0]
    assert got == "sliced" if n >= 4096 else got in ("sell", "csr")


@gpu
@pytest.mark.timeout(120)
def test_scan_edges_offdiagonal_compaction_two_ranks(monkeypatch):
    """Two ranks of 2048 rows (2049 items in compact_offdiag_rows' scan: one tile plus one), a ghost entry in every third row: the product of
    every rank equals the exact product of the whole matrix."""
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    rp, col, val = case("two_rank")
    x, y = reference("two_rank")[:2]

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        comm.install(ctx, rank)
        try:
            r0, r1 = 2048 * rank, 2048 * (rank + 1)
            p0, p1 = int(rp[r0]), int(rp[r1])
            A = ks.Mat.from_csr(ctx, rp[r0:r1 + 1] - p0, col[p0:p1], val[p0:p1], row_start=r0, n_global=4096)
            B = ks.BV(ctx, A.n, 2, N=A.N)
            B.set_column(0, x[r0:r1])
            A.mult_dev(B.column_ptr(0), B.column_ptr(1))
            out = B.column(1)
            B.destroy(); A.destroy()
            return out
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(2, pairwise=True, timeout=60), fn, join_timeout=120)
    for rank in range(2):
        _assert_exact(out[rank], y[2048 * rank:2048 * (rank + 1)], "rank %d of 2" % rank)
