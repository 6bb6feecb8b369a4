"""Block CSR (BAIJ) matrices (ks_mat_create_bsr, KS_MAT_LAYOUT_BSR): the creation call, what the matrix reports, and its products (ks_spmv.hip:
k_spmv_bsr and, below 2048 rows, k_spmv_bsr_vec; ks_spmm.hip: k_spmm_bsr) for every block size 2 .. 8, on every path of the walks: block rows without
blocks, one with one block, one longer than three chunks, unsorted and repeated block columns, a partial last group, x and y that are only 8-byte
aligned. Every case comes at 5 G + 3 block rows (fewer than 2048 rows: the small-matrix form) and at 10 G + 3 (the chunked walk and the block kernel).

Integer data is compared with the exact integer reference of the EXPANSION (bsr_cases.expand) by np.array_equal; real data bit for bit with the CSR
kernel (KSGPU_SPMV=csr) of the same arrays, given as blocks and given as the numpy expansion, and with the oracle to rounding. The two constants of
the product are read from bsr_info(); the cases are built once per block size and never written to."""
import ctypes as C
import functools

import numpy as np
import pytest

import bsr_cases as bc
import layout_cases as lc

gpu = pytest.mark.gpu
SIZES = list(range(2, 9))
GROUPS = [5, 10]      # 5 G + 3 block rows: fewer than 2048 rows, the small-matrix form of the product; 10 G + 3: the chunked walk (bsr_cases.small)
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
KS_ERR_ARG_SIZ, KS_ERR_ARG_WRONG, KS_ERR_ARG_OUTOFRANGE, KS_ERR_ARG_INCOMP = 60, 62, 63, 75      # include/ksgpu.h


def constants(ctx, bs):
    """(group_block_rows, chunk_entries) of the library for this block size: reported by any block CSR matrix."""
    import slepc_amd as ks
    A = ks.Mat.from_bsr(ctx, [0, 1], [0], np.ones((1, bs, bs)))
    i = A.bsr_info()
    assert A.layout() == "bsr" and i["bs"] == bs and i["block_rows"] == 1 and i["blocks"] == 1 and i["index_bytes"] == 12
    assert np.array_equal(A.mult(np.arange(1.0, bs + 1)), np.full(bs, bs * (bs + 1) / 2))
    A.destroy()
    G, chunk = i["group_block_rows"], i["chunk_entries"]
    assert G >= 4 and G % 4 == 0 and (G // 4) * bs <= 64 and chunk >= bs * bs and chunk % (bs * bs) == 0      # a wave has at most 64 scalar rows; chunks are whole blocks
    return G, chunk


@functools.lru_cache(maxsize=None)
def case(kind, bs, G, chunk, groups=5):
    a = (bc.small if kind == "int" else bc.small_real)(bs, G, chunk, groups=groups)
    e = bc.expand(*a)
    for v in a + e:
        v.setflags(write=False)
    return a, e


@functools.lru_cache(maxsize=None)
def exact(bs, G, chunk, groups=5):
    _, e = case("int", bs, G, chunk, groups)
    x = lc.int_vector(len(e[0]) - 1, 3)
    y = lc.exact_product(*e, x)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


def blocked(ctx, monkeypatch, a, fmt=None, **kw):
    import slepc_amd as ks
    if fmt is None:
        monkeypatch.delenv("KSGPU_SPMV", raising=False)
    else:
        monkeypatch.setenv("KSGPU_SPMV", fmt)
    return ks.Mat.from_bsr(ctx, *a, **kw)


def scalar(ctx, monkeypatch, e, fmt="csr"):
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", fmt)
    return ks.Mat.from_csr(ctx, *e)


@gpu
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("bs", SIZES)
def test_bsr_small_layout_info_and_exact_product(ctx, monkeypatch, bs, groups):
    G, chunk = constants(ctx, bs)
    a, e = case("int", bs, G, chunk, groups)
    x, y = exact(bs, G, chunk, groups)
    A = blocked(ctx, monkeypatch, a)
    assert A.layout() == "bsr"
    assert A.bsr_info() == dict(bc.predict_info(a[0], a[2]), group_block_rows=G, chunk_entries=chunk)
    assert (A.n, A.N, A.nnz) == (len(e[0]) - 1, len(e[0]) - 1, int(e[0][-1]))
    assert A.spmv_bytes() == bc.layout_bytes(a[0], a[2]) + 16 * A.n
    got = A.mult(x)
    assert np.array_equal(got, y)
    empty = np.diff(e[0]) == 0
    assert empty.any() and not got[empty].any() and not np.signbit(got[empty]).any()
    A.destroy()


@gpu
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("bs", SIZES)
def test_bsr_small_vectors_offset_by_one_double(ctx, monkeypatch, bs, groups):
    """x and y that are 8-byte but not 16-byte aligned, n odd for the odd block sizes."""
    import slepc_amd as ks
    G, chunk = constants(ctx, bs)
    a, e = case("int", bs, G, chunk, groups)
    x, y = exact(bs, G, chunk, groups)
    n = len(x)
    A = blocked(ctx, monkeypatch, a)
    W = ks.BV(ctx, n + 2, 2)
    sx, s = (1 if W.column_ptr(c) % 16 == 0 else 0 for c in (0, 1))      # both vectors on addresses that are no multiple of 16
    xin = np.full(n + 2, 99.0); xin[sx:sx + n] = x
    W.set_column(0, xin)
    W.set_column(1, np.full(n + 2, -7.0))
    assert (W.column_ptr(0) + 8 * sx) % 16 == 8 and (W.column_ptr(1) + 8 * s) % 16 == 8
    A.mult_dev(W.column_ptr(0) + 8 * sx, W.column_ptr(1) + 8 * s)
    ctx.synchronize()
    out = W.column(1)
    assert np.array_equal(out[s:s + n], y) and np.all(out[:s] == -7.0) and np.all(out[s + n:] == -7.0)      # and nothing outside y was written
    A.destroy()


@gpu
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("bs", SIZES)
def test_bsr_small_diagonal_and_norm(ctx, monkeypatch, bs, groups):
    G, chunk = constants(ctx, bs)
    a, e = case("int", bs, G, chunk, groups)
    A = blocked(ctx, monkeypatch, a)
    assert np.array_equal(A.get_diagonal(), lc.exact_diagonal(*e))
    assert A.norm_inf() == lc.exact_norm_inf(*e)
    A.destroy()


@gpu
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("bs", SIZES)
def test_bsr_small_block_product(ctx, monkeypatch, bs, groups):
    """1, 3, 8 and 11 columns: exact, every column with the bits of the single-vector product, and filed under the block kernel's own variant."""
    G, chunk = constants(ctx, bs)
    a, e = case("int", bs, G, chunk, groups)
    n = len(e[0]) - 1
    A = blocked(ctx, monkeypatch, a)
    for k in (1, 3, 8, 11):
        X = lc.int_vector(n, 40 + k, cols=k)
        Y = A.mult_multi(X)
        assert np.array_equal(Y, lc.exact_product(*e, X)), k
        for j in range(k):
            assert np.array_equal(Y[:, j], A.mult(X[:, j])), (k, j)
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    try:
        A.mult(lc.int_vector(n, 5)); A.mult_multi(lc.int_vector(n, 7, cols=11))
        ctx.synchronize()
        prof = ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)
    assert (n < 2048) == (groups == 5)
    want = {("spmv_csr", 25): 12} if n < 2048 else {("spmv_csr", 25): 1, ("spmv_csr", 26): 2}      # small: the column loop; else 11 columns are a pass of 8 and one of 3
    assert {k: v["launches"] for k, v in prof.items()} == want
    A.destroy()


@gpu
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("bs", SIZES)
def test_bsr_real_bits_are_the_csr_kernels(ctx, monkeypatch, bs, groups):
    from oracle import oracle as O
    G, chunk = constants(ctx, bs)
    a, e = case("real", bs, G, chunk, groups)
    n = len(e[0]) - 1
    rng = np.random.default_rng(5)
    x, X = rng.standard_normal(n), rng.standard_normal((n, 5))
    A = blocked(ctx, monkeypatch, a)
    Ab = blocked(ctx, monkeypatch, a, "csr")
    Ac = scalar(ctx, monkeypatch, e)
    assert (A.layout(), Ab.layout(), Ac.layout()) == ("bsr", "csr", "csr") and Ab.bsr_info()["bs"] == 0
    y = A.mult(x)
    assert np.array_equal(y, Ab.mult(x)) and np.array_equal(y, Ac.mult(x))
    # the reference's own error: n_row entries of size |a||x| summed in double, each fma one rounding
    rows = np.repeat(np.arange(n), np.diff(e[0]))
    bound = np.zeros(n); np.add.at(bound, rows, np.abs(e[2] * x[e[1]]))
    assert np.all(np.abs(y - O.CSR(n, *e).mult(x)) <= 2.0 ** -52 * np.diff(e[0]).max() * bound + 1e-300)
    Y = A.mult_multi(X)
    assert np.array_equal(Y, Ac.mult_multi(X))
    for j in range(5):
        assert np.array_equal(Y[:, j], A.mult(X[:, j]))
    assert np.array_equal(A.get_diagonal(), Ac.get_diagonal()) and A.norm_inf() == Ac.norm_inf()
    for M in (A, Ab, Ac):
        M.destroy()


@gpu
@pytest.mark.parametrize("bs", [1, 9])
def test_bsr_other_block_sizes_go_through_the_chooser(ctx, monkeypatch, bs):
    import slepc_amd as ks
    a = bc.small_real(bs, 16, 4 * bs * bs)
    e = bc.expand(*a)
    x = np.random.default_rng(2).standard_normal(len(e[0]) - 1)
    A = blocked(ctx, monkeypatch, a)
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    Ac = ks.Mat.from_csr(ctx, *e)
    assert A.layout() == Ac.layout() != "bsr" and A.bsr_info() == dict.fromkeys(A.bsr_info(), 0)
    assert (A.n, A.nnz) == (Ac.n, Ac.nnz)
    assert np.array_equal(A.mult(x), Ac.mult(x))
    A.destroy(); Ac.destroy()


@gpu
def test_bsr_forced_sell_is_sell_of_the_expansion(ctx, monkeypatch):
    G, chunk = constants(ctx, 3)
    a, e = case("int", 3, G, chunk)
    x, y = exact(3, G, chunk)
    A = blocked(ctx, monkeypatch, a, "sell")
    Ac = scalar(ctx, monkeypatch, e, "sell")
    assert A.layout() == Ac.layout() == "sell"
    assert np.array_equal(A.mult(x), y) and np.array_equal(Ac.mult(x), y)
    A.destroy(); Ac.destroy()
    monkeypatch.setenv("KSGPU_SPMV", "bsr")                          # no new name: the chooser refuses it, for block input too
    with pytest.raises(Exception, match="KSGPU_SPMV=bsr"):
        blocked(ctx, monkeypatch, a, "bsr")


def _create(ctx, bs, n_local, row_start, n_global, brp, bcol, bval, flags=0):
    brp = np.asarray(brp, dtype=np.int32); bcol = np.asarray(bcol, dtype=np.int32); bval = np.asarray(bval, dtype=np.float64)
    h = C.c_void_p()
    rc = ctx.L.ks_mat_create_bsr(ctx.h, bs, n_local, row_start, n_global, brp.ctypes.data_as(IP), bcol.ctypes.data_as(IP), bval.ctypes.data_as(DP), flags, C.byref(h))
    msg = ctx.L.ks_last_error_message()
    if rc == 0:
        ctx.L.ks_mat_destroy(h)
    return rc, (msg.decode() if isinstance(msg, bytes) else str(msg))


@gpu
def test_bsr_errors(ctx, monkeypatch):
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    ones = np.ones(3 * 4)
    ok = ([0, 1, 2, 3], [2, 0, 1], ones)
    assert _create(ctx, 2, 6, 0, 6, *ok)[0] == 0
    for bs in (0, -3):
        assert _create(ctx, bs, 6, 0, 6, *ok)[0] == KS_ERR_ARG_OUTOFRANGE
    assert _create(ctx, 2, 5, 0, 6, *ok)[0] == KS_ERR_ARG_SIZ                # local rows
    assert _create(ctx, 2, 6, 0, 7, *ok)[0] == KS_ERR_ARG_SIZ                # global size
    assert _create(ctx, 2, 6, 1, 8, *ok)[0] == KS_ERR_ARG_SIZ                # first row
    rc, msg = _create(ctx, 2, 6, 0, 6, [0, 2, 1, 3], [2, 0, 7], ones)           # the pointer is reported, not the column behind it
    assert rc == KS_ERR_ARG_WRONG and "rowptr not monotone at block row 1" in msg
    rc, msg = _create(ctx, 2, 6, 0, 6, [0, 1, 2, 3], [2, 0, 3], ones)
    assert rc == KS_ERR_ARG_OUTOFRANGE and "block column 3 out of range at block row 2" in msg
    rc, msg = _create(ctx, 2, 6, 0, 6, [0, 1, 2, 3], [2, -1, 1], ones)
    assert rc == KS_ERR_ARG_OUTOFRANGE and "block column -1 out of range at block row 1" in msg
    assert _create(ctx, 2, 6, 0, 6, [1, 1, 2, 3], [2, 0, 1], ones)[0] == KS_ERR_ARG_WRONG
    assert _create(ctx, 8, 8, 0, 8, [0, 2 ** 25], [0], np.ones(64))[0] == KS_ERR_ARG_OUTOFRANGE      # 2^31 stored scalars: refused before a block is read
    assert _create(ctx, 2, 6, 0, 6, *ok, flags=4)[0] == KS_ERR_ARG_OUTOFRANGE                         # flags are those of ks_mat_create_csr_flags
    assert _create(ctx, 2, 6, 0, 6, *ok, flags=2)[0] == KS_ERR_ARG_INCOMP
