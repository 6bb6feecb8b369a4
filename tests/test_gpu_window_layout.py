"""The windowed CSR layout (KS_MAT_LAYOUT_WINDOW): its plan (ks_csr.cpp: csr_window_plan), its builder and chooser rules (ks_mat.hip) and its kernel
(ks_spmv.hip: k_spmv_window), on every path the kernel has: window blocks with full and partial segments, the largest window, direct blocks, blocks
without entries, a partial last block; and around the product: diagonal, norm, block product, profile variant, row-sharded matrices with halos.

Integer data is compared with the exact integer reference by np.array_equal; real data bit for bit with the CSR kernel (KSGPU_SPMV=csr) of the same
arrays, and with the oracle to rounding. Everything the library reports about the layout is compared with window_cases.predict_window, which calls
nothing. The matrices are built once and never written to."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import layout_cases as lc
import window_cases as wc

gpu = pytest.mark.gpu

# what the tests below were written against; the library reports its own through window_info(), and the GPU tests use those
DEFAULT_BLOCK_ROWS, DEFAULT_MAX_SEGMENTS = 256, 64


@functools.lru_cache(maxsize=None)
def case(kind, *args):
    if kind == "small":
        a = wc.forced_small(*args)[:3]
    elif kind == "limit":
        a = wc.segment_limit(*args)
    elif kind == "scattered":
        a = wc.scattered(*args)
    elif kind == "mesh":
        a = wc.mesh27(*args)[:3]
    elif kind == "cover":
        a = wc.coverage_rule(*args)
    elif kind == "banded":
        a = wc.banded_random(*args)
    else:
        raise KeyError(kind)
    for x in a:
        x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def exact(kind, *args):
    a = case(kind, *args)
    x = lc.int_vector(len(a[0]) - 1, 3)
    y = lc.exact_product(*a, x)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


def constants(ctx):
    """(block_rows, max_segments) of the library: returned for any matrix."""
    import slepc_amd as ks
    A = ks.Mat.laplacian2d(ctx, 8)
    w = A.window_info()
    A.destroy()
    assert w["blocks"] == w["direct_blocks"] == w["window_entries"] == w["index_bytes"] == 0
    assert w["block_rows"] in (64, 256) and w["max_segments"] >= 64
    return w["block_rows"], w["max_segments"]


def forced(ctx, monkeypatch, a, fmt="window"):
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", fmt)
    return ks.Mat.from_csr(ctx, *a)


def automatic(ctx, monkeypatch, a):
    """No KSGPU_SPMV: the chooser's own pick."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    return ks.Mat.from_csr(ctx, *a)


def assert_plan(A, a, R, S, force="window"):
    p = wc.predict_window(a[0], a[1], R, S, val=a[2], force=force)
    assert A.layout() == p["layout"], (A.layout(), p["layout"])
    assert A.window_info() == (wc.info_of(p, R, S) if p["layout"] == "window" else wc.info_of_none(R, S))
    return p


# ---- the cases stand where the tests need them, the predictor and the host plan agree (no GPU) ------------------------------------------------
def test_window_case_generators_deliver_their_properties():
    R, S = DEFAULT_BLOCK_ROWS, DEFAULT_MAX_SEGMENTS
    rp, col, val, where = wc.forced_small(R)
    n, lens = len(rp) - 1, np.diff(rp)
    rows = np.repeat(np.arange(n), lens)
    assert n == 5 * R + 37 and n % 64 and n % R
    assert lens.max() == 1500 and lens[where["long"]] == 1500 and lens[where["one"]] == 1 and np.all(lens[where["run"]:where["run"] + 64] == 32)
    assert np.all(lens[::9][np.arange(0, n, 9) < where["run"]] == 0) and set(np.delete(lens, where["long"]).tolist()) >= set(range(33))
    short = rows != where["long"]
    assert np.abs(col[short] - rows[short]).max() <= 300
    assert len(np.unique(col[~short] >> 6)) == where["span"] == min(24, (n + 63) // 64)
    unsorted = dup = 0
    for r in range(n):
        c = col[rp[r]:rp[r + 1]]
        unsorted += bool(np.any(np.diff(c) < 0)); dup += len(np.unique(c)) < len(c)
    assert unsorted > 100 and dup > 100
    assert np.abs(val).max() <= 255 and np.array_equal(val, np.rint(val)) and np.all(val != 0)
    p = wc.predict_window(rp, col, R, S, force="window")
    assert p["blocks"] == 6 and p["direct_blocks"] == 0 and p["window_entries"] == rp[-1] and p["layout"] == "window"

    a = case("limit", R, S)
    n = len(a[0]) - 1
    p = wc.predict_window(a[0], a[1], R, S, force="window")
    assert n == 64 * (S + 2) + 5 and a[0][4 * R] == a[0][-1]                              # 4 block_rows rows carry the entries
    assert p["nseg"][:4].tolist()[:2] == [S, S + 1] and p["direct"].tolist()[:4] == [False, True, False, False] and p["direct_blocks"] == 1
    assert not p["nseg"][4:].any() and p["codes"].max() >= (S - 1) * 64                   # the last slot of the largest window is used
    b3 = slice(a[0][3 * R], a[0][4 * R])
    assert (a[1][b3] >> 6).max() == (n - 1) >> 6 and a[1].max() == n - 1                   # block 3 references the last, partial segment up to its last column

    a = case("scattered", 32 * R + 37)
    p = wc.predict_window(a[0], a[1], R, S, force="window")
    assert p["direct"].all() and p["window_entries"] == 0 and p["total_segments"] == 0 and p["layout"] == "window"


def test_the_mesh_and_mixed_matrices_are_what_the_tests_take_them_for():
    rp, col, val = a = case("mesh", 28)
    n = len(rp) - 1
    assert n == 65856 and 52.5 < rp[-1] / n < 53.5
    assert lc.predict_layout(*a) == ("csr", 0)                                             # ragged: no dictionary form, SELL-64 declines the padding
    p = wc.predict_window(rp, col, DEFAULT_BLOCK_ROWS, DEFAULT_MAX_SEGMENTS, force="window")
    assert p["nseg"].max() <= 24 and p["direct_blocks"] == 0                               # stripe-local: every block fits a window
    nb = 65536 // DEFAULT_BLOCK_ROWS
    rp, col, val = a = case("cover", DEFAULT_BLOCK_ROWS, nb // 8, 17, nb)
    p = wc.predict_window(rp, col, DEFAULT_BLOCK_ROWS, DEFAULT_MAX_SEGMENTS, force="window")
    assert len(rp) - 1 == 65536 and rp[-1] == 17 * 65536 and lc.predict_layout(*a) == ("csr", 0)
    assert p["direct_blocks"] == nb // 8 and 8 * p["window_entries"] == 7 * rp[-1]


@pytest.mark.parametrize("R,S", [(256, 64), (64, 64), (256, 32)])
def test_host_plan_matches_the_predictor(R, S):
    """csr_window_plan (ks_csr.cpp, host only) against predict_window on the forced and the segment-limit cases: segments per block, direct blocks,
    codes entry by entry, the concatenated segment lists, the direct column array and its aligned block starts."""
    import slepc_amd._lib as L
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    IP, LP, HP = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_ushort)
    lib.ksc_window_plan.argtypes = [C.c_int, IP, IP, C.c_int, C.c_int, IP, IP, HP, IP, C.c_longlong, LP]
    lib.ksc_window_plan.restype = C.c_longlong
    for a in (wc.forced_small(R)[:3], wc.segment_limit(R, S)):
        rp, col = np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.int32)
        n, nnz = len(rp) - 1, int(rp[-1])
        p = wc.predict_window(rp, col, R, S, force="window")
        nseg = np.zeros(p["blocks"], np.int32); dbase = np.zeros(p["blocks"], np.int32); codes = np.zeros(nnz, np.uint16)
        seg = np.zeros(max(p["total_segments"], 1), np.int32); tot = np.zeros(6, np.int64)
        got = lib.ksc_window_plan(n, rp.ctypes.data_as(IP), col.ctypes.data_as(IP), R, S, nseg.ctypes.data_as(IP), dbase.ctypes.data_as(IP),
                                  codes.ctypes.data_as(HP), seg.ctypes.data_as(IP), len(seg), tot.ctypes.data_as(LP))
        assert got == p["total_segments"]
        assert tot[:5].tolist() == [p["blocks"], p["direct_blocks"], p["window_entries"], p["direct_entries"], p["total_segments"]]
        assert np.array_equal(nseg, p["nseg"]) and np.array_equal(dbase != -2 ** 31, p["direct"]) and np.array_equal(codes, p["codes"])
        want = [np.unique(col[rp[b * R]:rp[min(n, (b + 1) * R)]] >> 6) for b in range(p["blocks"]) if not p["direct"][b]]
        assert np.array_equal(seg[:got], np.concatenate(want + [np.empty(0, np.int64)]))
        for b in np.flatnonzero(p["direct"]):
            assert dbase[b] % 4 == 0 and dbase[b] + rp[b * R] >= 0 and dbase[b] + rp[min(n, (b + 1) * R)] <= tot[5]


# ---- 2: forced, small, every path ---------------------------------------------------------------------------------------------------------------
@gpu
def test_window_forced_small_exact(ctx, monkeypatch):
    """Every path of a window block: empty rows, a row of 1, a row of 1500 over many segments (six chunks of 256), a run of rows of 32 (one LDS bank),
    duplicate and unsorted columns, a partial last block and a partial last segment."""
    R, S = constants(ctx)
    a = case("small", R)
    x, y = exact("small", R)
    A = forced(ctx, monkeypatch, a)
    p = assert_plan(A, a, R, S)
    assert p["layout"] == "window" and p["direct_blocks"] == 0
    got = A.mult(x)
    assert np.array_equal(got, y)
    empty = np.diff(a[0]) == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any()
    A.destroy()


# ---- 3, 4: the segment limit, direct blocks ---------------------------------------------------------------------------------------------------------
@gpu
def test_window_segment_limit_exact(ctx, monkeypatch):
    R, S = constants(ctx)
    a = case("limit", R, S)
    x, y = exact("limit", R, S)
    A = forced(ctx, monkeypatch, a)
    p = assert_plan(A, a, R, S)
    assert p["direct_blocks"] == 1 and p["direct"][1] and p["nseg"][0] == S
    assert np.array_equal(A.mult(x), y)
    A.destroy()


@gpu
def test_window_all_direct_exact(ctx, monkeypatch):
    R, S = constants(ctx)
    a = case("scattered", 32 * R + 37)
    x, y = exact("scattered", 32 * R + 37)
    A = forced(ctx, monkeypatch, a)
    p = assert_plan(A, a, R, S)
    assert p["direct_blocks"] == p["blocks"] == 33 and p["window_entries"] == 0
    assert np.array_equal(A.mult(x), y)
    A.destroy()


# ---- 5: bits ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_window_bits_are_the_csr_kernels(ctx, monkeypatch):
    """Real values on the mesh matrix: bit for bit the CSR kernel's y, the oracle's to rounding; NaN and infinities in x reach exactly the rows that
    reference them, with the bits the CSR kernel gives them, and no other row of their segments."""
    from oracle import oracle as O
    rp, col, val = a = case("mesh", 28)
    n = len(rp) - 1
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n)
    Aw, Ac = forced(ctx, monkeypatch, a), forced(ctx, monkeypatch, a, "csr")
    assert Aw.layout() == "window" and Ac.layout() == "csr"
    yw, yc = Aw.mult(x), Ac.mult(x)
    assert np.array_equal(yw, yc)
    assert np.allclose(yw, O.CSR(n, rp, col, val).mult(x), rtol=0, atol=1e-12)
    xs = x.copy()
    bad = [1000, 31007, n - 2]
    xs[bad] = [np.nan, np.inf, -np.inf]
    rows = np.repeat(np.arange(n), np.diff(rp))
    hit = np.zeros(n, bool); hit[rows[np.isin(col, bad)]] = True
    near = np.zeros(n, bool); near[rows[np.isin(col >> 6, np.asarray(bad) >> 6)]] = True
    assert hit.any() and (near & ~hit).any()                                               # rows that share a poisoned segment without referencing the position
    yw, yc = Aw.mult(xs), Ac.mult(xs)
    assert np.array_equal(yw, yc, equal_nan=True)
    assert np.isfinite(yw[~hit]).all() and not np.isfinite(yw[hit]).all()
    Aw.destroy(); Ac.destroy()


# ---- 6: the automatic choice never takes the layout ---------------------------------------------------------------------------------------------
@gpu
def test_window_is_never_the_automatic_choice(ctx, monkeypatch):
    """The layout is built only when forced (its product has not been timed against the CSR kernel's): the mesh matrix, a matrix of window and
    direct blocks at 65536 rows and csr_probe's banded random matrix keep what layout_cases.predict_layout says."""
    R, S = constants(ctx)
    for a in (case("mesh", 28), case("cover", R, 65536 // R // 8, 17, 65536 // R), case("banded", 131072, 32)):
        A = automatic(ctx, monkeypatch, a)
        assert A.layout() == lc.predict_layout(*a)[0] == "csr" and A.window_info() == wc.info_of_none(R, S)
        A.destroy()


@gpu
def test_window_mixed_blocks_exact(ctx, monkeypatch):
    """Window blocks and direct blocks side by side, 65536 rows (256 workgroups: the XCD remap of the grid), exact."""
    R, S = constants(ctx)
    nb = 65536 // R
    a = case("cover", R, nb // 8, 17, nb)
    x, y = exact("cover", R, nb // 8, 17, nb)
    A = forced(ctx, monkeypatch, a)
    p = assert_plan(A, a, R, S)
    assert p["direct_blocks"] == nb // 8
    assert np.array_equal(A.mult(x), y)
    A.destroy()


# ---- 7: around the product ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_window_diagonal_norm_block_product_and_profile(ctx, monkeypatch):
    R, S = constants(ctx)
    a = case("small", R)
    n = len(a[0]) - 1
    A = forced(ctx, monkeypatch, a)
    assert A.layout() == "window"
    assert np.array_equal(A.get_diagonal(), lc.exact_diagonal(*a))
    assert A.norm_inf() == lc.exact_norm_inf(*a)
    for k in (3, 9):
        X = lc.int_vector(n, 40 + k, cols=k)
        Y = A.mult_multi(X)
        assert np.array_equal(Y, lc.exact_product(*a, X))
        for j in range(k):
            assert np.array_equal(Y[:, j], A.mult(X[:, j]))
    x, _ = exact("small", R)
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    try:
        A.mult(x); A.mult_multi(lc.int_vector(n, 7, cols=3))
        ctx.synchronize()
        prof = ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)
    assert {k: v["launches"] for k, v in prof.items()} == {("spmv_csr", 19): 4}
    A.destroy()


@gpu
@pytest.mark.timeout(300)
def test_window_sharded_with_halos(monkeypatch):
    """Four row blocks with ghosts on both sides, every diagonal block forced to the windowed layout: the exact product, diagonal and norm."""
    from test_gpu_sharded_product import case as scase, vectors, _layout_rank, _threads, _assert_exact
    monkeypatch.setenv("KSGPU_SPMV", "window")
    c = scase("layouts-int")
    xs, ys = vectors("layouts-int")
    out = _threads(4, _layout_rank(c, xs))
    for rank in range(4):
        r0, r1 = c.range(rank)
        assert out[rank]["layout"] == "window", (rank, out[rank]["layout"])
        for j in range(2):
            _assert_exact(out[rank]["y"][j], ys[j][r0:r1], "layouts-int as window, rank %d" % rank)
        assert np.array_equal(out[rank]["diag"], c.diagonal()[r0:r1])
