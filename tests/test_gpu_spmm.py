"""Y = A X for a block of columns (ks_mat_mult_multi: MatMatMult with a dense column-major block) and BVMatMult's MAT method
(ks_bv_set_matmult_method). Every column is bit for bit the single-vector product A.mult(X(:,j)) on every device layout; the block
kernels (profiling variants 20-24 of the spmv_csr class) really run where they apply - one launch per pass of up to 8 columns - and
the column loop where they do not; the BV-level products give the same bits under both methods; argument checks, no host wait; two
ranks sharing one GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

NCOLS = [0, 1, 3, 7, 8, 9, 17, 32]
BLOCK_VARIANTS = {20, 21, 22, 23, 24}          # k_spmm_dict, k_spmm_odict, k_spmm_sell, k_spmm_csr direct / interleaved
SINGLE_VARIANTS = {0, 8, 16, 17, 18}           # CSR, SELL-64, dictionary, offset dictionary, binned


def _stencil27(N, const):
    import scipy.sparse as sp
    tri = lambda n: sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])       # noqa: E731
    P = sp.kron(tri(N), sp.kron(tri(N), tri(N))).tocsr(); P.sort_indices()
    n = P.shape[0]
    if const:
        val = np.full(P.nnz, -1.0); val[P.indices == np.repeat(np.arange(n), np.diff(P.indptr))] = 26.0
    else:
        val = np.random.default_rng(3).standard_normal(P.nnz)
    return O.CSR(n, P.indptr.astype(np.int32), P.indices.astype(np.int32), val)


def _ragged():
    """The matrix of test_spmv_csr_row_block_kernel: empty rows, rows of 1500 and 2600 entries, a run of rows of 32."""
    rng = np.random.default_rng(21)
    n = 5000
    lens = rng.integers(0, 40, n); lens[::9] = 0; lens[7] = 1500; lens[2048] = 2600; lens[100:164] = 32; lens[n - 1] = 64
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens] + [np.empty(0, int)]).astype(np.int32)
    return O.CSR(n, rowptr, col, rng.uniform(-1, 1, rowptr[-1]))


MATRICES = {
    "laplacian": lambda: O.laplacian3d(40, 30, 20),
    "stencil27": lambda: _stencil27(20, True),
    "stencil27_random": lambda: _stencil27(16, False),
    "ragged": _ragged,
    "small": lambda: O.laplacian3d(12, 10, 9),         # n = 1080 < 2048
}


def _block_product(ctx, A, X, pad=3):
    """ks_mat_mult_multi on a block with leading dimension n + pad and garbage in the padding rows of X and Y; returns
    (Y (n x ncols), the whole Y block as it came back, the block as it went in)."""
    import slepc_amd as ks
    n, ncols = X.shape
    ld, m = n + pad, max(ncols, 1)
    XB, YB = ks.BV(ctx, n, m + 1, ld=ld), ks.BV(ctx, n, m + 1, ld=ld)
    rng = np.random.default_rng(ncols + 17)
    xf = rng.uniform(-1e6, 1e6, (m + 1) * ld)
    for j in range(ncols):
        xf[j * ld:j * ld + n] = X[:, j]
    yf = rng.uniform(-1e6, 1e6, (m + 1) * ld)
    ctx.memcpy_h2d(XB.column_ptr(0), xf); ctx.memcpy_h2d(YB.column_ptr(0), yf)
    A.mult_multi_dev(XB.column_ptr(0), ld, YB.column_ptr(0), ld, ncols)
    out = np.empty_like(yf)
    ctx.memcpy_d2h(out, YB.column_ptr(0))
    Y = np.stack([out[j * ld:j * ld + n] for j in range(ncols)], axis=1) if ncols else np.zeros((n, 0))
    return Y, out, yf, ld


def _check_block(ctx, A, Ao, ncols, rng):
    n = A.n
    X = rng.standard_normal((n, ncols))
    if ncols >= 3:
        X[5, 1] = np.nan; X[n // 2, 2] = np.inf; X[7, 2] = -np.inf
    Y, out, yf, ld = _block_product(ctx, A, X)
    for j in range(ncols):
        assert np.array_equal(Y[:, j], A.mult(X[:, j]), equal_nan=True), "column %d of %d differs from the single-vector product" % (j, ncols)
        yo = Ao.mult(X[:, j])
        fin = np.isfinite(yo)
        assert np.allclose(Y[fin, j], yo[fin], rtol=1e-13, atol=1e-12 * max(1.0, np.abs(yo[fin]).max(initial=0.0))), j
    written = np.zeros(out.size, bool)
    for j in range(ncols):
        written[j * ld:j * ld + n] = True
    assert np.array_equal(out[~written], yf[~written]), "the padding rows or the columns beyond ncols of Y were written"


@pytest.mark.parametrize("layout", [None, "csr", "csrregs", "sell", "dict", "odict", "csrvec", "binned", "sliced"])
def test_block_product_every_layout_bit_for_bit(ctx, monkeypatch, layout):
    import slepc_amd as ks
    if layout is None:
        monkeypatch.delenv("KSGPU_SPMV", raising=False)
    else:
        monkeypatch.setenv("KSGPU_SPMV", layout)
    rng = np.random.default_rng(5)
    for name, make in MATRICES.items():
        Ao = make()
        A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
        for ncols in NCOLS:
            _check_block(ctx, A, Ao, ncols, rng)
        A.destroy()


def test_block_product_shell_matrix(ctx):
    import slepc_amd as ks
    Ao = O.laplacian3d(20, 16, 10)
    inner = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    A = ks.Mat.shell(ctx, Ao.n, lambda x, y: inner.mult_dev(x, y))
    assert A.layout() == "shell"
    rng = np.random.default_rng(6)
    for ncols in NCOLS:
        _check_block(ctx, A, Ao, ncols, rng)


def _launches(ctx, A, ncols):
    n = A.n
    X = np.random.default_rng(ncols).standard_normal((n, ncols))
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        Y, _, _, _ = _block_product(ctx, A, X)
        p = ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)
    cnt = {v: d["launches"] for (c, v), d in p.items() if c == "spmv_csr"}
    return Y, X, cnt


@pytest.mark.parametrize("layout,shape,variant", [
    ("dict", (128, 128, 128), 20), ("odict", (40, 30, 20), 21), ("sell", (40, 30, 20), 22), ("csr", (40, 30, 20), 23), ("csrregs", (40, 30, 20), 23)])
def test_block_kernels_run_one_launch_per_pass(ctx, monkeypatch, layout, shape, variant):
    """ceil(ncols / 8) launches of the block variant and none of the single-vector ones; the dictionary case at 128^3 runs the grid and the
    XCD remap at scale."""
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", layout)
    A = ks.Mat.laplacian3d(ctx, *shape)
    assert A.layout() == {"dict": "dict", "odict": "odict", "sell": "sell"}.get(layout, "csr")
    for ncols in ([9] if A.n > 10 ** 6 else [2, 8, 9, 17]):
        Y, X, cnt = _launches(ctx, A, ncols)
        assert cnt.get(variant, 0) == -(-ncols // 8), (ncols, cnt)
        assert not any(cnt.get(v, 0) for v in SINGLE_VARIANTS), (ncols, cnt)
        for j in (0, ncols - 1):
            assert np.array_equal(Y[:, j], A.mult(X[:, j]))


def test_csr_block_product_both_gather_forms(ctx, monkeypatch):
    """The interleaved form (n x KB row-major copy of the pass's columns, k_spmm_pack) is the automatic choice above 12 entries per row;
    KSGPU_SPMM forces either form; both give the single-vector bits."""
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", "csr")
    Ao = _ragged()
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    assert A.layout() == "csr" and A.nnz > 12 * A.n
    for form, variant in ((None, 24), ("direct", 23), ("interleaved", 24)):
        if form is None:
            monkeypatch.delenv("KSGPU_SPMM", raising=False)
        else:
            monkeypatch.setenv("KSGPU_SPMM", form)
        Y, X, cnt = _launches(ctx, A, 11)
        assert cnt.get(variant, 0) == 2 and not any(cnt.get(v, 0) for v in SINGLE_VARIANTS), (form, cnt)
        for j in range(11):
            assert np.array_equal(Y[:, j], A.mult(X[:, j]))


@pytest.mark.parametrize("layout,shape", [("binned", (32, 32, 32)), ("sliced", (32, 32, 32)), ("csrvec", (40, 30, 20)), ("csr", (12, 10, 9))])
def test_fallback_layouts_run_the_column_loop(ctx, monkeypatch, layout, shape):
    """BINNED, SLICED, the CSR-vector form and CSR below 2048 rows: ncols single-vector launches, none of the block variants."""
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", layout)
    A = ks.Mat.laplacian3d(ctx, *shape)
    assert A.layout() == {"csrvec": "csr"}.get(layout, layout)
    ncols = 9
    Y, X, cnt = _launches(ctx, A, ncols)
    assert not any(cnt.get(v, 0) for v in BLOCK_VARIANTS), cnt
    assert sum(cnt.values()) == ncols, cnt
    for j in range(ncols):
        assert np.array_equal(Y[:, j], A.mult(X[:, j]))


def _bv_pair(ctx, n, seed):
    import slepc_amd as ks
    V = ks.BV(ctx, n, 14, ld=n + 3)
    V.SetNumConstraints(2)
    V.SetActiveColumns(0, V.m); V.SetRandom(seed)
    V.SetActiveColumns(2, 11)
    W = ks.BV(ctx, n, 12, ld=n + 5)
    W.SetActiveColumns(1, 10)
    return V, W


def test_bv_matmult_methods_same_bits(ctx, monkeypatch):
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    A = ks.Mat.laplacian3d(ctx, 20, 20, 12)
    assert A.layout() == "dict"
    V, W = _bv_pair(ctx, A.n, 11)
    assert V.GetMatMultMethod() == ks.BV_MATMULT_VECS          # the default stays VECS
    res = {}
    for method in ("vecs", "mat"):
        V.SetMatMultMethod(method)
        W.SetActiveColumns(0, W.m); W.SetRandom(99); W.SetActiveColumns(1, 10)
        ctx.prof_enable(True); ctx.prof_reset()
        V.MatMult(A, W)
        ctx.synchronize()
        cnt = {v: d["launches"] for (c, v), d in ctx.prof_get(by_variant=True).items() if c == "spmv_csr"}
        ctx.prof_enable(False)
        res[method] = (W.dense(), cnt)
    assert np.array_equal(res["vecs"][0], res["mat"][0])
    assert res["vecs"][1] == {16: 9} and res["mat"][1] == {20: 2}, (res["vecs"][1], res["mat"][1])
    Vd = V.dense()
    for j in range(9):
        assert np.array_equal(res["mat"][0][:, 1 + j], A.mult(Vd[:, 2 + j]))


def test_bv_matproject_and_b_inner_dot_methods_same_bits(ctx, monkeypatch):
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    A = ks.Mat.laplacian3d(ctx, 20, 20, 12)
    X, Y = _bv_pair(ctx, A.n, 12)
    Y.SetActiveColumns(0, Y.m); Y.SetRandom(5); Y.SetActiveColumns(2, 9)
    out = {}
    for method in ("vecs", "mat"):
        X.SetMatMultMethod(method)
        M = np.zeros((Y.k, X.k), order="F")
        X.MatProject(A, Y, M)
        X.SetMatrix(A)
        D = np.zeros((Y.k, X.k), order="F")
        X.Dot(Y, D)
        X.SetMatrix(None)
        out[method] = (M, D)
    assert np.array_equal(out["vecs"][0], out["mat"][0]) and np.abs(out["mat"][0]).max() > 0
    assert np.array_equal(out["vecs"][1], out["mat"][1]) and np.abs(out["mat"][1]).max() > 0


def test_bv_matmult_method_values_and_duplicate(ctx):
    import slepc_amd as ks
    V = ks.BV(ctx, 100, 4)
    assert V.GetMatMultMethod() == ks.BV_MATMULT_VECS
    V.SetMatMultMethod("mat_save")
    assert V.GetMatMultMethod() == ks.BV_MATMULT_MAT               # MAT_SAVE is stored as MAT
    for bad in (3, -1):
        with pytest.raises(ks.KsError) as e:
            V.SetMatMultMethod(bad)
        assert e.value.rc == 63
    assert V.GetMatMultMethod() == ks.BV_MATMULT_MAT
    h = C.c_void_p()
    ks._lib.check(ctx.L.ks_bv_duplicate(V.h, C.byref(h)))
    try:
        m = C.c_int()
        ks._lib.check(ctx.L.ks_bv_get_matmult_method(h, C.byref(m)))
        assert m.value == ks.BV_MATMULT_MAT
    finally:
        ctx.L.ks_bv_destroy(h)
    V.SetMatMultMethod("vecs")
    assert V.GetMatMultMethod() == ks.BV_MATMULT_VECS


def test_block_product_argument_errors_and_no_host_wait(ctx, monkeypatch):
    import slepc_amd as ks
    monkeypatch.setenv("KSGPU_SPMV", "csr")
    Ao = _ragged()
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    n = A.n
    B = ks.BV(ctx, n, 6)
    B.SetRandom(1)
    p0, p3, ld = B.column_ptr(0), B.column_ptr(3), B.ld

    def rc(*args):
        with pytest.raises(ks.KsError) as e:
            A.mult_multi_dev(*args)
        return e.value.rc
    assert rc(p0, ld, B.column_ptr(1), ld, 2) == 62                 # Y's first column is X's second
    assert rc(p0, ld, p0, ld, 1) == 62
    assert rc(p0, n - 1, p3, ld, 2) == 60 and rc(p0, ld, p3, n - 1, 2) == 60
    assert rc(p0, ld, p3, ld, -1) == 63
    assert rc(0, ld, p3, ld, 2) == 85 and rc(p0, ld, 0, ld, 2) == 85
    A.mult_multi_dev(p0, ld, p3, ld, 0)                              # nothing to do
    ctx.synchronize()
    s0 = ctx.sync_count()
    for form in ("direct", "interleaved"):                           # the first interleaved pass allocates the matrix's scratch
        monkeypatch.setenv("KSGPU_SPMM", form)
        A.mult_multi_dev(p0, ld, p3, ld, 3)
    assert ctx.sync_count() == s0
    ctx.synchronize()
    Bd = B.dense()
    for j in range(3):
        assert np.array_equal(Bd[:, 3 + j], A.mult(Bd[:, j]))
    with pytest.raises(ks.KsError) as e:
        ks._lib.check(ctx.L.ks_mat_mult_multi(None, 1, C.c_void_p(p0), ld, C.c_void_p(p3), ld))
    assert e.value.rc == 85


def test_mult_multi_host_convenience(ctx):
    import slepc_amd as ks
    Ao = O.laplacian3d(16, 16, 16)
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    X = np.random.default_rng(2).standard_normal((A.n, 10))
    Y = A.mult_multi(X)
    assert Y.shape == (A.n, 10)
    for j in range(10):
        assert np.array_equal(Y[:, j], A.mult(X[:, j]))
    assert A.mult_multi(np.zeros((A.n, 0))).shape == (A.n, 0)


def _spmm_worker(rank, world, port, q):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import slepc_amd as ks
        from slepc_amd import gloo_provider
        from slepc_amd import partition as P
        ctx = ks.Context(0)
        gloo_provider.install(ctx, dist, torch, rank, world)
        nx, ny, nz = 40, 30, 8
        plane = nx * ny
        z0, z1 = P.split_ownership(nz, world)[rank]
        A = ks.Mat.laplacian3d(ctx, nx, ny, nz, z0, z1 - z0)
        n = A.n
        Xg = np.random.default_rng(4).standard_normal((nx * ny * nz, 9))
        X = Xg[z0 * plane:z1 * plane]
        XB, YB, ZB = (ks.BV(ctx, n, 9, N=nx * ny * nz) for _ in range(3))
        XB.set_dense(X)
        A.mult_multi_dev(XB.column_ptr(0), XB.ld, YB.column_ptr(0), YB.ld, 9)
        for j in range(9):
            A.mult_dev(XB.column_ptr(j), ZB.column_ptr(j))
        Y, Z = YB.dense(), ZB.dense()
        ref = np.stack([O.laplacian3d(nx, ny, nz).mult(Xg[:, j]) for j in range(9)], axis=1)[z0 * plane:z1 * plane]
        q.put((rank, {"layout": A.layout(), "equal": bool(np.array_equal(Y, Z)), "err": float(np.abs(Y - ref).max())}))
        dist.barrier()
    except Exception as e:              # noqa: BLE001
        import traceback
        q.put((rank, {"error": "%s\n%s" % (e, traceback.format_exc())}))
    finally:
        dist.destroy_process_group()


def test_block_product_two_ranks_sharing_one_gpu():
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_spmm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(_collect(q, procs, 2))
    for r in range(2):
        assert "error" not in out[r], out[r].get("error")
        assert out[r]["equal"], out[r]
        assert out[r]["err"] < 1e-12, out[r]
