"""The pair form of the dictionary product (ks_dict_pairs.h: two rows per lane, 16-byte loads of x, the neighbours' halves by a lane shift) against the
one-row form of the same matrix (test hook no_dict_pairs, read at launch) and against the SELL-64 build: y bit for bit, in MatMult and inside the
fused dot sweep, next to NaN-filled neighbours of x, and the one-row kernel for vectors that are not 16-byte aligned."""
import numpy as np
import pytest

from oracle import oracle as O

gpu = pytest.mark.gpu


def _stencil27(nx, ny, nz):
    """The 27-point generator of test_spmv_dictionary_layouts_27_point_stencil (constant coefficients)."""
    import scipy.sparse as sp

    def tri(n):
        return sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])
    P = sp.kron(tri(nz), sp.kron(tri(ny), tri(nx))).tocsr(); P.sort_indices()
    data = np.full(P.nnz, -1.0); data[P.indices == np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))] = 26.0
    return P.indptr, P.indices, data


def _banded(n, offs, vals):
    rp = [0]; cols = []; vv = []
    for i in range(n):
        for o, v in zip(offs, vals):
            if 0 <= i + o < n:
                cols.append(i + o); vv.append(v)
        rp.append(len(cols))
    return np.array(rp, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vv, dtype=np.float64)


CASES = {
    "lap3d-6": ("3d", (6, 6, 6), 5), "lap3d-8": ("3d", (8, 8, 8), 5), "lap3d-40": ("3d", (40, 40, 40), 5), "lap3d-4x6x10": ("3d", (4, 6, 10), 5),
    "lap2d-10": ("2d", (10,), 3), "lap2d-300": ("2d", (300,), 3), "27pt-18x14x12": ("27", (18, 14, 12), 9),
    "banded-odd-n": ("band", (1001,), 3),            # odd n: the last row on its own, and pairs of x whose second half lies behind x
    "banded-w16-odd-n": ("band16", (777,), 5),       # the same with W = 16 and W = 32: the last row decodes its code word with the table's real stride
    "banded-w32-odd-n": ("band32", (1001,), 6),
}
OFFS16 = [-8, -5, -4, -3, -1, 0, 1, 3, 4, 5, 8]
OFFS32 = [-9, -8, -7, -5, -4, -3, -1, 0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13]


def _make(ks, ctx, kind, dims):
    if kind == "3d":
        return ks.Mat.laplacian3d(ctx, *dims)
    if kind == "2d":
        return ks.Mat.laplacian2d(ctx, *dims)
    if kind == "band":
        return ks.Mat.from_csr(ctx, *_banded(dims[0], [-4, -1, 0, 1, 4], [-0.5, -1.0, 5.0, -2.0, -0.25]))
    if kind in ("band16", "band32"):
        offs = OFFS16 if kind == "band16" else OFFS32
        return ks.Mat.from_csr(ctx, *_banded(dims[0], offs, [26.0 if o == 0 else -1.0 - 0.125 * (o & 3) for o in offs]))
    return ks.Mat.from_csr(ctx, *_stencil27(*dims))


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_pair_form_has_the_bits_of_the_row_form_and_of_sell(ctx, debug, monkeypatch, case):
    import slepc_amd as ks
    kind, dims, nbases = CASES[case]
    A = _make(ks, ctx, kind, dims)
    info = A.dict_pairs_info()
    assert A.layout() == "dict" and A.dict_info()["patterns"] and info["eligible"] and info["nbases"] == nbases, (A.layout(), A.dict_info(), info)
    assert A.dict_info()["w"] == {"band16": 16, "band32": 32, "27": 32}.get(kind, 8)
    x = np.random.default_rng(14).standard_normal(A.n)
    y_pairs = A.mult(x)
    assert A.dict_pairs_info()["pair_launches"] == 1 and A.dict_pairs_info()["row_launches"] == 0
    debug("no_dict_pairs")
    y_rows = A.mult(x)                                            # the same matrix, the one-row kernel
    assert A.dict_pairs_info()["pair_launches"] == 1 and A.dict_pairs_info()["row_launches"] == 1
    debug("no_dict_pairs", 0)
    monkeypatch.setenv("KSGPU_SPMV", "sell")
    S = _make(ks, ctx, kind, dims)
    monkeypatch.delenv("KSGPU_SPMV")
    assert S.layout() in ("sell", "csr")
    y_sell = S.mult(x)
    assert np.array_equal(y_pairs, y_rows) and np.array_equal(y_pairs, y_sell)
    assert np.all(np.isfinite(y_pairs)) and np.abs(y_pairs).max() > 0.0


@gpu
def test_ineligible_matrices_keep_the_row_form(ctx):
    import slepc_amd as ks
    A = ks.Mat.laplacian2d(ctx, 301)                              # odd stride
    assert A.layout() == "dict" and not A.dict_pairs_info()["eligible"]
    x = np.random.default_rng(3).standard_normal(A.n)
    assert np.abs(A.mult(x) - O.laplacian2d(301).mult(x)).max() < 1e-12
    assert A.dict_pairs_info() == {"eligible": False, "nbases": 0, "pair_launches": 0, "row_launches": 1}


@gpu
@pytest.mark.parametrize("j", [1, 0])
def test_pair_form_next_to_nan_columns(ctx, debug, j):
    """x is column j of a BV whose neighbouring columns are NaN: a load in front of x or behind it would bring one in."""
    import slepc_amd as ks
    A = ks.Mat.laplacian3d(ctx, 8, 8, 8)
    assert A.dict_pairs_info()["eligible"]
    X = ks.BV(ctx, A.n, 3); Y = ks.BV(ctx, A.n, 1)
    x = np.random.default_rng(5).standard_normal(A.n)
    for c in range(3):
        X.set_column(c, x if c == j else np.full(A.n, np.nan))
    A.mult_dev(X.column_ptr(j), Y.column_ptr(0)); ctx.synchronize()
    y_pairs = Y.column(0)
    assert A.dict_pairs_info()["pair_launches"] == 1
    debug("no_dict_pairs")
    A.mult_dev(X.column_ptr(j), Y.column_ptr(0)); ctx.synchronize()
    y_rows = Y.column(0)
    assert np.all(np.isfinite(y_pairs)) and np.array_equal(y_pairs, y_rows)
    assert np.array_equal(y_pairs, A.mult(x))


@gpu
def test_unaligned_vectors_take_the_row_kernel(ctx):
    import slepc_amd as ks
    A = ks.Mat.laplacian3d(ctx, 8, 8, 8)
    X = ks.BV(ctx, A.n + 2, 1); Y = ks.BV(ctx, A.n + 2, 1)
    x = np.random.default_rng(6).standard_normal(A.n)
    X.set_column(0, np.concatenate([[np.nan], x, [np.nan]]))
    px, py = X.column_ptr(0), Y.column_ptr(0)
    assert px % 16 == 0 and py % 16 == 0
    A.mult_dev(px + 8, py); ctx.synchronize()                      # x 8 but not 16 bytes aligned
    assert A.dict_pairs_info()["pair_launches"] == 0 and A.dict_pairs_info()["row_launches"] == 1
    y1 = Y.column(0)[:A.n]
    A.mult_dev(px + 8, py + 8); ctx.synchronize()                  # y as well
    assert A.dict_pairs_info()["pair_launches"] == 0 and A.dict_pairs_info()["row_launches"] == 2
    y2 = Y.column(0)[1:A.n + 1]
    ref = A.mult(x)
    assert A.dict_pairs_info()["pair_launches"] == 1
    assert np.array_equal(y1, ref) and np.array_equal(y2, ref)


@gpu
@pytest.mark.parametrize("shape", [("3d", 40), ("2d", 300)])
def test_lanczos_through_the_fused_sweep_keeps_its_bits(ctx, debug, shape):
    """MatLanczos with the product inside the dot sweep (k_dot_spmv_dict), with and without the pair form: T and the basis bit for bit."""
    import slepc_amd as ks
    kind, N = shape
    m = 14
    outs = []
    for pairs in (True, False):
        if not pairs:
            debug("no_dict_pairs")
        A = ks.Mat.laplacian3d(ctx, N, N, N) if kind == "3d" else ks.Mat.laplacian2d(ctx, N)
        assert A.dict_pairs_info()["eligible"]
        V = ks.BV(ctx, A.n, m + 1)
        V.SetRandomColumn(0)
        _, nrm, _ = V.OrthogonalizeColumn(0); V.ScaleColumn(0, 1.0 / nrm)
        T = np.zeros((m + 1, 3), order="F")
        ctx.prof_enable(True); ctx.prof_reset()
        r = V.MatLanczos(A, T, 0, m)
        ctx.synchronize()
        p = ctx.prof_get(); ctx.prof_enable(False)
        assert p.get("spmv_dot_fused", {}).get("launches", 0) == m                       # the fused sweep ran every product
        info = A.dict_pairs_info()
        assert (info["pair_launches"], info["row_launches"]) == ((m, 0) if pairs else (0, m)), info
        outs.append((T.copy(), V.dense(), r))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
