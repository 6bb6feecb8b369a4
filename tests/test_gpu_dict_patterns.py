"""The row-pattern form of the dictionary layout: a matrix with at most 256 distinct rows of (offset, value) codes keeps one byte per row and a
table of code words instead of 2 W bytes per row. Same decode, same entry order and fma chain, so every product has the bits of the 2-byte form
(built with the no_dict_patterns hook) and of the SELL-64 build: the single product, the block product, the product fused into the dot sweep
and a whole Krylov-Schur solve. The pattern count the library reports is the one numpy computes from the CSR arrays; a matrix with more than
256 distinct rows keeps its codes."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

gpu = pytest.mark.gpu

OFFS13 = [-300, -150, -6, -3, -2, -1, 0, 1, 2, 3, 6, 150, 300]            # the 13-entry banded matrix of test_gpu_sweep_variants.py (W = 16)
VALS13 = [-0.25, -1.0, -0.5, -0.25, -1.0, -1.0, 12.0, -1.0, -1.0, -0.25, -0.5, -1.0, -0.25]


def pattern_count(rowptr, col, val, lo=0, hi=None):
    """Distinct rows of the block of columns [lo, hi) (the diagonal block of a row slab that starts at global row lo), a row being the
    sequence of its (column - row, value bits) in storage order: what the dictionary layout encodes, padding being implied by the length."""
    rowptr = np.asarray(rowptr, dtype=np.int64); col = np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    hi = lo + n if hi is None else hi
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    bits = np.ascontiguousarray(val, dtype=np.float64).view(np.int64)
    keep = (col >= lo) & (col < hi)
    rows, off, bits = rows[keep], col[keep] - lo - rows[keep], bits[keep]
    lens = np.bincount(rows, minlength=n)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    slot = np.arange(rows.size) - start[rows]
    w = int(lens.max())
    key = np.full((n, 2 * w), np.iinfo(np.int64).min, dtype=np.int64)
    key[rows, 2 * slot] = off; key[rows, 2 * slot + 1] = bits
    return len(np.unique(key, axis=0))


def banded(n, offs, vals):
    rp = [0]; cols = []; vv = []
    for i in range(n):
        for o, v in zip(offs, vals):
            if 0 <= i + o < n:
                cols.append(i + o); vv.append(v)
        rp.append(len(cols))
    return np.array(rp, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vv, dtype=np.float64)


def stencil27(nx, ny, nz):
    """27-point stencil with constant coefficients (26 on the diagonal, -1 elsewhere), natural ordering, columns ascending: rows of up to 27."""
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")      # x fastest in the row number
    row = (i + nx * (j + ny * k)).ravel()
    rr, cc, vv = [], [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                ok = ((i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz)).ravel()
                rr.append(row[ok]); cc.append(row[ok] + di + nx * (dj + ny * dk))
                vv.append(np.full(ok.sum(), 26.0 if (di, dj, dk) == (0, 0, 0) else -1.0))
    rr, cc, vv = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    order = np.lexsort((cc, rr))
    n = nx * ny * nz
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=n))])
    return rowptr.astype(np.int32), cc[order].astype(np.int32), vv[order]


def cut_stencil(target, seed, n=8192):
    """The 13-entry banded matrix with entries cut from pseudo-random interior rows (seeded) until it has exactly `target` distinct rows."""
    rng = np.random.default_rng(seed)
    rp, col, val = banded(n, OFFS13, VALS13)
    full = tuple(zip(OFFS13, VALS13))
    seen = set()
    for i in range(n):
        seen.add(tuple((o, v) for o, v in full if 0 <= i + o < n))
    assert len(seen) <= target
    drop = np.zeros(col.size, bool)
    used = set()
    while len(seen) < target:
        i = int(rng.integers(400, n - 400))
        if i in used:
            continue
        mask = int(rng.integers(1, 1 << 12))                               # which of the 12 off-diagonal entries go
        offd = [e for e in range(13) if OFFS13[e] != 0]
        gone = {offd[b] for b in range(12) if mask >> b & 1}
        key = tuple(e for t, e in enumerate(full) if t not in gone)
        if key in seen:
            continue
        seen.add(key); used.add(i)
        for t in gone:
            drop[rp[i] + t] = True
    rows = np.repeat(np.arange(n), np.diff(rp))[~drop]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rowptr, col[~drop], val[~drop]


def _csr(o):
    return o.rowptr, o.col, o.val


# name -> (CSR arrays for numpy, maker of the device matrix, W)
CASES = {
    "laplacian2d": (lambda: _csr(O.laplacian2d(80, 60)), lambda ks, ctx: ks.Mat.laplacian2d(ctx, 80, 60), 8),
    "laplacian3d_cube": (lambda: _csr(O.laplacian3d(17, 17, 17)), lambda ks, ctx: ks.Mat.laplacian3d(ctx, 17, 17, 17), 8),
    "laplacian3d_box": (lambda: _csr(O.laplacian3d(23, 19, 11)), lambda ks, ctx: ks.Mat.laplacian3d(ctx, 23, 19, 11), 8),
    "banded13": (lambda: banded(20011, OFFS13, VALS13), None, 16),
    "stencil27": (lambda: stencil27(18, 17, 16), None, 32),
    "cut256": (lambda: cut_stencil(256, 7), None, 16),
}
OVER = {"cut257": lambda: cut_stencil(257, 8), "cut400": lambda: cut_stencil(400, 9)}
SLAB = (24, 20, 24)                        # two ranks, twelve planes each: the diagonal block of a slab lacks the neighbour's plane


def test_pattern_counts_on_the_cpu():
    """The numpy helper on every matrix of the list: the known counts of the Dirichlet stencils, at most 256 except where built to exceed."""
    counts = {name: pattern_count(*c[0]()) for name, c in CASES.items()}
    assert counts["laplacian2d"] == 9 and counts["laplacian3d_cube"] == 27 and counts["laplacian3d_box"] == 27 and counts["cut256"] == 256, counts
    assert all(v <= 256 for v in counts.values()), counts
    assert pattern_count(*_csr(O.laplacian3d(8, 8, 8))) == 27 and pattern_count(*_csr(O.laplacian3d(9, 7, 5))) == 27 and pattern_count(*_csr(O.laplacian2d(6, 6))) == 9
    assert pattern_count(*OVER["cut257"]()) == 257 and pattern_count(*OVER["cut400"]()) == 400
    nx, ny, nz = SLAB
    for z0 in (0, nz // 2):
        s = O.laplacian3d(nx, ny, nz, z0, nz // 2)
        assert pattern_count(s.rowptr, s.col, s.val, z0 * nx * ny) == 27


def _x_with_specials(n, seed):
    x = np.random.default_rng(seed).standard_normal(n)
    x[0] = np.nan; x[n - 1] = np.inf; x[n // 2] = -np.inf                  # the first and last rows have padding where the matrix ends
    return x


def _make(ks, ctx, name, arrays):
    maker = CASES[name][1] if name in CASES else None
    return maker(ks, ctx) if maker else ks.Mat.from_csr(ctx, *arrays)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pattern_form_same_bits_as_codes_and_sell(ctx, debug, monkeypatch, name):
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    arrays = CASES[name][0]()
    n = len(arrays[0]) - 1
    assert n >= 4096
    want = pattern_count(*arrays)
    x = _x_with_specials(n, 3)
    A = _make(ks, ctx, name, arrays)
    info = A.dict_info()
    assert A.layout() == "dict" and info["patterns"] and info["npatterns"] == want and info["w"] == CASES[name][2], (info, want)
    assert info["index_bytes"] < n + 256                     # one byte per row: the 2 W n bytes of codes are gone
    (yp, prof) = _profiled(ctx, lambda: A.mult(x))
    assert prof == {16: 1}, prof
    debug("no_dict_patterns")
    B = _make(ks, ctx, name, arrays)
    debug("no_dict_patterns", 0)
    ib = B.dict_info()
    assert B.layout() == "dict" and not ib["patterns"] and ib["npatterns"] == 0 and ib["index_bytes"] == 2 * ib["w"] * n and ib["w"] == info["w"], ib
    yc = B.mult(x)
    monkeypatch.setenv("KSGPU_SPMV", "sell")
    S = _make(ks, ctx, name, arrays)
    assert S.layout() == "sell" and S.dict_info() == {"patterns": False, "npatterns": 0, "w": 0, "index_bytes": 0}
    ys = S.mult(x)
    assert np.isnan(yp).any() and np.isinf(yp).any() and np.isfinite(yp).sum() > n - 100
    assert np.array_equal(yp, yc, equal_nan=True) and np.array_equal(yp, ys, equal_nan=True)
    xf = np.random.default_rng(4).standard_normal(n)
    yo = O.CSR(n, *arrays).mult(xf)
    assert np.allclose(A.mult(xf), yo, rtol=1e-13, atol=1e-12 * np.abs(yo).max())
    for M in (A, B, S):
        M.destroy()


def _profiled(ctx, fn):
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        out = fn()
        ctx.synchronize()
        p = ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)
    return out, {v: d["launches"] for (c, v), d in p.items() if c == "spmv_csr"}


@gpu
@pytest.mark.parametrize("name", list(OVER))
def test_more_than_256_distinct_rows_keep_the_codes(ctx, monkeypatch, name):
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    arrays = OVER[name]()
    n = len(arrays[0]) - 1
    A = ks.Mat.from_csr(ctx, *arrays)
    info = A.dict_info()
    assert A.layout() == "dict" and info == {"patterns": False, "npatterns": 0, "w": 16, "index_bytes": 32 * n}, info
    x = _x_with_specials(n, 5)
    y = A.mult(x)
    monkeypatch.setenv("KSGPU_SPMV", "sell")
    S = ks.Mat.from_csr(ctx, *arrays)
    assert S.layout() == "sell"
    assert np.array_equal(y, S.mult(x), equal_nan=True)


@gpu
@pytest.mark.parametrize("name", ["laplacian3d_box", "banded13", "stencil27"])
def test_block_product_both_forms(ctx, debug, monkeypatch, name):
    """ks_mat_mult_multi at 1, 3 and 8 columns, padded leading dimensions: one launch of the block kernel per pass, every column the bits of
    ks_mat_mult, in both storage forms."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    arrays = CASES[name][0]()
    n = len(arrays[0]) - 1
    ys = {}
    for form in ("patterns", "codes"):
        if form == "codes":
            debug("no_dict_patterns")
        A = _make(ks, ctx, name, arrays)
        assert A.dict_info()["patterns"] == (form == "patterns")
        for ncols in (1, 3, 8):
            X = np.random.default_rng(ncols).standard_normal((n, ncols))
            if ncols >= 3:
                X[0, 1] = np.nan; X[n - 1, 2] = np.inf
            ldx, ldy = n + 3, n + 5
            XB, YB = ks.BV(ctx, n, ncols, ld=ldx), ks.BV(ctx, n, ncols, ld=ldy)
            for j in range(ncols):
                XB.set_column(j, X[:, j])
            _, cnt = _profiled(ctx, lambda: A.mult_multi_dev(XB.column_ptr(0), ldx, YB.column_ptr(0), ldy, ncols))
            assert cnt == ({16: 1} if ncols == 1 else {20: 1}), (form, ncols, cnt)        # a single column is the single-vector product itself
            Y = np.stack([YB.column(j) for j in range(ncols)], axis=1)
            for j in range(ncols):
                assert np.array_equal(Y[:, j], A.mult(X[:, j]), equal_nan=True), (form, ncols, j)
            ys[(form, ncols)] = Y
            XB.destroy(); YB.destroy()
        A.destroy()
    for ncols in (1, 3, 8):
        assert np.array_equal(ys[("patterns", ncols)], ys[("codes", ncols)], equal_nan=True)


@gpu
@pytest.mark.parametrize("w", [8, 16])
def test_product_fused_into_the_dot_sweep_both_forms(ctx, debug, monkeypatch, w):
    """Lanczos on a small basis (the product rides in the dot sweep): coefficients and basis bit-equal with and without no_spmv_dot and between
    the two storage forms."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    n, m = 20011, 24
    arrays = banded(n, [-150, -1, 0, 1, 150], [-1.0, -1.0, 4.0, -1.0, -1.0]) if w == 8 else banded(n, OFFS13, VALS13)
    outs = {}
    for patterns in (True, False):
        for fused in (True, False):
            debug("no_dict_patterns", 0 if patterns else 1)
            debug("no_spmv_dot", 0 if fused else 1)
            A = ks.Mat.from_csr(ctx, *arrays)
            assert A.layout() == "dict" and A.dict_info()["patterns"] == patterns and A.dict_info()["w"] == w
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
            assert (nf >= 1) if fused else (nf == 0), (patterns, fused, nf)
            outs[(patterns, fused)] = (T.copy(), V.dense(), r)
            V.destroy(); A.destroy()
    ref = outs[(False, False)]
    assert ref[2][0] == m and not ref[2][2]
    for key, o in outs.items():
        assert np.array_equal(o[0], ref[0]) and np.array_equal(o[1], ref[1]) and o[2] == ref[2], key


@gpu
def test_krylov_schur_solve_identical_in_both_forms(ctx, debug, monkeypatch):
    """A Krylov-Schur solve of the 48^3 Laplacian of at least 60 Arnoldi steps: iteration, step and pass counts and every Ritz value of every
    restart identical between the two forms."""
    import slepc_amd as ks
    monkeypatch.delenv("KSGPU_SPMV", raising=False)
    res = {}
    for form in ("patterns", "codes"):
        if form == "codes":
            debug("no_dict_patterns")
        A = ks.Mat.laplacian3d(ctx, 48, 48, 48)
        assert A.dict_info()["patterns"] == (form == "patterns") and A.dict_info()["npatterns"] == (27 if form == "patterns" else 0)
        eps = ks.EPS(ctx)
        eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(10, 30); eps.SetTolerances(1e-8, 4)
        ritz = []
        eps.MonitorSet(lambda its, nconv, eigr, eigi, errest: ritz.append((its, nconv, eigr.copy(), errest.copy())))
        eps.Solve()
        st = eps.GetStats()
        assert st["arnoldi_steps"] >= 60, st
        res[form] = (eps.GetIterationNumber(), eps.GetConverged(), st, ritz)
        eps.destroy(); A.destroy()
    p, c = res["patterns"], res["codes"]
    assert p[0] == c[0] and p[1] == c[1] and p[2] == c[2], (p[:3], c[:3])
    assert len(p[3]) == len(c[3]) and len(p[3]) >= 1
    for a, b in zip(p[3], c[3]):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _slab_worker(rank, world, port, q):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.pop("KSGPU_SPMV", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import slepc_amd as ks
        from slepc_amd import gloo_provider
        from slepc_amd import partition as P
        ctx = ks.Context(0)
        gloo_provider.install(ctx, dist, torch, rank, world)
        nx, ny, nz = SLAB
        plane = nx * ny
        z0, z1 = P.split_ownership(nz, world)[rank]
        xg = _x_with_specials(nx * ny * nz, 6)
        xg[z0 * plane] = np.nan; xg[z1 * plane - 1] = np.inf              # rows whose far neighbour lies outside the slab's diagonal block
        out = {}
        ys = {}
        for form in ("patterns", "codes", "sell"):
            ctx.set_debug("no_dict_patterns", 1 if form == "codes" else 0)
            if form == "sell":
                os.environ["KSGPU_SPMV"] = "sell"
            A = ks.Mat.laplacian3d(ctx, nx, ny, nz, z0, z1 - z0)
            out[form] = dict(A.dict_info(), layout=A.layout())
            B = ks.BV(ctx, A.n, 2, N=nx * ny * nz)
            B.set_column(0, xg[z0 * plane:z1 * plane])
            A.mult_dev(B.column_ptr(0), B.column_ptr(1))
            ys[form] = B.column(1)
            dist.barrier()
        s = O.laplacian3d(nx, ny, nz, z0, z1 - z0)
        out["want"] = pattern_count(s.rowptr, s.col, s.val, z0 * plane)
        out["n"] = (z1 - z0) * plane
        out["equal"] = bool(np.array_equal(ys["patterns"], ys["codes"], equal_nan=True) and np.array_equal(ys["patterns"], ys["sell"], equal_nan=True))
        out["nonfinite"] = int((~np.isfinite(ys["patterns"])).sum())
        q.put((rank, out))
        dist.barrier()
    except Exception as e:              # noqa: BLE001
        import traceback
        q.put((rank, {"error": "%s\n%s" % (e, traceback.format_exc())}))
    finally:
        dist.destroy_process_group()


@gpu
def test_z_slab_with_a_halo_two_ranks():
    """Two z-slabs of a 3-D grid on one GPU: the diagonal block of each takes the pattern form (its boundary planes are patterns of their own),
    the halo rows are added as before, and y has the bits of the 2-byte form and of SELL-64."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_slab_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(_collect(q, procs, 2))
    for r in range(2):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["n"] >= 4096 and o["equal"] and 0 < o["nonfinite"] < 64, o
        assert o["patterns"]["layout"] == "dict" and o["patterns"]["patterns"] and o["patterns"]["npatterns"] == o["want"] == 27, o
        assert o["codes"]["layout"] == "dict" and not o["codes"]["patterns"] and o["codes"]["index_bytes"] == 16 * o["n"], o
        assert o["sell"]["layout"] == "sell", o
