"""The forward form of the final Gram-Schmidt update (k_gs_update_fwd): the launch that stores column j + 1 of an enqueued Krylov
run also forms y = A v_{j+1} into column j + 2 and the first dots of the next step, tile by tile, with a flag hand-off between workgroups.

Every case runs the same Lanczos expansion twice on the same start vector - with the form on (test hooks: eligibility forced for a small basis, a
forced grid of G workgroups) and with KS_DEBUG_NO_STEP_FORWARD - and compares. With its own grid the launch leaves the bits of the three launches it
replaces and the whole run is compared bit for bit, for an even n and for an odd one (test_unforced_grid_leaves_the_bits_of_the_three_launches). With
a FORCED grid of at least as many workgroups as the problem has tiles, every workgroup of the launch and of the dot sweep it replaces holds one tile
at most, the sums have the dot sweep's order, and again the whole run - T, beta and every column of the basis, hence every y, every stored column
and every partial sum that went into them - must be bit for bit the run of k_spmv_dict and k_dot_sweep: the one-tile problems, n around a tile
edge, an odd n of many tiles (the last row on its own), far neighbours across tile borders. With a forced grid of FEWER workgroups than tiles the
stored columns and y keep their bits and the next step's dots are the same products summed in the order of that grid, so: column 1 (stored by the
first forward launch from identical inputs) is compared bit for bit; T is
held to the 1e-12 of the existing Lanczos tests (test_gpu_krylov.py), pass counts, step counts and breakdown flags must be identical, the basis
orthonormal, and the three-term relation A V - V T = beta v e^T must hold to 1e-12 with the products of the library's stand-alone kernel (Mat.mult,
k_spmv_dict: not the forward launch's walk; a tile of y formed from stale rows of the column, which held the previous product a moment before,
breaks it at O(1)). The whole storage of the basis is NaN bytes before the start vector is
written: rows n..ld-1 must still be NaN bytes afterwards, and a read past the guard shows in the results. The counters say that the form really ran
(or, for the refusals and the columns that leave the two-pass program, that the ordinary launches did)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12           # |T - T'| and the Lanczos relation: the tolerance of test_lanczos_matches_oracle
M = 14                # steps of a run (12 - 20)


def _banded(n, offs, vals):
    c = np.arange(n)[:, None] + np.asarray(offs)[None, :]
    ok = (c >= 0) & (c < n)
    rp = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return rp.astype(np.int32), c[ok].astype(np.int32), np.broadcast_to(np.asarray(vals, dtype=np.float64), c.shape)[ok].copy()


def _stencil27(nx, ny, nz):
    """27-point stencil with constant coefficients: nine bases, all wide."""
    import scipy.sparse as sp

    def tri(n):
        return sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])
    P = sp.kron(tri(nz), sp.kron(tri(ny), tri(nx))).tocsr(); P.sort_indices()
    data = np.full(P.nnz, -1.0); data[P.indices == np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))] = 26.0
    return P.indptr, P.indices, data


def _band5(ks, ctx, n):
    """Symmetric band with offsets -4, -1, 0, 1, 4: three bases, the centre one wide; any n, odd ones included (the last row on its own)."""
    return ks.Mat.from_csr(ctx, *_banded(n, [-4, -1, 0, 1, 4], [-0.5, -1.0, 5.0, -1.0, -0.5]))


def _lap2d(ks, ctx):
    """2-D 5-point stencil on 300 x 301 points in the orientation whose stride is even (the pair form needs an even offset next to every offset)."""
    for dims in ((300, 301), (301, 300)):
        A = ks.Mat.laplacian2d(ctx, *dims)
        if A.dict_pairs_info()["eligible"]:
            return A
    raise AssertionError("neither orientation of the 300 x 301 stencil has the pair form")


# name -> (matrix, forced grid). 3-D 64 x 64 x 20: n = 81 920 = 160 tiles, far offset 4096 rows = 8 tiles; grid 40: four rounds, neighbours in the
# round before, the same and the next one; grid 12: 8 + 2 <= 12, the bound itself. band5: one-tile problems and n around a tile edge; 6144 = 3 rounds
# of 4 workgroups x 512 rows exactly. The shapes whose grid holds every tile at once (one round): the whole run is compared bit for bit - 160 tiles with
# far neighbours 8 tiles away, 177 tiles of the 2-D stencil, 196 tiles of an odd n.
SHAPES = {
    "lap3d-64x64x20-g160": (lambda ks, ctx: ks.Mat.laplacian3d(ctx, 64, 64, 20), 160),
    "lap2d-300x301-g177": (_lap2d, 177),
    "band5-100003-g196": (lambda ks, ctx: _band5(ks, ctx, 100003), 196),
    "lap3d-64x64x20-g40": (lambda ks, ctx: ks.Mat.laplacian3d(ctx, 64, 64, 20), 40),
    "lap3d-64x64x20-g12": (lambda ks, ctx: ks.Mat.laplacian3d(ctx, 64, 64, 20), 12),
    "lap2d-300x301-g16": (_lap2d, 16),
    "band5-511-g4": (lambda ks, ctx: _band5(ks, ctx, 511), 4),
    "band5-512-g4": (lambda ks, ctx: _band5(ks, ctx, 512), 4),
    "band5-513-g4": (lambda ks, ctx: _band5(ks, ctx, 513), 4),
    "band5-100-g3": (lambda ks, ctx: _band5(ks, ctx, 100), 3),
    "band5-6144-g4": (lambda ks, ctx: _band5(ks, ctx, 6144), 4),
    "band5-100003-g24": (lambda ks, ctx: _band5(ks, ctx, 100003), 24),
}


def _nan_bytes(ctx, V, n):
    """True iff rows n..ld-1 of every column still hold the 0xFF bytes the storage was filled with."""
    if V.ld == n:
        return True
    raw = np.empty(V.m * V.ld)
    ctx.memcpy_d2h(raw, V.column_ptr(0)); ctx.synchronize()
    tail = raw.reshape(V.m, V.ld)[:, n:].view(np.uint64)
    return bool(np.all(tail == np.uint64(0xFFFFFFFFFFFFFFFF)))


def _run(ks, ctx, debug, A, v0, m, forward, grid=0, **hooks):
    n = A.n
    V = ks.BV(ctx, n, m + 1, ld=n + 2 if n % 2 == 0 else n + 1)
    ctx.memset(V.column_ptr(0), 0xFF, V.m * V.ld * 8); ctx.synchronize()
    V.set_column(0, v0)
    debug("no_step_forward", 0 if forward else 1)              # the conftest fixture puts the key back after the test
    V.step_forward_hooks(force=True, grid=grid, **hooks)
    T = np.zeros((m + 1, 3), order="F")
    mm, beta, brk = V.MatLanczos(A, T, 0, m)
    st = V.step_forward_stats()
    cols = np.stack([V.column(j) for j in range(mm + 1)], axis=1)
    return {"T": T, "mm": mm, "beta": beta, "brk": brk, "V": cols, "passes": V.gs_passes()[0], "last_passes": V.gs_passes()[1], "stats": st, "guard": _nan_bytes(ctx, V, n)}


def _start_vector(n, seed=5):
    v = np.random.default_rng(seed).standard_normal(n)
    return v / np.linalg.norm(v)


_CACHE = {}


def _pair(ks, ctx, debug, name):
    """(matrix, start vector, the run with the form off, the run with it on) of a shape: computed once, shared by the tests, never modified."""
    if name not in _CACHE:
        make, grid = SHAPES[name]
        A = make(ks, ctx)
        v0 = _start_vector(A.n)
        off = _run(ks, ctx, debug, A, v0, M, False)
        on = _run(ks, ctx, debug, A, v0, M, True, grid=grid)
        _CACHE[name] = (A, v0, off, on)
    return _CACHE[name]


def _same_run(a, b, m):
    assert (a["mm"], a["brk"]) == (b["mm"], b["brk"]) == (m, False)
    assert a["passes"] == b["passes"]
    assert np.abs(a["T"] - b["T"]).max() < TOL and abs(a["beta"] - b["beta"]) < TOL
    assert a["guard"] and b["guard"]
    assert np.isfinite(a["V"]).all() and np.isfinite(b["V"]).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_run_equals_the_ordinary_run(ctx, debug, name):
    import slepc_amd as ks
    A, v0, off, on = _pair(ks, ctx, debug, name)
    info = A.dict_pairs_info()
    assert A.layout() == "dict" and info["eligible"] and info["nbases"] <= 5, (A.layout(), info)
    # the form ran: every step but the last enqueues it (the last column's update waits for nobody's product), the device took it for every column
    # in the plain two-pass state and none gave up; a column that was final after one pass leaves its product to the ordinary launch
    so, sn = off["stats"], on["stats"]
    assert so["enqueued"] == 0 and so["taken"] == 0 and so["refused"].startswith("switched off")
    assert sn["enqueued"] == M - 1 and sn["refused"] == ""
    assert sn["taken"] >= M - 3 and sn["completed"] == sn["taken"] and sn["aborted"] == 0
    assert sn["fell_back"] == sn["enqueued"] - sn["taken"]
    _same_run(off, on, M)
    # column 1 is stored by the first launches from identical inputs: the same bits whichever form stored it
    assert np.array_equal(off["V"][:, 0], on["V"][:, 0]) and np.array_equal(off["V"][:, 1], on["V"][:, 1])
    ntiles = (A.n + 511) // 512
    print(name, "tiles", ntiles, "grid", SHAPES[name][1], "columns equal bit for bit", [bool(np.array_equal(off["V"][:, j], on["V"][:, j])) for j in range(M + 1)],
          "max |dT|", np.abs(off["T"] - on["T"]).max())
    if ntiles <= SHAPES[name][1]:
        # one tile per workgroup at most, in this launch and in the dot sweep it replaces: the sums have that sweep's order, so y, the stored column and
        # the partial sums of every step are the bits of k_spmv_dict and k_dot_sweep - T is made of those sums, every column of those y and of T
        assert ntiles <= ctx.device_info()["num_cu"]
        assert on["beta"] == off["beta"] and np.array_equal(on["T"], off["T"])
        assert np.array_equal(on["V"].view(np.uint64), off["V"].view(np.uint64))      # the bytes: a zero of the other sign is a difference
    Vd = on["V"]
    assert np.abs(Vd.T @ Vd - np.eye(M + 1)).max() < 1e-13
    # the Lanczos relation with an independent product: y of every step was formed from the NEW rows of the column
    T = on["T"]
    Tm = np.diag(T[:M, 0]) + np.diag(T[: M - 1, 1], 1) + np.diag(T[: M - 1, 1], -1)
    AV = np.stack([A.mult(Vd[:, j]) for j in range(M)], axis=1)
    R = AV - Vd[:, :M] @ Tm
    R[:, M - 1] -= on["beta"] * Vd[:, M]
    assert np.abs(R).max() < TOL


@pytest.mark.parametrize("name", ["lap3d-64x64x20-g40", "lap3d-64x64x20-g12", "band5-100003-g24", "band5-513-g4"])
def test_uneven_load_changes_nothing(ctx, debug, name):
    """Odd workgroups sleep before they publish every tile (a consumer that polls early, a producer that is late): the same bits as the even run -
    the order of every sum is fixed by the grid, not by timing - and no wait gives up."""
    import slepc_amd as ks
    A, v0, off, on = _pair(ks, ctx, debug, name)
    lag = _run(ks, ctx, debug, A, v0, M, True, grid=SHAPES[name][1], lag_odd=True)
    assert lag["stats"]["aborted"] == 0 and lag["stats"]["completed"] == on["stats"]["completed"] > 0
    assert np.array_equal(lag["T"], on["T"]) and np.array_equal(lag["V"], on["V"]) and lag["passes"] == on["passes"] and lag["guard"]


@pytest.mark.parametrize("hook", [{"budget": 0}, {"abort_wg": 1}], ids=["budget-0", "workgroup-1-gives-up"])
@pytest.mark.parametrize("name", ["lap3d-64x64x20-g40", "band5-513-g4", "band5-100003-g24"])
def test_a_wait_that_gives_up_costs_a_fallback(ctx, debug, name, hook):
    """The abort path: the kernel returns, every column is still stored, the ordinary product and dot sweep behind the launch redo y and the
    partials, and the results stay within the bounds of the ordinary run."""
    import slepc_amd as ks
    A, v0, off, on = _pair(ks, ctx, debug, name)
    ab = _run(ks, ctx, debug, A, v0, M, True, grid=SHAPES[name][1], **hook)
    st = ab["stats"]
    assert st["enqueued"] == M - 1 and st["taken"] == on["stats"]["taken"]
    assert st["aborted"] == st["taken"] > 0 and st["completed"] == 0 and st["fell_back"] == st["enqueued"]
    _same_run(off, ab, M)
    assert np.abs(ab["V"].T @ ab["V"] - np.eye(M + 1)).max() < 1e-13


def test_a_column_final_after_one_pass_keeps_the_ordinary_launches(ctx, debug):
    """A column whose first pass takes less than half of its squared norm is final after ONE pass (the refinement criterion): its slot 2 has no update
    to run, the forward launch enqueued there stores nothing and forms no product, and the ordinary product and dot sweep behind it run. The band
    with a diagonal of 1/16 has such columns at the start of a run from a random vector (A v is nearly orthogonal to v). No column of the run takes a
    third pass, so the pass count says how many there are: 2 M minus the total, less the run's last column, which has no forward launch. Exactly
    those fall back, the others take the form, and the run is the ordinary one."""
    import slepc_amd as ks
    n = 100003
    A = ks.Mat.from_csr(ctx, *_banded(n, [-4, -1, 0, 1, 4], [-0.5, -1.0, 0.0625, -1.0, -0.5]))
    v0 = _start_vector(n, 7)
    off = _run(ks, ctx, debug, A, v0, M, False)
    on = _run(ks, ctx, debug, A, v0, M, True, grid=24)
    _same_run(off, on, M)
    assert on["passes"] <= 2 * M and on["last_passes"] == off["last_passes"] and on["last_passes"] in (1, 2)
    one_pass = 2 * M - on["passes"] - (1 if on["last_passes"] == 1 else 0)
    st = on["stats"]
    print("passes", on["passes"], "last", on["last_passes"], st)
    assert 1 <= one_pass < M - 1
    assert st["enqueued"] == M - 1 and st["fell_back"] == one_pass and st["taken"] == st["completed"] == st["enqueued"] - one_pass and st["aborted"] == 0
    assert np.abs(on["V"].T @ on["V"] - np.eye(M + 1)).max() < 1e-13


def test_columns_that_leave_the_two_pass_program(ctx, debug):
    """A start vector inside an invariant subspace of dimension 3 (breakdown at column 3), and the same with a leak of 1e-20 into every other
    direction (column 3 is what rounding leaves: it needs the third pass and the host's completion program in the middle of the run). The slot
    that would have been the forward one runs the update kernel's generic form or nothing; the ordinary product and dot sweep run; steps,
    passes and flags are those of the run with the form off."""
    import slepc_amd as ks
    nx, ny, nz = 64, 64, 20
    A = ks.Mat.laplacian3d(ctx, nx, ny, nz)
    x, y, z = np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1)

    def mode(a, b, c):
        return np.einsum("k,j,i->kji", np.sin(np.pi * c * z / (nz + 1)), np.sin(np.pi * b * y / (ny + 1)), np.sin(np.pi * a * x / (nx + 1))).ravel()
    base = 1.0 * mode(1, 1, 1) / np.linalg.norm(mode(1, 1, 1)) + 2.0 * mode(3, 2, 1) / np.linalg.norm(mode(3, 2, 1)) - mode(2, 5, 4) / np.linalg.norm(mode(2, 5, 4))
    for leak in (0.0, 1e-20):
        v0 = base + leak
        v0 = v0 / np.linalg.norm(v0)
        off = _run(ks, ctx, debug, A, v0, 10, False)
        on = _run(ks, ctx, debug, A, v0, 10, True, grid=40)
        assert (on["mm"], on["brk"]) == (off["mm"], off["brk"]) and on["passes"] == off["passes"]
        assert on["guard"] and np.isfinite(on["V"]).all()
        st = on["stats"]
        assert st["enqueued"] >= 2 and st["aborted"] == 0
        assert st["taken"] < st["enqueued"] and st["fell_back"] == st["enqueued"] - st["taken"] >= 1      # the ordinary launches ran, and the counters say so
        assert np.abs(on["T"][:2] - off["T"][:2]).max() < TOL
        mm = on["mm"]
        assert np.abs(on["V"][:, :mm].T @ on["V"][:, :mm] - np.eye(mm)).max() < 1e-10


UNFORCED = {
    "lap3d-128x128x40": lambda ks, ctx: ks.Mat.laplacian3d(ctx, 128, 128, 40),
    "band5-655361": lambda ks, ctx: _band5(ks, ctx, 655361),
}


@pytest.mark.parametrize("hooks", [{}, {"lag_odd": True}, {"budget": 0}], ids=["even-load", "odd-workgroups-lag", "every-wait-gives-up"])
@pytest.mark.parametrize("key", list(UNFORCED))
def test_unforced_grid_leaves_the_bits_of_the_three_launches(ctx, debug, key, hooks):
    """With its own grid (one workgroup per CU) the forward launch keeps one set of accumulators per workgroup of the dot sweep it replaces and runs in
    that sweep's direction: y, the stored column AND the partial sums are the bits the three launches leave, so the whole run - every column of the
    basis, T, beta - is bit for bit the run with the form off. 128 x 128 x 40 points: 1280 tiles, enough for the dot sweep's full grid at every column
    count of the run (four, three and two workgroups per CU), far neighbours 32 tiles away. The band of 655 361 rows: 1281 tiles, the last of them the
    single last row of an odd n, which the launch forms, stores and adds on its own (fwd_last_row) in its sixth round. The same after every launch gave
    up: the fallbacks are the ordinary launches."""
    import slepc_amd as ks
    if key not in _CACHE:
        A = UNFORCED[key](ks, ctx)
        v0 = _start_vector(A.n)
        _CACHE[key] = (A, v0, _run(ks, ctx, debug, A, v0, M, False))
    A, v0, off = _CACHE[key]
    assert A.n >= 4 * 512 * ctx.device_info()["num_cu"]
    on = _run(ks, ctx, debug, A, v0, M, True, grid=0, **hooks)
    st = on["stats"]
    assert st["enqueued"] == M - 1 and st["taken"] >= M - 3
    if hooks.get("budget") == 0:
        assert st["aborted"] == st["taken"] and st["fell_back"] == st["enqueued"]
    else:
        assert st["aborted"] == 0 and st["completed"] == st["taken"]
    assert (on["mm"], on["brk"], on["passes"]) == (off["mm"], off["brk"], off["passes"])
    assert on["guard"] and off["guard"]
    assert on["beta"] == off["beta"] and np.array_equal(on["T"], off["T"])
    assert np.array_equal(on["V"].view(np.uint64), off["V"].view(np.uint64))


def _refused(ks, ctx, A, m=6, grid=40, ld=None, B=None, bvctx=None):
    c = bvctx or ctx
    V = ks.BV(c, A.n, m + 1, ld=ld if ld else (A.n + 2 if A.n % 2 == 0 else A.n + 1))
    if B is not None:
        V.SetMatrix(B)
    V.set_column(0, _start_vector(A.n, 9))
    if B is not None:
        _, nrm, _ = V.OrthogonalizeColumn(0); V.ScaleColumn(0, 1.0 / nrm)
    V.step_forward_hooks(force=True, grid=grid)
    T = np.zeros((m + 1, 3), order="F")
    mm, beta, brk = V.MatLanczos(A, T, 0, m)
    assert mm == m and not brk
    st = V.step_forward_stats()
    assert st["enqueued"] == 0 and st["taken"] == 0 and st["fell_back"] == 0, st
    return st["refused"]


def test_refusals(ctx):
    """What the host must not hand to the forward form takes the ordinary launches: a grid that would put the far neighbours more than one round
    away, a far offset beyond the grid, a B-inner product, an odd leading dimension, a matrix with nine bases."""
    import slepc_amd as ks
    A = ks.Mat.laplacian3d(ctx, 64, 64, 20)
    assert "one round away" in _refused(ks, ctx, A, grid=8)                      # 8 tiles + 2 > 8
    assert "one round away" in _refused(ks, ctx, ks.Mat.laplacian3d(ctx, 128, 128, 6), grid=12)      # far offset 16384 rows = 32 tiles
    assert "leading dimension" in _refused(ks, ctx, A, ld=A.n + 1)
    B = _band5(ks, ctx, A.n)
    assert "B-inner" in _refused(ks, ctx, A, B=B)
    A27 = ks.Mat.from_csr(ctx, *_stencil27(18, 14, 12))
    assert A27.dict_pairs_info()["nbases"] == 9
    assert "five bases" in _refused(ks, ctx, A27)
    # without the hooks a small basis is refused by its size alone
    V = ks.BV(ctx, A.n, 8)
    V.set_column(0, _start_vector(A.n, 9))
    T = np.zeros((8, 3), order="F")
    V.MatLanczos(A, T, 0, 6)
    st = V.step_forward_stats()
    assert st["enqueued"] == 0 and ("16 tiles" in st["refused"] or "resident" in st["refused"])


def test_refused_on_the_collective_path(ctx):
    """force_multi: the multi-rank path on one rank (the reductions go through the communicator) keeps the ordinary launches."""
    import slepc_amd as ks
    c2 = ks.Context(0)
    try:
        c2.set_debug("force_multi")
        c2.init_rccl(0, 1, ks.Context.get_unique_id())
        A = ks.Mat.laplacian3d(c2, 64, 64, 20)
        assert "one rank" in _refused(ks, c2, A, bvctx=c2)
    finally:
        c2.close()
