"""The oblique projection of the Jacobi-Davidson correction equation (ks_bv_oblique_project, slepc_amd/csrc/ks_jd.hip: k_oblique_dot, k_oblique_reduce,
k_oblique_update) and the Ritz-residual sweep that also stores its vectors (ks_bv_ritz_residual_vectors, ks_gd.hip).

Exact test. Integer-valued data: |u|, |v| <= 2, |a|, |b| <= 2, |s| <= 2, so |w0| = |s (a u + b v)| <= 2 (4 + 4) = 2^4; Z in {-1, 0, 1}: |h| <= n 2^4 <= 4099 2^4
< 2^17; Minv in {-1, 0, 1} with at most 4 entries per row: |c| < 2^19; Y in {-1, 0, 1} with at most 2 entries per row: |w| <= 2^4 + 2 2^19 < 2^20.01; |e| <= 2:
|e^T w| < 4099 2^21.01 < 2^34; e == w: w^2 < 2^40.02 and the sum over 4099 rows < 2^52.03. Every product and every sum, partial sums in any order
included, stays below 2^53 and is exact in double; the test also checks that on the data itself with sums of absolute values. w must equal numpy's bit
for bit and dot exactly.

The same exact test with nontemporal loads of Z (a few rows, the large leading dimension of tests/stream_cases.py) and with a second tile per workgroup
(n above 2^17: the bounds for those rows are in that test's docstring); every exact call asserts the load form the library reports.

Random doubles, against numpy.longdouble. With w0abs = |s| (|a u| + |b v|), Habs = |Z|^T w0abs, Cabs = |Minv| Habs: forming w0 is three roundings
(a u, the fma with b v, the scaling): 3 eps w0abs; h is a sum of n products in some order: (n + 1) eps Habs plus |Z|^T of the error of w0, together
(n + 4) eps Habs; c is a k-term fma chain on it: (n + k + 5) eps Cabs; w is a k-term fma chain from w0: (k + 1) eps (w0abs + |Y| Cabs) plus the errors
of w0 and of c. Entrywise
    |w - ref| <= (n + 2 k + 9) eps (w0abs + |Y| Cabs).
dot against the longdouble e^T w of the device's own w: (n + 1) eps |e|^T |w|.
Projection property, Minv = inv(Z^T Y) from numpy: Z^T w_out = (I - M Minv) h in exact arithmetic, so
    |Z^T w_out| <= (n + 2 k + 9) eps |Z|^T (w0abs + |Y| Cabs) + |I - M Minv| Habs,
the second term (the residual of numpy's inverse) evaluated in longdouble."""
import ctypes as C

import numpy as np
import pytest

import stream_cases as sc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
ARG_SIZ, ARG_WRONG, ARG_OUTOFRANGE, ARG_INCOMP, ARG_NULL = 60, 62, 63, 75, 85
KS = [0, 1, 2, 7, 8, 9, 33, 64, 65]
# oblique_kt_for compiles the column tiles 1..8, 10, 12, 16, 20, 24, 32, 40, 48, 56, 64: the ones KS does not reach, filled exactly, and one column past
# a tile (the next tile with its last columns clamped)
KS_TILES_EXACT = [3, 4, 5, 6, 12, 16, 20, 24, 32, 48, 56]
KS_TILES_PAST = [11, 13, 17, 21, 25, 41, 49, 57]
WCOLS = 68                           # columns of Y and Z: l <= 2, k <= 65
LIMIT = 2.0 ** 53


def _ints(rng, shape, bound):
    return rng.integers(-bound, bound + 1, size=shape).astype(np.float64)


def _odd_ld(n):
    return n + 3 if (n + 3) % 2 else n + 4


def _sparse_rows(rng, rows, cols, per_row):
    """entries in {-1, 0, 1}, at most per_row of them in a row"""
    M = np.zeros((rows, cols))
    if rows and cols:
        pick = np.argsort(rng.random((rows, cols)), axis=1)[:, :min(per_row, cols)]           # per row: distinct columns
        np.put_along_axis(M, pick, rng.integers(-1, 2, size=pick.shape).astype(np.float64), axis=1)
    return M


class _Harness:
    """Y, Z, six device vectors (columns of a third BV: u, v, s, w, e, spare) and a device copy of Minv, all of one local size"""

    def __init__(self, ctx, n, ld=0, N=None, wcols=WCOLS, kmax=65):
        import slepc_amd as ks
        self.ctx, self.n = ctx, n
        self.Y, self.Z, self.vec = ks.BV(ctx, n, wcols, ld=ld, N=N), ks.BV(ctx, n, wcols, ld=ld, N=N), ks.BV(ctx, n, 6, ld=ld, N=N)
        self.minv = ks.BV(ctx, (kmax + 4) * (kmax + 1), 1)         # ldm <= kmax + 3 rows, kmax columns, and room for k = 0
        self.ptr = [self.vec.column_ptr(j) for j in range(6)]

    def set_minv(self, Minv, ldm):
        k = Minv.shape[0]
        full = np.full(self.minv.n, 55.0)                      # entries outside the k x k block (rows k..ldm) are not read
        pad = np.full((ldm, max(k, 1)), 55.0, order="F"); pad[:k, :k] = Minv
        full[:pad.size] = pad.ravel(order="F")
        self.minv.set_column(0, full)

    def call(self, ldm, a, u, b, v, s, w, e, want_dot=True):
        """u, v, s, w, e: indices into the six vectors, or None; returns (rc, dot)"""
        q = lambda j: None if j is None else C.c_void_p(self.ptr[j])
        dot = C.c_double(-123.0)
        rc = self.ctx.L.ks_bv_oblique_project(self.Y.h, self.Z.h, C.c_void_p(self.minv.column_ptr(0)), ldm, float(a), q(u), float(b), q(v), q(s), q(w), q(e),
                                              C.byref(dot) if want_dot else None)
        return rc, dot.value

    def destroy(self):
        for b in (self.Y, self.Z, self.vec, self.minv):
            b.destroy()


def _reference(Zk, Yk, Minv, a, u, b, v, s, e_is_w, e):
    """numpy in double on integer data: (w, dot, largest sum of absolute values of any intermediate)"""
    w0 = a * u
    if v is not None:
        w0 = w0 + b * v
    if s is not None:
        w0 = s * w0
    h = Zk.T @ w0; c = Minv @ h; w = w0 - Yk @ c
    habs = np.abs(Zk).T @ np.abs(w0); cabs = np.abs(Minv) @ habs; wabs = np.abs(w0) + np.abs(Yk) @ cabs
    ev = w if e_is_w else e
    dot = None if ev is None else float(ev @ w)
    big = max([np.abs(w0).max(initial=0.0), habs.max(initial=0.0), cabs.max(initial=0.0), wabs.max(initial=0.0)]
              + ([float((wabs if e_is_w else np.abs(e)) @ wabs)] if ev is not None else []))
    return w, dot, big


def _exact_plan(every_tile):
    """(k, combinations of s, v and e) of an exact run: KS with all eight; every_tile: also the other tiles of oblique_kt_for, filled exactly with all
    eight and one column past with two (everything present, nothing present)"""
    plan = [(k, range(8)) for k in KS]
    if every_tile:
        plan += [(k, range(8)) for k in KS_TILES_EXACT] + [(k, (7, 0)) for k in KS_TILES_PAST]
    return plan


def _oblique_exact(ctx, H, n, rng, plan, form, idx):
    """The calls of `plan` on the harness H against numpy on integer data, bit for bit. `form`: the load form the library must report for the dot
    sweep of every call, "plain" or "streaming" (one verdict per chunk of 64 columns; none at k = 0, which has no sweep over Z)."""
    Zm = _ints(rng, (n, WCOLS), 1)
    Ym = _sparse_rows(rng, n, WCOLS, 2)
    H.Z.set_dense(Zm); H.Y.set_dense(Ym)
    for k, combos in plan:
        for combo in combos:
            has_s, has_v, has_e = bool(combo & 1), bool(combo & 2), bool(combo & 4)
            lz = (0, 2)[idx % 2]; ly = (0, 2)[(idx // 2) % 2]; ldm = max(k, 1) + (3 if idx % 3 == 0 else 0)
            u_is_w = idx % 2 == 1; e_is_w = has_e and (idx // 2) % 2 == 1
            idx += 1
            # at most 2 entries per row of Y INSIDE the active range: drawn per call on the active columns
            Yk = _sparse_rows(rng, n, k, 2)
            for j in range(k):
                H.Y.set_column(ly + j, Yk[:, j])
            Ym[:, ly:ly + k] = Yk
            Zk = Zm[:, lz:lz + k]
            Minv = _sparse_rows(rng, k, k, 4)
            H.set_minv(Minv, ldm)
            vecs = _ints(rng, (n, 6), 2)
            H.vec.set_dense(vecs)
            a, b = float(rng.choice([-2, -1, 1, 2])), float(rng.choice([-2, -1, 1, 2]))
            H.Z.SetActiveColumns(lz, lz + k); H.Y.SetActiveColumns(ly, ly + k)
            iw = 0 if u_is_w else 3
            ie = (iw if e_is_w else 4) if has_e else None
            (rc, dot), counts = sc.counted(ctx, lambda: H.call(ldm, a, 0, b, 1 if has_v else None, 2 if has_s else None, iw, ie, want_dot=has_e))
            assert rc == 0, (k, combo, rc)
            sweeps = (k + 63) // 64
            assert counts == ((sweeps, 0) if form == "plain" else (0, sweeps)), (k, combo, form, counts)
            w, dref, big = _reference(Zk, Yk, Minv, a, vecs[:, 0], b, vecs[:, 1] if has_v else None, vecs[:, 2] if has_s else None, e_is_w, vecs[:, 4] if has_e else None)
            assert big < LIMIT, (k, combo, big)
            got = H.vec.dense()
            assert np.array_equal(got[:, iw], w), (k, combo, lz, ly, u_is_w, np.argwhere(got[:, iw] != w)[:4])
            if has_e:
                assert dot == dref, (k, combo, e_is_w, dot, dref)
            else:
                assert dot == -123.0
            keep = [j for j in range(6) if j != iw]
            assert np.array_equal(got[:, keep], vecs[:, keep])
    H.Z.SetActiveColumns(0, WCOLS); H.Y.SetActiveColumns(0, WCOLS)
    assert np.array_equal(H.Z.dense(), Zm) and np.array_equal(H.Y.dense(), Ym)
    H.destroy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("odd_ld", [True, False])
def test_oblique_project_exact(ctx, n, odd_ld):
    """Every k of KS with every combination of s, v and e present or absent (8 per k), u == w on every other call, e == w on every other call that has an
    e, the active ranges of Y and Z starting at 0 or 2 independently, ldm > k on every third call. Odd ld: the scalar path; the default ld: the 16-byte
    path. Y, Z and the inputs keep their bits. At n = 65 and n = 4099 also the column tiles of oblique_kt_for that KS leaves out (_exact_plan). Y and Z
    of a few thousand rows: every dot sweep reports plain loads."""
    rng = np.random.default_rng(9000 * n + odd_ld)
    H = _Harness(ctx, n, ld=_odd_ld(n) if odd_ld else 0)
    assert (H.Y.ld % 2 == 1) == odd_ld
    _oblique_exact(ctx, H, n, rng, _exact_plan(n in (65, 4099)), "plain", int(odd_ld))


@pytest.mark.parametrize("n", [1, 511, 513, 4099])
def test_oblique_project_streaming_loads_exact(ctx, n):
    """The plain == 0 branch of k_oblique_dot<KT, 2> for every KT: the data and the bounds of test_oblique_project_exact on a few rows of Y and Z (68
    columns each) whose leading dimension puts their storage above the size at which the library streams the basis (stream_cases.streaming_ld asks
    the library). Every column tile filled exactly and one column past it, two combinations of s, v and e each and all eight at k = 7 and k = 33; k = 65
    is left out (its second chunk is a dot sweep of Z alone, which is resident). The rows n .. ld - 1 hold NaN bytes."""
    rng = np.random.default_rng(9500 * n)
    H = _Harness(ctx, n, ld=sc.streaming_ld(ctx, n, 2 * WCOLS))
    sc.fill_nan(ctx, H.Y, H.Z, H.vec)
    ks_ = sorted(set(KS[1:-1] + KS_TILES_EXACT + KS_TILES_PAST))
    assert max(ks_) == 64
    _oblique_exact(ctx, H, n, rng, [(k, (7, 0)) for k in ks_] + [(7, range(8)), (33, range(8))], "streaming", 0)


@pytest.mark.parametrize("k", [2, 8, 33])
@pytest.mark.parametrize("form", ["plain", "streaming"])
def test_oblique_project_second_tile_of_a_workgroup(ctx, k, form):
    """More tiles than workgroups: n = per_cu num_cu 512 + 513 rows with per_cu the factor of the dot sweep (4 at k = 2 and k = 8, 1 at k = 33), so every
    workgroup of k_oblique_dot walks its first tile, some a second one, and the last tile is a single row; at k = 2 and k = 8 the update sweep
    (4 workgroups per CU, eight columns in flight and the columns left over) walks the same way, at k = 33 it has one tile per workgroup.

    Exactness at these n. Z and Y are dense (entries -1, 0, 1) and u, v and e are zero outside at most 4096 rows, some in every tile. Then
    |w0| <= 2^4 on those rows and 0 elsewhere, and zeros add exactly nothing: |h| <= 4096 2^4 = 2^16, |c| <= 4 2^16 = 2^18 (four entries per row of
    Minv), |w| <= 2^4 + 33 2^18 < 2^24 in every row, and e^T w with |e| <= 2 on 4096 rows stays below 2^37: exact, and checked on the data itself
    (big < 2^53). The one quantity that cannot stay exact is the dot with e == w: w^2 < 2^48 summed over n > 2^17 rows passes 2^53. It is held to
    the bound of the random-doubles test, (n + 1) eps |w|^T |w| against the longdouble sum over the device's own w.

    Y and Z of k + 3 columns are resident (plain loads); of 24 columns (k = 2, 8) or 68 (k = 33) with the leading dimension of
    stream_cases.streaming_ld they stream. Two calls per case: s, v and a separate e; and none of them with u == w and e == w."""
    num_cu = ctx.device_info()["num_cu"]
    n = sc.two_round_n(sc.dot_per_cu(k), num_cu)
    ntiles, grid = sc.walk(n, sc.dot_per_cu(k), num_cu)
    assert ntiles > grid and ntiles < 2 * grid and n % sc.TILE == 1, (n, ntiles, grid)
    if k <= 8:
        assert ntiles > sc.walk(n, sc.SWEEP_PER_CU, num_cu)[1]                      # the update sweep too
    wcols = k + 3 if form == "plain" else (24 if k <= 8 else WCOLS)
    ld = sc.even_ld(n) if form == "plain" else sc.streaming_ld(ctx, n, 2 * wcols)
    rng = np.random.default_rng(4400 + 10 * k + (form == "plain"))
    H = _Harness(ctx, n, ld=ld, wcols=wcols, kmax=k)
    sc.fill_nan(ctx, H.Y, H.Z, H.vec)                                                  # the columns outside the active ranges and the rows past n: NaN bytes
    lz, ly = 2, 1
    Zk, Yk, Minv = _ints(rng, (n, k), 1), _ints(rng, (n, k), 1), _sparse_rows(rng, k, k, 4)
    for j in range(k):
        H.Z.set_column(lz + j, Zk[:, j]); H.Y.set_column(ly + j, Yk[:, j])
    H.Z.SetActiveColumns(lz, lz + k); H.Y.SetActiveColumns(ly, ly + k)
    H.set_minv(Minv, k + 3)
    rows = sc.spread_rows(n)
    for e_is_w in (False, True):
        vecs = np.zeros((n, 6))
        vecs[rows] = _ints(rng, (len(rows), 6), 2)
        vecs[:, 2] = _ints(rng, n, 2)                                                  # s is dense: it scales zeros
        H.vec.set_dense(vecs)
        a, b = float(rng.choice([-2, -1, 1, 2])), float(rng.choice([-2, -1, 1, 2]))
        if e_is_w:
            (rc, dot), counts = sc.counted(ctx, lambda: H.call(k + 3, a, 0, b, None, None, 0, 0))
            w, dref, big = _reference(Zk, Yk, Minv, a, vecs[:, 0], b, None, None, False, None)
        else:
            (rc, dot), counts = sc.counted(ctx, lambda: H.call(k + 3, a, 0, b, 1, 2, 3, 4))
            w, dref, big = _reference(Zk, Yk, Minv, a, vecs[:, 0], b, vecs[:, 1], vecs[:, 2], False, vecs[:, 4])
        assert rc == 0
        assert counts == ((1, 0) if form == "plain" else (0, 1)), (form, counts)
        assert big < LIMIT, big
        got = H.vec.column(0 if e_is_w else 3)
        assert np.array_equal(got, w), (k, form, e_is_w, np.argwhere(got != w)[:4])
        if e_is_w:
            wl = got.astype(np.longdouble)
            assert abs(dot - float(wl @ wl)) <= (n + 1) * EPS * float(np.abs(got) @ np.abs(got)), (dot, float(wl @ wl))
        else:
            assert dot == dref, (dot, dref)
    for j in range(k):
        assert np.array_equal(H.Z.column(lz + j), Zk[:, j]) and np.array_equal(H.Y.column(ly + j), Yk[:, j]), j
    H.destroy()


def _random_case(rng, n, k):
    Z = rng.standard_normal((n, k)); Y = Z + 0.3 * rng.standard_normal((n, k))
    vecs = rng.standard_normal((n, 6))
    return Z, Y, vecs, 1.7, -0.6


@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("k", [7, 33, 65])
def test_oblique_project_random_doubles_and_projection_property(ctx, n, k):
    rng = np.random.default_rng(77 * n + k)
    Z, Y, vecs, a, b = _random_case(rng, n, k)
    M = Z.T @ Y
    Minv = np.linalg.inv(M)
    H = _Harness(ctx, n)
    for j in range(k):
        H.Z.set_column(j, Z[:, j]); H.Y.set_column(j, Y[:, j])
    H.Z.SetActiveColumns(0, k); H.Y.SetActiveColumns(0, k)
    H.set_minv(Minv, k); H.vec.set_dense(vecs)
    rc, dot = H.call(k, a, 0, b, 1, 2, 3, 4)
    assert rc == 0
    ld_ = np.longdouble
    u, v, s, e = (vecs[:, j].astype(ld_) for j in (0, 1, 2, 4))
    w0 = s * (a * u + b * v)
    h = Z.astype(ld_).T @ w0; c = Minv.astype(ld_) @ h; ref = w0 - Y.astype(ld_) @ c
    w0abs = np.abs(vecs[:, 2]) * (np.abs(a * vecs[:, 0]) + np.abs(b * vecs[:, 1]))
    habs = np.abs(Z).T @ w0abs; cabs = np.abs(Minv) @ habs
    scale = w0abs + np.abs(Y) @ cabs
    bound = (n + 2 * k + 9) * EPS * scale
    w = H.vec.column(3)
    err = np.abs(w.astype(ld_) - ref).astype(np.float64)
    print("n=%d k=%d  max err / bound %.4f" % (n, k, (err / bound).max()))
    assert np.all(err <= bound)
    dref = float(e @ w.astype(ld_))
    assert abs(dot - dref) <= (n + 1) * EPS * float(np.abs(vecs[:, 4]) @ np.abs(w)), (dot, dref)
    # the projection property
    zw = np.abs((Z.astype(ld_).T @ w.astype(ld_)).astype(np.float64))
    inv_res = np.abs((np.eye(k).astype(ld_) - M.astype(ld_) @ Minv.astype(ld_)).astype(np.float64)) @ habs
    pbound = (n + 2 * k + 9) * EPS * (np.abs(Z).T @ scale) + inv_res
    print("          max |Z^T w| / bound %.4f, |Z^T w0| max %.3e" % ((zw / pbound).max(), np.abs(h).max()))
    assert np.all(zw <= pbound)
    # the same data on the scalar path (odd ld): the same bits of w (every entry depends on its own row and on c alone), the dot within its bound
    H1 = _Harness(ctx, n, ld=_odd_ld(n))
    for j in range(k):
        H1.Z.set_column(j, Z[:, j]); H1.Y.set_column(j, Y[:, j])
    H1.Z.SetActiveColumns(0, k); H1.Y.SetActiveColumns(0, k)
    H1.set_minv(Minv, k); H1.vec.set_dense(vecs)
    rc, dot1 = H1.call(k, a, 0, b, 1, 2, 3, 4)
    assert rc == 0
    w1 = H1.vec.column(3)
    assert np.all(np.abs(w1.astype(ld_) - ref).astype(np.float64) <= bound)
    assert abs(dot1 - float(e @ w1.astype(ld_))) <= (n + 1) * EPS * float(np.abs(vecs[:, 4]) @ np.abs(w1))
    H.destroy(); H1.destroy()


def test_a_call_without_a_dot_only_enqueues_and_the_wrapper_agrees(ctx):
    n, k = 257, 9
    rng = np.random.default_rng(12)
    H = _Harness(ctx, n)
    Z, Y, Minv, vecs = _ints(rng, (n, k), 1), _sparse_rows(rng, n, k, 2), _sparse_rows(rng, k, k, 4), _ints(rng, (n, 6), 2)
    for j in range(k):
        H.Z.set_column(j, Z[:, j]); H.Y.set_column(j, Y[:, j])
    H.Z.SetActiveColumns(0, k); H.Y.SetActiveColumns(0, k)
    H.set_minv(Minv, k); H.vec.set_dense(vecs)
    ctx.synchronize()
    before = ctx.sync_count()
    rc, dot = H.call(k, 2.0, 0, -1.0, 1, None, 3, None, want_dot=False)
    assert rc == 0 and ctx.sync_count() == before                      # no host wait
    rc, dot = H.call(k, 2.0, 0, -1.0, 1, None, 5, 4, want_dot=True)
    assert rc == 0 and ctx.sync_count() == before + 1                  # one, for the dot
    w, dref, _ = _reference(Z, Y, Minv, 2.0, vecs[:, 0], -1.0, vecs[:, 1], None, False, vecs[:, 4])
    got = H.vec.dense()
    assert np.array_equal(got[:, 3], w) and np.array_equal(got[:, 5], w) and dot == dref
    # BV.ObliqueProject (self is Y), Minv from the host
    H.vec.set_dense(vecs)
    d = H.Y.ObliqueProject(H.Z, Minv, 2.0, H.ptr[0], H.ptr[3], b=-1.0, v_ptr=H.ptr[1], e_ptr=H.ptr[4])
    assert d == dref and np.array_equal(H.vec.column(3), w)
    assert H.Y.ObliqueProject(H.Z, Minv, 2.0, H.ptr[0], H.ptr[5], b=-1.0, v_ptr=H.ptr[1]) is None
    assert np.array_equal(H.vec.column(5), w)
    H.destroy()


def _two_rank_data(n, k):
    rng = np.random.default_rng(606)
    return _ints(rng, (n, k), 1), _sparse_rows(rng, n, k, 2), _sparse_rows(rng, k, k, 4), _ints(rng, (n, 6), 2)


def _run_rows(ctx, Z, Y, Minv, vecs, N=None):
    n, k = Z.shape
    H = _Harness(ctx, n, N=N, wcols=k, kmax=k)
    if n:
        H.Z.set_dense(Z); H.Y.set_dense(Y); H.vec.set_dense(vecs)
    H.set_minv(Minv, k)
    rc, dot = H.call(k, -2.0, 0, 1.0, 1, 2, 3, 3)
    assert rc == 0
    w = H.vec.column(3) if n else np.zeros(0)
    H.destroy()
    return w, dot


def test_two_thread_ranks_give_the_bits_of_one_rank(ctx):
    """rows 0..2050 on rank 0 and the other 2048 on rank 1: row for row the bits of the one-rank w, the same exact ||w||^2 on both"""
    import slepc_amd as ks
    n, k = 4099, 9
    Z, Y, Minv, vecs = _two_rank_data(n, k)
    w, dot = _run_rows(ctx, Z, Y, Minv, vecs)
    ref, dref, big = _reference(Z, Y, Minv, -2.0, vecs[:, 0], 1.0, vecs[:, 1], vecs[:, 2], True, None)
    assert big < LIMIT and np.array_equal(w, ref) and dot == dref
    split = [(0, 2051), (2051, n)]

    def rank_fn(rank, comm):
        c = ks.Context(0)
        comm.install(c, rank)
        s0, s1 = split[rank]
        out = _run_rows(c, Z[s0:s1], Y[s0:s1], Minv, vecs[s0:s1], N=n)
        c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    for rank, (s0, s1) in enumerate(split):
        assert np.array_equal(res[rank][0], w[s0:s1])
        assert res[rank][1] == dot


def test_a_rank_with_no_rows_is_legal(ctx):
    import slepc_amd as ks
    n, k = 130, 3
    Z, Y, Minv, vecs = _two_rank_data(n, k)
    w, dot = _run_rows(ctx, Z, Y, Minv, vecs)
    split = [(0, n), (n, n)]

    def rank_fn(rank, comm):
        c = ks.Context(0)
        comm.install(c, rank)
        s0, s1 = split[rank]
        out = _run_rows(c, Z[s0:s1], Y[s0:s1], Minv, vecs[s0:s1], N=n)
        c.close()
        return out

    res = run_ranks(ThreadComm(2), rank_fn)
    assert np.array_equal(res[0][0], w) and res[0][1] == dot and res[1][1] == dot and len(res[1][0]) == 0


def test_oblique_project_arguments(ctx):
    """every row of the error table of include/ksgpu.h"""
    import slepc_amd as ks
    n = 10
    H = _Harness(ctx, n, wcols=8, kmax=8)
    f = ctx.L.ks_bv_oblique_project
    q = lambda j: C.c_void_p(H.ptr[j])
    mp = C.c_void_p(H.minv.column_ptr(0))
    H.set_minv(np.eye(4), 8); H.vec.set_dense(np.ones((n, 6)))
    H.Z.SetActiveColumns(0, 4); H.Y.SetActiveColumns(2, 6)
    dot = C.c_double()
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), q(4), C.byref(dot)) == 0
    assert f(H.Y.h, H.Z.h, mp, 3, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_SIZ                    # ldm < k
    H.Y.SetActiveColumns(2, 5)
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_INCOMP                 # 3 columns against 4
    H.Y.SetActiveColumns(2, 6)
    longer = ks.BV(ctx, n + 1, 8); longer.SetActiveColumns(0, 4)
    assert f(longer.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_INCOMP              # another local size
    assert f(H.Y.h, longer.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_INCOMP
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, None, None, None) == ARG_NULL                   # w
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, None, 0.0, None, None, q(3), None, None) == ARG_NULL                   # u
    assert f(None, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_NULL
    assert f(H.Y.h, None, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_NULL
    assert f(H.Y.h, H.Z.h, None, 8, 1.0, q(0), 0.0, None, None, q(3), None, None) == ARG_NULL                 # Minv with k > 0
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, q(3), None, C.byref(dot)) == ARG_NULL           # a dot without e
    for bv in (H.Y, H.Z):                                                                                     # w a column of Y or Z, active or not
        for j in (0, 7):
            assert f(H.Y.h, H.Z.h, mp, 8, 1.0, q(0), 0.0, None, None, C.c_void_p(bv.column_ptr(j)), None, None) == ARG_WRONG
    assert f(H.Y.h, H.Z.h, mp, 8, 1.0, C.c_void_p(H.Z.column_ptr(1)), 0.0, None, None, q(3), None, None) == 0    # u may be one
    H.Z.SetActiveColumns(3, 3); H.Y.SetActiveColumns(0, 0)
    assert f(H.Y.h, H.Z.h, None, 0, 1.0, q(0), 0.0, None, None, q(3), None, None) == 0                        # k = 0 needs no Minv
    longer.destroy(); H.destroy()


# ---- ks_bv_ritz_residual_vectors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("generalized", [False, True])
@pytest.mark.parametrize("odd_ld", [True, False])
def test_ritz_residual_vectors_exact(ctx, n, generalized, odd_ld):
    """The data and the bounds of tests/test_gpu_gd_kernels.py (|x| < 2^13, |bx| < 2^13: exact). X and BX equal numpy's bit for bit from their first
    active columns, with both, one or none of them asked for; R and the norms have the bits of ks_bv_ritz_residual on the same inputs; the columns of X
    and BX outside the result range keep their bits."""
    import slepc_amd as ks
    rng = np.random.default_rng(5000 * n + 10 * generalized + odd_ld)
    ld = _odd_ld(n) if odd_ld else 0
    WV, WR = 42, 19
    Vb, AVb, Rb, R2 = ks.BV(ctx, n, WV, ld=ld), ks.BV(ctx, n, WV, ld=ld), ks.BV(ctx, n, WR, ld=ld), ks.BV(ctx, n, WR, ld=ld)
    BVb = ks.BV(ctx, n, WV, ld=ld) if generalized else None
    Xb, BXb = ks.BV(ctx, n, WR, ld=ld), ks.BV(ctx, n, WR, ld=ld)
    V, AV, BV = _ints(rng, (n, WV), 16), _ints(rng, (n, WV), 64), _ints(rng, (n, WV), 16)
    Vb.set_dense(V); AVb.set_dense(AV)
    if generalized:
        BVb.set_dense(BV)
    # beyond one row: every pass width the dispatch compiles (1, 2, 4, 8 and, without B, 16) and, with B, second passes of 1, 2, 4 and 8 columns
    widths = (1, 3, 8, 9, 16) if n == 1 else (1, 2, 3, 4, 5, 8, 9, 10, 12, 16)
    idx = 0
    for m in (1, 7, 9, 40):
        idx += (len(widths) + 1) % 2 if m != 1 else 0        # an odd stride from one m to the next (5 or 11): over the four m every width meets all four
                                                             # choices of outputs and both l
        for ncols in widths:
            l = (0, 2)[idx % 2]; lX = (0, 3)[(idx // 2) % 2]; lBX = (3, 0)[(idx // 4) % 2]; outs = idx % 4            # 0: both, 1: X, 2: BX, 3: none
            idx += 1
            S = np.asfortranarray(_ints(rng, (m, ncols), 8)); theta = _ints(rng, ncols, 8)
            X0, BX0, R0 = _ints(rng, (n, WR), 5), _ints(rng, (n, WR), 5), _ints(rng, (n, WR), 5)
            Xb.set_dense(X0); BXb.set_dense(BX0); Rb.set_dense(R0); R2.set_dense(R0)
            for bvv in (Vb, AVb) + ((BVb,) if generalized else ()):
                bvv.SetActiveColumns(l, l + m)
            Xb.SetActiveColumns(lX, WR); BXb.SetActiveColumns(lBX, WR)
            Xa = Xb if outs in (0, 1) else None; BXa = BXb if outs in (0, 2) else None
            (rn, xn), counts = sc.counted(ctx, lambda: Rb.RitzResidualVectors(Vb, AVb, BVb, S, theta, X=Xa, BX=BXa))
            (rn2, xn2), counts2 = sc.counted(ctx, lambda: R2.RitzResidual(Vb, AVb, BVb, S, theta))
            assert counts == (1, 0) and counts2 == (1, 0), (m, ncols, counts, counts2)          # panels of a few thousand rows: plain loads
            assert np.array_equal(Rb.dense(), R2.dense()) and np.array_equal(rn, rn2) and np.array_equal(xn, xn2)
            x = V[:, l:l + m] @ S; bx = BV[:, l:l + m] @ S if generalized else x
            if Xa is not None:
                X0[:, lX:lX + ncols] = x
            if BXa is not None:
                BX0[:, lBX:lBX + ncols] = bx
            assert np.array_equal(Xb.dense(), X0), (m, ncols, outs)
            assert np.array_equal(BXb.dense(), BX0), (m, ncols, outs)
    assert np.array_equal(Vb.dense(), V) and np.array_equal(AVb.dense(), AV)


def test_ritz_residual_vectors_arguments(ctx):
    import slepc_amd as ks
    n = 10
    R, V, AV, BV, X, BX = (ks.BV(ctx, n, 8) for _ in range(6))
    S = np.zeros(8 * 8); th = np.zeros(8); rn = np.zeros(8); xn = np.zeros(8)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    f = ctx.L.ks_bv_ritz_residual_vectors
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), X.h, BX.h) == 0
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), None, None) == 0
    for bad in (R, V, AV, BV):
        assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), bad.h, BX.h) == ARG_WRONG
        assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), X.h, bad.h) == ARG_WRONG
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), X.h, X.h) == ARG_WRONG
    longer = ks.BV(ctx, n + 1, 8)
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), longer.h, None) == ARG_INCOMP
    X.SetActiveColumns(5, 8)
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 4, p(th), p(rn), p(xn), X.h, None) == ARG_SIZ                     # 3 columns from its first active one
    assert f(R.h, V.h, AV.h, BV.h, p(S), 8, 0, p(th), p(rn), p(xn), None, None) == ARG_OUTOFRANGE             # the checks of ks_bv_ritz_residual come first
