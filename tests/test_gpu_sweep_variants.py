"""Exact checks of every compiled variant of the row-sweep and panel kernels: the dot sweep (k_dot_sweep<KT, VEC>), the update of a
Gram-Schmidt pass (k_gs_update<KT, VEC, GS1> in both load policies), the SpMV fused into the dot sweep (k_dot_spmv_dict<KT, W>), the
panel products on the matrix cores (k_panel_dot_direct<MT, NT, SAME, U>, k_panel_mult_direct<KS4, NT, U>) and on the VALU
(k_panel_mult<KT, TRANSQ>), and k_multvec<VEC>.

The inputs are small integers or dyadic rationals whose every sum is exact in double precision (each test asserts the bound), so the
correct result does not depend on the order of the additions and is compared bit for bit with a numpy float64 reference. Rows n..ld-1
of the storage and the columns a kernel must not read hold NaN bytes: a read past the guard or the clamp shows up in the result. Each
case also asserts through the profiler that the (class, column tile) it means to reach was launched, so a change to the dispatch that
shrinks the coverage fails here."""
import math

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

ETA = 0.7071
# every compiled column tile (ks_kt_for), plus counts inside the 8-wide tiles above 32
KTS = list(range(1, 33)) + [33, 40, 41, 48, 55, 56, 57, 64]
# row counts around the tile edges (256 threads x VEC rows) and the chunk remainders of the panel kernels (8U / 32U rows)
NS = [1, 2, 255, 256, 257, 511, 513, 100003, 1000, 4097, 63, 95]
EXACT = 2.0 ** 53


def kt_for(ncols):
    if ncols <= 1:
        return 1
    if ncols <= 32:
        return ncols
    return min(64, (ncols + 7) // 8 * 8)


def ld_for(n, odd):
    """odd: an odd leading dimension (columns not 16-byte aligned: the one-row forms); otherwise an even one that is not a multiple of 32."""
    if odd:
        return n if n % 2 else n + 1
    return n + 2 if n % 2 == 0 else n + 1


def assert_exact(*terms):
    """Each term (x, y, count): the products x*y summed over `count` rows stay below 2^53 in units of the smallest power of two
    that makes every entry an integer - so any summation order gives the exact result."""
    for x, y, count in terms:
        x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
        ex = _unit_exp(x) + _unit_exp(y)
        mx = (np.abs(x).max() if x.size else 0.0) * (np.abs(y).max() if y.size else 0.0)
        assert mx * count * 2.0 ** ex < EXACT, (mx, count, ex)


def _unit_exp(x):
    f = x[np.isfinite(x) & (x != 0)]
    if not f.size:
        return 0
    e = 0
    while not np.all(np.mod(f * 2.0 ** e, 1.0) == 0.0):
        e += 1
        assert e < 60
    return e


def ints(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


class Store:
    """A BV whose whole storage is NaN bytes before the columns the case needs are written."""

    def __init__(self, ctx, n, m, odd=False, nc_cols=None, ld=None):
        import slepc_amd as ks
        self.ctx = ctx
        self.V = ks.BV(ctx, n, m, ld=ld_for(n, odd) if ld is None else ld)
        if nc_cols is not None:
            assert self.V.InsertConstraints(nc_cols) == nc_cols.shape[1]
        self.nc = self.V.nc
        self.n, self.ld = n, self.V.ld
        self.base = self.V.column_ptr(-self.nc)
        ctx.memset(self.base, 0xFF, (self.nc + self.V.m) * self.ld * 8)
        ctx.synchronize()

    def put(self, j, x):
        """Column j (negative: constraint) <- x, rows n..ld-1 keep their NaN bytes."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        self.ctx.memcpy_h2d(self.base + 8 * (j + self.nc) * self.ld, x)
        self.ctx.synchronize()

    def get(self, j):
        return self.V.column(j)


def profiled(ctx, fn):
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        out = fn()
        ctx.synchronize()
        return out, ctx.prof_get(by_variant=True)
    finally:
        ctx.prof_enable(False)


def launched(prof, cls, var):
    return prof.get((cls, var), {}).get("launches", 0)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["vec2", "vec1"])
def test_dot_sweep_every_tile(ctx, odd):
    """BVDotVec: k_dot_sweep<KT, VEC> for every KT, n around the tile edges; one case above 512 blocks (the second block-combine form)."""
    rng = np.random.default_rng(11 + odd)
    cases = [(nc, NS[i % len(NS)]) for i, nc in enumerate(KTS)] + [(nc, NS[(i + 5) % len(NS)]) for i, nc in enumerate(KTS)]
    cases += [(1, (1 << 19) + 3), (5, (1 << 19) + 3), (7, 1 << 19)]
    for nc, n in cases:
        S = Store(ctx, n, nc + 1, odd)
        A = ints(rng, (n, nc)); y = ints(rng, n)
        for j in range(nc):
            S.put(j, A[:, j])
        S.put(nc, y)
        assert_exact((A, y, n))
        S.V.SetActiveColumns(0, nc)
        out, prof = profiled(ctx, lambda: S.V.DotVec(S.V.column_ptr(nc)))
        assert np.array_equal(out, A.T @ y), (nc, n, odd)
        assert launched(prof, "bv_dot_sweep", kt_for(nc)) >= 1, (nc, prof.keys())
        S.V.destroy()


@pytest.mark.parametrize("n", [1, 511, 513, 4099])
def test_dot_sweep_streaming_loads_every_tile(ctx, n):
    """The plain == 0 branch of k_dot_sweep<KT, 2> for every KT: a few rows of a basis whose leading dimension puts its storage above the size at
    which the library streams it (stream_cases.streaming_ld asks the library, and the call must report one streaming verdict and no plain one)."""
    rng = np.random.default_rng(13 + n)
    for nc in KTS:
        S = Store(ctx, n, nc + 1, ld=sc.streaming_ld(ctx, n, nc + 1))
        A = ints(rng, (n, nc)); y = ints(rng, n)
        for j in range(nc):
            S.put(j, A[:, j])
        S.put(nc, y)
        assert_exact((A, y, n))
        S.V.SetActiveColumns(0, nc)
        (out, prof), counts = sc.counted(ctx, lambda: profiled(ctx, lambda: S.V.DotVec(S.V.column_ptr(nc))))
        assert counts == (0, 1), (nc, n, counts)
        assert np.array_equal(out, A.T @ y), (nc, n)
        assert launched(prof, "bv_dot_sweep", kt_for(nc)) >= 1, (nc, prof.keys())
        S.V.destroy()


@pytest.mark.parametrize("odd", [False, True], ids=["vec2", "vec1"])
def test_multvec_both_forms(ctx, odd):
    """BVMultVec y = beta*y + alpha*V q: k_multvec<VEC>; beta = 0 over NaN ignores y, 8-column groups and their remainder."""
    rng = np.random.default_rng(21 + odd)
    for i, nc in enumerate([1, 7, 8, 9, 16, 17, 31, 64]):
        n = NS[i % len(NS)]
        S = Store(ctx, n, nc + 1, odd)
        A = ints(rng, (n, nc)); q = ints(rng, nc)
        for j in range(nc):
            S.put(j, A[:, j])
        S.V.SetActiveColumns(0, nc)
        S.V.MultVec(0.5, 0.0, S.V.column_ptr(nc), q)                     # y holds NaN bytes: beta = 0 must not read it
        assert_exact((A, q, nc))
        assert np.array_equal(S.get(nc), 0.5 * (A @ q)), (nc, n)
        y = ints(rng, n)
        S.put(nc, y)
        S.V.MultVec(-1.0, 2.0, S.V.column_ptr(nc), q)
        assert np.array_equal(S.get(nc), 2.0 * y - A @ q), (nc, n)
        S.V.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
def _tile_counts():
    out = []
    for mt in range(1, 5):
        for nt in range(1, 5):
            out.append((mt, nt))
    return out


def _cols_in(t, salt):
    """A column count with `t` 16-column tiles: full or ending inside the last tile."""
    return 16 * t - (salt % 3) * 5 if t > 1 or salt % 3 != 2 else 16 * t - 15


@pytest.mark.parametrize("same", [False, True], ids=["xy", "gram"])
def test_panel_dot_every_tile_shape(ctx, same):
    """BVDot M = Y^T X on the matrix cores: k_panel_dot_direct for every (MT, NT) and the SAME (Gram) form, n with chunk remainders."""
    rng = np.random.default_rng(31 + same)
    shapes = [(t, t) for t in range(1, 5) for _ in range(2)] if same else _tile_counts()
    for i, (mt, nt) in enumerate(shapes):
        n = [1, 2, 255, 257, 513, 100003, 8 * 8 * 7 + 5, 16 * 9 + 3][i % 8]
        my = _cols_in(mt, i); nx = my if same else _cols_in(nt, i + 1)
        X = Store(ctx, n, nx)
        Xh = ints(rng, (n, nx))
        for j in range(nx):
            X.put(j, Xh[:, j])
        if same:
            Y, Yh = X, Xh
        else:
            Y = Store(ctx, n, my)
            Yh = ints(rng, (n, my))
            for j in range(my):
                Y.put(j, Yh[:, j])
        assert_exact((Yh, Xh, n))
        M = np.full((my, nx), np.nan, order="F")
        _, prof = profiled(ctx, lambda: X.V.Dot(Y.V, M))
        assert np.array_equal(M, Yh.T @ Xh), (mt, nt, same, n)
        assert launched(prof, "bv_dot_panel", 0) >= 1
        X.V.destroy()
        if not same:
            Y.V.destroy()


@pytest.mark.parametrize("odd_c", [False, True], ids=["vecC", "scalarC"])
def test_panel_mult_every_tile_shape(ctx, odd_c):
    """BVMult Y = beta*Y + alpha*X Q on the matrix cores: k_panel_mult_direct for every (KS4, NT); odd ldc stores one double at a time
    (vecC = 0); beta = 0 over NaN."""
    rng = np.random.default_rng(41 + odd_c)
    for i, (kt, nt) in enumerate(_tile_counts()):
        n = [1, 2, 255, 257, 513, 100003, 32 * 4 * 3 + 7, 32 * 2 + 1][i % 8]
        kin, nout = _cols_in(kt, i), _cols_in(nt, i + 2)
        X = Store(ctx, n, kin)
        Xh = ints(rng, (n, kin))
        for j in range(kin):
            X.put(j, Xh[:, j])
        Y = Store(ctx, n, nout, odd=odd_c)
        Q = np.asfortranarray(ints(rng, (kin, nout)))
        assert_exact((Xh, Q, kin))
        _, prof = profiled(ctx, lambda: Y.V.Mult(0.5, 0.0, X.V, Q))
        Yh = np.stack([Y.get(j) for j in range(nout)], axis=1)
        assert np.array_equal(Yh, 0.5 * (Xh @ Q)), (kt, nt, n)
        assert launched(prof, "bv_mult", 16 * kt) >= 1, (kt, nt, prof.keys())
        Y.V.Mult(-1.0, 2.0, X.V, Q)
        Yh2 = np.stack([Y.get(j) for j in range(nout)], axis=1)
        assert np.array_equal(Yh2, 2.0 * Yh - Xh @ Q), (kt, nt, n)
        X.V.destroy(); Y.V.destroy()


@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "valu"])
@pytest.mark.parametrize("trans", [False, True], ids=["q", "qT"])
def test_multinplace_every_tile(ctx, debug, mfma, trans):
    """BVMultInPlace V(:,s:e) = V(:,l:k) Q: the result overwrites columns it reads. MFMA: even ld; VALU: odd ld, k_panel_mult<KT, TRANSQ>
    for every KT. Active columns start at l > 0 and s > 0 in half of the cases."""
    rng = np.random.default_rng(51 + 2 * mfma + trans)
    kins = [1, 4, 16, 17, 31, 33, 48, 49, 64] if mfma else KTS
    for i, kin in enumerate(kins):
        n = NS[i % len(NS)]
        l = 2 if i % 2 else 0
        k = l + kin
        s = l + (1 if i % 3 else 0)
        e = min(k, s + [kin, 16, 33, 64][i % 4])
        m = k + 1
        S = Store(ctx, n, m, odd=not mfma)
        Vh = ints(rng, (n, m))
        for j in range(m):
            S.put(j, Vh[:, j])
        ldq = max(k, e)
        Q = np.asfortranarray(ints(rng, (ldq, ldq)))
        assert_exact((Vh, Q, kin))
        S.V.SetActiveColumns(l, k)
        _, prof = profiled(ctx, lambda: S.V.MultInPlace(Q, s, e, trans))
        blk = Q[s:e, l:k].T if trans else Q[l:k, s:e]
        want = Vh.copy()
        want[:, s:e] = Vh[:, l:k] @ blk
        got = np.stack([S.get(j) for j in range(m)], axis=1)
        assert np.array_equal(got, want), (kin, n, l, s, e, trans)
        var = 16 * ((kin + 15) // 16) if mfma else 0
        assert launched(prof, "bv_multinplace", var) >= 1, (kin, prof.keys())
        S.V.destroy()


def test_panel_mult_valu_every_tile(ctx, debug):
    """BVMult with the matrix cores switched off (the no_mfma hook): k_panel_mult<KT, false> for every KT, beta = 0 over NaN."""
    debug("no_mfma")
    rng = np.random.default_rng(61)
    for i, kin in enumerate(KTS):
        n = NS[(i + 3) % len(NS)]
        nout = [1, 5, 16, 33, 64][i % 5]
        X = Store(ctx, n, kin)
        Xh = ints(rng, (n, kin))
        for j in range(kin):
            X.put(j, Xh[:, j])
        Y = Store(ctx, n, nout)
        Q = np.asfortranarray(ints(rng, (kin, nout)))
        assert_exact((Xh, Q, kin))
        _, prof = profiled(ctx, lambda: Y.V.Mult(0.5, 0.0, X.V, Q))
        Yh = np.stack([Y.get(j) for j in range(nout)], axis=1)
        assert np.array_equal(Yh, 0.5 * (Xh @ Q)), (kin, n)
        assert launched(prof, "bv_mult", 0) >= 1
        X.V.destroy(); Y.V.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_panel_products_random_within_componentwise_bound(ctx, debug):
    """Random doubles: BVDot and BVMult (matrix cores and VALU) against a long-double reference, inside the componentwise bound
    |computed - exact| <= c * k * u * (|A| |B|) with u = 2^-53, c = 2."""
    u = 2.0 ** -53
    rng = np.random.default_rng(71)
    for mfma in (True, False):
        if not mfma:
            debug("no_mfma")
        for n, kin, nout in [(257, 17, 33), (20011, 64, 64), (513, 40, 7)]:
            X = Store(ctx, n, kin)
            Xh = rng.standard_normal((n, kin))
            for j in range(kin):
                X.put(j, Xh[:, j])
            Y = Store(ctx, n, nout)
            Yh = rng.standard_normal((n, nout))
            for j in range(nout):
                Y.put(j, Yh[:, j])
            M = np.zeros((nout, kin), order="F")
            X.V.Dot(Y.V, M)
            ref = Yh.astype(np.longdouble).T @ Xh.astype(np.longdouble)
            bound = 2.0 * n * u * (np.abs(Yh).T @ np.abs(Xh))
            assert np.all(np.abs(M - ref) <= bound), (mfma, n, kin, nout)
            Q = np.asfortranarray(rng.standard_normal((kin, nout)))
            Y.V.Mult(1.0, 0.0, X.V, Q)
            got = np.stack([Y.get(j) for j in range(nout)], axis=1)
            ref = Xh.astype(np.longdouble) @ Q.astype(np.longdouble)
            bound = 2.0 * kin * u * (np.abs(Xh) @ np.abs(Q))
            assert np.all(np.abs(got - ref) <= bound), (mfma, n, kin, nout)
            X.V.destroy(); Y.V.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# Gram-Schmidt. The previous columns are Walsh columns of order 64 on the rows S = the first 32 and the last 32 (entries +-d/8, d = 1:
# orthonormal, d = 2 on some regular columns for the refinement cases, which then have work for their second pass). The vector is
# V a + r with r on rows outside S. The sizes are chosen so that every v.v a norm is taken from is a perfect square: then every
# coefficient, the updated vector, onrm / nrm (one correctly rounded square root) and the normalised column are exact, and a numpy
# float64 run of the reference algorithm (bvorthog.c BVOrthogonalizeCGS1 / BVOrthogonalizeGS) gives the same bits.
def walsh64():
    H = np.array([[1.0]])
    while H.shape[0] < 64:
        H = np.block([[H, H], [H, -H]])
    return H


W64 = walsh64()


def rows_s(n):
    return np.r_[0:32, n - 32:n]


def rows_free(n):
    return np.array([32, n // 2, n - 33, n - 34])


def fit_square(q, unit):
    """y (a multiple of unit) with q + y^2 a perfect square of a multiple of unit; q must be a multiple of unit^2 that is not 2 mod 4."""
    N = int(round(q / unit ** 2))
    assert abs(N * unit ** 2 - q) == 0.0
    if N % 2:
        return (N - 1) // 2 * unit
    assert N % 4 == 0, N
    return (N // 4 - 1) * unit


def cgs_reference(VS, vS, rest, refine, with_norms_per_pass=None):
    """The reference's classical Gram-Schmidt on the compact form: VS (64 x k) the previous columns on the rows S, vS the vector there,
    rest its (fixed) part elsewhere. Returns the passes' (onrm, nrm), H, the final vS, nrm, lindep, passes."""
    v = vS.copy(); k = VS.shape[1]
    H = np.zeros(k)
    rr = float(rest @ rest)
    log = []

    def cgs1(norms):
        nonlocal v
        c = VS.T @ v
        vv = float(v @ v) + rr
        assert_exact((VS, v, 64), (v, v, 64 + 4))
        v = v - VS @ c
        H[:] += c
        if not norms:
            log.append((None, None))
            return None, None
        beta = math.sqrt(vv)
        assert beta * beta == vv, "the case must make v.v a perfect square"
        n2 = beta * beta - float(c @ c)
        nrm = math.sqrt(n2) if n2 > 0.0 else math.sqrt(float(v @ v) + rr)
        log.append((beta, nrm))
        return beta, nrm

    if refine == 0:                                    # IFNEEDED
        onrm, nrm = cgs1(True); passes = 1
        while passes < 3 and nrm != 0.0 and abs(nrm) < ETA * abs(onrm):
            passes += 1; onrm, nrm = cgs1(True)
        lindep = not (nrm != 0.0 and abs(nrm) >= ETA * abs(onrm))
    elif refine == 1:                                  # NEVER
        cgs1(False); passes = 1
        nrm = math.sqrt(float(v @ v) + rr); lindep = nrm == 0.0
    else:                                              # ALWAYS
        cgs1(False); onrm, nrm = cgs1(True); passes = 2
        lindep = not (nrm != 0.0 and abs(nrm) >= ETA * abs(onrm))
    return {"log": log, "H": H, "vS": v, "nrm": nrm, "lindep": lindep, "passes": passes}


def gs_case(rng, n, k, nc, refine, shape):
    """Previous columns (dense n x k, nc of them constraints) and a vector with a known Gram-Schmidt run. shape: "one" / "two" passes
    (orthonormal columns), "scaled" (d = 2 on some regular columns: the second pass has non-zero coefficients)."""
    S, F = rows_s(n), rows_free(n)
    d = np.ones(k)
    if shape == "scaled":
        d[nc:][np.arange(k - nc) % 3 == 2] = 2.0
    VS = W64[:, :k] * d / 8.0
    a = rng.integers(1, 4, size=k) * rng.choice([-1.0, 1.0], size=k)
    r = np.zeros(4)
    if shape == "two" and k >= 2:
        r[0] = 1.0                                     # |r|^2 = 1: the first pass leaves nrm = 1 against onrm >> 1
        q = float((VS[:, 1:] @ a[1:]) @ (VS[:, 1:] @ a[1:])) + 1.0
        if int(q) % 4 == 2:
            r[:] = 1.0; q += 3.0                       # |r|^2 = 4
        a[0] = fit_square(q, 1.0)              # |a|^2 + |r|^2 a perfect square (VS orthonormal here)
    else:
        r[1] = rng.integers(0, 3); r[2] = rng.integers(0, 2)
        vS = VS @ a
        if shape == "scaled" and refine == 2:
            # the norm is taken in the second pass: make the vector after the first pass have a square v.v
            v1 = vS - VS @ (VS.T @ vS)
            q = float(v1 @ v1) + float(r @ r)
        else:
            q = float(vS @ vS) + float(r @ r)
        if round(q * 64) % 4 == 2:
            r[3] = 0.125; q += 1.0 / 64.0
        r[0] = fit_square(q, 1.0 / 8.0)
    vS = VS @ a
    V = np.zeros((n, k)); V[S] = VS
    v = np.zeros(n); v[S] = vS; v[F] = r
    return V, v, VS, vS, r


def _gs_cases(big):
    """(n, k, nc) triples: every KT (k previous columns -> KT = ks_kt_for(k)), with and without constraints."""
    ks = KTS[:-1] + [63]
    out = []
    for i, k in enumerate(ks):
        nc = 3 if (i % 2 and k > 3) else 0
        n = [257, 100003, 513][i % 3] if not big else 4 ** 10
        out.append((n, k, nc))
    if big:
        out = [c for c in out if c[1] in (1, 2, 7, 13, 24, 31, 32, 33, 40, 41, 48, 56, 57, 63)]
    return out


def _run_gs_family(ctx, debug, vec1, refine, gs1, big):
    import slepc_amd as ks
    rng = np.random.default_rng(1000 + 100 * refine + 10 * vec1 + gs1 + 5 * big)
    shapes = {0: ["one", "two"], 1: ["scaled", "one"], 2: ["scaled", "two"]}[refine]
    seen = set()
    by_store = {}
    for idx, (n, k, nc) in enumerate(_gs_cases(big)):
        by_store.setdefault((n, nc), []).append((idx, k))
    for (n, nc), items in by_store.items():
        m = 64 - nc
        Cm = np.zeros((n, nc)); Cm[rows_s(n)] = W64[:, :nc] / 8.0
        St = Store(ctx, n, m, odd=vec1, nc_cols=Cm if nc else None)
        St.V.SetOrthogonalization(ks.CGS, refine, ETA)
        for idx, k in items:
            j = k - nc
            shape = shapes[idx % 2]
            V, v, VS, vS, r = gs_case(rng, n, k, nc, refine, shape)
            for c in range(-nc, j):
                St.put(c, V[:, c + nc])
            St.put(j, v)
            ref = cgs_reference(VS, vS, r, refine)
            if gs1:
                got_log, prof = _gs1_caller(ctx, St, j, refine)
                assert got_log == [(o, nr) for o, nr in ref["log"] if o is not None], (n, k, nc, refine, got_log, ref["log"])
                want = v.copy(); want[rows_s(n)] = ref["vS"]
                assert np.array_equal(St.get(j), want), (n, k, nc, refine, shape)
                Hb = St.V.buffer()[:, j]
                assert np.array_equal(Hb[:k], ref["H"]), (n, k, nc)
            else:
                ctx.prof_enable(True); ctx.prof_reset()
                if idx % 2:
                    nrm, lindep = St.V.OrthonormalizeColumn(j)
                    alpha = 1.0 / ref["nrm"] if ref["nrm"] not in (0.0, 1.0) else 1.0
                    want = v * alpha; want[rows_s(n)] = ref["vS"] * alpha
                else:
                    H, nrm, lindep = St.V.OrthogonalizeColumn(j)
                    want = v.copy(); want[rows_s(n)] = ref["vS"]
                ctx.synchronize(); prof = ctx.prof_get(by_variant=True); ctx.prof_enable(False)
                assert nrm == ref["nrm"] and lindep == ref["lindep"], (n, k, nc, refine, shape, nrm, ref["nrm"])
                assert St.V.gs_passes()[1] == ref["passes"], (n, k, nc, refine, shape, St.V.gs_passes(), ref["passes"])
                assert np.array_equal(St.get(j), want), (n, k, nc, refine, shape)
                if j > 0:
                    Hb = St.V.buffer()[:, j]
                    assert np.array_equal(Hb[:k], ref["H"]), (n, k, nc)
                    assert Hb[k] == (0.0 if ref["lindep"] else ref["nrm"])
            kt = kt_for(k)
            assert launched(prof, "gs_update_fused_dot", kt) + launched(prof, "gs_update", kt) >= 1, (k, sorted(prof.keys()))
            seen.add((shape, ref["passes"]))
        St.V.destroy()
    return seen


def _gs1_caller(ctx, St, j, refine):
    """BVOrthogonalizeColumn + BVOrthogonalizeGS on the caller's side of the ops->gramschmidt slot (as the SLEPc adapter drives it):
    BV_CleanCoefficients, then one GramSchmidtPass per pass of the refinement loop. Returns the passes' (onrm, nrm) and the profile."""
    V = St.V
    ldb = V.nc + V.m
    k = V.nc + j
    ctx.memset(V.buffer_ptr() + 8 * j * ldb, 0, 8 * k)
    ctx.prof_enable(True); ctx.prof_reset()
    log = []
    state = 100 + j
    V.SetState(state)
    if refine == 0:
        onrm, nrm = V.GramSchmidtPass(j); log.append((onrm, nrm)); passes = 1
        while passes < 3 and nrm != 0.0 and abs(nrm) < ETA * abs(onrm):
            passes += 1; V.SetState(state); onrm, nrm = V.GramSchmidtPass(j); log.append((onrm, nrm))
    elif refine == 1:
        V.GramSchmidtPass(j, False, False)
    else:
        V.GramSchmidtPass(j, False, False)
        V.SetState(state); onrm, nrm = V.GramSchmidtPass(j); log.append((onrm, nrm))
    ctx.synchronize(); prof = ctx.prof_get(by_variant=True); ctx.prof_enable(False)
    return log, prof


@pytest.mark.parametrize("refine", [0, 1, 2], ids=["ifneeded", "never", "always"])
@pytest.mark.parametrize("vec1", [False, True], ids=["vec2", "vec1"])
@pytest.mark.parametrize("gs1", [False, True], ids=["program", "slot"])
def test_gs_update_every_tile_exact(ctx, debug, refine, vec1, gs1):
    """k_gs_update<KT, VEC, GS1> for every KT, basis resident in the Infinity Cache (plain loads): OrthonormalizeColumn /
    OrthogonalizeColumn (GS1 false) and the GramSchmidtPass slot (GS1 true), with and without constraint columns."""
    seen = _run_gs_family(ctx, debug, vec1, refine, gs1, big=False)
    if refine == 0:
        assert ("one", 1) in seen and ("two", 2) in seen, seen


@pytest.mark.parametrize("refine", [0, 2], ids=["ifneeded", "always"])
@pytest.mark.parametrize("gs1", [False, True], ids=["program", "slot"])
def test_gs_update_streaming_loads_exact(ctx, debug, refine, gs1):
    """The same above 200 MB of basis storage (n = 4^10, 64 columns: 537 MB): the nontemporal-load forms of the update."""
    seen = _run_gs_family(ctx, debug, False, refine, gs1, big=True)
    if refine == 0:
        assert ("one", 1) in seen and ("two", 2) in seen, seen


# ---------------------------------------------------------------------------------------------------------------------------------
def banded_csr(n, offs, vals):
    """Rows with the entries vals at the column offsets offs (dropped at the borders): a dictionary matrix with len(offs) entries per row."""
    rp = [0]; cols = []; vv = []
    for i in range(n):
        for o, v in zip(offs, vals):
            if 0 <= i + o < n:
                cols.append(i + o); vv.append(v)
        rp.append(len(cols))
    return np.array(rp), np.array(cols), np.array(vv, dtype=np.float64)


@pytest.mark.parametrize("w", [8, 16])
def test_spmv_dot_dict_every_tile(ctx, debug, w):
    """k_dot_spmv_dict<KT, W> through BVMatLanczos for KT 2..64 (the Lanczos step j dots j + 1 columns), rows of 5 (W = 8) and 13 (W = 16)
    entries: the same bits as the separate launches (no_spmv_dot)."""
    import slepc_amd as ks
    n = 20011
    if w == 8:
        offs, vals = [-150, -1, 0, 1, 150], [-1.0, -1.0, 4.0, -1.0, -1.0]
    else:
        offs = [-300, -150, -6, -3, -2, -1, 0, 1, 2, 3, 6, 150, 300]
        vals = [-0.25, -1.0, -0.5, -0.25, -1.0, -1.0, 12.0, -1.0, -1.0, -0.25, -0.5, -1.0, -0.25]
    rp, cols, vv = banded_csr(n, offs, vals)
    m = 63
    outs = []
    for fused in (True, False):
        if not fused:
            debug("no_spmv_dot")
        A = ks.Mat.from_csr(ctx, rp, cols, vv)
        assert A.layout() == "dict"
        V = ks.BV(ctx, n, m + 1)
        V.SetRandomColumn(0)
        _, nrm, _ = V.OrthogonalizeColumn(0); V.ScaleColumn(0, 1.0 / nrm)
        T = np.zeros((m + 1, 3), order="F")
        r, prof = profiled(ctx, lambda: V.MatLanczos(A, T, 0, m))
        outs.append((T.copy(), V.dense(), r, prof))
        V.destroy(); A.destroy()
    assert outs[0][2][0] == m and not outs[0][2][2]
    for ncols in range(2, m + 2):
        assert launched(outs[0][3], "spmv_dot_fused", kt_for(ncols)) >= 1, (ncols, sorted(outs[0][3].keys()))
    assert outs[1][3].get(("spmv_dot_fused", 64), {}).get("launches", 0) == 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
