"""The restatement behind the smoothed-aggregation AMG tests (tests/test_amg_host.py on the host, tests/test_gpu_pc_amg.py on the GPU), their
matrices and the ctypes wrapper of the host hook (ksc_amg_plan of slepc_amd/csrc/ks_csr.cpp).

The set-up is restated level by level in numpy / scipy exactly as DESIGN section 25 words it: diagonal and Gershgorin bound, the symmetrised
strength graph with its weights, the three aggregation passes (plain loops, every one ascending), the tentative and the smoothed prolongator,
R = P^T and the Galerkin product. Patterns are structural - products of matrices of ones, which cannot cancel - and values are laid on them, so an
entry that happens to be 0.0 stays an entry, as in the library. `cycle` is the V(nu, nu) cycle with the Chebyshev smoother on a list of levels,
in any floating-point type: the GPU tests evaluate it on the hierarchy the library exports, once in float64 and once in longdouble."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from lu_cases import laplacian2d, laplacian3d  # noqa: F401  (shared matrices)

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LLP = C.POINTER(C.c_longlong)
LD = np.longdouble
AMG_NO_DIAGONAL, AMG_TOO_LARGE = 1, 2
MAX_LEVELS_CAP = 16


class ZeroDiagonal(Exception):
    def __init__(self, level, row):
        super().__init__("level %d, row %d" % (level, row))
        self.level, self.row = level, row


# ---- the set-up ------------------------------------------------------------------------------------------------------------------------
def summed(rp, col, val, n):
    """CSR arrays as the library reads them: rows sorted by column, repeated entries summed in stored order, explicit zeros kept."""
    orp, ocol, oval = [0], [], []
    for r in range(n):
        c = np.asarray(col[rp[r]:rp[r + 1]], dtype=np.int64); v = np.asarray(val[rp[r]:rp[r + 1]], dtype=np.float64)
        keep = (c >= 0) & (c < n); c, v = c[keep], v[keep]
        o = np.argsort(c, kind="stable")
        for ci, vi in zip(c[o], v[o]):
            if len(ocol) > orp[-1] and ocol[-1] == ci:
                oval[-1] = oval[-1] + vi
            else:
                ocol.append(int(ci)); oval.append(float(vi))
        orp.append(len(ocol))
    return _csr(np.array(oval, dtype=np.float64), np.array(ocol, dtype=np.int64), np.array(orp, dtype=np.int64), (n, n))


def _csr(data, indices, indptr, shape):
    M = sp.csr_matrix(shape, dtype=np.float64)
    M.data, M.indices, M.indptr = np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int32)
    return M


def ones_like(M):
    """The pattern of a CSR matrix as a matrix of ones (stored zeros included)."""
    M = sp.csr_matrix(M)
    return _csr(np.ones(M.indices.size), M.indices.copy(), M.indptr.copy(), M.shape)


def on_pattern(M, pat):
    """The values of M on the (sorted) pattern `pat`, 0.0 where M stores nothing."""
    pat = sp.csr_matrix(pat); pat.sort_indices()
    M = sp.csr_matrix(M)
    rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
    vals = np.asarray(M[rows, pat.indices]).ravel() if pat.indices.size else np.zeros(0)
    return _csr(vals, pat.indices.copy(), pat.indptr.copy(), pat.shape)


def stored_diagonal(A, level=0):
    """a_ii of a sorted CSR matrix; a row without a stored diagonal, or with a zero one, raises ZeroDiagonal."""
    n = A.shape[0]
    d = np.zeros(n)
    for i in range(n):
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]
        k = np.flatnonzero(c == i)
        if k.size == 0 or A.data[A.indptr[i] + k[0]] == 0.0:
            raise ZeroDiagonal(level, i)
        d[i] = A.data[A.indptr[i] + k[0]]
    return d


def strength(A, d, theta):
    """The symmetrised strength graph as a sorted CSR matrix of weights max(|a_ij|, |a_ji|)."""
    C_ = A.tocoo()
    r, c, v = C_.row, C_.col, C_.data
    m = (r != c) & (v != 0.0) & (np.abs(v) >= theta * np.sqrt(np.abs(d[r] * d[c])))
    S = sp.csr_matrix((np.abs(v[m]), (r[m], c[m])), shape=A.shape)
    W = S.maximum(S.T).tocsr(); W.sort_indices()
    return W


def aggregate(W):
    """The three passes on the weighted graph W: (aggregate of every node, -1 outside all of them; number of aggregates)."""
    n = W.shape[0]
    agg = np.full(n, -1, dtype=np.int64)
    nagg = 0
    nb = [W.indices[W.indptr[i]:W.indptr[i + 1]] for i in range(n)]
    for i in range(n):                                             # pass 1
        if nb[i].size and agg[i] < 0 and np.all(agg[nb[i]] < 0):
            agg[i] = nagg; agg[nb[i]] = nagg; nagg += 1
    after1 = agg.copy()
    for i in range(n):                                             # pass 2, judged on the state after pass 1
        if after1[i] >= 0 or nb[i].size == 0:
            continue
        w = W.data[W.indptr[i]:W.indptr[i + 1]]
        best = -1
        for k, j in enumerate(nb[i]):
            if after1[j] >= 0 and (best < 0 or w[k] > w[best]):
                best = k
        if best >= 0:
            agg[i] = after1[nb[i][best]]
    for i in range(n):                                             # pass 3
        if agg[i] < 0 and nb[i].size:
            agg[i] = nagg
            for j in nb[i]:
                if agg[j] < 0:
                    agg[j] = nagg
            nagg += 1
    return agg, nagg


def tentative(agg, nagg):
    n = agg.size
    inside = np.flatnonzero(agg >= 0)
    size = np.bincount(agg[inside], minlength=nagg)
    T = sp.csr_matrix((1.0 / np.sqrt(size[agg[inside]].astype(np.float64)), (inside, agg[inside])), shape=(n, nagg))
    T.sort_indices()
    return T


def hierarchy(A, theta=0.0, coarse_limit=200, max_levels=10, smooth=True, stall=0.8):
    """The levels as dicts: A, n, and on every level but the last d, rho, agg, nagg, T, P, R, and P_scale, Ac_scale: per entry of P and of the
    next level's operator the sum of the absolute products it is made of."""
    A = sp.csr_matrix(A); A.sort_indices()
    levels = []
    while True:
        n = A.shape[0]
        lev = {"A": A, "n": n, "rho": 0.0}
        levels.append(lev)
        if n <= coarse_limit or len(levels) >= max_levels:
            break
        d = stored_diagonal(A, len(levels) - 1)
        rho = float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(d)))
        agg, nagg = aggregate(strength(A, d, theta))
        if nagg == 0 or nagg > stall * n:
            break
        T = tentative(agg, nagg)
        if smooth:
            pat = ones_like(A) @ ones_like(T) + ones_like(T)
            P = on_pattern(T - sp.diags([(4.0 / (3.0 * rho)) / d], [0]) @ (A @ T), pat)
        else:
            P = T
        R = P.T.tocsr(); R.sort_indices()
        AP = on_pattern(A @ P, ones_like(A) @ ones_like(P))
        Ac = on_pattern(R @ AP, ones_like(R) @ ones_like(AP))
        # what an entry's rounding error is relative to: the sum of the absolute values of the products it is made of (equal to the entry where nothing cancels)
        P_scale = on_pattern(abs(T) + sp.diags([(4.0 / (3.0 * rho)) / np.abs(d)], [0]) @ (abs(A) @ abs(T)), P) if smooth else abs(T)
        Ac_scale = on_pattern(abs(R) @ (abs(A) @ abs(P)), Ac)
        lev.update(d=d, rho=rho, agg=agg, nagg=nagg, T=T, P=P, R=R, P_scale=P_scale, Ac_scale=Ac_scale)
        A = Ac
    return levels


# ---- the cycle -------------------------------------------------------------------------------------------------------------------------
def mv(S, x, dtype):
    """S x in `dtype` (rows may be empty)."""
    S = sp.csr_matrix(S)
    out = np.zeros(S.shape[0], dtype=dtype)
    if S.indices.size:
        prod = S.data.astype(dtype) * np.asarray(x, dtype=dtype)[S.indices]
        nz = np.flatnonzero(np.diff(S.indptr) > 0)
        out[nz] = np.add.reduceat(prod, S.indptr[:-1][nz])
    return out


def dense_solve(A, b, dtype):
    """Gaussian elimination with partial pivoting in `dtype` (the coarsest level: a handful of rows)."""
    M = np.array(sp.csr_matrix(A).toarray(), dtype=dtype); x = np.array(b, dtype=dtype)
    n = M.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]; x[[k, p]] = x[[p, k]]
        for i in range(k + 1, n):
            f = M[i, k] / M[k, k]
            if f != 0:
                M[i, k:] = M[i, k:] - f * M[k, k:]; x[i] = x[i] - f * x[k]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - M[i, i + 1:] @ x[i + 1:]) / M[i, i]
    return x


def chebyshev(A, dinv, rho, b, x, degree, dtype):
    """`degree` steps of Chebyshev on D^-1 A over [0.1 rho, rho]; x None: the zero initial guess (no product in the first step)."""
    one = dtype(1.0)
    lo, hi = dtype(0.1) * dtype(rho), dtype(rho)
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    sigma = theta / delta
    rk = one / sigma
    d = None
    for k in range(degree):
        r = b if x is None else b - mv(A, x, dtype)
        z = dinv * r
        if k == 0:
            d = z / theta
        else:
            rn = one / (2 * sigma - rk)
            d = rn * rk * d + (2 * rn / delta) * z
            rk = rn
        x = d.copy() if x is None else x + d
    return x


def cycle(levels, b, degree=2, dtype=np.float64, l=0):
    """y = M^-1 b: the V(degree, degree) cycle on `levels` (dicts with A and, but for the last, d, rho, P)."""
    lev = levels[l]
    b = np.asarray(b, dtype=dtype)
    if l == len(levels) - 1:
        return dense_solve(lev["A"], b, dtype)
    dinv = dtype(1.0) / lev["d"].astype(dtype)
    x = chebyshev(lev["A"], dinv, lev["rho"], b, None, degree, dtype)
    rc = mv(lev["P"].T.tocsr(), b - mv(lev["A"], x, dtype), dtype)
    x = x + mv(lev["P"], cycle(levels, rc, degree, dtype, l + 1), dtype)
    return chebyshev(lev["A"], dinv, lev["rho"], b, x, degree, dtype)


def pcg_iterations(A, apply_m, b, rtol=1e-8, max_it=1000):
    """Preconditioned CG iterations to ||r|| <= rtol ||b||."""
    x = np.zeros_like(b); r = b.copy(); z = apply_m(r); p = z.copy(); rz = r @ z
    for it in range(1, max_it + 1):
        Ap = A @ p
        a = rz / (p @ Ap)
        x += a * p; r -= a * Ap
        if np.linalg.norm(r) <= rtol * np.linalg.norm(b):
            return it
        z = apply_m(r); rz_new = r @ z
        p = z + (rz_new / rz) * p; rz = rz_new
    return max_it


def gmres_iterations(A, apply_m, b, rtol=1e-8, restart=30, max_it=3000):
    """Left-preconditioned GMRES(restart) with modified Gram-Schmidt: iterations until the preconditioned residual is <= rtol times its start."""
    n = b.size
    x = np.zeros(n)
    r = apply_m(b)
    beta0 = np.linalg.norm(r); tol = rtol * beta0
    its = 0
    while its < max_it:
        beta = np.linalg.norm(r)
        if beta <= tol:
            return its
        V = np.zeros((n, restart + 1)); H = np.zeros((restart + 1, restart)); V[:, 0] = r / beta
        g = np.zeros(restart + 1); g[0] = beta
        for j in range(restart):
            w = apply_m(A @ V[:, j])
            for i in range(j + 1):
                H[i, j] = V[:, i] @ w; w = w - H[i, j] * V[:, i]
            H[j + 1, j] = np.linalg.norm(w)
            if H[j + 1, j] != 0.0:
                V[:, j + 1] = w / H[j + 1, j]
            its += 1
            y, *_ = np.linalg.lstsq(H[:j + 2, :j + 1], g[:j + 2], rcond=None)
            res = np.linalg.norm(H[:j + 2, :j + 1] @ y - g[:j + 2])
            if res <= tol or its >= max_it:
                break
        x = x + V[:, :j + 1] @ y
        if res <= tol:
            return its
        r = apply_m(b - A @ x)
    return its


# ---- matrices --------------------------------------------------------------------------------------------------------------------------
def _t(k):
    return sp.diags([np.full(k - 1, -1.0), np.full(k, 2.0), np.full(k - 1, -1.0)], [-1, 0, 1])


def grid2d(nx, ny):
    """The 5-point Laplacian on ny lines of nx points (x fastest)."""
    return laplacian2d(ny, nx)


def laplacian2d_eigenvalues(nx, ny):
    tx = 2.0 - 2.0 * np.cos(np.arange(1, nx + 1) * np.pi / (nx + 1)); ty = 2.0 - 2.0 * np.cos(np.arange(1, ny + 1) * np.pi / (ny + 1))
    return np.sort((ty[:, None] + tx[None, :]).ravel())


def laplacian3d_eigenvalues(m):
    t = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
    return np.sort((t[:, None, None] + t[None, :, None] + t[None, None, :]).ravel())


def anisotropic(m=40, eps=0.01):
    """kron(I, T) + eps kron(T, I): strong coupling along a grid line (consecutive indices), weak across the lines."""
    A = (sp.kron(sp.identity(m), _t(m)) + eps * sp.kron(_t(m), sp.identity(m))).tocsr(); A.sort_indices()
    return A


def upwind(m=40, wind=(8.0, 3.0)):
    """Convection-diffusion on m x m, first-order upwind convection: non-symmetric, an M-matrix."""
    I = sp.identity(m)
    U = sp.diags([np.full(m - 1, -1.0), np.full(m, 1.0)], [-1, 0])
    A = (sp.kron(I, _t(m)) + sp.kron(_t(m), I) + (wind[0] / m) * sp.kron(I, U) + (wind[1] / m) * sp.kron(U, I)).tocsr(); A.sort_indices()
    return A


def blocks_with_isolated_rows(nx=17, ny=9, iso=5):
    """Two grids on the diagonal with `iso` identity rows between them."""
    G = grid2d(nx, ny)
    A = sp.block_diag([G, 3.0 * sp.identity(iso), G]).tocsr(); A.sort_indices()
    return A


def random_scrambled(n=60, seed=5):
    """A random unsymmetric pattern as CSR arrays with unsorted columns and repeated entries; values are multiples of 1/4, some repeated pairs cancel."""
    rng = np.random.default_rng(seed)
    rp, col, val = [0], [], []
    for r in range(n):
        off = rng.choice(np.delete(np.arange(n), r), size=4, replace=False)
        c = np.concatenate([off, off[:2], [r, r]])
        v = np.concatenate([-rng.integers(1, 5, 4) / 4.0, -rng.integers(1, 5, 2) / 4.0, [5.0, 1.5]])
        if r % 7 == 3:
            v[4] = -v[0]                                           # the two entries of column off[0] sum to 0.0: stored, but no edge
        o = rng.permutation(c.size)
        col.extend(c[o]); val.extend(v[o]); rp.append(len(col))
    return np.array(rp, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val)


def arrays(S):
    S = sp.csr_matrix(S)
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)


# ---- the host hook ---------------------------------------------------------------------------------------------------------------------
def load(path=None):
    import slepc_amd._lib as L
    lib = C.CDLL(path or os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_amg_plan.argtypes = [C.c_int, IP, IP, DP, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, LLP, DP, C.c_int, IP, IP, DP, IP, IP, DP, IP]
    lib.ksc_amg_plan.restype = C.c_int
    return lib


def _i(a):
    return None if a is None else a.ctypes.data_as(IP)


def _d(a):
    return None if a is None else a.ctypes.data_as(DP)


def plan(lib, arr, theta=0.0, coarse_limit=200, max_levels=10, smooth=True, stall=0.8):
    """The library's hierarchy as a list of dicts like `hierarchy`'s (A, n, rho; d, agg, nagg, P but for the last level), or (status, level, row)."""
    rp, col, val = (np.ascontiguousarray(a, dtype=t) for a, t in zip(arr, (np.int32, np.int32, np.float64)))
    n = len(rp) - 1
    info = np.zeros(4 + 4 * MAX_LEVELS_CAP, dtype=np.int64); rho = np.zeros(MAX_LEVELS_CAP)
    args = (n, _i(rp), _i(col), _d(val), theta, coarse_limit, max_levels, int(smooth), stall, info.ctypes.data_as(LLP), _d(rho))
    st = lib.ksc_amg_plan(*args, -1, *([None] * 7))
    if st:
        return int(info[0]), int(info[2]), int(info[1])
    out = []
    for l in range(int(info[3])):
        nl, za, zp, na = (int(v) for v in info[4 + 4 * l:8 + 4 * l])
        arp = np.zeros(nl + 1, np.int32); acol = np.zeros(max(za, 1), np.int32); aval = np.zeros(max(za, 1))
        prp = np.zeros(nl + 1, np.int32); pcol = np.zeros(max(zp, 1), np.int32); pval = np.zeros(max(zp, 1))
        agg = np.zeros(max(nl, 1), np.int32)
        assert lib.ksc_amg_plan(*args, l, _i(arp), _i(acol), _d(aval), _i(prp), _i(pcol), _d(pval), _i(agg)) == 0
        lev = {"A": _csr(aval[:za], acol[:za], arp, (nl, nl)), "n": nl, "rho": float(rho[l])}
        if l + 1 < int(info[3]):
            lev.update(P=_csr(pval[:zp], pcol[:zp], prp, (nl, na)), agg=agg[:nl].astype(np.int64), nagg=na, d=lev["A"].diagonal())
        out.append(lev)
    return out
