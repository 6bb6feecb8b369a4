"""The reference of the sparse LU tests (tests/test_lu_host.py on the host, tests/test_gpu_pc_lu.py on the GPU), their matrices and the ctypes
wrappers of the host hooks (ksc_lu_ordering, ksc_lu_plan of slepc_amd/csrc/ks_csr.cpp).

The reference is Gaussian elimination in IKJ order without pivoting on P[perm][:, perm], perm being the library's own permutation: for every
k < i ascending l_ik = a_ik / u_kk, then a_ij = a_ij - l_ik u_kj, one rounding per operation. `dense_lu` does that on a dense array, every k;
`lu_nopivot` skips the k with a_ik == 0 (an update with l_ik = 0 changes nothing) so that it can be used at a few thousand rows. With L, U of the
reference and Q the permutation, y = PCApply(x) must satisfy, componentwise,

    |L U (Q y) - Q x| <= 8 (k + 1) 2^-53 |L| |U| |Q y|            k = the longest row of L + U

- the backward error of two substitutions (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5) plus the rounding of the factors
(Thm 9.3), as tests/ilu_cases.py derives it. The transposed solve substitutes with the columns of the factors, so its k is the larger of the
longest row and the longest column: |U^T L^T (Q y) - Q x| <= 8 (k + 1) 2^-53 |U^T| |L^T| |Q y|. The left sides are evaluated in longdouble."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from ilu_cases import LD, U53, _mv, arrays, line_pencil, shifted  # noqa: F401  (shared with the ILU tests)

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LLP = C.POINTER(C.c_longlong)
ND, NATURAL = 0, 1
LU_ZERO_PIVOT = 1


# ---- reference -------------------------------------------------------------------------------------------------------------------------
def summed(rp, col, val, n=None):
    """The matrix of CSR arrays as the library reads it: rows sorted by column, repeated entries summed in stored order. Dense (n x n)."""
    n = len(rp) - 1 if n is None else n
    P = np.zeros((n, n))
    for r in range(n):
        c = np.asarray(col[rp[r]:rp[r + 1]]); v = np.asarray(val[rp[r]:rp[r + 1]], dtype=np.float64)
        o = np.argsort(c, kind="stable")
        first = np.ones(n, dtype=bool)
        for ci, vi in zip(c[o], v[o]):
            P[r, ci] = vi if first[ci] else P[r, ci] + vi
            first[ci] = False
    return P


def dense_lu(P):
    """IKJ elimination without pivoting on a dense array, every k < i: (L unit lower, U) dense. Raises ZeroDivisionError-free: a zero pivot gives inf/nan."""
    A = np.array(P, dtype=np.float64)
    n = A.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            for k in range(i):
                l = A[i, k] / A[k, k]
                A[i, k] = l
                A[i, k + 1:] = A[i, k + 1:] - l * A[k, k + 1:]
    return np.tril(A, -1) + np.eye(n), np.triu(A)


def lu_nopivot(Pp):
    """The same elimination on a sparse matrix (already permuted), skipping the k with a_ik == 0: (L strict lower part, U with the diagonal) as scipy CSR."""
    Pp = sp.csr_matrix(Pp); Pp.sort_indices()
    n = Pp.shape[0]
    urows, lrows = [], []
    w = np.zeros(n)
    for i in range(n):
        w[:] = 0.0
        w[Pp.indices[Pp.indptr[i]:Pp.indptr[i + 1]]] = Pp.data[Pp.indptr[i]:Pp.indptr[i + 1]]
        k = -1
        while True:
            nz = np.flatnonzero(w[k + 1:i])
            if nz.size == 0:
                break
            k = k + 1 + int(nz[0])
            uc, uv = urows[k]
            l = w[k] / uv[0]
            w[k] = l
            w[uc[1:]] = w[uc[1:]] - l * uv[1:]
        lc = np.flatnonzero(w[:i]); uc = i + np.flatnonzero(w[i:])
        if uc.size == 0 or uc[0] != i:
            uc = np.concatenate([[i], uc])
        lrows.append((lc, w[lc].copy())); urows.append((uc, w[uc].copy()))

    def csr(rows):
        ind = np.concatenate([[0], np.cumsum([c.size for c, _ in rows])])
        return sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]).astype(np.int64), ind), shape=(n, n))
    return csr(lrows), csr(urows)


class Reference:
    """Reference factors of P (scipy sparse, entries already summed) under the permutation `perm` (perm[i] = the original row eliminated i-th)."""

    def __init__(self, P, perm):
        P = sp.csr_matrix(P)
        self.n = P.shape[0]
        self.perm = np.asarray(perm, dtype=np.int64)
        assert np.array_equal(np.sort(self.perm), np.arange(self.n)), "not a permutation"
        Ls, self.U = lu_nopivot(P[self.perm][:, self.perm])
        self.L = (Ls + sp.identity(self.n)).tocsr()
        rows = np.diff(Ls.indptr) + np.diff(self.U.indptr)
        cols = np.diff(Ls.tocsc().indptr) + np.diff(self.U.tocsc().indptr)
        self.k = int(rows.max()) if self.n else 0
        self.kt = max(self.k, int(cols.max()) if self.n else 0)
        self.Lt = self.L.T.tocsr(); self.Ut = self.U.T.tocsr()

    def ratio(self, x, y, transpose=False):
        """max over the rows of |L U Qy - Qx| / bound (0/0 counts as 0: an exact row)."""
        qy = np.asarray(y)[self.perm]; qx = np.asarray(x)[self.perm].astype(LD)
        first, second, k = (self.Ut, self.Lt, self.kt) if transpose else (self.L, self.U, self.k)
        res = np.abs(_mv(first, _mv(second, qy)) - qx)
        bound = 8.0 * (k + 1) * U53 * _mv(abs(first), _mv(abs(second), np.abs(qy)))
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(res == 0, 0.0, res / bound)
        return float(np.max(q)) if self.n else 0.0

    def check(self, x, y, what="", transpose=False):
        assert np.all(np.isfinite(y)), what
        r = self.ratio(x, y, transpose)
        print("%s%s: largest |LU Qy - Qx| / bound %.3g (n %d, k %d)" % (what, " (transposed)" if transpose else "", r, self.n, self.kt if transpose else self.k))
        assert r <= 1.0, (what, r)
        return r


def levels_and_stages(T, lower, wide):
    """Level sets of a strict triangle (scipy CSR) as section 17 of DESIGN defines them, and their cut into stages: (rows in level order, level starts,
    [(first level, levels, wide)])."""
    T = sp.csr_matrix(T); n = T.shape[0]
    level = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = T.indices[T.indptr[i]:T.indptr[i + 1]]
        level[i] = level[c].max() + 1 if c.size else 0
    nlev = int(level.max()) + 1 if n else 0
    order = np.argsort(level, kind="stable")                      # ascending row inside a level
    starts = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=nlev))]) if n else np.zeros(1, dtype=np.int64)
    stages = []
    for l in range(nlev):
        w = int(starts[l + 1] - starts[l] >= wide)
        if stages and stages[-1][2] == w:
            stages[-1][1] += 1
        else:
            stages.append([l, 1, w])
    return order, starts, [tuple(s) for s in stages]


def launches(stages):
    """(wide launches, narrow launches) of a stage list: a wide stage launches once per level, a narrow one once."""
    return sum(s[1] for s in stages if s[2]), sum(1 for s in stages if not s[2])


# ---- matrices --------------------------------------------------------------------------------------------------------------------------
def laplacian2d(m, mx=None):
    mx = m if mx is None else mx
    T = lambda k: sp.diags([np.full(k - 1, -1.0), np.full(k, 2.0), np.full(k - 1, -1.0)], [-1, 0, 1])
    A = (sp.kron(sp.identity(m), T(mx)) + sp.kron(T(m), sp.identity(mx))).tocsr(); A.sort_indices()
    return A


def laplacian2d_eigenvalues(m):
    t = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
    return np.sort((t[:, None] + t[None, :]).ravel())


def laplacian3d(m):
    T = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1]); I = sp.identity(m)
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr(); A.sort_indices()
    return A


def tridiagonal(n):
    A = sp.diags([np.full(n - 1, -1.0 + 0.1 * np.sin(np.arange(n - 1))), np.full(n, 2.5), np.full(n - 1, -0.8)], [-1, 0, 1]).tocsr(); A.sort_indices()
    return A


def arrow_last_row(m, seed=11):
    """The identity of order m + 1 whose last row is coupled to all m others, diagonally dominant: one row of m entries in L."""
    rng = np.random.default_rng(seed)
    S = sp.lil_matrix((m + 1, m + 1))
    S.setdiag(1.0 + rng.uniform(0.0, 1.0, m + 1))
    if m:
        v = rng.uniform(-1.0, 1.0, m); v[v == 0.0] = 0.5
        S[m, :m] = v
        S[m, m] = 1.0 + np.abs(v).sum()
    A = S.tocsr(); A.sort_indices()
    return A


def pairs(m, seed=12):
    """m independent 2 x 2 blocks [[d, 0], [c, d']]: under the natural ordering L has two levels of m rows each."""
    rng = np.random.default_rng(seed)
    n = 2 * m
    r = np.arange(1, n, 2)
    A = (sp.diags([2.0 + rng.uniform(0.0, 1.0, n)], [0]) + sp.csr_matrix((rng.uniform(0.25, 1.0, m), (r, r - 1)), shape=(n, n))).tocsr(); A.sort_indices()
    return A


def wide_narrow_wide(w, chain=5, seed=13):
    """w pairs, a chain of `chain` rows each coupled to the one before, then w rows coupled to the end of the chain. Natural ordering, L: levels 0 and 1
    hold w + 1 rows each (wide), levels 2 .. chain - 1 one chain row each (narrow), level `chain` the w last rows (wide)."""
    rng = np.random.default_rng(seed)
    n = 2 * w + chain + w
    rows = list(range(1, 2 * w, 2)); cols = [r - 1 for r in rows]
    c0 = 2 * w
    rows += list(range(c0 + 1, c0 + chain)); cols += list(range(c0, c0 + chain - 1))
    rows += list(range(c0 + chain, n)); cols += [c0 + chain - 1] * w
    A = (sp.diags([2.0 + rng.uniform(0.0, 1.0, n)], [0]) + sp.csr_matrix((rng.uniform(0.25, 1.0, len(rows)), (rows, cols)), shape=(n, n))).tocsr(); A.sort_indices()
    return A


def random_unsymmetric(n, per_row, seed):
    """A random unsymmetric pattern, strictly diagonally dominant by rows."""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=min(1.0, per_row / n), random_state=rng, format="csr", data_rvs=lambda k: rng.uniform(-1, 1, k))
    S.setdiag(0.0); S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 1.0 + rng.uniform(0.0, 1.0, n)
    A = (S + sp.diags([d], [0])).tocsr(); A.sort_indices()
    return A


def scrambled(n, seed=14):
    """CSR arrays with unsorted columns and repeated entries (the diagonal among them); values are small multiples of 1/4."""
    rng = np.random.default_rng(seed)
    rp, col, val = [0], [], []
    for r in range(n):
        off = rng.choice(np.delete(np.arange(n), r), size=min(n - 1, 4), replace=False)
        c = np.concatenate([off, off[:2], [r, r, r]])
        v = np.concatenate([rng.integers(1, 4, off.size + 2) / 4.0, [6.0, 2.5, 1.25]])
        o = rng.permutation(c.size)
        col.extend(c[o]); val.extend(v[o]); rp.append(len(col))
    return np.array(rp, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val)


def fill_makes_the_diagonal(n=12):
    """Row n - 1 stores no diagonal entry; the elimination of its entry in column 0 with row 0's entry in column n - 1 makes it non-zero."""
    S = sp.lil_matrix((n, n))
    S.setdiag(3.0 + 0.25 * np.arange(n))
    S[n - 1, n - 1] = 0.0
    S[0, n - 1] = 1.5; S[n - 1, 0] = -0.75; S[3, 2] = 0.5; S[2, 5] = -0.25
    A = S.tocsr(); A.eliminate_zeros(); A.sort_indices()
    assert A[n - 1, n - 1] == 0.0 and (n - 1) not in A.indices[A.indptr[n - 1]:A.indptr[n]]
    return A


def symmetric_indefinite(m=14, sigma=1.7):
    """The 2-D Laplacian shifted into its spectrum."""
    return shifted(laplacian2d(m), sigma)


# ---- host hooks ------------------------------------------------------------------------------------------------------------------------
def load(path=None):
    import slepc_amd._lib as L
    lib = C.CDLL(path or os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_lu_ordering.argtypes = [C.c_int, IP, IP, C.c_int, IP]
    lib.ksc_lu_ordering.restype = None
    lib.ksc_lu_plan.argtypes = [C.c_int, IP, IP, DP, C.c_int, C.c_int, LLP, IP, IP, IP, DP, IP, IP, DP, IP, IP, IP, DP, IP, IP, DP, IP, DP, DP, DP]
    lib.ksc_lu_plan.restype = C.c_int
    return lib


def _i(a):
    return None if a is None else a.ctypes.data_as(IP)


def _d(a):
    return None if a is None else a.ctypes.data_as(DP)


def ordering(lib, arr, which):
    rp, col, _ = arr
    n = len(rp) - 1
    perm = np.full(max(n, 1), -1, dtype=np.int32)
    lib.ksc_lu_ordering(n, _i(np.ascontiguousarray(rp, dtype=np.int32)), _i(np.ascontiguousarray(col, dtype=np.int32)), which, _i(perm))
    return perm[:n]


def plan(lib, arr, which, wide, x=None):
    """The plan as a dict, or (status, bad_row) when the factorisation stops."""
    rp, col, val = (np.ascontiguousarray(a, dtype=t) for a, t in zip(arr, (np.int32, np.int32, np.float64)))
    n = len(rp) - 1
    info = np.zeros(16, dtype=np.int64)
    none = [None] * 15
    st = lib.ksc_lu_plan(n, _i(rp), _i(col), _d(val), which, wide, info.ctypes.data_as(LLP), *none, None, None, None)
    if st:
        return int(info[0]), int(info[1])
    nl, nu, ent, nlev, nst = int(info[2]), int(info[3]), int(info[11]), int(info[4] + info[5]), int(info[6] + info[7])
    o = {"perm": np.zeros(max(n, 1), np.int32), "lrp": np.zeros(n + 1, np.int32), "lcol": np.zeros(max(nl, 1), np.int32), "lval": np.zeros(max(nl, 1)),
         "urp": np.zeros(n + 1, np.int32), "ucol": np.zeros(max(nu, 1), np.int32), "uval": np.zeros(max(nu, 1)),
         "rows": np.zeros(max(2 * n, 1), np.int32), "rp": np.zeros(2 * n + 1, np.int32), "col": np.zeros(max(ent, 1), np.int32), "val": np.zeros(max(ent, 1)),
         "lev": np.zeros(nlev + 1, np.int32), "lanes": np.zeros(max(nlev, 1), np.int32), "dinv": np.zeros(max(n, 1)), "stages": np.zeros(max(3 * nst, 1), np.int32)}
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    yf = None if x is None else np.full(max(n, 1), np.nan); yt = None if x is None else np.full(max(n, 1), np.nan)
    st = lib.ksc_lu_plan(n, _i(rp), _i(col), _d(val), which, wide, info.ctypes.data_as(LLP), _i(o["perm"]), _i(o["lrp"]), _i(o["lcol"]), _d(o["lval"]),
                         _i(o["urp"]), _i(o["ucol"]), _d(o["uval"]), _i(o["rows"]), _i(o["rp"]), _i(o["col"]), _d(o["val"]), _i(o["lev"]), _i(o["lanes"]),
                         _d(o["dinv"]), _i(o["stages"]), _d(xx), _d(yf), _d(yt))
    assert st == 0
    o["perm"] = o["perm"][:n]; o["rows"] = o["rows"][:2 * n]; o["lanes"] = o["lanes"][:nlev]; o["dinv"] = o["dinv"][:n]
    o["stages"] = [tuple(int(v) for v in o["stages"][3 * s:3 * s + 3]) for s in range(nst)]
    o["L"] = sp.csr_matrix((o["lval"][:nl], o["lcol"][:nl], o["lrp"]), shape=(n, n))
    o["U"] = sp.csr_matrix((o["uval"][:nu], o["ucol"][:nu], o["urp"]), shape=(n, n))
    o.update(n=n, nnz_l=nl, nnz_u=nu, levels=(int(info[4]), int(info[5])), nstage=(int(info[6]), int(info[7])), neg=int(info[8]), pos=int(info[9]),
             longest_row=int(info[10]), levels_t=(int(info[12]), int(info[13])), nstage_t=(int(info[14]), int(info[15])),
             y=None if x is None else yf[:n], yt=None if x is None else yt[:n])
    return o
