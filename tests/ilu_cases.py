"""The reference of the ILU(0) block-Jacobi tests (tests/test_gpu_pc_ilu.py on the GPU, tests/test_ilu_host.py on the host) and their matrices.

The reference is a plain numpy ILU(0) of every diagonal block, with the library's pattern rule (the entries a row stores inside its block, sorted,
repeated entries summed in stored order, explicit zeros kept) and its order (IKJ: l_ik = a_ik / u_kk, then a_ij -= l_ik u_kj for the j > k of row k
that row i stores; one rounding per operation, no fused multiply-add). With M = L U of that reference, y = PCApply(x) must satisfy, componentwise,

    |M y - x| <= 8 (k + 1) 2^-53 (|L| |U| |y|)            k = the longest row of the block

- the backward error of two substitutions (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5) plus the rounding of the factors
themselves (Thm 9.3); the 8 covers the three sources and the reciprocal of the pivots. The left side is evaluated in extended precision, so that
its own rounding (which is of the size of the bound in double) stays out of the comparison."""
import numpy as np
import scipy.sparse as sp

U53 = 2.0 ** -53
LD = np.longdouble


def block_rows(rp, col, val, c0, b0, bl):
    """Rows b0 .. b0 + bl - 1 of the CSR arrays, the columns c0 + b0 .. c0 + b0 + bl - 1 only, as sorted block-local (cols, vals) per row."""
    out = []
    for r in range(b0, b0 + bl):
        c = np.asarray(col[rp[r]:rp[r + 1]], dtype=np.int64) - (c0 + b0); v = np.asarray(val[rp[r]:rp[r + 1]], dtype=np.float64)
        keep = (c >= 0) & (c < bl)
        c, v = c[keep], v[keep]
        o = np.argsort(c, kind="stable")
        c, v = c[o], v[o]
        if c.size and np.any(c[1:] == c[:-1]):
            cc, vv = [], []
            for ci, vi in zip(c, v):
                if cc and cc[-1] == ci:
                    vv[-1] = vv[-1] + vi
                else:
                    cc.append(ci); vv.append(vi)
            c, v = np.array(cc, dtype=np.int64), np.array(vv)
        out.append((c, v.copy()))
    return out


class MissingDiagonal(Exception):
    pass


class ZeroPivot(Exception):
    pass


def ilu0(rows):
    """ILU(0) in IKJ order of a block given as sorted rows; returns (L, U) as scipy CSR: L unit lower triangular, U with the diagonal."""
    bl = len(rows)
    diag = np.empty(bl, dtype=np.int64)
    for i, (c, v) in enumerate(rows):
        d = np.flatnonzero(c == i)
        if d.size == 0:
            raise MissingDiagonal(i)
        diag[i] = d[0]
    pos = np.full(bl, -1, dtype=np.int64)
    for i, (c, v) in enumerate(rows):
        pos[c] = np.arange(c.size)
        for p in range(diag[i]):
            k = c[p]
            ck, vk = rows[k]
            l = v[p] / vk[diag[k]]
            v[p] = l
            t = pos[ck[diag[k] + 1:]]
            m = t >= 0
            v[t[m]] = v[t[m]] - l * vk[diag[k] + 1:][m]
        pos[c] = -1
        if v[diag[i]] == 0.0:
            raise ZeroPivot(i)
    ind = np.concatenate([[0], np.cumsum([c.size for c, _ in rows])])
    allc = np.concatenate([c for c, _ in rows]); allv = np.concatenate([v for _, v in rows])
    F = sp.csr_matrix((allv, allc, ind), shape=(bl, bl))
    rr = np.repeat(np.arange(bl), np.diff(ind))
    lower = allc < rr
    L = sp.csr_matrix((np.concatenate([allv[lower], np.ones(bl)]), (np.concatenate([rr[lower], np.arange(bl)]), np.concatenate([allc[lower], np.arange(bl)]))), shape=(bl, bl))
    U = sp.csr_matrix((allv[~lower], (rr[~lower], allc[~lower])), shape=(bl, bl))
    L.sort_indices(); U.sort_indices()
    return L, U, F


class Reference:
    """The blocks' reference factors of P given by CSR arrays (global columns, this rank's rows start at column c0)."""

    def __init__(self, rp, col, val, bs, c0=0):
        n = len(rp) - 1
        self.n, self.bs, self.blocks = n, bs, []
        for b0 in range(0, n, bs):
            bl = min(bs, n - b0)
            rows = block_rows(rp, col, val, c0, b0, bl)
            k = max(c.size for c, _ in rows)
            P = sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]), np.concatenate([[0], np.cumsum([c.size for c, _ in rows])])), shape=(bl, bl))
            L, U, F = ilu0(rows)
            self.blocks.append((b0, bl, L, U, k, P, F))

    @classmethod
    def of(cls, P, bs, c0=0):
        P = P.tocsr()
        return cls(P.indptr, P.indices, P.data, bs, c0)

    def solve(self, x):
        """M^-1 x in double (for the iteration-count restatement on the CPU, not for the bound)."""
        import scipy.sparse.linalg as spl
        y = np.empty(self.n)
        for b0, bl, L, U, *_ in self.blocks:
            y[b0:b0 + bl] = spl.spsolve_triangular(U, spl.spsolve_triangular(L, x[b0:b0 + bl], lower=True, unit_diagonal=True), lower=False)
        return y

    def ratios(self, x, y):
        """max over the rows of |M y - x| / (8 (k + 1) u |L||U||y|), one figure per block (0/0 counts as 0: an exact row)."""
        out = []
        for b0, bl, L, U, k, *_ in self.blocks:
            yb = y[b0:b0 + bl]
            res = np.abs(_mv(L, _mv(U, yb)) - x[b0:b0 + bl].astype(LD))
            bound = 8.0 * (k + 1) * U53 * _mv(abs(L), _mv(abs(U), np.abs(yb)))
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(res == 0, 0.0, res / bound)
            out.append(float(np.max(q)))
        return out

    def check(self, x, y, what=""):
        assert np.all(np.isfinite(y)), what
        r = self.ratios(x, y)
        print("%s: largest |My - x| / bound per block: max %.3g over %d blocks" % (what, max(r), len(r)))
        assert max(r) <= 1.0, (what, r)
        return max(r)


def _mv(S, x):
    """S x with extended-precision products and sums (every row of S stores at least its diagonal)."""
    S = S.tocsr()
    prod = S.data.astype(LD) * np.asarray(x, dtype=LD)[S.indices]
    return np.add.reduceat(prod, S.indptr[:-1])


# ---- matrices: each returns A (scipy CSR, sorted) with a strictly diagonally dominant A - sigma I for the sigma it names ---------------------------
SIGMA = -1.5


def _dominant(S, rng=None):
    """S with its diagonal replaced by 1 + the row's absolute off-diagonal sum + sigma: A - sigma I is strictly diagonally dominant."""
    S = sp.csr_matrix(S); S.setdiag(0.0); S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 1.0 + SIGMA
    if rng is not None:
        d = d + rng.uniform(0.0, 1.0, d.size)
    A = (S + sp.diags([d], [0])).tocsr(); A.sort_indices()
    return A


def diagonal(n):
    return sp.diags([2.0 + np.cos(np.arange(n))], [0]).tocsr()


def bidiagonal(n):
    return _dominant(sp.diags([0.5 + 0.25 * np.sin(np.arange(n - 1))], [-1], shape=(n, n)))


def arrow(n, seed=3):
    """Last row dense to the left, first row dense to the right, a diagonal between: the longest rows, column code n - 1, two levels per solve."""
    rng = np.random.default_rng(seed)
    S = sp.lil_matrix((n, n))
    S[n - 1, :n - 1] = rng.uniform(-1, 1, n - 1)
    S[0, 1:] = rng.uniform(-1, 1, n - 1)
    return _dominant(S.tocsr(), rng)


def random_sparse(n, per_row, seed):
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=min(1.0, per_row / n), random_state=rng, format="csr", data_rvs=lambda k: rng.uniform(-1, 1, k))
    return _dominant(S, rng)


def line_pencil(nx, ny):
    """The pencil of tests/test_gpu_st.py: A = 2-D 5-point Laplacian with a convective term, B = a diagonal mass matrix."""
    n = nx * ny
    T = sp.diags([np.full(nx - 1, -1.3), np.full(nx, 4.0), np.full(nx - 1, -0.7)], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), T) + sp.kron(sp.diags([np.full(ny - 1, -0.2), np.full(ny - 1, -0.2)], [-1, 1]), sp.identity(nx))).tocsr()
    B = sp.diags([1.0 + 0.1 * np.cos(np.arange(n))], [0]).tocsr()
    A.sort_indices(); B.sort_indices()
    return A, B


def scrambled(n, seed=9):
    """CSR arrays with unsorted columns and repeated entries (the diagonal among them), and the same matrix summed and sorted. All values are small
    multiples of 1/4 and sigma is SIGMA, so that every order of summation gives the same bits."""
    rng = np.random.default_rng(seed)
    rp, col, val = [0], [], []
    for r in range(n):
        off = rng.choice(np.delete(np.arange(n), r), size=min(n - 1, 5), replace=False)
        c = np.concatenate([off, off[:2], [r, r, r]])                 # two off-diagonal entries twice, the diagonal three times
        v = np.concatenate([rng.integers(1, 4, off.size + 2) / 4.0, [4.0, 2.5, 1.25]])      # no sum cancels: the pattern has no zero that a tool might drop
        o = rng.permutation(c.size)
        col.extend(c[o]); val.extend(v[o]); rp.append(len(col))
    rp = np.array(rp, dtype=np.int32); col = np.array(col, dtype=np.int32); val = np.array(val)
    S = sp.csr_matrix((val, col, rp), shape=(n, n)); S.sum_duplicates(); S.sort_indices()
    return (rp, col, val), S


def arrays(S):
    S = S.tocsr()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)


def shifted(A, sigma, B=None):
    """P = A - sigma B entry by entry as the library forms it: a_ij + ((-sigma) b_ij); B None = I."""
    Bm = sp.identity(A.shape[0], format="csr") if B is None else B
    P = (A + (-sigma) * Bm).tocsr(); P.sort_indices()
    return P
