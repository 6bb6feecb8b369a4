"""Row splits, exact integer data and high-precision references for the block BV operations on row-sharded bases (tests/test_gpu_bv_ranks.py).

Splits. A split names the rows every rank owns of a basis of N rows. The ragged ones put a rank on every edge of the tall-skinny QR kernels (64-row
tiles): exactly one tile, two tiles and one row, fewer rows than columns, one row, no rows at all - at the head of the rank order, where the
all-zero triangular factor is the seed of the combine across ranks, and in the middle. "big2" depends on the device: TSQR gives every block one
tile while a rank has at most T = 64 * 2 * num_cu rows, so its first rank has T + 101 rows (blocks of two tiles, a last block of 64 + 37 rows).

Exactness. Bases hold integers with 1 <= |x| <= 8, coefficient matrices and vectors integers with |q| <= 3, B has the diagonal 6 and -1 on the
offsets +-1 and +-7 (absolute row sum 10). A Gram entry is at most 8 * 8 * N, one in the B-inner product 8 * 80 * N, an entry of X Q at most
8 * 3 * k, and the scalars of BVMult are powers of two: every product and every partial sum is an integer (or a multiple of 1/2) far below 2^53,
exact in binary64 in any order of additions, on the matrix cores or the vector ALUs. Every exact reference asserts its bound on the sums of the
absolute values, which bounds every partial sum too. A test compares with np.array_equal.

References of the orthogonalisations: a Householder QR in np.longdouble (R with a positive diagonal), the longdouble Cholesky factor of the exact
integer Gram matrix, and compare_R, which measures the relative distance of a method's R from the reference under the freedom that method has.

R_TOL. The distance allowed between a block method's R and the longdouble R is 8 times the largest relative distance between numpy's float64
np.linalg.qr R and the longdouble R over the cases of the GPU test (measure_r_distance(), run on the CPU; nothing here comes from the library):
measured 2.28e-16 (the largest at k = 64 with the window l = 3 of the 1000-row splits), hence R_TOL = 1.83e-15, relative to max|R|. The margin
covers the different but equally stable order of a tree reduction. SVQB's R is compared through its Gram factor R^T R, so its bound is measured in
that measure (measure_r_distance("svqb")): numpy's QR lies 4.18e-16 (relative to max|R^T R|, the largest at k = 100) from the longdouble R, hence
R_TOL_SVQB = 3.34e-15.

Only numpy; nothing here imports the library."""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
T_ROWS_PER_CU = 64 * 2            # TSQR: rows up to which every block of a rank has one tile, per compute unit
COND_B = 5.0                      # Gershgorin: the eigenvalues of B lie in [6 - 4, 6 + 4], cond(B) <= 10 / 2

R_DISTANCE_MEASURED = 2.28e-16    # max over R_CASES of compare_R("gs", R of np.linalg.qr, longdouble R), measured on the CPU
R_TOL = 8 * R_DISTANCE_MEASURED
R_DISTANCE_MEASURED_SVQB = 4.18e-16   # the same with compare_R("svqb", ...): the distance of the Gram factors R^T R
R_TOL_SVQB = 8 * R_DISTANCE_MEASURED_SVQB
TINY4 = [0, 5, 0, 0]              # 5 rows in all for 12 columns: a rank-deficient panel, fewer non-zero rows in the ranks' stack than columns


# ---- splits ---------------------------------------------------------------------------------------------------------------------------------
_FIXED = {
    "even2": [500, 500],                  # the plain case
    "ragged3": [64, 129, 807],            # one tile exactly; two tiles and one row
    "ragged4": [0, 5, 63, 932],           # rank 0 empty: the seed of the rank combine is a zero R; 5 rows < k; a tile short of one row
    "ragged4b": [65, 0, 934, 1],          # an empty rank in the middle; a last rank of one row
}
SMALL_SPLITS = list(_FIXED)
ALL_SPLITS = SMALL_SPLITS + ["big2"]


def split(name, num_cu=256):
    """(N, rows per rank). num_cu only matters for "big2"."""
    if name == "big2":
        T = T_ROWS_PER_CU * num_cu
        counts = [T + 101, 70]
    else:
        counts = list(_FIXED[name])
    return sum(counts), counts


def split_like(name, N):
    """The shape of a named split on another global size: the same number of ranks, the small ranks kept, the largest rank takes the rest."""
    _, counts = split(name)
    if name == "even2":
        return [N // 2, N - N // 2]
    big = int(np.argmax(counts))
    out = list(counts)
    out[big] = N - (sum(counts) - counts[big])
    assert out[big] > 0 and sum(out) == N
    return out


def ranges(counts):
    o = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [(int(o[r]), int(o[r + 1])) for r in range(len(counts))]


# ---- exact integer data -------------------------------------------------------------------------------------------------------------------
def int_basis(n, cols, seed):
    """Integers with 1 <= |x| <= 8: no zeros, so every entry shows in every product."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 9, size=(n, cols)) * rng.choice([-1, 1], size=(n, cols))).astype(np.float64)


def int_coeffs(shape, seed):
    """Small integers, |q| <= 3, zeros allowed; Fortran order, as the coefficient arguments want them."""
    return np.asfortranarray(np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float64))


B_OFFSETS = (1, 7)


def b_csr(N):
    """B as CSR arrays with global, sorted column indices: diagonal 6, -1 at the offsets +-1 and +-7. Symmetric and strictly diagonally dominant,
    so positive definite; the offsets cross every rank border of the splits."""
    rows, cols, vals = [], [], []
    for d, v in [(-7, -1.0), (-1, -1.0), (0, 6.0), (1, -1.0), (7, -1.0)]:
        i = np.arange(max(0, -d), min(N, N - d))
        rows.append(i); cols.append(i + d); vals.append(np.full(len(i), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(N + 1, dtype=np.int32)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols[order].astype(np.int32), vals[order]


def b_apply(X):
    """B X for any dtype (int64 stays int64)."""
    Y = 6 * X
    for d in B_OFFSETS:
        Y[d:] -= X[:-d]
        Y[:-d] -= X[d:]
    return Y


def b_dense(N):
    return b_apply(np.eye(N))


def _ints(a):
    i = np.asarray(a).astype(np.int64)
    assert np.array_equal(i, a), "integer-valued data only"
    return i


def _exact(value, bound):
    """value (integers, or integers times a power of two) as float64, after the check that the sum of the absolute values stays below 2^53."""
    assert np.max(bound, initial=0) < 2 ** 53, "not exact in binary64"
    return np.asarray(value, dtype=np.float64)


def exact_gram(Y, X, with_b=False):
    """Y^T X, or Y^T B X, in int64."""
    Yi, Xi = _ints(Y), _ints(X)
    BX = b_apply(Xi) if with_b else Xi
    absBX = b_apply(-np.abs(Xi)) + 12 * np.abs(Xi) if with_b else np.abs(Xi)          # |B| |X|: 6|x| + the neighbours' |x|
    return _exact(Yi.T @ BX, np.abs(Yi).T @ absBX)


def exact_mult(alpha, beta, Y, X, Q):
    """beta Y + alpha X Q for integer Y, X, Q and alpha, beta multiples of 1/2: twice the value in int64, halved."""
    a2, b2 = int(_ints(2 * alpha)), int(_ints(2 * beta))
    Yi, Xi, Qi = _ints(Y), _ints(X), _ints(Q)
    return _exact(b2 * Yi + a2 * (Xi @ Qi), abs(b2) * np.abs(Yi) + abs(a2) * (np.abs(Xi) @ np.abs(Qi))) / 2.0


def exact_matmat(X, Q):
    Xi, Qi = _ints(X), _ints(Q)
    return _exact(Xi @ Qi, np.abs(Xi) @ np.abs(Qi))


def exact_norm1(X):
    s = np.abs(_ints(X)).sum(axis=0)
    return float(_exact(s.max(initial=0), s))


def exact_norm_inf(X):
    s = np.abs(_ints(X)).sum(axis=1)
    return float(_exact(s.max(initial=0), s))


def exact_sumsq(X):
    """The sum of the squares of all entries, an integer."""
    Xi = _ints(X)
    s = int((Xi * Xi).sum())
    assert s < 2 ** 53
    return s


def ulps(a, b):
    """|a - b| in units of the last place of b."""
    return abs(a - b) / np.spacing(abs(b))


# ---- high-precision references ----------------------------------------------------------------------------------------------------------------
def householder_qr(X):
    """(Q, R) of X in np.longdouble by Householder reflections, R upper triangular with a POSITIVE diagonal, Q explicit (n x k)."""
    A = np.array(X, dtype=np.longdouble)
    n, k = A.shape
    assert n >= k
    vs = []
    for j in range(k):
        x = A[j:, j].copy()
        nrm = np.sqrt(np.sum(x * x))
        v = x.copy()
        v[0] += nrm if x[0] >= 0 else -nrm
        vn = np.sum(v * v)
        if vn != 0:
            A[j:, j:] -= np.outer(v, (2 / vn) * (v @ A[j:, j:]))
        vs.append((v, vn))
    R = np.triu(A[:k, :k])
    Q = np.zeros((n, k), dtype=np.longdouble)
    Q[:k, :k] = np.eye(k, dtype=np.longdouble)
    for j in range(k - 1, -1, -1):
        v, vn = vs[j]
        if vn != 0:
            Q[j:, :] -= np.outer(v, (2 / vn) * (v @ Q[j:, :]))
    s = np.where(np.diag(R) < 0, -1, 1).astype(np.longdouble)
    return Q * s[None, :], R * s[:, None]


def cholesky_upper(G):
    """R upper triangular with a positive diagonal and R^T R = G, in np.longdouble (G: the exact integer Gram matrix)."""
    G = np.array(G, dtype=np.longdouble)
    k = G.shape[0]
    R = np.zeros((k, k), dtype=np.longdouble)
    for j in range(k):
        for i in range(j):
            R[i, j] = (G[i, j] - R[:i, i] @ R[:i, j]) / R[i, i]
        d = G[j, j] - R[:j, j] @ R[:j, j]
        assert d > 0, "the Gram matrix is not positive definite"
        R[j, j] = np.sqrt(d)
    return R


def compare_R(method, R, Rref, l=0):
    """Relative distance (in max|Rref|) of the columns l.. of a method's R from the reference with the positive diagonal, under the freedom of the method:
       gs, chol         entrywise (the factor with a positive diagonal is unique);
       tsqr, tsqrchol   Householder R: every row from l on is defined up to its sign (rows before l are the coefficients against the given leading
                        columns: entrywise);
       svqb             R is not triangular and its rows depend on the eigenvectors' signs and order; the Gram factor R^T R of the rows and columns
                        from l on does not (rows before l entrywise). The distance of the Gram factors is relative to max|Rref^T Rref|."""
    R = np.asarray(R, dtype=np.longdouble)
    k = Rref.shape[0]
    R, Rr = R[:k, l:k], np.asarray(Rref, dtype=np.longdouble)[:, l:k]
    scale = np.abs(Rr).max()
    if method in ("gs", "chol"):
        return float(np.abs(R - Rr).max() / scale)
    head = float(np.abs(R[:l] - Rr[:l]).max(initial=0) / scale)
    if method in ("tsqr", "tsqrchol"):
        s = np.where(np.diag(R[l:]) < 0, -1, 1).astype(np.longdouble)
        return max(head, float(np.abs(R[l:] * s[:, None] - Rr[l:]).max() / scale))
    assert method == "svqb"
    G, Gr = R[l:].T @ R[l:], Rr[l:].T @ Rr[l:]
    return max(head, float(np.abs(G - Gr).max() / np.abs(Gr).max()))


def r_tolerance(method):
    """8 times the measured distance of numpy's QR from the longdouble R, in the measure compare_R uses for the method."""
    return R_TOL_SVQB if method == "svqb" else R_TOL


# ---- the inputs of the orthogonalisation tests ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_basis(N, k, l):
    """Standard-normal columns with a fixed seed, the first l orthonormal; read-only."""
    X = np.random.default_rng(1000 * k + l + N).standard_normal((N, k))
    if l:
        X[:, :l] = np.linalg.qr(X[:, :l])[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def normal_basis_R(N, k, l):
    """The longdouble R (positive diagonal) of normal_basis(N, k, l); computed once and shared."""
    R = householder_qr(normal_basis(N, k, l))[1]
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def ill_conditioned_basis(N, k, cond=1e12):
    """U diag(1 .. 1/cond) W^T with orthonormal U (N x k) and W: where Q = V inv(R) is no longer orthogonal."""
    rng = np.random.default_rng(N + k)
    U = np.linalg.qr(rng.standard_normal((N, k)))[0]
    W = np.linalg.qr(rng.standard_normal((k, k)))[0]
    X = U @ np.diag(np.logspace(0, -np.log10(cond), k)) @ W.T
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def nearly_orthonormal_basis(N, k, p):
    """Q (I + p S) with orthonormal Q and a symmetric S of order one: the input of a second orthogonalisation pass. Its scaled Gram matrix is
    I + O(p), with eigenvalue gaps of about p."""
    rng = np.random.default_rng(N + k + 7)
    Q = np.linalg.qr(rng.standard_normal((N, k)))[0]
    S = rng.standard_normal((k, k))
    X = Q @ (np.eye(k) + p * (S + S.T))
    X.setflags(write=False)
    return X


# (split, k, windows l) of test_block_orthogonalize_across_ranks: what R_TOL is measured over
R_CASES = [(s, 12, (0, 3)) for s in ALL_SPLITS] + [("ragged4", 64, (0, 3)), ("ragged3", 64, (0, 3)), ("ragged4", 100, (0, 3))]


def measure_r_distance(method="gs", num_cu=256):
    """The largest distance, in compare_R's measure for the method, between the R of numpy's float64 QR and the longdouble R over R_CASES."""
    worst = 0.0
    for name, k, windows in R_CASES:
        N, _ = split(name, num_cu)
        for l in windows:
            Rn = np.linalg.qr(normal_basis(N, k, l))[1]
            Rn = Rn * np.where(np.diag(Rn) < 0, -1.0, 1.0)[:, None]
            worst = max(worst, compare_R(method, Rn, normal_basis_R(N, k, l), l))
    return worst


# ---- the generalized symmetric problem of the solve across ranks ----------------------------------------------------------------------------
def ghep_test1_pencil(n=18):
    """(A, B) as CSR arrays (rowptr, col, val): A the 5-point Laplacian of the n x n grid (diagonal 4, -1 to the grid neighbours, row i n + j),
    B diagonal with 2 / log(i + 2): the pencil test_gpu_ghep.py solves in test_eps_test1_ghep_golden."""
    N = n * n
    i, j = np.divmod(np.arange(N), n)
    rows, cols, vals = [], [], []
    for ok, d, v in [(i > 0, -n, -1.0), (j > 0, -1, -1.0), (np.ones(N, bool), 0, 4.0), (j < n - 1, 1, -1.0), (i < n - 1, n, -1.0)]:
        r = np.flatnonzero(ok)
        rows.append(r); cols.append(r + d); vals.append(np.full(len(r), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int32)
    A = (rowptr, cols[order].astype(np.int32), vals[order])
    B = (np.arange(N + 1, dtype=np.int32), np.arange(N, dtype=np.int32), 2.0 / np.log(np.arange(N) + 2.0))
    return A, B
