"""Host-side inputs of the fused-restart tests (test_gpu_restart_fused.py): matrices of any row count, seeded orthogonal restart
matrices, the shapes the kernel level walks through and the comparison of two runs' outputs bit for bit."""
import numpy as np

# rows: one row group of one wave; a partial 32-row group; two; a partial last tile of 128 rows on either side of 512; more than one
# workgroup; more tiles than waves on the device (70002 rows = 547 tiles)
SIZES = [2, 30, 34, 510, 514, 4098, 70002]
LAST_COLUMNS = [1, 2, 4, 5, 16, 17, 30]        # k-steps of the product: 4 up to 16 active columns, 8 beyond; update chains of every parity
STARTS = [0, 2]
WIDTHS = [1, 15, 16]


def laplacian_rows(n):
    """(nx, ny) of a 2-D Laplacian with n rows: a stencil matrix, which takes the dictionary layout."""
    return (n // 2, 2) if n % 2 == 0 and n > 2 else (n, 1)


def random_csr(n, nnz_row=5, seed=3):
    """Seeded sparse matrix, symmetric (Lanczos needs it), n rows, about 2 * nnz_row entries per row."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed + n)
    rows = np.repeat(np.arange(n), nnz_row)
    cols = rng.integers(0, n, n * nnz_row)
    vals = rng.standard_normal(n * nnz_row)
    S = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    S = (S + S.T + sp.diags(np.linspace(1.0, 2.0, n))).tocsr()
    S.sum_duplicates(); S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)


def restart_q(m, lo, hi, seed=11):
    """m x m identity with a seeded orthogonal block on rows and columns [lo, hi): what the projected solve hands to the restart."""
    Q = np.eye(m)
    if hi > lo:
        rng = np.random.default_rng(seed + 131 * lo + hi)
        Q[lo:hi, lo:hi] = np.linalg.qr(rng.standard_normal((hi - lo, hi - lo)))[0]
    return np.asfortranarray(Q)


def start_vector(n, seed=5):
    v = np.random.default_rng(seed + n).standard_normal(n)
    return v / np.linalg.norm(v)


def windows(k):
    """(s, e) windows of a restart after a run whose last column is k: every start and width that leaves the copy's target e at or before k."""
    out = []
    for s in STARTS:
        for w in WIDTHS:
            e = min(s + w, k)
            if s < k and e > s and (s, e) not in out:
                out.append((s, e))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def first_difference(outa, outb):
    """Name of the first entry of two result dictionaries that differs (arrays bit for bit), or None."""
    assert outa.keys() == outb.keys(), (sorted(outa), sorted(outb))
    for key in outa:
        x, y = outa[key], outb[key]
        if isinstance(x, np.ndarray):
            if not same_bits(x, y):
                return key
        elif x != y:
            return key
    return None
