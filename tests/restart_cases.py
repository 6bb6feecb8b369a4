"""Host-side inputs of the fused-restart tests (test_gpu_restart_fused.py): matrices of any row count, seeded orthogonal restart
matrices, the shapes the kernel level walks through and the comparison of two runs' outputs bit for bit."""
import numpy as np

# rows: one row group of one wave; a partial 32-row group; two; a partial last tile of 128 rows on either side of 512; more than one
# workgroup; several hundred workgroups (70002 rows = 547 tiles of 128 rows: on 256 CUs that is 137 workgroups of four waves, one tile per wave
# at most); TWO_ROUNDS: more tiles than waves on the device - every wave takes a second tile and the last tile is a partial 32-row group. That
# size depends on the device (rows()), so the list carries its name.
TWO_ROUNDS = "two_rounds"
SIZES = [2, 30, 34, 510, 514, 4098, 70002, TWO_ROUNDS]
LAST_COLUMNS = [1, 2, 4, 5, 16, 17, 30]        # k-steps of the product: 4 up to 16 active columns, 8 beyond; update chains of every parity
STARTS = [0, 2]
WIDTHS = [1, 15, 16]


def rows(n, num_cu):
    """An entry of SIZES as a row count on a device of num_cu CUs. k_restart_fused runs min(ceil(tiles / 4), num_cu) workgroups of four waves, a
    wave owns tiles of 128 rows: 128 * 4 * num_cu * 2 + 34 rows are two full rounds of every wave and a third tile of 34 rows for the first."""
    return 128 * 4 * num_cu * 2 + 34 if n == TWO_ROUNDS else n


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


def restart_stages(Vpre, V, Q, nc, s, e, k):
    """One run's restart against that run's own basis before it (Vpre: the nc constraints and the columns before k), stage by stage; the names of the
    stages that are off, () if none. The product V(:, s:e) = Vpre(:, s:k) Q(s:k, s:e) against numpy inside a componentwise bound: the device's chain
    of kin fused multiply-adds and numpy's kin products and sums are each within gamma_kin |Vpre| |Q| of the exact product, together below
    2 (kin + 1) 2^-53 |Vpre| |Q|. The copy of column k to column e and the columns no stage writes bit for bit. This cannot see a last-bit difference
    of the product - the comparison of the two runs does - but it says which run is wrong when one of them is."""
    off = []
    A = Vpre[:, nc + s:nc + k]; B = Q[s:k, s:e]
    err = np.abs(V[:, nc + s:nc + e] - A @ B)
    bound = 2.0 * (k - s + 1) * 2.0 ** -53 * (np.abs(A) @ np.abs(B))
    if not np.all(err <= bound):
        off.append("product: %d entries outside the bound, largest error %.3e" % (int((~(err <= bound)).sum()), float(np.nanmax(err))))
    if not same_bits(V[:, nc + e], V[:, nc + k]):
        off.append("copy of column %d to column %d" % (k, e))
    keep = list(range(0, nc + s)) + list(range(nc + e + 1, nc + k))
    if not same_bits(V[:, keep], Vpre[:, keep]):
        off.append("columns outside the window changed")
    return tuple(off)


def describe_difference(outa, outb):
    """For a failure message: every entry of two result dictionaries that differs; of arrays the differing columns, the number of differing rows with
    the first and the last of them, and the largest absolute difference."""
    out = []
    for key in outa:
        x, y = outa[key], outb[key]
        if not isinstance(x, np.ndarray):
            if x != y:
                out.append((key, x, y))
            continue
        if same_bits(x, y):
            continue
        d = bits(x) != bits(y)
        if d.ndim == 2:
            bad = np.flatnonzero(d.any(axis=1))
            out.append((key, "columns", np.flatnonzero(d.any(axis=0)).tolist(), "rows", len(bad), bad[:4].tolist(), bad[-4:].tolist(), "max", float(np.abs(x - y).max())))
        else:
            out.append((key, "entries", np.flatnonzero(d)[:8].tolist(), "max", float(np.abs(x - y).max())))
    return out


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
