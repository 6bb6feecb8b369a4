"""Block CSR (BAIJ) inputs for Mat.from_bsr (tests/test_gpu_bsr*.py, tests/test_bsr_host.py, scripts/bsr_probe.py): the expansion that defines such a
matrix, the predicted bsr_info, and the generators. Only numpy; nothing here imports the library.

The expansion. Scalar row bs I + i holds, for each block k of block row I in stored order and then c = 0 .. bs - 1, the entry with column
bs bcol[k] + c and value blocks[k, i, c]; explicit zeros inside blocks are entries. The matrix behaves as from_csr of these arrays.

Exactness of `small`. Integer values with |v| <= 255, block rows of at most 200 blocks of at most 8 x 8: a scalar row has at most 1600 entries, and with
layout_cases.int_vector (|x| <= 8) every partial sum is below 1600 * 255 * 8 < 2^22: exact in binary64 in any order, with or without fma."""
import numpy as np

LONG_ROW_BLOCKS_MAX = 200


def expand(browptr, bcol, blocks):
    """(rowptr, col, val) of the expansion, int32 / int32 / float64."""
    browptr = np.asarray(browptr, dtype=np.int64)
    bcol = np.asarray(bcol, dtype=np.int64)
    blocks = np.asarray(blocks, dtype=np.float64)
    nb, bs = len(browptr) - 1, blocks.shape[1]
    lens = np.diff(browptr)
    rowptr = np.concatenate([[0], np.cumsum(np.repeat(lens * bs, bs))])
    nnz = int(rowptr[-1])
    assert nnz < 2 ** 31
    col = np.empty(nnz, dtype=np.int32)
    val = np.empty(nnz, dtype=np.float64)
    I = np.repeat(np.arange(nb, dtype=np.int64), lens)                        # block row of block k
    first = browptr[I] * bs * bs + (np.arange(len(bcol), dtype=np.int64) - browptr[I]) * bs      # entry (k, 0, 0): behind the row's earlier blocks
    for i in range(bs):
        for c in range(bs):
            e = first + i * lens[I] * bs + c                                  # scalar row i of the block row starts i row lengths further on
            col[e] = bs * bcol + c
            val[e] = blocks[:, i, c]
    return rowptr.astype(np.int32), col, val


def predict_info(browptr, blocks):
    """What bsr_info() must report apart from the two constants of the product, which a test reads from it."""
    nb, nnzb = len(browptr) - 1, int(browptr[-1])
    return {"bs": int(np.asarray(blocks).shape[1]), "block_rows": nb, "blocks": nnzb, "index_bytes": 4 * nnzb + 4 * (nb + 1)}


def layout_bytes(browptr, blocks):
    """8 bs^2 nnzb + 4 nnzb + 4 (nb + 1): the stream of the block CSR layout."""
    nb, nnzb, bs = len(browptr) - 1, int(browptr[-1]), int(np.asarray(blocks).shape[1])
    return 8 * bs * bs * nnzb + 4 * nnzb + 4 * (nb + 1)


def _small_pattern(bs, G, chunk, seed, groups=5):
    rng = np.random.default_rng(seed)
    nb = groups * G + 3
    lens = rng.integers(0, 13, size=nb)
    lens[::7] = 0                                           # every 7th block row is empty
    one, long_row = 2, 2 * G + 1                            # neither a multiple of 7 for any G = 4 * (64 // bs)
    assert one % 7 and long_row % 7, (G, long_row)
    lens[one] = 1
    nlong = 3 * chunk // (bs * bs) + 1                      # its scalars exceed three chunks
    assert bs * bs * nlong > 3 * chunk and nlong <= LONG_ROW_BLOCKS_MAX, (bs, chunk, nlong)
    lens[long_row] = nlong
    browptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    bcol = rng.integers(0, nb, size=int(browptr[-1])).astype(np.int32)      # unsorted, repeats as they fall ...
    for I in np.flatnonzero(lens >= 3)[::2]:
        bcol[browptr[I] + 2] = bcol[browptr[I]]                             # ... and a certain repeat in every other longer block row
    return rng, nb, browptr, bcol


def small(bs, G, chunk, seed=0, groups=5):
    """(browptr, bcol, blocks): nb = 5 G + 3 block rows of 0 .. 12 blocks, every 7th empty, one with one block, one with more than three chunks'
    worth (at most 200 blocks); block columns unsorted and repeated; a zero in roughly every fifth block; integers with |v| <= 255.
    groups = 10: the same rules on 10 G + 3 block rows - at least 2415 scalar rows for every block size 2 .. 8 with G = 4 (64 // bs). A block matrix of
    fewer than 2048 rows runs the small-matrix form of the product (lanes share a row, as the CSR-vector kernel does), so 5 G + 3 block rows reach that
    form and 10 G + 3 the chunked walk; the row lengths, and with them the exactness premise, are the same."""
    rng, nb, browptr, bcol = _small_pattern(bs, G, chunk, seed, groups)
    nnzb = int(browptr[-1])
    blocks = (rng.integers(1, 256, size=(nnzb, bs, bs)) * rng.choice([-1, 1], size=(nnzb, bs, bs))).astype(np.float64)
    z = np.arange(0, nnzb, 5)
    blocks[z, rng.integers(0, bs, size=len(z)), rng.integers(0, bs, size=len(z))] = 0.0
    return browptr, bcol, blocks


def small_real(bs, G, chunk, seed=0, groups=10):
    """The twin of `small` with real values (standard normal, the explicit zeros kept), for bit-for-bit comparisons between layouts; by default on
    10 G + 3 block rows, where both the block CSR product and the CSR kernel it is compared with are the chunked entry-order walks (groups = 5: both
    are the small-matrix forms)."""
    rng, nb, browptr, bcol = _small_pattern(bs, G, chunk, seed, groups)
    nnzb = int(browptr[-1])
    blocks = rng.standard_normal((nnzb, bs, bs))
    z = np.arange(0, nnzb, 5)
    blocks[z, rng.integers(0, bs, size=len(z)), rng.integers(0, bs, size=len(z))] = 0.0
    return browptr, bcol, blocks


def longest_row_bound(browptr, blocks, xmax=8):
    """Largest possible |partial sum| of any scalar row: entries of the longest row times max|v| times max|x|."""
    bs = blocks.shape[1]
    return int(np.diff(browptr).max(initial=0)) * bs * int(np.abs(blocks).max(initial=0)) * xmax


def mesh_blocks(m, bs, keep, symmetric=True, seed=0):
    """(browptr, bcol, blocks) of an m^3 node mesh with the 27-point node pattern, bs unknowns per node: whole off-diagonal node blocks are kept with
    probability `keep` (pairwise: the pattern is symmetric), the diagonal block always; block columns ascending. Values are standard normal with
    27 bs added on the diagonal (strictly diagonally dominant rows are not claimed, only safe pivots). symmetric: block (J, I) is the transpose of
    block (I, J) and the diagonal blocks are symmetric; otherwise every block is drawn on its own."""
    rng = np.random.default_rng(seed)
    nn = m * m * m
    ids = np.arange(nn, dtype=np.int64)
    x, y, z = ids % m, (ids // m) % m, ids // (m * m)
    up_i, up_j = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                off = dx + m * (dy + m * dz)
                if off <= 0:
                    continue
                ok = (x + dx >= 0) & (x + dx < m) & (y + dy >= 0) & (y + dy < m) & (z + dz >= 0) & (z + dz < m)
                up_i.append(ids[ok]); up_j.append(ids[ok] + off)
    ui, uj = np.concatenate(up_i), np.concatenate(up_j)
    kept = rng.random(len(ui)) < keep
    ui, uj = ui[kept], uj[kept]
    ub = rng.standard_normal((len(ui), bs, bs))
    lb = ub.transpose(0, 2, 1) if symmetric else rng.standard_normal((len(ui), bs, bs))
    db = rng.standard_normal((nn, bs, bs))
    if symmetric:
        db = 0.5 * (db + db.transpose(0, 2, 1))
    db = db + 27.0 * bs * np.eye(bs)[None, :, :]
    I = np.concatenate([ids, ui, uj]); J = np.concatenate([ids, uj, ui])
    order = np.lexsort((J, I))
    blocks = np.concatenate([db, ub, lb])[order]
    browptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=nn))]).astype(np.int32)
    return browptr, J[order].astype(np.int32), np.ascontiguousarray(blocks)
