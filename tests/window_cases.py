"""Matrices for the windowed CSR layout (tests/test_gpu_window_layout.py) and an independent restatement of its plan and of the automatic choice.

The layout cuts the rows into blocks of block_rows; a block whose entries reference at most max_segments 64-double segments of x (col >> 6) is a
window block and stores a 16-bit code per entry, slot * 64 + (col & 63), slot being the segment's rank in the block's ascending list; a block that
references more is a direct block. predict_window is written from DESIGN.md section 16 and the comment above choose_layout; layered on
layout_cases.predict_layout, which is the whole automatic choice: the windowed layout is built only when it is forced.

Exactness: as in layout_cases - integer values with |v| <= 255, x from layout_cases.int_vector; the longest row here has 1500 entries, so every
partial sum stays below 2^22, exact in binary64 in any order. Only numpy; nothing here imports the library."""
import numpy as np

import layout_cases as lc


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _entry_blocks(rowptr, block_rows):
    return lc._rows(rowptr) // block_rows


def block_segments(rowptr, col, block_rows):
    """(blocks, per entry: its block, per entry: the rank of its segment in the block's ascending list, per block: segments referenced)."""
    n = len(rowptr) - 1
    blocks = (n + block_rows - 1) // block_rows
    nsegs = (n + 63) // 64 + 1
    eb = _entry_blocks(rowptr, block_rows)
    key = eb * nsegs + (np.asarray(col, dtype=np.int64) >> 6)
    uniq, inv = np.unique(key, return_inverse=True)                      # ascending: block-major, segments ascending inside a block
    nseg = np.bincount(uniq // nsegs, minlength=blocks).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(nseg)])[:-1]
    slot = inv.reshape(-1) - first[eb]
    return blocks, eb, slot, nseg


def predict_window(rowptr, col, block_rows, max_segments, val=None, force=None):
    """The plan's numbers and the layout a single-rank matrix ends in. force: None (the automatic choice; needs val, for layout_cases.predict_layout)
    or "window". Returns a dict: nseg (per block), direct (per block), blocks, direct_blocks, window_entries, direct_entries, total_segments (listed:
    those of window blocks), index_bytes, codes (per entry; 0 in direct blocks), layout."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    blocks, eb, slot, nseg = block_segments(rowptr, col, block_rows)
    direct = nseg > max_segments
    per_block = np.bincount(eb, minlength=blocks).astype(np.int64)
    we = int(per_block[~direct].sum())
    de = nnz - we
    listed = int(nseg[~direct].sum())
    codes = np.where(direct[eb], 0, slot * 64 + (np.asarray(col, dtype=np.int64) & 63)).astype(np.uint16) if nnz else np.zeros(0, np.uint16)
    if force == "window":
        layout = "window" if n > 0 and nnz > 0 else "csr"
    else:
        assert force is None
        layout = lc.predict_layout(rowptr, col, val)[0]                                 # no automatic rule picks the windowed layout
    out = dict(nseg=nseg, direct=direct, blocks=blocks, direct_blocks=int(direct.sum()), window_entries=we, direct_entries=de, total_segments=listed,
               index_bytes=2 * we + 4 * de + 4 * listed, codes=codes, layout=layout)
    return out


def info_of(p, block_rows, max_segments):
    """What Mat.window_info() must return for a matrix whose plan is p and whose layout is "window"."""
    return dict(block_rows=block_rows, max_segments=max_segments, blocks=p["blocks"], direct_blocks=p["direct_blocks"], window_entries=p["window_entries"],
                index_bytes=p["index_bytes"])


def info_of_none(block_rows, max_segments):
    return dict(block_rows=block_rows, max_segments=max_segments, blocks=0, direct_blocks=0, window_entries=0, index_bytes=0)


# ---- generators ---------------------------------------------------------------------------------------------------------------------------
def _int_values(rng, size):
    return (rng.integers(1, 256, size=size) * rng.choice([-1, 1], size=size)).astype(np.float64)


def forced_small(block_rows, seed=11):
    """n = 5 block_rows + 37: a partial last block and a partial last segment. Columns within +-300 of the row, unsorted and with duplicates; row
    lengths 0 ... 40, every 9th row empty, one row of 1 entry, a run of 64 rows of exactly 32 and one row of 1500 entries that has an entry in each
    of up to 24 segments (in every segment of the matrix where it has fewer than 24: n = 1317 has 21). Integer values."""
    rng = np.random.default_rng(seed)
    n = 5 * block_rows + 37
    lens = rng.integers(0, 41, n)
    lens[::9] = 0
    run0 = 2 * block_rows + 11 if 2 * block_rows + 11 + 64 <= n else 10
    lens[run0:run0 + 64] = 32
    one, long_ = 4, block_rows + 7
    lens[one], lens[long_] = 1, 1500
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows + rng.integers(-300, 301, rows.size), 0, n - 1)
    nseg_all = (n + 63) // 64
    span = min(24, nseg_all)
    s0 = min(max((long_ >> 6) - span // 2, 0), nseg_all - span)
    sel = np.flatnonzero(rows == long_)
    lcols = (s0 + rng.integers(0, span, sel.size)) * 64 + rng.integers(0, 64, sel.size)
    lcols[:span] = (s0 + np.arange(span)) * 64 + rng.integers(0, 64, span)              # every one of the span's segments at least once
    cols[sel] = np.minimum(lcols, n - 1)
    dup = np.flatnonzero((lens >= 2) & (np.arange(n) % 5 == 1))                          # a duplicate column in every such row
    starts = np.cumsum(lens) - lens
    cols[starts[dup] + 1] = cols[starts[dup]]
    return lc._csr(n, rows, cols, _int_values(rng, rows.size)) + (dict(one=one, long=long_, run=run0, span=span),)


def segment_limit(block_rows, max_segments, seed=12, per_row=8):
    """n = 64 (max_segments + 2) + 5 rows and columns; the first 4 block_rows rows carry the entries, the rows behind them are empty.
    Block 0: row i has one entry in each of the per_row segments (i per_row + t) mod max_segments - the block references exactly max_segments
    segments (0 ... max_segments - 1): the largest window. Block 1: the same over max_segments + 1 segments: direct. Block 2: five entries around the
    diagonal. Block 3: the diagonal and the columns of the last segment, which has 5 doubles."""
    rng = np.random.default_rng(seed)
    S = max_segments
    n = 64 * (S + 2) + 5
    assert 4 * block_rows <= n and block_rows * per_row >= S + 1
    R, Cc = [], []
    i = np.arange(block_rows, dtype=np.int64)
    for b, width in ((0, S), (1, S + 1)):
        for t in range(per_row):
            R.append(b * block_rows + i); Cc.append(((i * per_row + t) % width) * 64 + (i * 7 + t * 13) % 64)
    r2 = 2 * block_rows + i
    for o in (-2, -1, 0, 1, 2):
        R.append(r2); Cc.append(r2 + o)
    r3 = 3 * block_rows + i
    R.append(r3); Cc.append(r3)
    for t in range(2):
        R.append(r3); Cc.append(n - 5 + (i + 3 * t) % 5)
    R, Cc = np.concatenate(R), np.concatenate(Cc)
    order = np.lexsort((rng.random(R.size), R))                                        # any order inside a row
    return lc._csr(n, R[order], Cc[order], _int_values(rng, R.size))


def scattered(n, seed=13):
    """Rows of 10 ... 40 entries with columns anywhere in [0, n): every block references far more segments than a window holds."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(10, 41, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    return lc._csr(n, rows, rng.integers(0, n, rows.size), _int_values(rng, rows.size))


def mesh27(m, dofs=3, keep=0.7, seed=1, integer=False, planes=None):
    """A 27-point pattern on an m^3 grid (natural ordering, x fastest) with `dofs` unknowns per node, every off-diagonal entry kept with probability
    `keep`: ragged rows (mean 53 at 3 unknowns and keep 0.7) whose columns are stripe-local. Generated plane by plane (one random stream per z-plane),
    so that large grids need one plane of candidates at a time; planes = (z0, z1) returns those planes' rows only (global columns).
    Values uniform in (-1, 1), or integers."""
    n = dofs * m ** 3
    z0, z1 = planes if planes is not None else (0, m)
    lens_all, cols_all, vals_all = [], [], []
    yy, xx = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    for z in range(z0, z1):
        rng = np.random.default_rng([seed, z])
        node = (z * m + yy) * m + xx                                                    # the plane's nodes, ascending
        C, K = [], []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ok = (z + dz >= 0) & (z + dz < m) & (yy + dy >= 0) & (yy + dy < m) & (xx + dx >= 0) & (xx + dx < m)
                    C.append(node + (dz * m + dy) * m + dx); K.append(ok)
        C, K = np.stack(C, axis=1), np.stack(K, axis=1)                                 # [nodes, 27], ascending neighbours
        cols = (C[:, None, :, None] * dofs + np.arange(dofs)[None, None, None, :])      # [nodes, dof of the row, 27, dof of the column]
        cols = np.broadcast_to(cols, (len(node), dofs, 27, dofs)).reshape(len(node) * dofs, 27 * dofs)
        rows = (node[:, None] * dofs + np.arange(dofs)[None, :]).reshape(-1)
        ok = np.broadcast_to(K[:, None, :, None], (len(node), dofs, 27, dofs)).reshape(len(node) * dofs, 27 * dofs)
        ok = ok & ((cols == rows[:, None]) | (rng.random(cols.shape) < keep))
        lens_all.append(ok.sum(axis=1)); cols_all.append(cols[ok])
        vals_all.append(_int_values(rng, int(ok.sum())) if integer else rng.uniform(-1.0, 1.0, int(ok.sum())))
    lens = np.concatenate(lens_all)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rowptr, np.concatenate(cols_all).astype(np.int32), np.concatenate(vals_all), n


def coverage_rule(block_rows, direct_blocks, mean=17, nblocks=256, seed=14):
    """n = nblocks block_rows rows of `mean` entries on average, every block holding exactly mean block_rows entries; the first row of every 64 has 40
    entries and the others share the rest (lengths mean - 1 and mean), so SELL-64 declines the padding and no dictionary form takes rows of 40: without
    the windowed layout the matrix is CSR. `direct_blocks` blocks, spread evenly, scatter their columns over the whole matrix (direct blocks); the
    others stay within +-20 of the diagonal: a matrix with window blocks and direct blocks side by side, at a size the automatic choice sees."""
    rng = np.random.default_rng(seed)
    n = nblocks * block_rows
    rest = mean * 64 - 40
    q, rem = divmod(rest, 63)
    slice_lens = np.concatenate([[40], np.full(63, q)])
    slice_lens[1:1 + rem] += 1
    assert slice_lens.sum() == mean * 64 and slice_lens.max() == 40
    lens = np.tile(slice_lens, n // 64)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    slot = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
    cols = np.clip(rows + slot - 20, 0, n - 1)
    which = (np.arange(direct_blocks) * nblocks) // max(direct_blocks, 1)
    isdir = np.zeros(nblocks, bool); isdir[which] = True
    assert isdir.sum() == direct_blocks
    d = isdir[rows // block_rows]
    cols[d] = (rows[d] * 17 + slot[d] * 4099 + 5) % n
    return lc._csr(n, rows, cols, _int_values(rng, rows.size))


def banded_random(n, mean, seed=1):
    """scripts/csr_probe.py's ragged matrices: Poisson row lengths, every 17th row empty, every column drawn uniformly from +-32768 around the row."""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.poisson(mean, n), 0, None); lens[::17] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = (np.repeat(np.arange(n), lens) + rng.integers(-32768, 32768, nnz)).clip(0, n - 1).astype(np.int32)
    return rowptr, col, rng.uniform(-1, 1, nnz)
