"""Matrices that stand ON the limits of the layout builders (tests/test_gpu_layout_builders.py), the exact reference of their products and an
independent restatement of the automatic layout choice.

Exactness. Every generator that feeds exact_product uses integer values with |v| <= 255, integer x with |x| <= 8 and rows of at most 64 entries:
every product and every partial sum is an integer below 2^18, exact in binary64 in any order of additions, with or without fma and with the
padding fmas of the dictionary kernels. A test compares with np.array_equal: no tolerance, whatever layout the matrix got.

Only numpy; nothing here imports the library. predict_layout is written from DESIGN.md section 3 and the comment above choose_layout."""
import numpy as np

N_DICT = 4096 + 37            # more than one 4096-entry round of dictionary discovery, a last 64-row group of 37 rows


# ---- the exact reference ------------------------------------------------------------------------------------------------------------------
def _rows(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def _ints(a):
    i = np.asarray(a).astype(np.int64)
    assert np.array_equal(i, a), "integer-valued data only"
    return i


def exact_product(rowptr, col, val, x):
    """A x (x a vector or a block of columns) in int64, returned as float64; duplicates and unsorted columns allowed."""
    v, xi, rows = _ints(val), _ints(x), _rows(rowptr)
    y = np.zeros((len(rowptr) - 1,) + xi.shape[1:], dtype=np.int64)
    np.add.at(y, rows, (v if xi.ndim == 1 else v[:, None]) * xi[np.asarray(col, dtype=np.int64)])
    assert np.abs(y).max(initial=0) < 2 ** 53
    return y.astype(np.float64)


def exact_diagonal(rowptr, col, val):
    rows = _rows(rowptr)
    d = np.zeros(len(rowptr) - 1, dtype=np.int64)
    on = np.asarray(col) == rows
    np.add.at(d, rows[on], _ints(val)[on])
    return d.astype(np.float64)


def exact_norm_inf(rowptr, col, val):
    s = np.zeros(len(rowptr) - 1, dtype=np.int64)
    np.add.at(s, _rows(rowptr), np.abs(_ints(val)))
    return float(s.max(initial=0))


def int_vector(n, seed, cols=None):
    """Integers with 1 <= |x| <= 8 (no zeros: every stored entry shows in the product)."""
    rng = np.random.default_rng(seed)
    shape = (n,) if cols is None else (n, cols)
    return (rng.integers(1, 9, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float64)


# ---- what the rules read ------------------------------------------------------------------------------------------------------------------
def distinct_values(val):
    return len(np.unique(np.ascontiguousarray(val, dtype=np.float64).view(np.int64)))


def distinct_offsets(rowptr, col):
    return len(np.unique(np.asarray(col, dtype=np.int64) - _rows(rowptr)))


def max_row_length(rowptr):
    return int(np.diff(rowptr).max(initial=0))


def dict_width(maxlen):
    return 8 if maxlen <= 8 else 16 if maxlen <= 16 else 32


def slice_widths(rowptr):
    """The longest row of every 64-row slice."""
    lens = np.diff(np.asarray(rowptr, dtype=np.int64))
    pad = np.zeros((len(lens) + 63) // 64 * 64, dtype=np.int64)
    pad[:len(lens)] = lens
    return pad.reshape(-1, 64).max(axis=1)


def sell_slots(rowptr):
    """64 * sum of the slice widths: the entries SELL-64 stores."""
    return 64 * int(slice_widths(rowptr).sum())


def padding_sides(rowptr, W):
    """(W n, 4 nnz + 4096): the dictionary forms are refused as mostly padding when the first exceeds the second."""
    return W * (len(rowptr) - 1), 4 * int(rowptr[-1]) + 4096


def sell_sides(rowptr):
    """(8 * 64 sum width, 9 nnz + 8 * 4096): 64 sum width <= 1.125 nnz + 4096 in integers."""
    return 8 * sell_slots(rowptr), 9 * int(rowptr[-1]) + 8 * 4096


def predict_layout(rowptr, col, val, force=None):
    """(layout, w) of a single-rank matrix that is not wide-scatter; w is the code width of "dict" and 0 otherwise. force: None for the
    automatic choice, or "dict" / "odict" / "sell" / "sliced" for what a forced layout ends in (a forced dictionary form that cannot be built
    falls through to SELL-64 under its padding rule, or CSR)."""
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    if n == 0 or nnz == 0:
        return ("csr", 0)
    if force == "sliced" and n >= 4096:
        return ("sliced", 0)
    maxlen = max_row_length(rowptr)
    if force in (None, "dict", "odict") and 0 < maxlen <= 32:
        W = dict_width(maxlen)
        lhs, rhs = padding_sides(rowptr, W)
        if not lhs > rhs:
            nval, noff = distinct_values(val), distinct_offsets(rowptr, col)
            if force != "odict" and nval <= 255 and noff <= 256:
                return ("dict", W)
            if (force == "odict" or nval > 255) and noff <= 255:
                return ("odict", 0)
    lhs, rhs = sell_sides(rowptr)
    return ("sell", 0) if force == "sell" or lhs <= rhs else ("csr", 0)


def codes(rowptr, col, val):
    """Per entry (value index, offset index) in the sorted dictionaries: values ordered by their bit patterns as signed 64-bit integers."""
    _, vi = np.unique(np.ascontiguousarray(val, dtype=np.float64).view(np.int64), return_inverse=True)
    _, oi = np.unique(np.asarray(col, dtype=np.int64) - _rows(rowptr), return_inverse=True)
    return vi, oi


# ---- generators ---------------------------------------------------------------------------------------------------------------------------
def _csr(n, rows, cols, vals):
    """Entries given in row order -> CSR arrays."""
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return rowptr.astype(np.int32), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float64)


def value_set(nval):
    """nval distinct non-zero integers, 1, -1, 2, -2, ...; the largest positive one has the highest bit pattern, i.e. the last dictionary index."""
    k = np.arange(nval)
    v = (k // 2 + 1) * np.where(k % 2 == 0, 1, -1)
    assert np.abs(v).max() <= 255
    return v.astype(np.float64)


def dict_boundary(nval, noff, maxlen, n=N_DICT):
    """Exactly nval distinct values and noff distinct offsets, the longest row exactly maxlen entries.

    Offsets are the contiguous window [-(noff // 2), noff - noff // 2) around 0; slot j of row r is meant for offset number (r maxlen + j) mod noff
    and is DROPPED where it leaves the matrix, never clamped. Rows are full except a stretch in the middle with every length 0 ... maxlen and three
    empty rows (one in the first and one in the last 64 rows); n is no multiple of 64. The value of an entry follows its offset number, shifted
    in every second period of the offsets, so that rows repeat (the row-pattern form can take the matrix) and yet every value occurs in the first
    64 and in the last 64 rows. Of the offsets, those that fit there do: every offset >= 0 in the first 64 rows, every offset <= 0 in the last 64
    (a negative offset below -63 cannot occur in the first 64 rows of any matrix). One entry in the middle carries the highest value index
    together with the highest offset index: code 0xfeff at 255 values and 256 offsets."""
    lo = -(noff // 2)
    mid = n // 2
    assert n % 64 and n > 2 * noff + 2 * maxlen + 256 and mid - noff > 64
    lens = np.full(n, maxlen)
    lens[mid:mid + maxlen + 1] = np.arange(maxlen + 1)
    lens[[5, mid - 9, n - 3]] = 0
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    slot = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
    oi = (rows * maxlen + slot) % noff
    period = min(32, noff // int(np.gcd(noff, maxlen)))                 # the offsets of a row repeat after noff / gcd rows: 32 at (256, 8)
    planted = int(np.flatnonzero(rows == mid + maxlen)[0]) if maxlen else None
    vals = value_set(nval)
    top = int(np.argmax(vals))
    for shift in range(nval):
        vi = (oi + shift * ((rows // period) % 2)) % nval
        if planted is not None:
            oi[planted] = noff - 1; vi[planted] = top
        cols = rows + lo + oi
        keep = (cols >= 0) & (cols < n)
        if len(np.unique(vi[keep & (rows < 64)])) == nval and len(np.unique(vi[keep & (rows >= n - 64)])) == nval:
            break
    else:
        raise ValueError("no value shift puts all %d values into the first and the last 64 rows" % nval)
    return _csr(n, rows[keep], cols[keep], vals[vi[keep]])


def symmetric_boundary(nval, noff, period, n=N_DICT):
    """A symmetric matrix with exactly nval distinct values and the noff (even) distinct offsets +-1 ... +-noff/2, no diagonal: row r holds the
    upper offsets o = r (mod period) and so, period being odd, the lower offsets of exactly one class of rows - rows of about 2 (noff / 2) / period
    entries (period 43: at most 6, W = 8; period 21: at most 14, W = 16). Entries that leave the matrix are dropped with their mirror images;
    a_rc = a_cr; the highest value index sits on the highest offset."""
    assert noff % 2 == 0 and period % 2 == 1
    h = noff // 2
    r = np.arange(n, dtype=np.int64)
    R, Cc = [], []
    for o in range(1, h + 1):
        rr = r[(r % period == o % period) & (r + o < n)]
        R.append(rr); Cc.append(rr + o)
    R, Cc = np.concatenate(R), np.concatenate(Cc)
    order = np.lexsort((Cc, R))
    R, Cc = R[order], Cc[order]
    vals = value_set(nval)
    vi = np.arange(R.size) % nval
    vi[np.flatnonzero(Cc - R == h)[len(R) // (4 * h)]] = int(np.argmax(vals))
    rows = np.concatenate([R, Cc]); cols = np.concatenate([Cc, R]); v = np.concatenate([vals[vi], vals[vi]])
    order = np.lexsort((cols, rows))
    return _csr(n, rows[order], cols[order], v[order])


def _fitting_band(n, lens, values):
    """Row r of length L: offsets 0 ... L-1 in the upper half of the rows, -(L-1) ... 0 in the lower half (nothing leaves the matrix)."""
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    slot = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
    cols = np.where(rows < n // 2, rows + slot, rows - slot)
    assert cols.min() >= 0 and cols.max() < n
    return _csr(n, rows, cols, np.asarray(values, dtype=np.float64)[np.arange(rows.size) % len(values)])


def padding_rule(n, W, delta):
    """nnz = (W n - 4096) / 4 + delta with the longest row W entries: delta = 0 stands on the rule W n > 4 nnz + 4096 (equality: a dictionary),
    delta = -1 one entry beyond it (mostly padding: refused). Three values, at most 2 W - 1 offsets, every 97th row empty."""
    assert (W * n - 4096) % 4 == 0 and delta in (0, -1)
    nnz = (W * n - 4096) // 4 + delta
    lens = np.zeros(n, dtype=np.int64)
    lens[n // 2] = W
    others = np.flatnonzero((np.arange(n) != n // 2) & (np.arange(n) % 97 != 3))      # every 97th row stays empty
    q, rem = divmod(nnz - W, len(others))
    assert 0 < q + 1 <= W
    lens[others] = q
    lens[others[:rem]] += 1
    assert lens.sum() == nnz
    return _fitting_band(n, lens, [1.0, -2.0, 3.0])


def sell_rule(n, delta):
    """Too many values (400) and offsets (thousands) for a dictionary form, and 64 sum width - (1.125 nnz + 4096) = delta exactly: 0 is the last
    matrix SELL-64 admits, +64 (one slice one entry wider) the first it refuses. Slice widths 6 ... 14, four slices of empty rows only (width 0),
    a ragged last slice; inside a slice only its first row is kept at full width."""
    assert delta in (0, 64) and n % 64
    ns = (n + 63) // 64
    width = 6 + (np.arange(ns) * 5) % 9
    width[[3, 4, 17, ns - 2]] = 0
    d = delta // 64
    width[0] += (64 + d - width.sum()) % 9                              # sum width = 9 t + 64 + d
    t = (int(width.sum()) - 64 - d) // 9
    nnz = 512 * t                                                        # 1.125 nnz = 576 t: 64 sum width = 1.125 nnz + 4096 + delta
    lens = np.repeat(width, 64)[:n].astype(np.int64)
    deficit = int(lens.sum()) - nnz
    assert deficit >= 0
    cand = np.flatnonzero(np.arange(n) % 64 != 0)
    while deficit > 0:
        live = cand[lens[cand] > 0][:deficit]
        lens[live] -= 1
        deficit -= len(live)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    slot = np.arange(rows.size) - np.repeat(np.cumsum(lens) - lens, lens)
    cols = (rows * 131 + slot * 977 + 7) % n
    k = np.arange(rows.size) % 400
    vals = (k // 2 + 1) * np.where(k % 2 == 0, 1, -1)
    return _csr(n, rows, cols, vals)


LAYER_ROWS = 600              # 7 entries a row: 4200 entries a block, more than one round of discovery records


def layered(layers, vary="values", per_row=7, n=None):
    """A 7-entry band in `layers` consecutive blocks of LAYER_ROWS rows (the last one 37 rows longer). vary = "values": offsets 0, +-1, +-7, +-50
    everywhere, block b holds the two values b + 1 (off the diagonal) and -(b + 101) (on it) and no other block does: 2 layers values.
    vary = "offsets": the values depend on the slot only and block b holds the offsets 0, +-(3 b + 1), +-(3 b + 2), +-(3 b + 3): 6 layers + 1."""
    assert per_row == 7
    n = layers * LAYER_ROWS + 37 if n is None else n
    r = np.arange(n, dtype=np.int64)
    b = np.minimum(r // LAYER_ROWS, layers - 1)
    R, Cc, V = [], [], []
    for j, s in enumerate((-3, -2, -1, 0, 1, 2, 3)):
        if vary == "values":
            off = np.full(n, (0, 1, 7, 50)[abs(s)] * np.sign(s))
            v = np.where(s == 0, -(b + 101), b + 1)
        else:
            off = np.sign(s) * (3 * b + abs(s)) * (s != 0)
            v = np.full(n, (1, 2, 3, -9, 3, 2, 1)[j])
        c = r + off
        keep = (c >= 0) & (c < n)
        R.append(r[keep]); Cc.append(c[keep]); V.append(v[keep])
    R, Cc, V = np.concatenate(R), np.concatenate(Cc), np.concatenate(V)
    order = np.lexsort((Cc, R))
    return _csr(n, R[order], Cc[order], V[order])


OFFS13 = (-300, -150, -6, -3, -2, -1, 0, 1, 2, 3, 6, 150, 300)
_Z, _NZ, _D, _ND, _ONE, _MONE = 0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0
_ONEP, _BIG = float(np.nextafter(1.0, 2.0)), 1e308
_NAN1, _INF, _NINF = float("nan"), float("inf"), float("-inf")
_NAN2 = float(np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0])      # a second quiet NaN: another payload, another key
SPECIAL_KEYS = (_Z, _NZ, _NAN1, _NAN2, _INF, _NINF, _D, _ND, _ONE, _ONEP, _MONE, _BIG)
SPECIAL_ROWS = (                                                                           # row r takes line r mod 6, one value per offset of OFFS13
    (_ONE, _Z, _NZ, _D, _ND, _MONE, _ONE, _MONE, _D, _Z, _NZ, _ND, _ONE),                  # 0: zeros, denormals and +-1 only
    (_ONE, _ONEP, _Z, _D, _BIG, _MONE, _ONEP, _NZ, _ND, _ONE, _ONEP, _MONE, _Z),           # 1: finite; 1 and its neighbour, one huge value
    (_ONE, _Z, _MONE, _NAN1, _D, _ONE, _ONEP, _MONE, _NZ, _ONE, _ND, _MONE, _ONE),         # 2: a NaN
    (_MONE, _D, _ONE, _Z, _ONE, _MONE, _ONE, _NZ, _ONE, _NAN2, _ND, _ONE, _MONE),          # 3: the other NaN
    (_INF, _ONE, _Z, _MONE, _D, _ONE, _MONE, _ONEP, _NZ, _ONE, _ND, _MONE, _ONE),          # 4: +inf
    (_ONE, _MONE, _D, _ONE, _Z, _MONE, _ONE, _NZ, _ONE, _ND, _MONE, _ONEP, _NINF),         # 5: -inf
)


def special_values(n=N_DICT):
    """A 13-entry band (entries that leave the matrix dropped) whose values are the 12 keys of SPECIAL_KEYS; row r follows SPECIAL_ROWS[r mod 6].
    Returns the CSR arrays and the line of every row."""
    table = np.array(SPECIAL_ROWS, dtype=np.float64)
    r = np.arange(n, dtype=np.int64)
    R, Cc, V = [], [], []
    for j, o in enumerate(OFFS13):
        keep = (r + o >= 0) & (r + o < n)
        R.append(r[keep]); Cc.append(r[keep] + o); V.append(table[r[keep] % 6, j])
    R, Cc, V = np.concatenate(R), np.concatenate(Cc), np.concatenate(V)
    order = np.lexsort((Cc, R))                                         # ascending columns = the order of OFFS13
    return _csr(n, R[order], Cc[order], V[order]) + (r % 6,)


def special_x(n, seed=5):
    """Finite, 0.5 < |x| < 1: 1e308 x stays finite, and a denormal times x is one denormal unit, with or without fma."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5 + 2.0 ** -20, 1.0 - 2.0 ** -20, n) * rng.choice([-1.0, 1.0], n)


def ragged(n, seed):
    """Rows of 0 ... 9 entries (about a quarter of the rows empty, the first row never), columns anywhere in [0, n), unsorted, duplicates
    possible; integers up to 8."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, size=n) * (rng.random(n) >= 0.25)
    lens[0] = 3
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rng.integers(0, n, size=rows.size)
    vals = rng.integers(1, 9, size=rows.size) * rng.choice([-1, 1], size=rows.size)
    return _csr(n, rows, cols, vals)


def two_rank_ghosts(nlocal=2048, seed=23):
    """Two row blocks of nlocal rows: ragged local entries (columns inside the rank's own block) and, in every third row, one ghost entry - a column
    of the other rank. Global CSR arrays."""
    rng = np.random.default_rng(seed)
    N = 2 * nlocal
    r = np.arange(N, dtype=np.int64)
    lens = rng.integers(0, 8, size=N) * (rng.random(N) >= 0.2)
    rows = np.repeat(r, lens)
    cols = (rows // nlocal) * nlocal + rng.integers(0, nlocal, size=rows.size)
    g = r[r % 3 == 0]
    gcols = (1 - g // nlocal) * nlocal + rng.integers(0, nlocal, size=g.size)
    rows, cols = np.concatenate([rows, g]), np.concatenate([cols, gcols])
    order = np.lexsort((rng.random(rows.size), rows))
    vals = rng.integers(1, 9, size=rows.size) * rng.choice([-1, 1], size=rows.size)
    return _csr(N, rows[order], cols[order], vals)
