"""General matrices for the row-sharded product (tests/test_gpu_sharded_product.py): ragged, unsorted, with duplicates, with ghosts owned by
any rank, under an ownership given rank by rank.

Exactness. Matrix values are integers, or dyadic rationals k / 1024; every x is integer-valued with |x| <= 64. Every product and every partial
sum is then a multiple of 2^-10 far below 2^53 in magnitude, i.e. exact in binary64 in ANY summation order, with or without fma, with the ghost
contributions added in a pass of their own. The reference is the integer product (scipy int64 CSR times int64 vector, divided by the scale),
and a test compares with np.array_equal: no tolerance, whatever layout the diagonal block has.

Only numpy and scipy; everything is vectorised (a case builds in tens of milliseconds)."""
import numpy as np
import scipy.sparse as sp

I64_EXACT = 2 ** 53


class Case:
    """A global CSR (rows unsorted, duplicates kept) plus the row count of every rank. val = ival / scale."""

    def __init__(self, name, counts, rowptr, col, ival, scale=1, fval=None):
        self.name = name
        self.counts = [int(c) for c in counts]
        self.world = len(counts)
        self.starts = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.N = int(self.starts[-1])
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.scale = scale
        self.ival = None if ival is None else np.ascontiguousarray(ival, dtype=np.int64)
        self.val = np.ascontiguousarray(fval, dtype=np.float64) if fval is not None else self.ival / float(scale)
        assert len(self.rowptr) == self.N + 1 and self.rowptr[-1] == len(self.col) == len(self.val)
        self.row = np.repeat(np.arange(self.N, dtype=np.int64), np.diff(self.rowptr))       # row of every entry
        self.owner_of_row = np.repeat(np.arange(self.world), self.counts)

    # -- per rank
    def range(self, rank):
        return int(self.starts[rank]), int(self.starts[rank + 1])

    def block(self, rank):
        """(rowptr, col, val) of the rank's rows with GLOBAL column indices: what Mat.from_csr takes."""
        r0, r1 = self.range(rank)
        p0, p1 = int(self.rowptr[r0]), int(self.rowptr[r1])
        return self.rowptr[r0:r1 + 1] - p0, self.col[p0:p1], self.val[p0:p1]

    def entry_is_local(self):
        """Per entry: is its column owned by the rank that owns its row."""
        s = self.starts[self.owner_of_row[self.row]]
        e = self.starts[self.owner_of_row[self.row] + 1]
        return (self.col >= s) & (self.col < e)

    def row_stats(self):
        """Per global row: local entries, ghost entries, 'a local column occurs twice', 'a ghost column occurs twice'."""
        loc = self.entry_is_local()
        nloc = np.bincount(self.row, weights=loc, minlength=self.N).astype(np.int64)
        ngho = np.bincount(self.row, weights=~loc, minlength=self.N).astype(np.int64)
        order = np.lexsort((self.col, self.row))
        r, c, l = self.row[order], self.col[order], loc[order]
        same = (r[1:] == r[:-1]) & (c[1:] == c[:-1])
        dup_loc = np.zeros(self.N, bool); dup_loc[r[1:][same & l[1:]]] = True
        dup_gho = np.zeros(self.N, bool); dup_gho[r[1:][same & ~l[1:]]] = True
        return nloc, ngho, dup_loc, dup_gho

    # -- references
    def int_matrix(self):
        return sp.csr_matrix((self.ival, self.col, self.rowptr), shape=(self.N, self.N))

    def reference(self, x):
        """Exact A x for an integer-valued x (float64 array), as float64."""
        xi = np.asarray(x).astype(np.int64)
        assert np.array_equal(xi, x)
        y = self.int_matrix() @ xi
        assert np.abs(y).max(initial=0) < I64_EXACT
        return y / float(self.scale)

    def abs_row_sums(self):
        """Exact sum_j |a_ij| per row."""
        s = np.bincount(self.row, weights=np.abs(self.ival).astype(np.float64), minlength=self.N)      # integers below 2^53: exact
        return s / float(self.scale)

    def diagonal(self):
        """Exact a_ii per row, duplicates summed."""
        on = self.col == self.row
        d = np.bincount(self.row[on], weights=self.ival[on].astype(np.float64), minlength=self.N)
        return d / float(self.scale)

    def rows_referencing(self, j):
        return np.unique(self.row[self.col == j])


def int_vectors(N, count, seed):
    """count integer-valued vectors with |x| <= 64 (no zeros: every stored entry shows in the product)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 65, size=(count, N)) * rng.choice([-1, 1], size=(count, N))
    return x.astype(np.float64)


def _assemble(N, rows, cols, vals, rng):
    """Entry lists -> CSR with the entries of a row in RANDOM order (unsorted columns, duplicates kept apart)."""
    rows = np.concatenate(rows); cols = np.concatenate(cols); vals = np.concatenate(vals)
    order = np.lexsort((rng.random(len(rows)), rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
    return rowptr, cols[order], vals[order]


def _small_ints(rng, size, top=8):
    return rng.integers(1, top + 1, size=size) * rng.choice([-1, 1], size=size)


FAR_COUNTS = {4: [9935, 0, 65, 10000],                          # a zero-row rank between two large ones, and a 65-row rank
              8: [4000, 0, 1, 63, 5000, 64, 65, 10807]}         # zero rows, one row, and 63 / 64 / 65 rows (one below, at and above a wave of rows)
FAR_EVEN = [4608] * 4                                           # the same pattern where every rank can take the binned and sliced layouts (>= 4096 rows)


def far(world=4, seed=7, counts=None, values="int"):
    """Ragged rows of 0...40 entries, columns uniform over ALL of [0, N), unsorted. Of the rows about 5 % are empty, 5 % hold only ghost entries,
    5 % only local ones, 5 % a repeated column both in their local part (the diagonal entry, twice) and in their ghost part. The first row of
    every non-empty rank holds one entry in every other non-empty rank's block, so every non-empty rank is every other one's peer, both ways.
    Row `planted` (owned by rank 0) carries the largest absolute row sum of the matrix, nearly all of it in ghost entries.
    values: "int" (integers up to 8 in magnitude), "dyadic" (k / 1024, |k| <= 4096), "normal" (standard normal: no exact reference)."""
    rng = np.random.default_rng(seed)
    counts = list(FAR_COUNTS[world] if counts is None else counts)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(starts[-1])
    owner = np.repeat(np.arange(len(counts)), counts)
    s_row, n_row = starts[owner], np.asarray(counts)[owner]
    kind = rng.random(N)                                           # < .05 empty, < .10 ghosts only, < .15 local only, < .20 duplicates, else mixed
    first = starts[:-1][np.asarray(counts) > 0]
    kind[first] = 0.5
    planted = int(starts[0] + counts[0] // 2) if counts[0] > 2 else int(first[-1] + 1)
    kind[planted] = 0.5
    length = rng.integers(1, 41, size=N)
    length[kind < 0.05] = 0
    length[first] = np.minimum(length[first], 30); length[planted] = 5                                    # room for the entries added below
    length[(kind >= 0.15) & (kind < 0.20)] = np.minimum(length[(kind >= 0.15) & (kind < 0.20)], 36)       # + 4 duplicate entries: still <= 40
    rows = np.repeat(np.arange(N, dtype=np.int64), length)
    k_e, s_e, n_e = kind[rows], s_row[rows], n_row[rows]
    cols = rng.integers(0, N, size=len(rows))
    gh = (k_e >= 0.05) & (k_e < 0.10)                              # ghosts only: uniform over the columns of the OTHER ranks
    c = rng.integers(0, N - n_e[gh]); cols[gh] = np.where(c >= s_e[gh], c + n_e[gh], c)
    lo = (k_e >= 0.10) & (k_e < 0.15)                              # local only
    cols[lo] = s_e[lo] + rng.integers(0, n_e[lo])
    R, Cc = [rows], [cols]
    d = np.flatnonzero((kind >= 0.15) & (kind < 0.20))             # the diagonal twice, one ghost column twice
    g = rng.integers(0, N - n_row[d]); g = np.where(g >= s_row[d], g + n_row[d], g)
    R += [d, d, d, d]; Cc += [d, d, g, g]
    nonempty = np.flatnonzero(np.asarray(counts) > 0)
    for p in nonempty:                                             # every ordered pair of non-empty ranks exchanges something
        others = nonempty[nonempty != p]
        R.append(np.full(len(others), starts[p])); Cc.append(starts[others] + np.asarray(counts)[others] // 2)
    others = nonempty[nonempty != owner[planted]]
    pg = np.repeat(starts[others] + np.asarray(counts)[others] // 3, 5)[:30]
    R.append(np.full(len(pg), planted)); Cc.append(pg)
    n_all = sum(len(r) for r in R)
    if values == "normal":
        vals = rng.standard_normal(n_all)
        rowptr, col, val = _assemble(N, R, Cc, np.split(vals, np.cumsum([len(r) for r in R])[:-1]), rng)
        case = Case("float", counts, rowptr, col, None, fval=val)
    else:
        top, scale = (8, 1) if values == "int" else (4096, 1024)
        V = [_small_ints(rng, len(r), top) for r in R]
        V[-1] = np.full(len(pg), 4096 * scale)                     # the planted row: 30 ghost entries of 4096 against rows whose sums stay below 41 * 8
        rowptr, col, ival = _assemble(N, R, Cc, V, rng)
        case = Case("far", counts, rowptr, col, ival, scale)
    case.planted = planted
    return case


ISLAND_COUNTS = [700, 500, 600, 900]


def islands(seed=11):
    """World 4, one-way pairs only. Rank 0 needs entries of rank 3 and of nobody else (not its neighbour; rank 3 needs nothing back). Rank 1 has no
    off-diagonal entries and nobody needs it: it never enters an exchange. Rank 2 needs nothing and serves rank 3: it only sends. Rank 3 only
    receives from rank 2 (and serves rank 0). Local blocks are ragged (0...12 entries, unsorted)."""
    rng = np.random.default_rng(seed)
    counts = ISLAND_COUNTS
    starts = np.concatenate([[0], np.cumsum(counts)])
    N = int(starts[-1])
    owner = np.repeat(np.arange(4), counts)
    length = rng.integers(0, 13, size=N)
    rows = np.repeat(np.arange(N, dtype=np.int64), length)
    cols = starts[owner[rows]] + rng.integers(0, np.asarray(counts)[owner[rows]])
    R, Cc = [rows], [cols]
    for p, q in ((0, 3), (3, 2)):                                  # rank p reads columns of rank q: 0...3 ghost entries per row
        k = rng.integers(0, 4, size=counts[p])
        r = np.repeat(np.arange(starts[p], starts[p + 1], dtype=np.int64), k)
        R.append(r); Cc.append(starts[q] + rng.integers(0, counts[q], size=len(r)))
    V = [_small_ints(rng, len(r)) for r in R]
    rowptr, col, ival = _assemble(N, R, Cc, V, rng)
    return Case("islands", counts, rowptr, col, ival)


BIGHALO_NLOCAL = 6400          # one peer can then serve more than 3 * 2048 entries: the peer halo's kernels run four workgroups at world 2 already


def bighalo(world=4, seed=13):
    """Every row holds a few local offsets out of {0, +-1, +-5, +-64} plus ghost entries at (r + n_local k) mod N, k = 1...world-1: k = 1 in every
    row, k = 2 in every second, k = 3 in every third - three peers of 6400, 3200 and 2134 entries at world 4, one of 6400 at world 2."""
    rng = np.random.default_rng(seed)
    nl = BIGHALO_NLOCAL
    counts = [nl] * world
    N = nl * world
    r = np.arange(N, dtype=np.int64)
    s = (r // nl) * nl
    R, Cc = [], []
    for off in (0, 1, -1, 5, -5, 64, -64):
        c = r + off
        keep = (c >= s) & (c < s + nl) & ((rng.random(N) < 0.6) | (off == 0))
        R.append(r[keep]); Cc.append(c[keep])
    for k in range(1, world):
        keep = (r - s) % k == 0
        R.append(r[keep]); Cc.append((r[keep] + nl * k) % N)
    V = [_small_ints(rng, len(x)) for x in R]
    rowptr, col, ival = _assemble(N, R, Cc, V, rng)
    return Case("bighalo", counts, rowptr, col, ival)


LAYOUTS_NLOCAL = 4608


def layouts(values="int", seed=17):
    """World 4, 4608 rows per rank. Banded: column offsets 0, +-1, +-7, +-130 (those that cross a block boundary are ghosts of the neighbour), ghost
    entries at r +- n_local and at (r + 2 n_local) mod N, the rank two further on: at most 10 entries per row.
    values "int": eight distinct integers (the value dictionary of the dict layout takes them); "dyadic": k / 1024 with thousands of
    distinct k (only the offsets go into a dictionary: odict). Row `planted` carries the largest absolute row sum, in a ghost entry."""
    rng = np.random.default_rng(seed)
    nl = LAYOUTS_NLOCAL
    counts = [nl] * 4
    N = 4 * nl
    r = np.arange(N, dtype=np.int64)
    R, Cc = [], []
    for off in (0, 1, -1, 7, -7, 130, -130, nl, -nl):
        c = r + off
        keep = (c >= 0) & (c < N)
        R.append(r[keep]); Cc.append(c[keep])
    R.append(r); Cc.append((r + 2 * nl) % N)
    if values == "int":
        eight = np.array([-7, -3, -2, -1, 1, 2, 4, 5])
        V = [eight[rng.integers(0, 8, size=len(x))] for x in R]
        scale = 1
    else:
        V = [_small_ints(rng, len(x), 4096) for x in R]
        scale = 1024
    planted = nl + 1000                                            # a row of rank 1
    V[-1][planted] = 4096 * 100 * scale                            # its far ghost entry (the last list holds one entry per row, in row order)
    rowptr, col, ival = _assemble(N, R, Cc, V, rng)
    case = Case("layouts-" + values, counts, rowptr, col, ival, scale)
    case.planted = planted
    return case


def halo_plan(case):
    """Per rank, from partition.ghost_columns: needs[rank] = {owner: how many of its columns the rank reads}, nghost[rank], nsend[rank]."""
    from slepc_amd import partition as P
    needs, nghost = [], []
    for rank in range(case.world):
        r0, r1 = case.range(rank)
        _, col, _ = case.block(rank)
        g = np.asarray(P.ghost_columns(col, r0, r1), dtype=np.int64)
        own = np.searchsorted(case.starts, g, side="right") - 1
        needs.append({int(p): int(np.count_nonzero(own == p)) for p in np.unique(own)})
        nghost.append(len(g))
    nsend = [sum(needs[q].get(p, 0) for q in range(case.world)) for p in range(case.world)]
    return needs, nghost, nsend


def forward_plan(c):
    """What build_halo_plan leaves on every rank, in numpy: the sorted ghost list, the peers (ascending), recv/send counts and offsets per peer, and
    send_idx - peer after peer, the peer's ghosts inside this rank's rows in ascending order, as local row indices."""
    world = c.world
    ghosts = []
    for p in range(world):
        r0, r1 = c.range(p)
        col = c.block(p)[1]
        ghosts.append(np.unique(col[(col < r0) | (col >= r1)]).astype(np.int32))
    own = [np.searchsorted(c.starts, g, side="right") - 1 for g in ghosts]
    plans = []
    for p in range(world):
        r0, _ = c.range(p)
        peers, rcnt, scnt, seg = [], [], [], []
        for q in range(world):
            if q == p:
                continue
            r = int(np.count_nonzero(own[p] == q))
            mine = ghosts[q][own[q] == p]
            if r == 0 and mine.size == 0:
                continue
            peers.append(q); rcnt.append(r); scnt.append(int(mine.size)); seg.append(mine - r0)
        send_idx = np.concatenate(seg).astype(np.int32) if seg else np.zeros(0, np.int32)
        roff = np.concatenate([[0], np.cumsum(rcnt)])[:-1].astype(int) if peers else np.zeros(0, int)
        soff = np.concatenate([[0], np.cumsum(scnt)])[:-1].astype(int) if peers else np.zeros(0, int)
        plans.append({"ghosts": ghosts[p], "peers": peers, "rcnt": rcnt, "scnt": scnt, "roff": roff, "soff": soff, "send_idx": send_idx})
    return plans
