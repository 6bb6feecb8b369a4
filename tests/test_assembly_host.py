"""The host planning of Mat assembly (slepc_amd/csrc/ks_csr.cpp): the diagonal / ghost split of ks_mat_create_csr, the arithmetic of the halo plan
between its collectives, and the host build of the binned layout - the product's own functions through the ksc_* hooks of libksgpu.so, CPU only.
The halo plan of a whole world is made rank by rank, the two allgathers and the exchange of ids simulated in numpy, and compared with the independent
numpy statement of it (sharded_cases.forward_plan). The binned plan is walked on the host the way its two kernels walk it; values and vectors are small
integers, so the product is exact in any order and compared with the int64 scipy product by np.array_equal."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import assembly_hooks as ah
import sharded_cases as sc
from slepc_amd import partition as P


@pytest.fixture(scope="module")
def lib():
    return ah.load()


def banded8(seed=23):
    """World 8, 301 rows split the way PetscSplitOwnership does (38 rows on five ranks, 37 on three): offsets 0, +-1, +-7, +-130 and a far entry at
    (r + N / 2) mod N - every rank has ghosts of its neighbours and of ranks three to four further on, entries unsorted."""
    rng = np.random.default_rng(seed)
    N = 301
    counts = [b - a for a, b in P.split_ownership(N, 8)]
    assert len(set(counts)) > 1
    r = np.arange(N, dtype=np.int64)
    R, Cc = [], []
    for off in (0, 1, -1, 7, -7, 130, -130):
        c = r + off
        keep = (c >= 0) & (c < N)
        R.append(r[keep]); Cc.append(c[keep])
    R.append(r); Cc.append((r + N // 2) % N)
    V = [sc._small_ints(rng, len(x)) for x in R]
    rowptr, col, ival = sc._assemble(N, R, Cc, V, rng)
    return sc.Case("banded8", counts, rowptr, col, ival)


WORLDS = [("far", 4), ("far", 8), ("islands", 4), ("bighalo", 2), ("bighalo", 4)]


@functools.lru_cache(maxsize=None)
def case(name, world):
    return {"far": lambda: sc.far(world), "islands": sc.islands, "bighalo": lambda: sc.bighalo(world), "banded8": banded8}[name]()


def split_rank(lib, c, rank):
    r0, r1 = c.range(rank)
    rp, col, val = c.block(rank)
    return ah.split_block(lib, r1 - r0, r0, c.N, rp, col, val)


@pytest.mark.parametrize("name,world", WORLDS)
def test_split_block(lib, name, world):
    c = case(name, world)
    for rank in range(world):
        r0, r1 = c.range(rank)
        rp, col, val = c.block(rank)
        s = split_rank(lib, c, rank)
        assert s["status"] == 0
        assert np.array_equal(s["garray"], np.asarray(P.ghost_columns(col, r0, r1), dtype=np.int32))       # sorted, distinct
        loc = (col >= r0) & (col < r1)
        rows = np.repeat(np.arange(r1 - r0), np.diff(rp))
        # both blocks keep the stored order of a row's entries: the entries of each kind, in order, row by row
        assert np.array_equal(s["col_d"], col[loc] - r0) and np.array_equal(s["val_d"], val[loc])
        assert np.array_equal(s["garray"][s["col_o"]], col[~loc]) and np.array_equal(s["val_o"], val[~loc])
        assert np.array_equal(s["rp_d"], np.concatenate([[0], np.cumsum(np.bincount(rows[loc], minlength=r1 - r0))]))
        assert np.array_equal(s["rp_o"], np.concatenate([[0], np.cumsum(np.bincount(rows[~loc], minlength=r1 - r0))]))
        assert np.array_equal(s["rp_d"] + s["rp_o"], rp)


def test_split_block_rejections(lib):
    """The row and the column ks_mat_create_csr names in its two messages; rows are checked in order, a row's pointer before its columns."""
    s = ah.split_block(lib, 3, 0, 3, [0, 2, 1, 3], [0, 1, 2], [1.0, 2.0, 3.0])
    assert (s["status"], s["bad_row"]) == (ah.SPLIT_ROWPTR, 1)
    s = ah.split_block(lib, 3, 0, 3, [0, 1, 2, 3], [0, 1, -1], [1.0, 2.0, 3.0])
    assert (s["status"], s["bad_row"], s["bad_col"]) == (ah.SPLIT_COLUMN, 2, -1)
    s = ah.split_block(lib, 2, 4, 7, [0, 1, 3], [5, 2, 7], [1.0, 2.0, 3.0])                  # column n_global; column 2 before it is a ghost
    assert (s["status"], s["bad_row"], s["bad_col"]) == (ah.SPLIT_COLUMN, 1, 7)
    s = ah.split_block(lib, 3, 0, 3, [0, 1, 0, 1], [9], [1.0])                                # row 0's column is met before row 1's pointer
    assert (s["status"], s["bad_row"], s["bad_col"]) == (ah.SPLIT_COLUMN, 0, 9)
    s = ah.split_block(lib, 2, 4, 7, [0, 1, 3], [5, 2, 4], [1.0, 2.0, 3.0])                  # nothing to refuse: one ghost
    assert s["status"] == 0 and list(s["garray"]) == [2] and list(s["col_d"]) == [1, 0] and list(s["col_o"]) == [0]


@pytest.mark.parametrize("name,world", WORLDS + [("banded8", 8)])
def test_halo_plan_rank_by_rank(lib, name, world):
    c = case(name, world)
    want = sc.forward_plan(c)
    starts = c.starts.astype(np.int32)
    garray = [split_rank(lib, c, rank)["garray"] for rank in range(world)]
    counts = []
    for rank in range(world):
        st, cnt = ah.halo_recv_counts(lib, garray[rank], starts, rank)
        assert st == 0 and cnt.sum() == len(garray[rank]) and cnt[rank] == 0
        assert not np.any(cnt[np.asarray(c.counts) == 0])                                    # a rank without rows owns nothing
        counts.append(cnt)
    all_cnt = np.stack(counts)                                                                # the allgather: row p = rank p's counts
    plans = [ah.halo_peers(lib, rank, counts[rank], all_cnt) for rank in range(world)]
    for rank in range(world):
        pl, w = plans[rank], want[rank]
        assert np.array_equal(garray[rank], w["ghosts"])
        for k in ("peers", "rcnt", "scnt", "roff", "soff"):
            assert np.array_equal(pl[k], np.asarray(w[k], dtype=np.int32)), (name, rank, k)
        assert pl["nsend"] == len(w["send_idx"]) == int(np.sum(pl["scnt"]))
    for rank in range(world):                                                                 # the exchange: every rank sends its ghost segments, as global ids, to their owners
        pl = plans[rank]
        ids = np.full(pl["nsend"], -1, np.int32)
        for i, q in enumerate(pl["peers"]):
            pq = plans[q]
            j = list(pq["peers"]).index(rank)
            assert pq["rcnt"][j] == pl["scnt"][i]
            ids[pl["soff"][i]:pl["soff"][i] + pl["scnt"][i]] = garray[q][pq["roff"][j]:pq["roff"][j] + pq["rcnt"][j]]
        r0, r1 = c.range(rank)
        st, sidx = ah.halo_localize_send_idx(lib, r0, r1 - r0, ids)
        assert st == 0 and np.array_equal(sidx, want[rank]["send_idx"]), (name, rank)
    if name == "islands":                                                                     # no exchange at all, send only, receive only
        assert len(plans[1]["peers"]) == 0
        assert list(plans[2]["peers"]) == [3] and list(plans[2]["rcnt"]) == [0] and plans[2]["scnt"][0] > 0
        assert list(plans[3]["peers"]) == [0, 2] and list(plans[3]["rcnt"])[0] == 0 and plans[3]["scnt"][1] == 0


def test_halo_plan_rejections(lib):
    st, _ = ah.halo_recv_counts(lib, [1], [0, 5, 3, 10], 0)
    assert st == ah.HALO_UNORDERED                                                           # "row blocks must be contiguous and ordered by rank"
    st, _ = ah.halo_recv_counts(lib, [1, 4, 7], [0, 3, 6, 9], 1)
    assert st == ah.HALO_SELF                                                                # "ghost column owned by self"
    st, cnt = ah.halo_recv_counts(lib, [1, 7, 8], [0, 3, 3, 6, 9], 2)                         # rank 1 has no rows: column 3 onwards is rank 2's
    assert st == 0 and list(cnt) == [1, 0, 0, 2]
    assert ah.halo_localize_send_idx(lib, 3, 3, [3, 5, 6])[0] == ah.HALO_NOT_OWNED           # "peer requested a row this rank does not own"
    assert ah.halo_localize_send_idx(lib, 3, 3, [2])[0] == ah.HALO_NOT_OWNED
    st, sidx = ah.halo_localize_send_idx(lib, 3, 3, [5, 3, 3])
    assert st == 0 and list(sidx) == [2, 0, 0]


@functools.lru_cache(maxsize=None)
def binned_matrix(n):
    """Rows of 0 ... 40 entries (about 5 % of the rows empty), columns uniform over [0, n): unsorted, with duplicates; integer values of at most 8 in
    magnitude and an integer x with |x| <= 64 - every sum is an integer below 40 * 8 * 64, exact in any order. -> rowptr, col, val, x, A x"""
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 41, size=n); lens[rng.random(n) < 0.05] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.integers(0, n, size=int(rowptr[-1])).astype(np.int32)
    col[1::17] = col[0:-1:17]                                                # repeated columns next to each other (mostly inside a row)
    ival = sc._small_ints(rng, len(col))
    x = sc.int_vectors(n, 1, seed=n + 1)[0]
    S = sp.csr_matrix((ival.copy(), col.copy(), rowptr.copy()), shape=(n, n))                  # (scipy may sort its arrays in place: copies)
    ref = S @ x.astype(np.int64)
    return rowptr, col, ival.astype(np.float64), x, ref


@pytest.mark.timeout(120)
@pytest.mark.parametrize("ncu", [4, 256])                  # few long slices; many slices of a few columns each
@pytest.mark.parametrize("n", [4096, 5000, 70001])
def test_binned_plan(lib, n, ncu):
    rowptr, col, val, x, ref = binned_matrix(n)
    pad = ah.BN_SEG_PAD
    p = ah.binned_plan(lib, n, rowptr, col, val, ncu, x=x)
    ns, cs, wb, wr, nwin, entries = (p[k] for k in ("ns", "cs", "wb", "wr", "nwin", "entries"))
    st, geo = ah.binned_geometry(lib, n, len(col), ncu)
    assert st == 0 and geo == {"ns": ns, "cs": cs, "wb": wb, "wr": wr}
    assert ns % ncu == 0 and cs <= ah.BN_CS_MAX and ns * cs >= n and wb == 4 * ns and wb * wr >= n
    assert ns == (8 if (n, ncu) == (70001, 4) else ncu)                                      # 70001 columns on 4 CUs: two rounds of slices
    # the product, through the walk of the two kernels
    assert np.array_equal(p["y"], ref.astype(np.float64))
    # the segments: entries of wave-bin b (rows) in slice s (columns), padded
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    cnt = np.bincount((rows // wr) * ns + col // cs, minlength=wb * ns).reshape(wb, ns)
    length = (cnt + pad - 1) // pad * pad
    assert np.array_equal(np.diff(p["log2"], axis=1), length) and np.all(p["log2"][:, 0] == 0)
    assert np.array_equal(p["log2"][:, ns], length.sum(axis=1))                              # the padded entry count of the wave-bin
    assert np.array_equal(np.diff(p["off1"], axis=1), length.T) and np.all(p["off1"][:, 0] == 0)
    assert np.all(p["off2"] % pad == 0) and np.all(length % pad == 0) and np.array_equal(p["off2t"], p["off2"].T)
    assert p["sbase"][0] == 0 and np.array_equal(np.diff(p["sbase"]), length.sum(axis=0)) and p["sbase"][ns] == entries == length.sum()
    # bin-major: the segments tile [0, entries) without overlap
    order = np.lexsort((length.ravel(), p["off2"].ravel()))       # by start; an empty segment before the one that starts where it does
    o2, ln = p["off2"].ravel()[order], length.ravel()[order]
    assert o2[0] == 0 and np.array_equal(o2[1:], np.cumsum(ln)[:-1])
    # padding: behind the real entries of every segment - row wr (the spare accumulator), value 0, column 0
    def behind(start, real):                                   # positions start[i] + real[i] ... start[i] + length[i] - 1 of every segment i
        npad = (length.ravel() - real).astype(np.int64)
        first = (start + real).astype(np.int64)
        return np.repeat(first - np.concatenate([[0], np.cumsum(npad)[:-1]]), npad) + np.arange(npad.sum())
    pad2 = behind(p["off2"].ravel(), cnt.ravel())
    is_pad = np.zeros(entries, bool); is_pad[pad2] = True
    assert entries - len(pad2) == len(col)
    assert np.array_equal(p["row16"] == wr, is_pad) and np.all(p["val2"][is_pad] == 0.0) and np.all(p["val2"][~is_pad] != 0.0)
    pad1 = behind((p["sbase"][:ns, None] + p["off1"][:, :wb]).T.ravel(), cnt.ravel())      # the same segments in slice-major order
    assert len(pad1) == len(pad2) and np.all(p["col16"][pad1] == 0) and int(p["col16"].max()) < cs
    # wseg: the segment that holds the first entry of each 1024-entry window of a slice
    assert nwin == max(1, int((p["off1"][:, wb].max() + 1023) // 1024))
    for s in range(ns):
        o1 = p["off1"][s]
        base = np.arange(0, o1[wb], 1024)
        sg = p["wseg"][s, :len(base)]
        assert np.all(o1[sg] <= base) and np.all(base < o1[sg + 1])


def test_binned_geometry_refusals(lib):
    """Rows and columns are stored in 16 bits, wr itself being the spare accumulator's index. With the product's slices of at most 9984 columns
    wr (about cs / 4) stays far below that; the refusal shows with a larger cs_max: one CU, n = 300000 -> one slice, wr + 1 = 75001 > 65535."""
    st, geo = ah.binned_geometry(lib, 300000, 10 ** 6, 1, cs_max=1 << 20)
    assert geo["ns"] == 1 and geo["wr"] + 1 == 75001 and st == ah.BINNED_16BIT
    st, geo = ah.binned_geometry(lib, 200000, 10 ** 6, 1, cs_max=1 << 20)                     # wr + 1 = 50001 fits, cs = 200000 does not
    assert geo["wr"] + 1 == 50001 and geo["cs"] == 200000 and st == ah.BINNED_16BIT
    assert ah.binned_geometry(lib, 70001, 2 ** 31 - 1 - 8 * 32 * 7, 4)[0] == ah.BINNED_32BIT        # ns = 8, wb = 32: 7 entries of padding per segment at most
    assert ah.binned_geometry(lib, 70001, 2 ** 31 - 2 - 8 * 32 * 7, 4)[0] == 0
