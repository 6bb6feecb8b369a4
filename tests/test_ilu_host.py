"""ILU(0) of the diagonal blocks on the host (ksc::csr_ilu0_blocks, slepc_amd/csrc/ks_csr.cpp): the factorisation and the level layout that
k_bjacobi_ilu_apply walks, through the test hook libksgpu.so exports. CPU only. The reference and the bound: tests/ilu_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import ilu_cases as ic
import slepc_amd._lib as L

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LLP = C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_ilu0_blocks.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, DP, IP, IP, DP, C.c_longlong, DP, DP, LLP]
    lib.ksc_ilu0_blocks.restype = C.c_longlong
    return lib


def _i(a):
    return a.ctypes.data_as(IP)


def _d(a):
    return a.ctypes.data_as(DP)


def factor(lib, arr, bs, x=None, row_start=0):
    """(factors as CSR arrays on the blocks' sorted patterns, y = (LU)^-1 x through the level layout, info) or the failing (status, block, row)."""
    rp, col, val = arr
    n = len(rp) - 1
    info = np.zeros(6, dtype=np.int64)
    frp = np.zeros(n + 1, dtype=np.int32); fcol = np.zeros(max(len(col), 1), dtype=np.int32); fval = np.zeros(max(len(col), 1))
    x = np.zeros(n) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(n, np.nan)
    nnz = lib.ksc_ilu0_blocks(n, row_start, bs, _i(rp), _i(col), _d(val), _i(frp), _i(fcol), _d(fval), len(fcol), _d(x), _d(y), info.ctypes.data_as(LLP))
    if nnz < 0:
        return tuple(int(v) for v in info[:3])
    return (frp, fcol[:nnz], fval[:nnz]), y, info


def _check(lib, arr, bs, ref, seed, what, row_start=0):
    x = np.random.default_rng(seed).standard_normal(ref.n)
    (frp, fcol, fval), y, info = factor(lib, arr, bs, x, row_start)
    ref.check(x, y, what)
    # the factors themselves: same pattern, same order, one rounding per operation on both sides - the same numbers
    for b0, bl, Lr, Ur, k, P, F in ref.blocks:
        sl = slice(frp[b0], frp[b0 + bl])
        assert np.array_equal(fcol[sl], F.indices) and np.array_equal(np.diff(frp[b0:b0 + bl + 1]), np.diff(F.indptr)), (what, b0)
        assert np.array_equal(fval[sl], F.data), (what, b0)
        # and the defining property of ILU(0): L U equals P on the pattern, to the rounding of a dot product of k terms
        LU = (Lr @ Ur).tocsr(); bound = 8.0 * (k + 1) * ic.U53 * (abs(Lr) @ abs(Ur)).tocsr()
        rr = np.repeat(np.arange(bl), np.diff(P.indptr))
        assert np.all(np.abs(np.asarray(LU[rr, P.indices]).ravel() - P.data) <= np.asarray(bound[rr, P.indices]).ravel()), (what, b0)
    assert info[3] == max(b[4] for b in ref.blocks)
    return info


@pytest.mark.parametrize("n,bs", [(8192, 8192), (64, 64), (150, 64)])
def test_longest_rows_and_the_largest_column_code(lib, n, bs):
    """Item 3 of the kernel cases: a last row dense to the left and a first row dense to the right (at 8192: code 8191, a level of one row with
    8191 slots); with 150 rows in blocks of 64 the dense rows lose what lies outside their block and the last block has 22 rows."""
    A = ic.arrow(n)
    P = ic.shifted(A, ic.SIGMA)
    info = _check(lib, ic.arrays(P), bs, ic.Reference.of(P, bs), 1, "arrow n=%d bs=%d" % (n, bs))
    if n == bs:
        assert info[3] == n and info[4] == 4 and info[5] == 2 * (n - 1)          # two levels per solve, no padding


def test_unsorted_rows_with_repeated_entries(lib):
    """Item 5: unsorted columns, repeated entries, a diagonal stored three times - the factors of the summed, sorted matrix."""
    raw, S = ic.scrambled(200)
    ref = ic.Reference.of(S, 64)
    (frp, fcol, fval), y, _ = factor(lib, raw, 64, np.ones(200))
    (grp, gcol, gval), y2, _ = factor(lib, ic.arrays(S), 64, np.ones(200))
    assert np.array_equal(frp, grp) and np.array_equal(fcol, gcol) and np.array_equal(fval, gval) and np.array_equal(y, y2)
    _check(lib, raw, 64, ref, 2, "scrambled")


@pytest.mark.parametrize("n,bs,per_row", [(193, 64, 6), (63, 64, 4), (300, 128, 20)])
def test_random_patterns_partial_blocks_and_a_row_offset(lib, n, bs, per_row):
    """Level widths of every kind, a short last block (one row at n = 193), one partial block (n = 63); with a row offset the columns are global
    and the entries outside the rank's own columns are dropped."""
    A = ic.random_sparse(n, per_row, n)
    P = ic.shifted(A, ic.SIGMA)
    _check(lib, ic.arrays(P), bs, ic.Reference.of(P, bs), 3, "random n=%d" % n)
    # the same rows as rows 1000 .. 1000 + n - 1 of a wider matrix: ghost columns on both sides
    rng = np.random.default_rng(4)
    G = sp.hstack([sp.random(n, 1000, density=0.002, random_state=rng), P, sp.random(n, 500, density=0.002, random_state=rng)]).tocsr(); G.sort_indices()
    _check(lib, ic.arrays(G), bs, ic.Reference.of(P, bs), 5, "offset n=%d" % n, row_start=1000)


def test_levels_of_diagonal_and_bidiagonal_blocks(lib):
    P = ic.shifted(ic.diagonal(130), ic.SIGMA)
    info = _check(lib, ic.arrays(P), 64, ic.Reference.of(P, 64), 6, "diagonal")
    assert info[4] == 2 * 3 and info[5] == 0                                       # one L and one U level per block, nothing off the diagonal
    P = ic.shifted(ic.bidiagonal(130), ic.SIGMA)
    info = _check(lib, ic.arrays(P), 64, ic.Reference.of(P, 64), 7, "bidiagonal")
    assert info[4] == (64 + 1) * 2 + (2 + 1) and info[5] == 63 * 2 + 1            # L: a level per row; U: one level


def test_missing_diagonal_and_zero_pivot(lib):
    S = sp.lil_matrix(ic.shifted(ic.random_sparse(100, 5, 8), ic.SIGMA))
    S[70, 70] = 0.0
    T = S.tocsr(); T.eliminate_zeros()
    assert factor(lib, ic.arrays(T), 64) == (1, 1, 70)
    Z = sp.lil_matrix(ic.shifted(ic.random_sparse(100, 5, 8), ic.SIGMA))
    Z[64, :] = 0.0; Z[65, :] = 0.0; Z[64, 64] = Z[64, 65] = Z[65, 64] = Z[65, 65] = 1.0
    assert factor(lib, ic.arrays(Z.tocsr()), 64) == (2, 1, 65)
    # an explicit zero on the diagonal is a stored entry: it is the pivot that is zero, not the entry that is missing
    rp, col, val = ic.arrays(T)
    E = sp.lil_matrix(T); E[70, 70] = 1.0; rp, col, val = ic.arrays(E.tocsr()); val[(col == 70) & (np.repeat(np.arange(100), np.diff(rp)) == 70)] = 0.0
    st = factor(lib, (rp, col, val), 64)
    assert st[0] == 2 and st[1] == 1 and st[2] == 70
