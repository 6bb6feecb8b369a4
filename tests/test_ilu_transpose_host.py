"""The transposed level layout of the ILU(0) blocks on the host (the second plan of ksc::csr_ilu0_blocks and ksc::ilu0_apply_transpose_host,
slepc_amd/csrc/ks_csr.cpp: what k_bjacobi_ilu_apply_t walks), through the test hook libksgpu.so exports. CPU only. The matrices are those of
tests/test_ilu_host.py; the reference is tests/ilu_cases.py's, the bound tests/ilu_transpose_cases.py's:

    |M^T y - x| <= 8 (k + 1) 2^-53 (|U^T||L^T||y|),   M = L U,   k = the larger of the block's longest row and longest column.

With scipy's triangular solves as the solver the reference itself stays at or below 0.12 of that bound on every case here."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import ilu_cases as ic
import ilu_transpose_cases as itc
import slepc_amd._lib as L

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LLP = C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_ilu0_blocks_transpose.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, DP, DP, DP, DP, IP, LLP]
    lib.ksc_ilu0_blocks_transpose.restype = C.c_longlong
    return lib


def transposed(lib, arr, bs, x, row_start=0):
    """(y_t = (LU)^-T x and y_f = (LU)^-1 x through the two level layouts, the six figures per block, info)."""
    rp, col, val = arr
    n = len(rp) - 1
    nblk = (n + bs - 1) // bs
    info = np.zeros(7, dtype=np.int64); per = np.zeros((nblk, 6), dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    yt = np.full(n, np.nan); yf = np.full(n, np.nan)
    ent = lib.ksc_ilu0_blocks_transpose(n, row_start, bs, rp.ctypes.data_as(IP), col.ctypes.data_as(IP), val.ctypes.data_as(DP), x.ctypes.data_as(DP),
                                        yt.ctypes.data_as(DP), yf.ctypes.data_as(DP), per.ctypes.data_as(IP), info.ctypes.data_as(LLP))
    assert ent >= 0, info
    return yt, yf, per, info


def _check(lib, arr, bs, ref, seed, what, row_start=0):
    x = np.random.default_rng(seed).standard_normal(ref.n)
    yt, yf, per, info = transposed(lib, arr, bs, x, row_start)
    itc.check_t(ref, x, yt, what)
    r = max(itc.ratios_t(ref, x, itc.solve_t(ref, x)))
    print("%s: scipy's triangular solves sit at %.3g of the bound" % (what, r))
    assert r <= 0.12, (what, r)
    ref.check(x, yf, what + " (forward plan built beside the transposed one)")
    assert info[6] == 1, what                                                  # the forward plan's arrays are what they are without the transposed one
    assert len(per) == len(ref.blocks)
    for (nLf, nUf, n1t, n2t, top, bl), blk in zip(per, ref.blocks):
        assert bl == blk[1]
        assert n1t + n2t == nLf + nUf, (what, per)                             # as many levels as the forward solve ...
        assert n1t == nUf and n2t == nLf, (what, per)                          # ... phase by phase: U^T is as deep as U, L^T as deep as L
        assert top < bl, (what, per)                                           # every code and every listed row inside the block
    assert info[3] == max(int(np.max(np.bincount(b[6].indices, minlength=b[1]))) for b in ref.blocks)     # the longest column
    return per, info


@pytest.mark.parametrize("n,bs", [(8192, 8192), (64, 64), (150, 64)])
def test_dense_row_and_dense_column_swap_roles(lib, n, bs):
    A = ic.arrow(n)
    P = ic.shifted(A, ic.SIGMA)
    per, info = _check(lib, ic.arrays(P), bs, ic.Reference.of(P, bs), 1, "arrow n=%d bs=%d" % (n, bs))
    if n == bs:
        # the dense row of U is now a column of U^T: a level of n - 1 rows with one slot each, reading code 0 (L^T: code n - 1); the longest
        # column holds three entries; two levels per phase, no padding
        assert info[3] == 3 and info[4] == 4 and info[5] == 2 * (n - 1) and per[0][4] == n - 1


def test_unsorted_rows_with_repeated_entries(lib):
    raw, S = ic.scrambled(200)
    ref = ic.Reference.of(S, 64)
    x = np.random.default_rng(2).standard_normal(200)
    y_raw = transposed(lib, raw, 64, x)[0]
    y_sorted = transposed(lib, ic.arrays(S), 64, x)[0]
    assert np.array_equal(y_raw, y_sorted)
    _check(lib, raw, 64, ref, 2, "scrambled")


@pytest.mark.parametrize("n,bs,per_row", [(193, 64, 6), (63, 64, 4), (300, 128, 20)])
def test_random_patterns_partial_blocks_and_a_row_offset(lib, n, bs, per_row):
    A = ic.random_sparse(n, per_row, n)
    P = ic.shifted(A, ic.SIGMA)
    _check(lib, ic.arrays(P), bs, ic.Reference.of(P, bs), 3, "random n=%d" % n)
    rng = np.random.default_rng(4)
    G = sp.hstack([sp.random(n, 1000, density=0.002, random_state=rng), P, sp.random(n, 500, density=0.002, random_state=rng)]).tocsr(); G.sort_indices()
    _check(lib, ic.arrays(G), bs, ic.Reference.of(P, bs), 5, "offset n=%d" % n, row_start=1000)


def test_levels_of_diagonal_and_bidiagonal_blocks(lib):
    P = ic.shifted(ic.diagonal(130), ic.SIGMA)
    per, info = _check(lib, ic.arrays(P), 64, ic.Reference.of(P, 64), 6, "diagonal")
    assert info[4] == 2 * 3 and info[5] == 0
    P = ic.shifted(ic.bidiagonal(130), ic.SIGMA)
    per, info = _check(lib, ic.arrays(P), 64, ic.Reference.of(P, 64), 7, "bidiagonal")
    # the lower bidiagonal's chain now sits in the second phase (L^T, upper bidiagonal); the first phase (U^T, diagonal) is one level
    assert [tuple(p[2:4]) for p in per] == [(1, 64), (1, 64), (1, 2)] and info[5] == 63 * 2 + 1


def test_the_transposed_solve_is_not_the_forward_one(lib):
    """On the arrow and on the convection pencil the forward result misses the transposed bound: the test tells the two apart."""
    for S, bs in ((ic.arrow(64), 64), (ic.line_pencil(32, 11)[0], 128)):
        P = ic.shifted(S, ic.SIGMA)
        ref = ic.Reference.of(P, bs)
        x = np.random.default_rng(8).standard_normal(ref.n)
        yt, yf, _, _ = transposed(lib, ic.arrays(P), bs, x)
        itc.check_t(ref, x, yt, "transposed")
        assert max(itc.ratios_t(ref, x, yf)) > 1.0
