"""The host LU inverse behind the Jacobi-Davidson projector (ksd::lu_inverse, slepc_amd/csrc/ks_dense.cpp) against numpy. CPU only: the C hook is
exported by libksgpu.so and does not touch the GPU.

Bound. LU with partial pivoting is backward stable up to the growth factor, which is of order one on the random matrices here: the computed inverse X
satisfies |X - M^-1| <= c n eps cond(M) |M^-1| entrywise in norm; asserted as ||X - inv(M)||_max <= 8 n eps cond_2(M) ||inv(M)||_max, and the residual
||M X - I||_max <= 8 n eps ||M||_inf ||X||_inf. A matrix of rank n - 1 built from integers (its elimination is exact, the last pivot is exactly 0) and one
whose last pivot is a rounding error of size eps ||M|| must both be reported singular: the test is pivot <= n eps ||M||_inf."""
import ctypes as C
import os

import numpy as np
import pytest

import slepc_amd._lib as L

P = C.POINTER(C.c_double)
EPS = np.finfo(float).eps


def p(a):
    return a.ctypes.data_as(P)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksd_lu_inverse.argtypes = [C.c_int, P, C.c_int, P, C.c_int]
    lib.ksd_lu_inverse.restype = C.c_int
    return lib


def _inverse(lib, M, ldm=None, ldi=None):
    n = M.shape[0]
    ldm = ldm or n; ldi = ldi or n
    Mp = np.full((ldm, n), 77.0, order="F"); Mp[:n] = M
    Xp = np.full((ldi, n), -5.0, order="F")
    rc = lib.ksd_lu_inverse(n, p(Mp), ldm, p(Xp), ldi)
    assert np.array_equal(Mp[:n], M, equal_nan=True) and np.all(Mp[n:] == 77.0)            # M is left alone
    assert np.all(Xp[n:] == -5.0)                                          # rows past n of Minv are not written
    return rc, Xp[:n].copy()


@pytest.mark.parametrize("n", [1, 2, 7, 33, 64])
def test_lu_inverse_against_numpy(lib, n):
    rng = np.random.default_rng(900 + n)
    for trial, pad in enumerate((0, 3)):
        M = rng.standard_normal((n, n)) + (2.0 if trial else 0.0) * np.eye(n)
        rc, X = _inverse(lib, M, n + pad, n + 2 * pad)
        assert rc == 0
        ref = np.linalg.inv(M)
        cond = np.linalg.cond(M)
        err = np.abs(X - ref).max(); res = np.abs(M @ X - np.eye(n)).max()
        print("n=%d cond %.2e  err %.2e (bound %.2e)  residual %.2e" % (n, cond, err, 8 * n * EPS * cond * np.abs(ref).max(), res))
        assert err <= 8 * n * EPS * cond * np.abs(ref).max()
        assert res <= 8 * n * EPS * np.abs(M).sum(axis=1).max() * np.abs(X).sum(axis=1).max()


def test_identity_and_permutation_are_exact(lib):
    rc, X = _inverse(lib, np.eye(5))
    assert rc == 0 and np.array_equal(X, np.eye(5))
    Pm = np.eye(6)[[3, 0, 5, 1, 2, 4]]
    rc, X = _inverse(lib, 2.0 * Pm)
    assert rc == 0 and np.array_equal(X, 0.5 * Pm.T)


@pytest.mark.parametrize("n", [2, 7, 33])
def test_rank_deficient_matrix_is_reported_singular(lib, n):
    rng = np.random.default_rng(40 + n)
    Z = rng.integers(-3, 4, size=(n, n - 1)).astype(float)
    M = Z @ rng.integers(-3, 4, size=(n - 1, n)).astype(float)             # rank <= n - 1, integer entries
    rc, X = _inverse(lib, M)
    assert rc == 1 and np.all(X == -5.0)                                   # Minv untouched
    # rank n - 1 in floating point: the last pivot is rounding noise, far below n eps ||M||_inf
    G = rng.standard_normal((n, n - 1)); Mf = G @ rng.standard_normal((n - 1, n))
    rc, X = _inverse(lib, Mf)
    assert rc == 1
    assert _inverse(lib, np.zeros((3, 3)))[0] == 1
    nanm = np.eye(3); nanm[1, 1] = np.nan
    assert _inverse(lib, nanm)[0] == 1                                     # not finite: singular, never an inverse of NaNs
    # well inside the regular side of the threshold
    assert _inverse(lib, np.eye(n) + 1e-3 * rng.standard_normal((n, n)))[0] == 0
