"""The projected problem of Generalized Davidson (slepc_amd/csrc/ks_ds.cpp: DsGd - H = V^T A V, its sorted eigenvectors Q, the Q of the previous
iteration) against numpy. CPU only: the hook ksd_gd works on caller-owned ld x ld arrays.

Tolerance, on the scale of tests/test_dense_host.py: tol = 50 m eps max(1, max|H|), m the order. It applies to the orthonormality of the restart
basis Z, to its span (the projector Z Z^T against the one of numpy.linalg.qr of the same block), to Z^T H Z and to the eigenvalues; the order
under each `which` is checked on spectra whose values are separated by 1e3 tol."""
import ctypes as C
import os

import numpy as np
import pytest

import slepc_amd._lib as L

P = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
EPS = np.finfo(float).eps
LARGEST_MAGNITUDE, SMALLEST_MAGNITUDE, LARGEST_REAL, SMALLEST_REAL, TARGET_MAGNITUDE, TARGET_REAL = 1, 2, 3, 4, 7, 8
GROW, SOLVE, LOCK, RESTART, PROJECT, SAVE = 0, 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksd_gd.argtypes = [C.c_int, C.c_int, IP, P, P, P, P, C.c_int, C.c_double, C.c_int, C.c_int, P, C.c_int]
    return lib


def p(a):
    return a.ctypes.data_as(P)


class Gd:
    """the arrays of one DsGd on the Python side"""

    def __init__(self, lib, ld, which=SMALLEST_REAL, target=0.0):
        self.lib, self.ld, self.which, self.target = lib, ld, which, target
        self.H = np.zeros((ld, ld), order="F"); self.Q = np.zeros((ld, ld), order="F"); self.U = np.zeros((ld, ld), order="F"); self.w = np.zeros(ld)
        self.dims = np.zeros(2, dtype=np.int32)
        self.Z = np.zeros((ld, ld), order="F")

    def step(self, op, a0=0, a1=0):
        return self.lib.ksd_gd(op, self.ld, self.dims.ctypes.data_as(IP), p(self.H), p(self.Q), p(self.U), p(self.w), self.which, self.target, a0, a1, p(self.Z), self.ld)

    @property
    def n(self):
        return int(self.dims[0])

    def load(self, Hm):
        m = Hm.shape[0]
        self.H[:] = 0.0; self.H[:m, :m] = Hm; self.dims[0] = m


def sym(rng, n, scale=1.0):
    M = rng.standard_normal((n, n)) * scale
    return (M + M.T) / 2


def tol_of(m, H):
    return 50 * m * EPS * max(1.0, np.abs(H).max())


@pytest.mark.parametrize("m", [2, 7, 20, 48])
def test_grow_by_columns_gives_the_symmetric_matrix(lib, m):
    rng = np.random.default_rng(10 + m)
    Hm = sym(rng, m)
    g = Gd(lib, m + 3)
    first = max(1, m // 2)
    for n0, n1 in ((0, first), (first, m)):
        if n1 == n0:
            continue
        g.Z[:] = 0.0; g.Z[:n1, :n1 - n0] = Hm[:n1, n0:n1]
        assert g.step(GROW, n1 - n0) == 0 and g.n == n1
    assert np.array_equal(g.H[:m, :m], Hm) and not g.H[m:, :].any() and not g.H[:, m:].any()


@pytest.mark.parametrize("m", [2, 7, 20, 48])
@pytest.mark.parametrize("which,target", [(SMALLEST_REAL, 0.0), (LARGEST_REAL, 0.0), (LARGEST_MAGNITUDE, 0.0), (SMALLEST_MAGNITUDE, 0.0), (TARGET_MAGNITUDE, 0.7), (TARGET_REAL, -0.3)])
def test_solve_and_sort(lib, m, which, target):
    """Eigenvalues against numpy.linalg.eigvalsh; H = Q diag(w) Q^T with orthonormal Q; the order under `which` on a spectrum separated by 1e3 tol."""
    rng = np.random.default_rng(100 * which + m)
    Qm, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = rng.permutation(np.linspace(-1.0, 1.3, m) + 0.011)              # distinct values and distinct magnitudes, gaps > 1e3 tol
    Hm = (Qm * lam) @ Qm.T; Hm = (Hm + Hm.T) / 2
    tol = tol_of(m, Hm)
    key = {SMALLEST_REAL: lambda x: x, LARGEST_REAL: lambda x: -x, LARGEST_MAGNITUDE: lambda x: -abs(x), SMALLEST_MAGNITUDE: lambda x: abs(x),
           TARGET_MAGNITUDE: lambda x: abs(x - target), TARGET_REAL: lambda x: abs(x - target)}[which]
    ref = np.array(sorted(np.linalg.eigvalsh(Hm), key=key))
    keys = np.array([key(x) for x in ref])
    assert m == 1 or np.diff(keys).min() > 1e3 * tol
    g = Gd(lib, m + 2, which, target); g.load(Hm)
    assert g.step(SOLVE) == 0
    w, Q = g.w[:m], g.Q[:m, :m]
    print("m=%d which=%d  eig err %.2e  (tol %.2e)" % (m, which, np.abs(w - ref).max(), tol))
    assert np.abs(w - ref).max() <= tol
    assert np.abs(Q.T @ Q - np.eye(m)).max() <= tol
    assert np.abs((Q * w) @ Q.T - Hm).max() <= tol
    assert np.array_equal(g.H[:m, :m], Hm)                                  # H is kept


@pytest.mark.parametrize("m,npre", [(2, 1), (7, 1), (7, 3), (20, 4), (48, 16), (3, 3)])
def test_locking_leaves_the_diagonal_of_the_remaining_ritz_values(lib, m, npre):
    rng = np.random.default_rng(300 + m + npre)
    g = Gd(lib, m + 1); g.load(sym(rng, m))
    assert g.step(SOLVE) == 0
    w = g.w[:m].copy()
    g.dims[1] = m                                                           # an oldU is there: locking forgets it
    assert g.step(LOCK, npre) == 0
    assert g.n == m - npre and g.dims[1] == 0
    assert np.array_equal(g.H[:m - npre, :m - npre], np.diag(w[npre:]))
    assert np.array_equal(g.w[:m - npre], w[npre:])


def restart_case(lib, m, size_X, size_plusk, mu, seed, old_equals_q=False):
    """H of order m, solved; oldU of order mu <= m (orthonormal columns of a random matrix, or Q itself); returns the objects of the checks"""
    rng = np.random.default_rng(seed)
    Hm = sym(rng, m, 3.0)
    g = Gd(lib, m + 2); g.load(Hm)
    assert g.step(SOLVE) == 0
    Q = g.Q[:m, :m].copy()
    if old_equals_q:
        g.U[:m, :m] = Q; g.dims[1] = m
    else:
        Um, _ = np.linalg.qr(rng.standard_normal((mu, mu)))
        g.U[:] = 0.0; g.U[:mu, :mu] = Um; g.dims[1] = mu
    Upad = np.zeros((m, size_plusk)); k = int(g.dims[1])
    Upad[:k, :] = g.U[:k, :size_plusk]
    block = np.hstack([Q[:, :size_X], Upad])
    kept = g.step(RESTART, size_X, size_plusk)
    return g, Hm, block, kept


@pytest.mark.parametrize("m", [2, 7, 20, 48])
@pytest.mark.parametrize("size_plusk", [0, 1, 2])
@pytest.mark.parametrize("short", [False, True])
def test_restart_basis_against_numpy_qr(lib, m, size_plusk, short):
    """Z = orth([Q(:, 0:size_X), oldU(:, 0:size_plusk)]), oldU of the current order or shorter (zero-padded); then H <- Z^T H Z"""
    size_X = max(1, min(6, m // 2))
    size_plusk = min(size_plusk, m - size_X)                                # the block has at most as many columns as rows (the solver's rule too)
    mu = max(1, size_plusk, m - 3) if short else m
    g, Hm, block, kept = restart_case(lib, m, size_X, size_plusk, mu, 1000 * m + 10 * size_plusk + short)
    ncol = block.shape[1]
    tol = tol_of(m, Hm)
    assert kept == ncol                                                      # a random orthonormal oldU is independent of the Ritz vectors
    Z = g.Z[:m, :kept].copy()
    Qn, _ = np.linalg.qr(block)
    print("m=%d plusk=%d short=%d  orth %.2e  span %.2e  (tol %.2e)" % (m, size_plusk, short, np.abs(Z.T @ Z - np.eye(kept)).max(), np.abs(Z @ Z.T - Qn @ Qn.T).max(), tol))
    assert np.abs(Z.T @ Z - np.eye(kept)).max() <= tol
    assert np.abs(Z @ Z.T - Qn @ Qn.T).max() <= tol
    assert np.abs(Z[:, :size_X] - g.Q[:m, :size_X]).max() <= tol             # the Ritz vectors are orthonormal already: they stay
    assert g.step(PROJECT, kept) == 0
    assert g.n == kept and g.dims[1] == 0
    G = g.H[:kept, :kept]
    assert np.abs(G - Z.T @ Hm @ Z).max() <= tol
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("m", [2, 7, 20, 48])
@pytest.mark.parametrize("size_plusk", [1, 2])
def test_restart_basis_drops_dependent_columns(lib, m, size_plusk):
    """oldU equal to Q: every added column lies in the span of the Ritz vectors kept, the kept count is size_X"""
    size_X = max(size_plusk, min(6, m // 2))
    g, Hm, block, kept = restart_case(lib, m, size_X, size_plusk, m, 2000 * m + size_plusk, old_equals_q=True)
    assert kept == size_X
    Z = g.Z[:m, :kept]
    tol = tol_of(m, Hm)
    assert np.abs(Z.T @ Z - np.eye(kept)).max() <= tol
    assert np.abs(Z - g.Q[:m, :size_X]).max() <= tol


def test_save_old_u_copies_q_and_its_order(lib):
    rng = np.random.default_rng(7)
    g = Gd(lib, 9); g.load(sym(rng, 6))
    assert g.step(SOLVE) == 0
    g.U[:] = 5.0
    assert g.step(SAVE) == 0 and g.dims[1] == 6
    assert np.array_equal(g.U[:6, :6], g.Q[:6, :6]) and not g.U[6:, :].any() and not g.U[:, 6:].any()
