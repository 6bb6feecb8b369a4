"""The projected problem of LOBPCG (slepc_amd/csrc/ks_ds.cpp: DS GHEP, G_A q = theta G_B q with G_B positive definite) against numpy: the
test reduces the pencil by Cholesky itself, C = L^-1 G_A L^-T, and calls eigh. CPU only: the hook works on caller-owned arrays.

Bounds (eps = 2^-52, n = the order):
  eigenvalues          n eps ||C||_2              what a backward-stable symmetric solver of the reduced problem owes
  Q^T G_B Q = I        n eps cond_2(G_B)          the back substitution Q = L^-T Z
  G_A Q = G_B Q Theta  n eps cond_2(G_B), relative to ||G_A||_2 ||Q||_2 + ||G_B||_2 ||Q||_2 max|theta|"""
import ctypes as C
import os

import numpy as np
import pytest

import slepc_amd._lib as L

P = C.POINTER(C.c_double)
EPS = np.finfo(float).eps
SMALLEST_REAL, LARGEST_REAL = 4, 3


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksd_ghep.argtypes = [C.c_int, C.c_int, P, P, P, P, C.c_int]
    return lib


def p(a):
    return a.ctypes.data_as(P)


def ghep(lib, GA, GB, which=SMALLEST_REAL, pad=0):
    n = GA.shape[0]; ld = n + pad
    A = np.zeros((ld, ld), order="F"); B = np.zeros((ld, ld), order="F"); Q = np.zeros((ld, ld), order="F"); w = np.zeros(ld)
    A[:n, :n] = GA; B[:n, :n] = GB
    rc = lib.ksd_ghep(n, ld, p(A), p(B), p(Q), p(w), which)
    return rc, w[:n].copy(), Q[:n, :n].copy()


def sym(rng, n):
    M = rng.standard_normal((n, n))
    return (M + M.T) / 2


def spd(rng, n, cond):
    """orthogonal * diag(1 .. 1/cond, log-spaced) * orthogonal^T"""
    if n == 1:
        return np.array([[1.0]])
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    B = (Qm * np.logspace(0, -np.log10(cond), n)) @ Qm.T
    return (B + B.T) / 2


def graded_spd(rng, n, cond):
    """D S D with S of condition 10 and D = diag(1 .. cond^-1/2, log-spaced): the ill-conditioning of a Gram matrix [X R P]^T B [X R P] whose
    blocks have norms 1, ||r||, ||p|| - in the scaling of its columns, not in their directions"""
    d = np.logspace(0, -np.log10(cond) / 2, n)
    return spd(rng, n, 10.0) * np.outer(d, d)


def check(lib, GA, GB, which=SMALLEST_REAL, pad=0):
    n = GA.shape[0]
    rc, w, Q = ghep(lib, GA, GB, which, pad)
    assert rc == 0
    Lc = np.linalg.cholesky(GB)
    Cm = np.linalg.solve(Lc, np.linalg.solve(Lc, GA).T).T
    Cm = (Cm + Cm.T) / 2
    ref = np.linalg.eigvalsh(Cm)
    if which == LARGEST_REAL:
        ref = ref[::-1]
    nC = np.linalg.norm(Cm, 2); cond = np.linalg.cond(GB)
    print("n=%d  eig err %.2e (bound %.2e)" % (n, np.abs(w - ref).max(), n * EPS * nC))
    assert np.abs(w - ref).max() <= n * EPS * nC
    orth = np.abs(Q.T @ GB @ Q - np.eye(n)).max()
    print("      orth %.2e (bound %.2e)" % (orth, n * EPS * cond))
    assert orth <= n * EPS * cond
    scale = np.linalg.norm(Q, 2) * (np.linalg.norm(GA, 2) + np.linalg.norm(GB, 2) * np.abs(w).max())
    res = np.abs(GA @ Q - GB @ Q * w).max() / scale
    print("      res  %.2e (bound %.2e)" % (res, n * EPS * cond))
    assert res <= n * EPS * cond
    return w, Q


@pytest.mark.parametrize("n", [1, 2, 3, 12, 47, 48])
def test_identity_b(lib, n):
    rng = np.random.default_rng(100 + n)
    check(lib, sym(rng, n), np.eye(n))


@pytest.mark.parametrize("n", [1, 2, 3, 12, 47, 48])
def test_well_conditioned_b(lib, n):
    rng = np.random.default_rng(200 + n)
    check(lib, sym(rng, n), spd(rng, n, 10.0), pad=3)


@pytest.mark.parametrize("n", [2, 3, 12, 47, 48])
def test_b_with_condition_1e8(lib, n):
    """A G_B of condition 1e7 .. 1e9 whose ill-conditioning is a grading. With the ill-conditioning in the directions instead (a rotated diagonal)
    the Cholesky factor's last pivot is a difference of numbers 1e8 times its size, the eigenvalue next to -||C|| moves by eps cond(G_B) ||C|| with
    the rounding of that pivot, and numpy's own reduction misses the exact eigenvalue by 1e6 times the bound n eps ||C||: two Cholesky
    reductions can then agree to that bound only by being the same arithmetic. A graded matrix has a componentwise accurate factor, and it is
    the case the solver meets."""
    rng = np.random.default_rng(300 + n)
    GB = graded_spd(rng, n, 1e8)
    assert 1e7 < np.linalg.cond(GB) < 1e9
    check(lib, sym(rng, n), GB)


@pytest.mark.parametrize("n", [1, 2, 3, 12, 47, 48])
def test_rotated_b_with_condition_1e8(lib, n):
    """The ill-conditioning in the directions: G_B = orthogonal * diag(1 .. 1e-8) * orthogonal^T. The rounding of G_B's entries alone moves an
    eigenvalue theta by |theta| eps ||G_B|| ||q||^2 <= eps cond(G_B) ||C|| (q^T G_B q = 1), and every Cholesky reduction commits that much in its
    last pivots, numpy's included: the eigenvalues are compared to n eps cond(G_B) ||C||, the two other properties to the bounds of check()."""
    rng = np.random.default_rng(700 + n)
    GA, GB = sym(rng, n), spd(rng, n, 1e8)
    rc, w, Q = ghep(lib, GA, GB)
    assert rc == 0
    Lc = np.linalg.cholesky(GB)
    Cm = np.linalg.solve(Lc, np.linalg.solve(Lc, GA).T).T
    ref = np.linalg.eigvalsh((Cm + Cm.T) / 2)
    nC = np.linalg.norm(Cm, 2); cond = np.linalg.cond(GB)
    print("n=%d  eig err %.2e (bound %.2e)" % (n, np.abs(w - ref).max(), n * EPS * cond * nC))
    assert np.abs(w - ref).max() <= n * EPS * cond * nC
    assert np.abs(Q.T @ GB @ Q - np.eye(n)).max() <= n * EPS * cond
    scale = np.linalg.norm(Q, 2) * (np.linalg.norm(GA, 2) + np.linalg.norm(GB, 2) * np.abs(w).max())
    assert np.abs(GA @ Q - GB @ Q * w).max() / scale <= n * EPS * cond


@pytest.mark.parametrize("n", [3, 12, 48])
def test_largest_real_order(lib, n):
    rng = np.random.default_rng(400 + n)
    w, _ = check(lib, sym(rng, n), spd(rng, n, 10.0), which=LARGEST_REAL)
    assert np.all(np.diff(w) <= 0)


@pytest.mark.parametrize("n", [3, 12, 48])
def test_repeated_eigenvalue(lib, n):
    """G_A = G_B X diag(theta) X^T G_B with X^T G_B X = I and theta holding one value three times (twice for n = 3)"""
    rng = np.random.default_rng(500 + n)
    GB = spd(rng, n, 10.0)
    Lc = np.linalg.cholesky(GB)
    Z, _ = np.linalg.qr(rng.standard_normal((n, n)))
    theta = np.arange(1.0, n + 1.0); theta[1:min(4, n)] = 2.0
    Cm = (Z * theta) @ Z.T
    GA = Lc @ Cm @ Lc.T
    GA = (GA + GA.T) / 2
    w, _ = check(lib, GA, GB)
    assert np.abs(w - np.sort(theta)).max() <= n * EPS * np.abs(theta).max() * np.linalg.cond(GB)


@pytest.mark.parametrize("n", [2, 12, 48])
def test_indefinite_b_is_an_error(lib, n):
    rng = np.random.default_rng(600 + n)
    GB = spd(rng, n, 10.0)
    GB[n - 1, n - 1] = -1.0
    rc, _, _ = ghep(lib, sym(rng, n), GB)
    assert rc > 0                                         # the order of the leading minor that is not positive definite
    rc, _, _ = ghep(lib, sym(rng, n), np.zeros((n, n)))
    assert rc == 1
