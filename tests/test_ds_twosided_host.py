"""DS NHEPTS of the two-sided Krylov-Schur solver (slepc_amd/csrc/ks_ds.cpp: DsNhepTs, stepped through the ksd_nhepts hook) and the LU pair of its
Rayleigh-quotient update (ks_dense.cpp: lu_factor / lu_solve), on the CPU.

References: the restatement of tests/twosided_cases.py (two oracle.DSNHEP halves on LAPACK plus the permutation step) on the projected matrices a
restated solve dumps, scipy.linalg.lu_factor / lu_solve, and defining properties (Schur relations, eigenvector residuals). Tolerances are those of
tests/test_ds_host.py: tol = 50 n eps max(1, max|A|) for residuals and orthogonality, 1e3 tol where eigenvalues of the C++ Francis iteration are
compared with LAPACK's. Orders are compared only where the spectrum leaves no choice: the dumps come from criteria without ties, and the cases
that must enter the permutation plant a gap of 1e-6 (far above both sqrt(eps), the correspondence threshold, and the rounding) between the
eigenvalues whose order differs between the halves. Steps that depend on the signs of the Schur vectors start from the oracle's state on both sides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

import slepc_amd as ks
import slepc_amd._lib as L
from oracle import oracle as O

import nhep_cases
import twosided_cases as TS

P = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE, SORT, EXTRA_ROW, TRUNCATE, TRUNCATE_SIZE, RITZ, VECTORS = range(7)
CODES = {"largest_magnitude": 1, "largest_real": 3}


class Cmp(C.Structure):
    _fields_ = [("which", C.c_int), ("target", C.c_double), ("fn", ks.EIG_COMPARE_FN), ("st_type", C.c_int), ("sigma", C.c_double), ("nu", C.c_double)]


def p(a):
    return a.ctypes.data_as(P)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksd_nhepts.argtypes = [C.c_int, C.c_int, IP] + [P] * 10 + [C.POINTER(Cmp), C.c_int, C.c_int, C.c_int, P]
    lib.ksd_lu_factor.argtypes = [C.c_int, P, C.c_int, IP]
    lib.ksd_lu_solve.argtypes = [C.c_int, P, C.c_int, IP, P, C.c_int]
    lib.ksd_lu_solve.restype = None
    return lib


class Ts:
    """caller-owned arrays of one DS NHEPTS, stepped through the hook"""

    def __init__(self, lib, ld, which):
        self.lib, self.ld = lib, ld
        self.cmp = Cmp(CODES[which], 0.0, ks.EIG_COMPARE_FN(), -1, 0.0, 0.0)
        self.A, self.Q, self.X, self.B, self.Z, self.Y = (np.zeros((ld, ld), order="F") for _ in range(6))
        self.wr, self.wi, self.wr2, self.wi2 = (np.zeros(ld) for _ in range(4))
        self.dims = np.zeros(5, dtype=np.int32); self.out = np.zeros(3)

    def load(self, ds):
        """from a twosided_cases.DSNHEPTS"""
        a, b = ds.a, ds.b
        self.A[:], self.Q[:], self.X[:], self.B[:], self.Z[:], self.Y[:] = a.A, a.Q, a.X, b.A, b.Q, b.X
        self.wr2[:], self.wi2[:] = ds.wr2, ds.wi2
        self.dims[:] = [a.n, a.l, a.k, a.t, a.state]

    def step(self, op, a0=0, a1=0, a2=0):
        return self.lib.ksd_nhepts(op, self.ld, self.dims.ctypes.data_as(IP), p(self.A), p(self.Q), p(self.X), p(self.B), p(self.Z), p(self.Y),
                                   p(self.wr), p(self.wi), p(self.wr2), p(self.wi2), C.byref(self.cmp), a0, a1, a2, p(self.out))


def copy_ds(src, compare):
    d = TS.DSNHEPTS(src.ld, compare)
    for h, s in ((d.a, src.a), (d.b, src.b)):
        h.A[:], h.Q[:], h.X[:] = s.A, s.Q, s.X
        h.n, h.l, h.k, h.t, h.state = s.n, s.l, s.k, s.t, s.state
    d.wr2[:], d.wi2[:] = src.wr2, src.wi2
    return d


@pytest.fixture(scope="module")
def dumps():
    """The projected problems (both halves, as RQUpdate1 leaves them) of every restart of two restated solves without ties in the criterion: the Markov
    chain (real spectrum) and the Brusselator (conjugate pairs), largest real part. Computed once, never modified: every test works on copies."""
    out = []
    for name, A in (("markov", O.markov_matrix(15)), ("brusselator", nhep_cases.brusselator(50))):
        box = []
        orig = TS.DSNHEPTS.Solve

        def spy(self, wr, wi, box=box):
            box.append(copy_ds(self, self.a.compare))
            return orig(self, wr, wi)
        TS.DSNHEPTS.Solve = spy
        try:
            TS.eps_krylovschur_twosided(A, 4, which="largest_real")
        finally:
            TS.DSNHEPTS.Solve = orig
        out += [(name, i, d) for i, d in enumerate(box[:6])]
    assert len(out) == 12 and any(d.a.l > 0 for _, _, d in out) and any(d.a.state == O.DS_STATE_RAW for _, _, d in out)
    return out


def tol_of(M, n):
    return 50 * n * EPS * max(1.0, np.abs(M[:n, :n]).max())


def check_schur(A0, T, Q, n, tol):
    assert np.abs(A0[:n, :n] @ Q[:n, :n] - Q[:n, :n] @ T[:n, :n]).max() <= tol
    assert np.abs(Q[:n, :n].T @ Q[:n, :n] - np.eye(n)).max() <= tol
    assert np.abs(np.tril(T[:n, :n], -2)).max() == 0.0


def test_solve_and_sort_follow_the_restatement(lib, dumps):
    for name, i, d in dumps:
        ref = copy_ds(d, d.a.compare); ld = d.ld; n = d.a.n
        wr, wi = np.zeros(ld), np.zeros(ld)
        ref.Solve(wr, wi); perm_ref = ref.Sort(wr, wi)
        t = Ts(lib, ld, "largest_real"); t.load(d)
        assert t.step(SOLVE) == 0 and t.dims[4] == O.DS_STATE_CONDENSED
        assert t.step(SORT) == 0
        tol = max(tol_of(d.a.A, n), tol_of(d.b.A, n))
        check_schur(d.a.A, t.A, t.Q, n, tol); check_schur(d.b.A, t.B, t.Z, n, tol)
        evtol = 1e3 * tol
        assert np.abs(t.wr[:n] - wr[:n]).max() <= evtol and np.abs(t.wi[:n] - wi[:n]).max() <= evtol, (name, i)
        assert np.abs(t.wr2[:n] - ref.wr2[:n]).max() <= evtol and np.abs(t.wi2[:n] - ref.wi2[:n]).max() <= evtol, (name, i)
        assert bool(t.out[1]) == perm_ref


def planted(n, ld, diag, blk, re, im, seed):
    """quasi-triangular with the given diagonal (and a 2x2 block re +- i im at blk), behind a random orthogonal similarity, extra row beta e_n^T"""
    rng = np.random.default_rng(seed)
    T = np.triu(0.1 * rng.standard_normal((n, n)), 1) + np.diag(diag)
    if blk is not None:
        T[blk, blk] = T[blk + 1, blk + 1] = re; T[blk, blk + 1] = 2.0 * im; T[blk + 1, blk] = -0.5 * im
    G, _ = np.linalg.qr(rng.standard_normal((n, n)))
    M = np.zeros((ld, ld), order="F"); M[:n, :n] = G @ T @ G.T; M[n, n - 1] = 0.25
    return M


@pytest.mark.parametrize("with_pair", [False, True])
def test_sort_enters_the_permutation_when_the_halves_order_differently(lib, with_pair):
    """largest magnitude with moduli 1 + 1e-6 against 1: the first half leads with the positive value (or the pair), the second with the negative
    one, so the second half has to be permuted; the block that moves up is 1x1 in one case and 2x2 in the other"""
    n, ld, dl, th = 7, 9, 1e-6, 0.8
    if not with_pair:
        A = planted(n, ld, [0.5, 1 + dl, 0.3, -1.0, 0.1, -0.2, 0.7], None, 0, 0, 1)
        B = planted(n, ld, [-(1 + dl), 0.3, 0.7, 0.5, 1.0, 0.1, -0.2], None, 0, 0, 2)
        want_a = [1 + dl, -1.0, 0.7, 0.5, 0.3, -0.2, 0.1]; want_b = [1.0, -(1 + dl), 0.7, 0.5, 0.3, -0.2, 0.1]
        wanti = np.zeros(n)
    else:
        A = planted(n, ld, [0.5, 0, 0, -1.0, 0.1, -0.2, 0.7], 1, (1 + dl) * np.cos(th), (1 + dl) * np.sin(th), 1)
        B = planted(n, ld, [0.7, -(1 + dl), 0.5, 0, 0, 0.1, -0.2], 3, np.cos(th), np.sin(th), 2)
        want_a = [(1 + dl) * np.cos(th)] * 2 + [-1.0, 0.7, 0.5, -0.2, 0.1]; want_b = [np.cos(th)] * 2 + [-(1 + dl), 0.7, 0.5, -0.2, 0.1]
        wanti = np.array([np.sin(th), -np.sin(th), 0, 0, 0, 0, 0])
    ref = TS.DSNHEPTS(ld, O.WHICH["largest_magnitude"]); ref.a.A[:] = A; ref.b.A[:] = B
    ref.SetDimensions(n, 0, 0); ref.SetState(O.DS_STATE_RAW)
    t = Ts(lib, ld, "largest_magnitude"); t.load(ref)
    wr, wi = np.zeros(ld), np.zeros(ld)
    ref.Solve(wr, wi); assert ref.Sort(wr, wi)                      # the restatement takes the branch too
    assert t.step(SOLVE) == 0 and t.step(SORT) == 0
    assert t.out[1] == 1.0
    tol = 1e3 * tol_of(A, n)
    assert np.abs(t.wr[:n] - want_a).max() <= tol and np.abs(t.wr2[:n] - want_b).max() <= tol
    assert np.abs(np.abs(t.wi[:n]) - np.abs(wanti)).max() <= 2 * dl and np.abs(np.abs(t.wi2[:n]) - np.abs(wanti)).max() <= 2 * dl
    assert np.abs(t.wr[:n] - wr[:n]).max() <= tol and np.abs(t.wr2[:n] - ref.wr2[:n]).max() <= tol
    check_schur(A, t.A, t.Q, n, tol_of(A, n)); check_schur(B, t.B, t.Z, n, tol_of(B, n))


def test_extra_row_truncation_and_vectors_from_the_oracles_state(lib, dumps):
    for name, i, d in dumps:
        ref = copy_ds(d, d.a.compare); ld = d.ld; n = d.a.n; l = d.a.l
        wr, wi = np.zeros(ld), np.zeros(ld)
        ref.Solve(wr, wi); ref.Sort(wr, wi)
        t = Ts(lib, ld, "largest_real"); t.load(ref); t.wr[:], t.wi[:] = wr, wi
        ref.UpdateExtraRow(); assert t.step(EXTRA_ROW) == 0
        tol = max(tol_of(d.a.A, n), tol_of(d.b.A, n))
        assert np.abs(t.A - ref.a.A).max() <= tol and np.abs(t.B - ref.b.A).max() <= tol and t.dims[2] == n
        # eigenvectors of both sides, back-transformed: residual against the matrix the half started from, unit norm, rnorm = |last component|
        k = l
        while k < n:
            for left, M0, T, X in ((0, d.a.A, t.A, t.X), (1, d.b.A, t.B, t.Y)):
                newk = t.step(VECTORS, k, 1, left)
                lam = complex(T[k, k], np.sqrt(abs(T[k + 1, k] * T[k, k + 1])) if newk == k + 1 else 0.0)
                z = X[:n, k] + (1j * X[:n, newk] if newk == k + 1 else 0.0)
                assert abs(np.linalg.norm(z) - 1.0) <= tol
                assert np.linalg.norm(M0[:n, :n] @ z - lam * z) <= 1e3 * tol, (name, i, k, left)
                assert abs(t.out[0] - abs(z[n - 1])) <= tol
            assert (newk == k + 1) == (ref.a.A[k + 1, k] != 0.0 if k < n - 1 else False)
            k = newk + 1
        # truncate sizes for every cut, then one truncation
        for kk in range(1, n - l):
            assert t.step(TRUNCATE_SIZE, l, n, kk) == ref.GetTruncateSize(l, n, kk)
        kk = ref.GetTruncateSize(l, n, max(1, (n - l) // 2))
        ref.Truncate(l + kk, False); assert t.step(TRUNCATE, l + kk, 0) == 0
        assert list(t.dims) == [ref.a.n, ref.a.l, ref.a.k, ref.a.t, ref.a.state]
        assert np.abs(t.A - ref.a.A).max() <= tol and np.abs(t.B - ref.b.A).max() <= tol


@pytest.mark.parametrize("half", ["first", "second", "neither", "last"])
def test_truncate_size_keeps_a_2x2_block_of_either_half(lib, half):
    n, ld, l, kk = 8, 10, 1, 3
    t = Ts(lib, ld, "largest_real")
    t.A[:n, :n] = np.triu(np.ones((n, n))); t.B[:n, :n] = np.triu(np.ones((n, n)))
    t.dims[:] = [n, l, n, n, O.DS_STATE_CONDENSED]
    if half == "first":
        t.A[l + kk, l + kk - 1] = -0.5
    if half == "second":
        t.B[l + kk, l + kk - 1] = -0.5
    if half == "last":                         # the block is the last one: the cut moves down, not up
        kk = n - 1 - l; t.B[l + kk, l + kk - 1] = -0.5
    want = {"first": kk + 1, "second": kk + 1, "neither": kk, "last": kk - 1}[half]
    assert t.step(TRUNCATE_SIZE, l, n, kk) == want


@pytest.mark.parametrize("n", [1, 2, 7, 30])
def test_lu_pair_matches_lapack(lib, n):
    """factor once, solve with the matrix and with its transpose: scipy.linalg.lu_factor / lu_solve (dgetrf / dgetrs) on the same matrix"""
    rng = np.random.default_rng(n)
    A = np.asfortranarray(rng.standard_normal((n, n))); b = rng.standard_normal(n)
    lu_ref, piv_ref = sl.lu_factor(A)
    F = A.copy(order="F"); piv = np.zeros(n, dtype=np.int32)
    assert lib.ksd_lu_factor(n, p(F), n, piv.ctypes.data_as(IP)) == 0
    assert np.array_equal(piv, piv_ref)
    tol = 50 * n * EPS * max(1.0, np.abs(lu_ref).max())
    assert np.abs(F - lu_ref).max() <= tol
    cond = np.linalg.cond(A)
    for trans in (0, 1):
        x = b.copy(); lib.ksd_lu_solve(n, p(F), n, piv.ctypes.data_as(IP), p(x), trans)
        assert np.abs(x - sl.lu_solve((lu_ref, piv_ref), b, trans=trans)).max() <= 50 * n * EPS * cond * max(1.0, np.abs(x).max())
    Z = np.asfortranarray(np.array([[0.0, 1.0], [0.0, 2.0]])); pz = np.zeros(2, dtype=np.int32)
    assert lib.ksd_lu_factor(2, p(Z), 2, pz.ctypes.data_as(IP)) == 1          # exactly zero pivot: what the solver reports as serious breakdown


def test_fixed_start_vector_cases_decide_far_from_the_tolerance():
    """tests/test_gpu_twosided.py compares restart counts of the GPU solve with the restatement for ex41's start vectors, with and without a shift:
    no estimate a restart decided on may lie within 1e-3 (relative) of the tolerance, or rounding could legitimately decide otherwise"""
    A = O.markov_matrix(15)
    v0, w0 = TS.ex41_start_vectors(A.n)
    for sigma in (0.0, 0.3):
        r = TS.eps_krylovschur_twosided(A, 4, which="largest_real", v0=v0, w0=w0, sigma=sigma)
        assert r.reason == 1 and r.nconv >= 4 and r.margin > 1e-3, (sigma, r.margin)


def test_convection_diffusion_converges_within_max_it():
    A, exact = TS.convection_diffusion(32)
    r = TS.eps_krylovschur_twosided(A, 4, which="largest_real")
    assert r.reason == 1 and r.nconv >= 4
    lam = r.eigr[r.perm][:4]
    assert np.abs(lam - exact[:4]).max() <= 1e-6


def test_replay_program_under_address_and_undefined_sanitizers(tmp_path):
    """ks_ds.cpp and ks_dense.cpp with a main of their own (tests/c_abi/ds_twosided_replay.cpp: two permutation cases through every step of a
    restart), built with -fsanitize=address,undefined and run as a program: no preload, nothing loaded into Python"""
    csrc = os.path.join(ROOT, "slepc_amd", "csrc")
    exe = str(tmp_path / "ds_twosided_replay")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "c_abi", "ds_twosided_replay.cpp"), os.path.join(csrc, "ks_ds.cpp"), os.path.join(csrc, "ks_dense.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
