"""The references of tests/test_gpu_bv_ranks.py checked on the CPU: the splits, the exactness bounds of the integer data, the longdouble QR and
Cholesky factors against numpy's, the comparison rule of every block method, and B positive definite. Nothing here touches the library."""
import numpy as np
import pytest

import bv_rank_cases as bc


@pytest.mark.parametrize("name", bc.ALL_SPLITS)
def test_every_split_sums_to_its_size(name):
    for num_cu in (256, 304, 8):
        N, counts = bc.split(name, num_cu)
        assert sum(counts) == N and all(c >= 0 for c in counts) and len(counts) <= 4
        rg = bc.ranges(counts)
        assert rg[0][0] == 0 and rg[-1][1] == N and all(a[1] == b[0] for a, b in zip(rg, rg[1:]))
        assert [b - a for a, b in rg] == counts
    N, counts = bc.split(name)
    if name == "big2":
        T = 64 * 2 * 256
        assert counts == [T + 101, 70] and N == T + 171
    else:
        assert N == 1000
    assert bc.split("ragged4")[1][0] == 0 and 0 < bc.split("ragged4")[1][1] < 12            # an empty first rank; fewer rows than columns
    assert bc.split("ragged4b")[1][1] == 0 and bc.split("ragged4b")[1][-1] == 1
    for like in ("even2", "ragged4"):
        c = bc.split_like(like, 324)
        assert sum(c) == 324 and len(c) == len(bc.split(like)[1])
    assert bc.split_like("ragged4", 324)[:3] == [0, 5, 63]


def test_b_is_symmetric_positive_definite_and_crosses_the_rank_borders():
    N = 1000
    rp, col, val = bc.b_csr(N)
    B = np.zeros((N, N))
    for i in range(N):
        assert np.all(np.diff(col[rp[i]:rp[i + 1]]) > 0)                                    # sorted, no duplicates
        B[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
    assert np.array_equal(B, B.T) and np.array_equal(B, bc.b_dense(N))
    off = np.abs(B).sum(axis=1) - np.abs(np.diag(B))
    assert np.all(np.diag(B) == 6) and off.max() == 4                                       # Gershgorin: the spectrum lies in [2, 10]
    w = np.linalg.eigvalsh(B)
    assert 2.0 <= w[0] and w[-1] <= 10.0 and w[-1] / w[0] <= bc.COND_B
    x = bc.int_basis(N, 3, 1).astype(np.int64)
    assert np.array_equal(bc.b_apply(x), (B.astype(np.int64) @ x))
    for name in bc.SMALL_SPLITS:                                                            # every border between two non-empty ranks is crossed
        for r0, r1 in bc.ranges(bc.split(name)[1]):
            if 0 < r0 < N and r1 > r0:
                assert B[r0, r0 - 1] == -1 and B[r0 - 1, r0] == -1 and (r0 < 7 or B[r0, r0 - 7] == -1)


def test_exactness_bounds_hold_and_are_asserted():
    for N in (1000, 64 * 2 * 304 + 171):
        X, Y = bc.int_basis(N, 9, 2), bc.int_basis(N, 6, 3)
        assert np.abs(X).min() == 1 and np.abs(X).max() == 8 and np.array_equal(X, np.rint(X))
        G = bc.exact_gram(Y, X)
        assert np.abs(G).max() <= 8 * 8 * N < 2 ** 53 and np.array_equal(G, Y.T @ X)
        GB = bc.exact_gram(Y, X, with_b=True)
        assert np.abs(GB).max() <= 8 * 80 * N < 2 ** 53
        assert np.array_equal(GB, Y.T @ bc.b_apply(X))
    Q = bc.int_coeffs((100, 100), 4)
    assert np.abs(Q).max() <= 3 and Q.flags.f_contiguous
    W = bc.int_basis(1000, 100, 5)
    P = bc.exact_matmat(W, Q)
    assert np.abs(P).max() <= 8 * 3 * 100 and np.abs(bc.exact_matmat(P, Q)).max() <= 8 * 3 * 100 * 3 * 100 < 2 ** 53
    M = bc.exact_mult(0.5, -2.0, Y, X, bc.int_coeffs((9, 6), 6))
    assert np.array_equal(2 * M, np.rint(2 * M)) and np.array_equal(M, -2.0 * Y + 0.5 * (X @ bc.int_coeffs((9, 6), 6)))
    big = np.full((4, 2), 2.0 ** 27)
    with pytest.raises(AssertionError):
        bc.exact_gram(big, big)                                                             # 4 * 2^54: the generator refuses
    with pytest.raises(AssertionError):
        bc.exact_gram(np.full((3, 1), 0.5), np.ones((3, 1)))
    assert bc.exact_norm1(X) == np.abs(X).sum(axis=0).max() and bc.exact_norm_inf(X) == np.abs(X).sum(axis=1).max()
    assert bc.exact_sumsq(X) == int((X * X).sum())
    assert bc.ulps(np.nextafter(3.0, 4.0), 3.0) == 1.0


@pytest.mark.parametrize("n,k", [(12, 12), (1000, 12), (1000, 100), (64 * 2 * 256 + 171, 12)])
def test_longdouble_qr_against_numpy(n, k):
    X = np.random.default_rng(n + k).standard_normal((n, k))
    Q, R = bc.householder_qr(X)
    assert Q.dtype == np.longdouble and np.all(np.diag(R) > 0) and np.all(np.tril(R, -1) == 0)
    ld = np.finfo(np.longdouble).eps
    assert np.abs(Q.T @ Q - np.eye(k)).max() < 100 * ld * np.sqrt(n) and np.abs(Q @ R - X).max() < 100 * ld * np.sqrt(n) * np.abs(X).max()
    Rn = np.linalg.qr(X)[1]
    Rn = Rn * np.where(np.diag(Rn) < 0, -1.0, 1.0)[:, None]
    assert bc.compare_R("gs", Rn, R) < bc.R_TOL
    G = X.T @ X
    assert np.abs(np.asarray(R.T @ R, dtype=np.float64) - G).max() < 1e-13 * np.abs(G).max()


def test_the_measured_distance_stands_behind_r_tol():
    """Re-measures over all of R_CASES (big2 at 256 compute units) what R_TOL and R_TOL_SVQB are eight times of; another LAPACK may differ in the
    last bit, not by the margin."""
    assert bc.R_TOL == 8 * bc.R_DISTANCE_MEASURED and bc.R_TOL_SVQB == 8 * bc.R_DISTANCE_MEASURED_SVQB
    worst = bc.measure_r_distance()
    assert worst < 4 * bc.R_DISTANCE_MEASURED, worst
    worst = bc.measure_r_distance("svqb")
    assert worst < 4 * bc.R_DISTANCE_MEASURED_SVQB, worst
    assert bc.r_tolerance("svqb") == bc.R_TOL_SVQB and all(bc.r_tolerance(m) == bc.R_TOL for m in ("gs", "chol", "tsqr", "tsqrchol"))


def test_longdouble_cholesky_of_the_exact_gram_matrix():
    X = bc.int_basis(1000, 12, 7)
    G = bc.exact_gram(X, X)
    R = bc.cholesky_upper(G)
    assert np.all(np.diag(R) > 0) and np.all(np.tril(R, -1) == 0)
    assert np.abs(R.T @ R - G.astype(np.longdouble)).max() < 100 * np.finfo(np.longdouble).eps * np.abs(G).max()
    assert bc.compare_R("chol", np.linalg.cholesky(G).T, R) < bc.R_TOL
    assert bc.compare_R("gs", np.asarray(bc.householder_qr(X)[1], dtype=np.float64), R) < bc.R_TOL
    GB = bc.exact_gram(X, X, with_b=True)
    RB = bc.cholesky_upper(GB)
    assert np.abs(RB.T @ RB - GB.astype(np.longdouble)).max() < 100 * np.finfo(np.longdouble).eps * np.abs(GB).max()


def test_compare_r_follows_the_freedom_of_each_method():
    k, l = 8, 3
    X = np.array(bc.normal_basis(1000, k, l))
    Rref = bc.householder_qr(X)[1]
    R = np.asarray(Rref, dtype=np.float64)
    flip = np.ones(k); flip[[4, 6]] = -1.0
    Rs = R * flip[:, None]                                       # rows 4 and 6 negated: a Householder R, not the Gram-Schmidt one
    for method in ("tsqr", "tsqrchol"):
        assert bc.compare_R(method, Rs, Rref, l) < bc.R_TOL and bc.compare_R(method, Rs, Rref, 0) < bc.R_TOL
    assert bc.compare_R("gs", Rs, Rref, l) > 0.1 and bc.compare_R("chol", Rs, Rref, l) > 0.1
    flip0 = np.ones(k); flip0[1] = -1.0
    assert bc.compare_R("tsqr", R * flip0[:, None], Rref, l) > 1e-3        # a row before the window has no freedom
    U = np.linalg.qr(np.random.default_rng(3).standard_normal((k - l, k - l)))[0]
    Rq = R.copy(); Rq[l:, l:] = U @ R[l:, l:]                    # any orthogonal factor in front: what SVQB returns
    assert bc.compare_R("svqb", Rq, Rref, l) < bc.r_tolerance("svqb") and bc.compare_R("tsqr", Rq, Rref, l) > 1e-3
    Rw = R.copy(); Rw[5, 7] *= 1 + 1e-9
    for method in ("gs", "chol", "tsqr", "tsqrchol", "svqb"):
        assert bc.compare_R(method, Rw, Rref, l) > bc.r_tolerance(method), method
    Rcol = R.copy(); Rcol[:, :l] = 99.0                          # the columns before the window are not referenced
    assert bc.compare_R("gs", Rcol, Rref, l) < bc.R_TOL


def test_ghep_pencil_is_the_one_of_the_single_rank_test():
    from oracle import oracle as O
    (rp, col, val), (brp, bcol, bval) = bc.ghep_test1_pencil(18)
    Ao = O.laplacian2d(18)
    assert np.array_equal(rp, Ao.rowptr) and np.array_equal(col, Ao.col) and np.array_equal(val, Ao.val)
    assert np.array_equal(brp, np.arange(325)) and np.array_equal(bcol, np.arange(324)) and np.array_equal(bval, 2.0 / np.log(np.arange(324) + 2.0))
    assert sum(bc.TINY4) < 12 and bc.TINY4[0] == 0


def test_ill_conditioned_basis_has_the_stated_condition():
    X = bc.ill_conditioned_basis(1000, 12)
    s = np.linalg.svd(X, compute_uv=False)
    assert abs(s[0] - 1.0) < 1e-12 and abs(np.log10(s[0] / s[-1]) - 12) < 1e-3
    assert not X.flags.writeable and bc.normal_basis(1000, 12, 3) is bc.normal_basis(1000, 12, 3)
    for pp in (1e-13, 1e-6):
        V = bc.nearly_orthonormal_basis(1000, 12, pp)
        G = V.T @ V
        assert pp < np.abs(G - np.eye(12)).max() < 40 * pp + 1e-14 and not V.flags.writeable
    Q3 = bc.normal_basis(1000, 12, 3)[:, :3]
    assert np.abs(Q3.T @ Q3 - np.eye(3)).max() < 1e-14
