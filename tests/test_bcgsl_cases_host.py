"""What the GPU tests of KS_KSP_BCGSL rely on, pinned on the CPU with the restatement of tests/bcgsl_cases.py: rounding cannot move the counts they
require. Every case runs under four summation orders of the inner products (numpy's, reversed, two shuffles), which is what distinguishes the
device's sums from numpy's.

I (x) T systems, rtol 1e-12: T has m distinct complex eigenvalues, so BiCG ends at step m and BiCGStab(l) at m rounded up to a multiple of l. The
relative residual one cycle before the end is at least 100 tol and at the end at most tol / 100 in every order, so no rounding of the size of a
summation order moves the count. Measured here (l = 1..4): one cycle early >= 4.1e-9, at the end <= 3.1e-18.

Convection-diffusion systems, rtol 1e-8, point Jacobi: the count moves with the summation order, so only convergence of l = 2 and l = 4 in every
order is required, and that l = 1 fails in at least one order at c = 3, sigma = 2 (measured: it breaks down in all four, as on the two others).
Counts measured here in the four orders, l = 2 / l = 4:  45 x 31, c = 3, sigma = 2: 306-336 / 244-260;  45 x 31, c = 8: 112-124 / 108;
24 x 24, c = 20: 210-222 / 196-212."""
import numpy as np
import pytest

import bcgsl_cases as bc


@pytest.mark.parametrize("ell", [1, 2, 3, 4])
@pytest.mark.parametrize("idx", range(len(bc.KRON)))
def test_kron_counts_do_not_move_with_the_summation_order(idx, ell):
    m, blocks, pc = bc.KRON[idx]
    case = bc.kron(m, blocks)
    minv = bc.jacobi(case.P) if pc == "jacobi" else None
    T = case.P[:m, :m].toarray()
    lam = np.linalg.eigvals(T / np.diag(T)[:, None] if pc == "jacobi" else T)
    assert np.all(np.abs(lam.imag) > 1e-3) and len(np.unique(np.round(lam, 8))) == m        # all complex, all distinct
    want = bc.kron_count(idx, ell)
    assert want == {(8, 1): 8, (8, 2): 8, (8, 3): 9, (8, 4): 8, (6, 1): 6, (6, 2): 6, (6, 3): 6, (6, 4): 8}[(m, ell)]
    for p in bc.perms(case.n):
        ref = bc.bcgsl_reference(case.P, case.b, minv, ell=ell, rtol=1e-12, perm=p)
        print("%s l %d: its %d, before %.2e, after %.2e, gap %.2e" % (case.name, ell, ref.its, ref.hist[-2], ref.hist[-1], ref.gap))
        assert ref.reason == "converged" and ref.its == want
        assert ref.hist[-2] >= 100 * 1e-12 and ref.hist[-1] <= 1e-12 / 100
        assert np.linalg.norm(ref.y - np.linalg.solve(case.P.toarray(), case.b)) <= 1e-11 * np.linalg.norm(ref.y)


@pytest.mark.parametrize("idx", range(len(bc.CONVDIFF)))
def test_convdiff_l2_and_l4_converge_in_every_order(idx):
    nx, ny, c, sigma = bc.CONVDIFF[idx]
    case = bc.convdiff(nx, ny, c)
    P = bc.shifted(case, sigma)
    minv = bc.jacobi(P)
    failed_l1 = 0
    for p in bc.perms(case.n):
        for ell in (2, 4):
            ref = bc.bcgsl_reference(P, case.b, minv, ell=ell, rtol=1e-8, max_it=4000, perm=p)
            print("%s sigma %g l %d: %s after %d steps, residual %.2e, gap %.2e" % (case.name, sigma, ell, ref.reason, ref.its, ref.hist[-1], ref.gap))
            assert ref.reason == "converged"
        one = bc.bcgsl_reference(P, case.b, minv, ell=1, rtol=1e-8, max_it=4000, perm=p)
        print("%s sigma %g l 1: %s after %d steps, residual %.2e" % (case.name, sigma, one.reason, one.its, one.hist[-1]))
        failed_l1 += one.reason != "converged"
    if idx == 0:
        assert failed_l1 >= 1


def test_endings_of_the_restatement():
    """The exact constructions the GPU tests force: a skew-symmetric P gives sigma = (P r_0, r_0) = 0 in integers; P = 2 I gives alpha = 1/2 and
    r_0 = 0 after the first BiCG step, so the Gram matrix of l = 1 is zero; a zero right-hand side, max_it, NaN."""
    import scipy.sparse as sp
    n = 600
    b = np.random.default_rng(7).integers(-8, 9, n).astype(np.float64)
    S = sp.kron(sp.identity(n // 2), np.array([[0.0, 1.0], [-1.0, 0.0]])).tocsr()
    for ell in (1, 2):
        ref = bc.bcgsl_reference(S, b, None, ell=ell)
        assert ref.reason == "breakdown" and ref.its == 0 and ref.values["sigma"] == 0.0
    ref = bc.bcgsl_reference(2.0 * sp.identity(n).tocsr(), b, None, ell=1)
    assert ref.reason == "singular" and ref.its == 1 and ref.values["pivot"] == 0.0
    ref = bc.bcgsl_reference(2.0 * sp.identity(n).tocsr(), b, None, ell=2)
    assert ref.reason == "breakdown" and ref.its == 1
    case = bc.kron(8, 151)
    assert bc.bcgsl_reference(case.P, np.zeros(case.n), None).its == 0 and bc.bcgsl_reference(case.P, np.zeros(case.n), None).reason == "converged"
    ref = bc.bcgsl_reference(case.P, case.b, None, ell=2, max_it=3)
    assert ref.reason == "its" and ref.its == 4                              # tested at the start of a cycle only
    bn = case.b.copy(); bn[5] = np.nan
    assert bc.bcgsl_reference(case.P, bn, None).reason == "not a number"
