"""The CG yardstick pinned without a GPU: the properties of tests/cg_cases.py that tests/test_gpu_cg.py and tests/test_gpu_cg_ranks.py rely on."""
import numpy as np
import pytest

import cg_cases as cc


@pytest.mark.parametrize("idx", range(len(cc.KRON)))
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_kron_ends_at_iteration_m(idx, pc):
    """m distinct eigenvalues: the count is m, and it is not a matter of rounding - the residual is far above 1e-8 at m - 1 and far below at m."""
    m, blocks = cc.KRON[idx]
    case, ref = cc.kron_reference(idx, pc)
    assert case.n == m * blocks and ref.reason == "converged"
    print("%s %s: its %d, h[m-1] %.3e, h[m] %.3e" % (case.name, pc, ref.its, ref.hist[m - 1], ref.hist[m]))
    assert ref.its == m
    assert ref.hist[m - 1] >= 1.6e-6 and ref.hist[m] <= 3.1e-17
    dense = case.P.toarray()
    assert np.linalg.cond(dense) < 30
    x = np.linalg.solve(dense, case.b)
    assert np.linalg.norm(ref.y - x) <= 1e-12 * np.linalg.norm(x)


@pytest.mark.parametrize("idx", range(len(cc.LAP)))
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("sigma", [0.0, -0.5])
@pytest.mark.parametrize("near", [1e-8, 1e-12])
def test_lap_tolerance_is_derived_from_a_factor_two_step(idx, pc, sigma, near):
    """rtol = sqrt(h[k-1] h[k]) at an iteration k with h[k-1] / h[k] >= 2: the restatement then stops at exactly k, several batches in."""
    case, P, rtol, ref, k = cc.lap_reference(idx, pc, sigma, near)
    print("%s %s sigma %g: k %d, rtol %.3e, h[k-1] %.3e, h[k] %.3e, gap %.2e" % (case.name, pc, sigma, k, rtol, ref.hist[k - 1], ref.hist[k], ref.gap))
    assert ref.reason == "converged" and ref.its == k and k >= 9
    assert ref.hist[k - 1] / ref.hist[k] >= 2.0 and ref.hist[k - 1] > rtol > ref.hist[k]
    assert near / 30 < rtol < near * 30
    x = np.linalg.solve(P.toarray(), case.b)
    assert np.linalg.norm(ref.y - x) <= 100 * rtol * np.linalg.cond(P.toarray()) * np.linalg.norm(x)


def test_sizes_cover_the_tail_and_the_tile():
    assert [cc.kron(*c).n for c in cc.KRON] == [1057, 1027, 512, 513]
    assert [cc.lap(*c).n for c in cc.LAP] == [1023, 1073]
    for c in cc.KRON:
        assert np.array_equal(cc.kron(*c).b, np.round(cc.kron(*c).b)) and np.abs(cc.kron(*c).b).max() <= 8


def test_restatement_names_the_failures():
    case = cc.lap(*cc.LAP[0])
    lam = np.linalg.eigvalsh(case.P.toarray())
    inside = 0.5 * (lam[3] + lam[4])
    assert cc.cg_reference(cc.shifted(case, inside), case.b).reason == "indefinite matrix"
    assert cc.cg_reference(case.P, case.b, lambda r: -r).reason == "indefinite preconditioner"
    r = cc.cg_reference(case.P, case.b, rtol=1e-8, max_it=2)
    assert r.reason == "its" and r.its == 2
    z = cc.cg_reference(case.P, np.zeros(case.n))
    assert z.reason == "converged" and z.its == 0 and not z.y.any()
