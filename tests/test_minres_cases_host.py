"""The MINRES yardstick pinned without a GPU: the properties of tests/minres_cases.py that tests/test_gpu_minres.py and
tests/test_gpu_minres_ranks.py rely on - iteration counts that rounding cannot move."""
import numpy as np
import pytest

import cg_cases as cc
import minres_cases as mc

KRON_CASES = [(m, b, pc) for (m, b) in mc.KRON for pc in ("jacobi-abs", "none")] + [(13, 79, "none")]


@pytest.mark.parametrize("m,blocks,pc", KRON_CASES)
def test_kron_ends_at_iteration_m(m, blocks, pc):
    """m distinct eigenvalues of the (preconditioned) operator: the count is m, and not by a matter of rounding - the residual is above 0.17 of the
    first at m - 1 and below 3e-11 of it at m."""
    case, ref = mc.kron_reference(m, blocks, pc)
    T = case.P[:m, :m].toarray()
    lam = np.linalg.eigvalsh(T)
    print("%s %s: its %d, h[m-1] %.3e, h[m] %.3e, gap %.2e" % (case.name, pc, ref.its, ref.hist[m - 1], ref.hist[m], ref.gap))
    assert case.n == m * blocks and (lam < 0).sum() == 3 and (np.diag(T) < 0).any()
    assert ref.reason == "converged" and ref.its == m
    assert ref.hist[m - 1] >= 0.17 and ref.hist[m] <= 3e-11
    assert np.all(np.diff(ref.hist) <= 0)                                        # the residual of MINRES is monotone
    x = np.linalg.solve(case.P.toarray(), case.b)
    assert np.linalg.norm(ref.y - x) <= 1e-9 * np.linalg.norm(x)


def test_kron_13_with_jacobi_abs_is_not_a_count_case():
    """Why (13, 79) is used without a preconditioner only: scaled by |diag|, T no longer ends at m."""
    case, ref = mc.kron_reference(13, 79, "jacobi-abs")
    assert ref.reason == "converged" and ref.its != 13


NEG = {0: 4, 1: 5, 2: 0}
K = {(0, "none"): 168, (0, "jacobi-abs"): 114, (1, "none"): 179, (1, "jacobi-abs"): 159, (2, "none"): 45, (2, "jacobi-abs"): 31}


def _permuted(which, pc, seeds):
    """(margin, largest relative deviation at h[k-1] and h[k], counts) of restatements that sum every dot over randomly permuted unknowns."""
    case, P, rtol, ref, k, ratio = mc.lap_reference(which, pc)
    minv = mc.minv_of(P, pc)
    assert (np.linalg.eigvalsh(P.toarray()) < 0).sum() == NEG[which]
    assert ref.reason == "converged" and ref.its == k == K[which, pc] and ratio >= 1.4
    assert ref.hist[k - 1] > rtol > ref.hist[k]
    dev, counts = 0.0, []
    for seed in seeds:
        perm = np.random.default_rng(1000 + seed).permutation(case.n)
        run = mc.minres_reference(P, case.b, minv, rtol=rtol, perm=perm)
        assert run.reason == "converged"
        counts.append(run.its)
        dev = max(dev, abs(run.hist[k - 1] / ref.hist[k - 1] - 1.0), abs(run.hist[k] / ref.hist[k] - 1.0))
    margin = np.sqrt(ratio) - 1.0
    print("%s sigma %g %s: k %d, rtol %.3e, ratio %.3f, margin %.3f, deviation %.2e, gap %.2e" % (case.name, mc.LAP[which][1], pc, k, rtol, ratio, margin, dev, ref.gap))
    return margin, dev, counts, k


@pytest.mark.parametrize("which,pc", mc.LAP_COUNTS)
def test_lap_tolerance_sits_in_a_step_rounding_cannot_cross(which, pc):
    """rtol is the geometric mean of h[k-1] and h[k] at the step with the largest ratio in (1e-10, 1e-5). The count is k as long as rounding moves
    neither value by the margin sqrt(ratio) - 1; six restatements that sum every dot in another order (randomly permuted unknowns, seeds fixed
    before the first run) stay within a tenth of it, and all six count k."""
    margin, dev, counts, k = _permuted(which, pc, range(6))
    assert counts == [k] * 6
    assert dev < 0.1 * margin


def test_lap_1_without_preconditioner_fails_the_rule():
    """LAP[1] at sigma 1.1 without a preconditioner, k = 179, ratio 1.49, margin 0.222: the six permuted runs all count 179, but their deviation is
    heavy-tailed - 7.8e-2 at the third seed, 4.9e-2 at the second (of twenty seeds four exceeded 1.5e-2, the others stayed below 4e-3) - and so
    above a tenth of the margin. By the rule of this file the case is not used for an exact count (minres_cases.LAP_COUNTS leaves it out; the
    GPU tests run it for the residual only). What does hold is pinned here: every permuted run counts k and stays inside the margin itself."""
    margin, dev, counts, k = _permuted(1, "none", range(6))
    assert (1, "none") not in mc.LAP_COUNTS
    assert counts == [k] * 6 and dev < margin


def test_block_jacobi_count_is_exact_above_the_floor():
    """LAP[0] at sigma 1.5 with dense blocks of 8 rows. At rtol 1e-8 the history is flat (h[104] = 1.25e-8, h[105] = 9.4e-9) and the six permuted
    runs count 101 to 106: no exact count there. Over all of (1e-10, 1e-5) the widest step is k = 116, ratio 1.70, margin 0.303, but the permuted
    runs deviate by up to 6.0e-2 at it, above a tenth of the margin. Above the floor of 1e-7 the widest step is k = 87, ratio 1.56, margin 0.250,
    deviation 2.1e-5: the rule of this file holds, and the GPU test of the one-row sweeps takes its tolerance there."""
    case = cc.lap(*cc.LAP[mc.LAP[0][0]])
    P = cc.shifted(case, mc.LAP[0][1])
    minv = mc.block_jacobi(P, mc.BJACOBI_BLOCK)
    long = mc.minres_reference(P, case.b, minv, rtol=1e-12)
    k, rtol, ratio = mc.pick_k(long.hist, mc.BJACOBI_FLOOR)
    ref = mc.minres_reference(P, case.b, minv, rtol=rtol)
    assert ref.reason == "converged" and ref.its == k == 87 and ratio >= 1.4
    dev, counts = 0.0, []
    for seed in range(6):
        run = mc.minres_reference(P, case.b, minv, rtol=rtol, perm=np.random.default_rng(1000 + seed).permutation(case.n))
        counts.append(run.its)
        dev = max(dev, abs(run.hist[k - 1] / ref.hist[k - 1] - 1.0), abs(run.hist[k] / ref.hist[k] - 1.0))
    margin = np.sqrt(ratio) - 1.0
    print("k %d, rtol %.3e, ratio %.3f, margin %.3f, deviation %.2e" % (k, rtol, ratio, margin, dev))
    assert counts == [k] * 6 and dev < 0.1 * margin


def test_sizes_cover_the_tail_and_the_tile():
    assert [mc.kron(*c).n for c in mc.KRON_NONE] == [1057, 512, 513, 1027]
    assert [cc.lap(*cc.LAP[i]).n for i, _ in mc.LAP] == [1023, 1073, 1023]


def test_restatement_names_the_failures():
    case = mc.kron(*mc.KRON[0])
    assert mc.minres_reference(case.P, case.b, cc.jacobi(case.P)).reason == "indefinite preconditioner"      # plain Jacobi: negative entries
    assert mc.minres_reference(case.P, case.b, mc.jacobi_abs(case.P)).reason == "converged"
    r = mc.minres_reference(case.P, case.b, rtol=1e-8, max_it=2)
    assert r.reason == "its" and r.its == 2
    z = mc.minres_reference(case.P, np.zeros(case.n))
    assert z.reason == "converged" and z.its == 0 and not z.y.any()
    b = case.b.copy(); b[5] = np.nan
    assert mc.minres_reference(case.P, b).reason == "not a number"
    D = np.diag(-1.0 - np.arange(5.0))
    assert mc.minres_reference(D, np.ones(5), cc.jacobi(D)).reason == "indefinite preconditioner"            # (b, z) < 0 before the first iteration


def test_reported_norm_is_the_true_residual_in_the_m_inverse_norm():
    for pc in ("none", "jacobi-abs"):
        case, ref = mc.kron_reference(*mc.KRON[0], pc)
        assert ref.gap <= 1e-10 * ref.beta1
        assert abs(mc.mnorm(mc.minv_of(case.P, pc), case.b - case.P @ ref.y) - ref.true) == 0.0
