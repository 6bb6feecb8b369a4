"""One EPS object solved five times with different solvers and settings leaves, after each solve, exactly what a fresh object with the
same settings leaves: the set-up of every solver resets the results of the last solve in one place (eps_setup_common, ks_eps.hip), and a
result array, counter or flag that one solver's set-up forgot would show here as a difference.

The sequence on the reused object:
  (a) two-sided Krylov-Schur on the Brusselator model (nhep_cases.brusselator(30), n = 60, the size test_gpu_nhep.py uses), largest real
      part: conjugate pairs are among the wanted values
  (b) the same matrix one-sided, with one-sided balancing
  (c) new operators (2-D Laplacian 30 x 30, EPS_HEP): LOBPCG, nev = 4
  (d) Krylov-Schur on the same problem with a deflation space of two vectors
  (e) (d) again without setting the deflation space again: it was consumed by (d), so this is a solve without one

The reference of every comparison is the same solve on a fresh object of the same context, and the comparison is bitwise (np.array_equal):
both objects make the same library calls on the same data in the same order, so there is no rounding to allow for."""
import numpy as np
import pytest

import nhep_cases as nc

pytestmark = pytest.mark.gpu
NEV = 4


def _results(eps):
    """everything a solve leaves behind; the left eigenvectors, or the refusal of the call"""
    import slepc_amd as ks
    n = eps.GetConverged()
    out = {"nconv": n, "its": eps.GetIterationNumber(), "reason": eps.GetConvergedReason(), "stats": eps.GetStats(),
           "dims": eps.GetDimensions(), "lobpcg": eps.LOBPCGGetStats(), "permutations": eps.GetTwoSidedStats(),
           "eig": np.array([eps.GetEigenvalue(i) for i in range(n)]), "errest": np.array([eps.GetErrorEstimate(i) for i in range(n)])}
    pairs = [eps.GetEigenpair(i) for i in range(n)]
    out["pair_eig"] = np.array([p[:2] for p in pairs])
    out["xr"] = np.array([p[2] for p in pairs]); out["xi"] = np.array([p[3] for p in pairs])
    try:
        left = [eps.GetLeftEigenvector(i) for i in range(n)]
        out["left"] = "returned"
        out["yr"] = np.array([y[0] for y in left]); out["yi"] = np.array([y[1] for y in left])
    except ks.KsError as e:
        out["left"] = "refused with %d" % e.rc
    return out


def _assert_same(step, got, want):
    assert got.keys() == want.keys(), (step, sorted(got), sorted(want))
    for key in want:
        g, w = got[key], want[key]
        print("(%s) %s: %s" % (step, key, w if not isinstance(w, np.ndarray) or w.ndim < 2 or key in ("eig", "pair_eig") else "array %s" % (w.shape,)))
        same = np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
        assert same, "(%s) %s of the reused object differs from a fresh one: %r != %r" % (step, key, g, w)


def test_reused_solver_equals_fresh_ones(ctx):
    import slepc_amd as ks
    Ao = nc.brusselator(30)
    An = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)
    L = ks.Mat.laplacian2d(ctx, 30)
    Cm = np.random.default_rng(7).standard_normal((L.n, 2))

    def nonsymmetric(eps):
        eps.SetOperators(An); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(NEV); eps.SetWhichEigenpairs("largest_real")
        eps.SetTolerances(1e-8, 1000)

    def symmetric(eps):
        eps.SetOperators(L); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(NEV); eps.SetWhichEigenpairs("smallest_real")
        eps.SetTolerances(1e-8, 1000)

    # what a fresh object needs for each solve, and the changes that take the reused object there from the solve before
    def fresh_a(eps): nonsymmetric(eps); eps.SetTwoSided(True)
    def fresh_b(eps): nonsymmetric(eps); eps.SetBalance("oneside")
    def fresh_c(eps): symmetric(eps); eps.SetType("lobpcg")
    def fresh_d(eps): symmetric(eps); eps.SetDeflationSpace(Cm)
    def fresh_e(eps): symmetric(eps)
    def change_b(eps): eps.SetTwoSided(False); eps.SetBalance("oneside")
    def change_c(eps): symmetric(eps); eps.SetBalance("none"); eps.SetType("lobpcg")
    def change_d(eps): eps.SetType("krylovschur"); eps.SetDeflationSpace(Cm)
    def change_e(eps): pass

    reused = ks.EPS(ctx)
    seen = {}
    for step, change, fresh in (("a", fresh_a, fresh_a), ("b", change_b, fresh_b), ("c", change_c, fresh_c), ("d", change_d, fresh_d), ("e", change_e, fresh_e)):
        change(reused); reused.Solve()
        got = _results(reused)
        other = ks.EPS(ctx)
        fresh(other); other.Solve()
        want = _results(other)
        other.destroy()
        assert want["nconv"] >= NEV and want["reason"] == ks.EPS_CONVERGED_TOL, (step, want["nconv"], want["reason"])
        _assert_same(step, got, want)
        seen[step] = want
    # the cases are what they claim to be
    assert np.any(seen["a"]["eig"][:NEV, 1] != 0.0) and seen["a"]["left"] == "returned"          # (a): a conjugate pair among the wanted values
    assert seen["b"]["left"].startswith("refused")                                                 # (b): one-sided, non-symmetric: no left vectors
    assert seen["c"]["lobpcg"]["iterations"] > 0 and seen["d"]["lobpcg"]["iterations"] == 0
    assert not np.array_equal(seen["d"]["eig"], seen["e"]["eig"])                                  # (d) deflated two vectors, (e) did not
