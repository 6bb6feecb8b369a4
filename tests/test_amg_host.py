"""The hierarchy of the smoothed-aggregation multigrid preconditioner on the host (ksc::amg_plan of slepc_amd/csrc/ks_csr.cpp) through the test hook
libksgpu.so exports. CPU only. The restatement it is compared with: tests/amg_cases.py. Values are compared entry by entry with
|got - ref| <= 1e-13 s, s being the sum of the absolute values of the products the entry is made of (the entry's own size where nothing cancels;
an entry that cancels to nearly nothing has no relative accuracy to ask for - neither summation order has it; numpy's allclose with rtol 1e-13 would
let 1e-8 pass there): sums of at most a few hundred products, and any structural mistake is many orders above. The sanitizer run is a program of its own (tests/host/amg_plan.cpp)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-13


@pytest.fixture(scope="module")
def lib():
    return ac.load()


def _same_pattern(G, R):
    return G.shape == R.shape and np.array_equal(G.indptr, R.indptr) and np.array_equal(G.indices, R.indices)


def _compare(got, ref, what):
    """Levels, aggregates, patterns and values of the library's hierarchy against the restatement's."""
    assert [l["n"] for l in got] == [l["n"] for l in ref], what
    for l, (g, r) in enumerate(zip(got, ref)):
        assert _same_pattern(g["A"], r["A"]), (what, l)
        if l:
            assert np.all(np.abs(g["A"].data - r["A"].data) <= RTOL * ref[l - 1]["Ac_scale"].data), (what, l)
        else:
            assert np.array_equal(g["A"].data, r["A"].data), what
        assert abs(g["rho"] - r["rho"]) <= RTOL * r["rho"], (what, l)
        assert ("agg" in g) == ("agg" in r), (what, l)
        if "agg" in r:
            assert np.array_equal(g["agg"], r["agg"]) and g["nagg"] == r["nagg"], (what, l)
            assert _same_pattern(g["P"], r["P"]), (what, l)
            assert np.all(np.abs(g["P"].data - r["P"].data) <= RTOL * r["P_scale"].data), (what, l)


def _invariants(levels):
    for lev in levels[:-1]:
        agg, nagg = lev["agg"], lev["nagg"]
        assert agg.min() >= -1 and agg.max() == nagg - 1
        assert np.all(np.bincount(agg[agg >= 0], minlength=nagg) > 0)                      # no aggregate is empty; a node has one index: at most one aggregate
        T = ac.tentative(agg, nagg)
        assert np.allclose((T.T @ T).toarray(), np.eye(nagg), rtol=0, atol=4 * 2.0 ** -52)


CASES = {
    "grid 45x31": (lambda: ac.arrays(ac.grid2d(45, 31)), dict(coarse_limit=8)),
    "grid 17x9": (lambda: ac.arrays(ac.grid2d(17, 9)), dict(coarse_limit=8)),
    "12^3": (lambda: ac.arrays(ac.laplacian3d(12)), dict(coarse_limit=8)),
    "two grids and five identity rows": (lambda: ac.arrays(ac.blocks_with_isolated_rows()), dict(coarse_limit=8)),
    "upwind": (lambda: ac.arrays(ac.upwind()), dict(coarse_limit=8)),
    "random unsymmetric, scrambled": (lambda: ac.random_scrambled(), dict(coarse_limit=4)),
    "grid 17x9, plain aggregation": (lambda: ac.arrays(ac.grid2d(17, 9)), dict(coarse_limit=8, smooth=False)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hierarchy_equals_the_restatement(lib, name):
    make, kw = CASES[name]
    arr = make()
    n = len(arr[0]) - 1
    ref = ac.hierarchy(ac.summed(*arr, n), **kw)
    got = ac.plan(lib, arr, **kw)
    assert len(got) >= 2, name
    _compare(got, ref, name)
    _invariants(got)
    if name == "two grids and five identity rows":
        assert np.array_equal(np.flatnonzero(got[0]["agg"] < 0), 153 + np.arange(5))       # the isolated rows are outside every aggregate
        assert np.all(np.diff(got[0]["P"].indptr)[153:158] == 0)                            # and their prolongator rows are empty
    if name == "random unsymmetric, scrambled":
        A = ac.summed(*arr, n)
        assert (A.data == 0.0).sum() > 0                                                    # entries that cancelled are stored, and are no edges


def test_diagonal_matrix_stays_one_level(lib):
    arr = ac.arrays(sp.diags([2.0 + np.cos(np.arange(300))], [0]).tocsr())
    got = ac.plan(lib, arr)
    assert [l["n"] for l in got] == [300] and "agg" not in got[0]
    agg, nagg = ac.aggregate(ac.strength(ac.summed(*arr, 300), 2.0 + np.cos(np.arange(300)), 0.0))
    assert nagg == 0 and np.all(agg == -1)


def test_one_row(lib):
    got = ac.plan(lib, (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-3.0])))
    assert [l["n"] for l in got] == [1] and got[0]["A"].data[0] == -3.0
    got = ac.plan(lib, (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-3.0])), coarse_limit=1, max_levels=1)
    assert [l["n"] for l in got] == [1]


def test_anisotropic_threshold_keeps_aggregates_in_grid_lines(lib):
    """kron(I, T) + 0.01 kron(T, I) on 40 x 40: with theta = 0.25 only the couplings along a line are strong."""
    arr = ac.arrays(ac.anisotropic(40, 0.01))

    def in_lines(agg, nagg):
        return all(np.unique(np.flatnonzero(agg == a) // 40).size == 1 for a in range(nagg))
    strong = ac.plan(lib, arr, theta=0.25)
    weak = ac.plan(lib, arr, theta=0.0)
    assert in_lines(strong[0]["agg"], strong[0]["nagg"])
    assert not in_lines(weak[0]["agg"], weak[0]["nagg"])
    _compare(strong, ac.hierarchy(ac.anisotropic(40, 0.01), theta=0.25), "anisotropic, theta 0.25")


@pytest.mark.parametrize("name", ["grid 45x31", "12^3"])
def test_galerkin_operators_are_symmetric(lib, name):
    make, kw = CASES[name]
    got = ac.plan(lib, make(), **kw)
    ref = ac.hierarchy(ac.summed(*make(), len(make()[0]) - 1), **kw)
    for l in range(1, len(got)):
        A = got[l]["A"]; At = A.T.tocsr(); At.sort_indices()
        assert _same_pattern(A, At)
        assert np.all(np.abs(A.data - At.data) <= RTOL * ref[l - 1]["Ac_scale"].data), (name, l)
        # R A P itself, from the library's own P
        P = got[l - 1]["P"]
        assert np.all(np.abs(A.data - ac.on_pattern(P.T @ got[l - 1]["A"] @ P, A).data) <= RTOL * ref[l - 1]["Ac_scale"].data)


def test_level_rows(lib):
    assert [l["n"] for l in ac.plan(lib, ac.arrays(ac.grid2d(45, 31)), coarse_limit=8)] == [1395, 247, 31, 4]
    assert [l["n"] for l in ac.plan(lib, ac.arrays(ac.laplacian3d(12)), coarse_limit=8)] == [1728, 219, 9, 1]
    assert [l["n"] for l in ac.plan(lib, ac.arrays(ac.grid2d(64, 64)))] == [4096, 704, 80]


def test_limits_stop_the_hierarchy(lib):
    arr = ac.arrays(ac.grid2d(45, 31))
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=8, max_levels=2)] == [1395, 247]
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=8, max_levels=1)] == [1395]
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=8, max_levels=40)] == [1395, 247, 31, 4]      # more than the cap of 16 asks for 16
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=1395)] == [1395]
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=247)] == [1395, 247]
    # the stall rule: a level whose aggregates number more than `stall` times its rows is the last. An aggregate of this algorithm has at least two
    # nodes, so the library's 0.8 is a safeguard no matrix reaches; the hook takes the ratio so that the rule itself can be exercised. The ratios of
    # this hierarchy are 247 / 1395 = 0.177, 31 / 247 = 0.126, 4 / 31 = 0.129; of 12^3: 219 / 1728 = 0.127, 9 / 219 = 0.041, 1 / 9 = 0.111
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=8, stall=0.18)] == [1395, 247, 31, 4]
    assert [l["n"] for l in ac.plan(lib, arr, coarse_limit=8, stall=0.17)] == [1395]
    assert [l["n"] for l in ac.hierarchy(ac.grid2d(45, 31), coarse_limit=8, stall=0.17)] == [1395]
    cube = ac.arrays(ac.laplacian3d(12))
    assert [l["n"] for l in ac.plan(lib, cube, coarse_limit=8, stall=0.127)] == [1728, 219, 9, 1]
    assert [l["n"] for l in ac.plan(lib, cube, coarse_limit=8, stall=0.126)] == [1728]
    assert [l["n"] for l in ac.plan(lib, cube, coarse_limit=0, stall=0.127)] == [1728, 219, 9, 1]           # one row: no edge, no aggregate, the last level


def test_zero_or_missing_diagonal_names_the_row(lib):
    S = ac.grid2d(17, 9).tolil()
    S[40, 40] = 0.0
    Z = S.tocsr()                                                    # the zero stays stored
    assert ac.plan(lib, ac.arrays(Z), coarse_limit=8) == (ac.AMG_NO_DIAGONAL, 0, 40)
    Z.eliminate_zeros()                                              # now row 40 stores no diagonal
    assert ac.plan(lib, ac.arrays(Z), coarse_limit=8) == (ac.AMG_NO_DIAGONAL, 0, 40)
    with pytest.raises(ac.ZeroDiagonal) as e:
        ac.hierarchy(Z, coarse_limit=8)
    assert (e.value.level, e.value.row) == (0, 40)
    assert len(ac.plan(lib, ac.arrays(Z), coarse_limit=153)) == 1   # a level that is solved directly needs no diagonal


def test_restated_cycle_converges_like_multigrid():
    """The restatement itself: preconditioned CG with its cycle needs a grid-independent handful of iterations, point Jacobi does not."""
    for m, most in ((32, 10), (64, 12)):
        A = ac.grid2d(m, m)
        L = ac.hierarchy(A)
        b = np.random.default_rng(m).standard_normal(m * m)
        its = ac.pcg_iterations(A, lambda r: ac.cycle(L, r), b)
        jac = ac.pcg_iterations(A, lambda r: r / A.diagonal(), b)
        print("grid %d^2: PCG iterations %d with the cycle, %d with point Jacobi" % (m, its, jac))
        assert its <= most and jac >= 8 * its
    # the cycle is symmetric
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal(m * m), rng.standard_normal(m * m)
    a, b_ = u @ ac.cycle(L, v), v @ ac.cycle(L, u)
    assert abs(a - b_) <= 1e-12 * abs(a)


# ---- sanitizers --------------------------------------------------------------------------------------------------------------------------
def test_plan_under_asan_ubsan(tmp_path):
    """tests/host/amg_plan.cpp, a program of its own built together with ks_csr.cpp with -fsanitize=address,undefined: the hierarchies of three of the
    cases above with their invariants. Nothing is preloaded and nothing is loaded into Python."""
    exe = str(tmp_path / "amg_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", os.path.join(ROOT, "tests", "host", "amg_plan.cpp"),
                           os.path.join(ROOT, "slepc_amd", "csrc", "ks_csr.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    for name in ("grid 45x31", "two grids and five identity rows", "random unsymmetric 60", "zero diagonal", "n = 0, n = 1 and a diagonal"):
        assert any(line.startswith("ok " + name) for line in lines), (name, lines)
