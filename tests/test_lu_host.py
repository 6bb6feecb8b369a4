"""Sparse LU with fill on the host (ksc::lu_ordering, ksc::csr_lu_plan, ksc::lu_apply_host of slepc_amd/csrc/ks_csr.cpp): the nested dissection
ordering, the factors, the level sets and stages that the kernels of ks_pc_lu.hip walk, and the host applies, through the test hooks libksgpu.so
exports. CPU only. The reference and the bound: tests/lu_cases.py. The sanitizer run is a program of its own (tests/host/lu_plan.cpp)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import lu_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 64


@pytest.fixture(scope="module")
def lib():
    return lc.load()


def _is_perm(p, n):
    return p.size == n and np.array_equal(np.sort(p), np.arange(n))


# ---- ordering ----------------------------------------------------------------------------------------------------------------------------
def _graphs():
    path = sp.diags([np.ones(39), np.ones(40), np.ones(39)], [-1, 0, 1]).tocsr()
    two = sp.block_diag([lc.laplacian2d(7), lc.laplacian2d(5), lc.laplacian2d(2)]).tocsr()
    isolated = sp.block_diag([sp.identity(3), lc.laplacian2d(6), sp.identity(2)]).tocsr()
    dense = sp.csr_matrix(np.ones((20, 20)))
    one = sp.csr_matrix(np.array([[3.0]]))
    unsym = lc.random_unsymmetric(150, 4, 1)
    return {"path": path, "disconnected": two, "isolated nodes": isolated, "dense": dense, "n = 1": one, "unsymmetric": unsym, "grid": lc.laplacian2d(17, 9)}


@pytest.mark.parametrize("name", list(_graphs()))
def test_ordering_is_a_permutation_and_deterministic(lib, name):
    S = _graphs()[name]
    n = S.shape[0]
    arr = lc.arrays(S)
    p1 = lc.ordering(lib, arr, lc.ND); p2 = lc.ordering(lib, arr, lc.ND)
    assert _is_perm(p1, n), p1
    assert np.array_equal(p1, p2)
    assert np.array_equal(lc.ordering(lib, arr, lc.NATURAL), np.arange(n))
    # the ordering depends on the pattern of P + P^T only: the transposed matrix gets the same one
    assert np.array_equal(lc.ordering(lib, lc.arrays(S.T.tocsr()), lc.ND), p1)
    if name in ("dense", "n = 1"):                      # one level structure of at most two levels: listed ascending
        assert np.array_equal(p1, np.arange(n))
    if name == "isolated nodes":                        # components in the order of their smallest nodes; small ones ascending
        assert np.array_equal(p1[:3], [0, 1, 2]) and np.array_equal(p1[-2:], [n - 2, n - 1])
    if name == "path":
        # the separator of a path from one of its ends is the middle node, and it goes last
        assert p1[-1] == 20, p1


def test_nested_dissection_against_natural_on_the_63x63_laplacian(lib):
    S = lc.laplacian2d(63)
    n = S.shape[0]
    nd = lc.plan(lib, lc.arrays(S), lc.ND, WIDE); nat = lc.plan(lib, lc.arrays(S), lc.NATURAL, WIDE)
    stored = lambda p: p["nnz_l"] + p["nnz_u"]
    print("entries of L + U: ND %d, natural %d (ratio %.3f); levels of L: ND %d, natural %d" % (stored(nd), stored(nat), stored(nd) / stored(nat), nd["levels"][0], nat["levels"][0]))
    assert nat["nnz_u"] == 250109 and nat["levels"][0] == n           # the band fills completely
    assert 2 * stored(nd) <= stored(nat)
    assert nd["levels"][0] <= n // 8


# ---- factors -----------------------------------------------------------------------------------------------------------------------------
def _factor_cases():
    return {"random 300": (lc.arrays(lc.random_unsymmetric(300, 5, 2)), lc.ND), "random 301 denser": (lc.arrays(lc.random_unsymmetric(301, 9, 3)), lc.ND),
            "random natural": (lc.arrays(lc.random_unsymmetric(120, 5, 4)), lc.NATURAL), "repeated and unsorted": (lc.scrambled(90), lc.ND),
            "diagonal made by fill": (lc.arrays(lc.fill_makes_the_diagonal()), lc.NATURAL), "symmetric indefinite": (lc.arrays(lc.symmetric_indefinite()), lc.ND)}


@pytest.mark.parametrize("name", list(_factor_cases()))
def test_factors_bit_for_bit(lib, name):
    arr, which = _factor_cases()[name]
    n = len(arr[0]) - 1
    x = np.random.default_rng(5).standard_normal(n)
    p = lc.plan(lib, arr, which, WIDE, x)
    assert isinstance(p, dict), p
    perm = p["perm"]
    assert _is_perm(perm, n)
    P = lc.summed(*arr)
    Lr, Ur = lc.dense_lu(P[perm][:, perm])
    L = p["L"].toarray() + np.eye(n); U = p["U"].toarray()
    assert np.array_equal(np.tril(p["L"].toarray(), -1), p["L"].toarray()) and np.array_equal(np.triu(U), U)
    assert np.array_equal(L, Lr), name
    assert np.array_equal(U, Ur), name
    # stored patterns: ascending columns, the pivot first in every row of U; nothing dropped - the pattern holds every non-zero of the reference
    for T in (p["L"], p["U"]):
        for r in range(n):
            c = T.indices[T.indptr[r]:T.indptr[r + 1]]
            assert np.all(np.diff(c) > 0)
    assert np.array_equal(p["U"].indices[p["U"].indptr[:-1]], np.arange(n))
    assert p["neg"] == int((np.diag(Ur) < 0).sum()) and p["pos"] == int((np.diag(Ur) > 0).sum())
    # the sparse restatement the GPU tests use agrees with the dense one
    Ls, Us = lc.lu_nopivot(sp.csr_matrix(P[perm][:, perm]))
    assert np.array_equal(Ls.toarray() + np.eye(n), Lr) and np.array_equal(Us.toarray(), Ur)
    # host applies, forward and transposed
    ref = lc.Reference(sp.csr_matrix(P), perm)
    ref.check(x, p["y"], name)
    ref.check(x, p["yt"], name, transpose=True)
    if name == "diagonal made by fill":
        assert P[n - 1, n - 1] == 0.0 and Ur[n - 1, n - 1] != 0.0
    if name == "symmetric indefinite":
        lam = np.linalg.eigvalsh(P)
        assert p["neg"] == int((lam < 0).sum()) and 0 < p["neg"] < n


def test_zero_pivot(lib):
    n = 40
    S = sp.lil_matrix(sp.diags([np.full(n, 2.0)], [0]))
    S[17, 17] = 0.0; S[18, 18] = 0.0; S[17, 18] = 1.0; S[18, 17] = 1.0
    S[5, 30] = 0.5; S[30, 5] = -0.5
    A = S.tocsr(); A.sort_indices()
    assert lc.plan(lib, lc.arrays(A), lc.NATURAL, WIDE) == (lc.LU_ZERO_PIVOT, 17)
    # under another numbering of the same matrix the zero pivot is reported with its ORIGINAL row
    q = np.random.default_rng(6).permutation(n)
    B = A[q][:, q].tocsr(); B.sort_indices()
    st = lc.plan(lib, lc.arrays(B), lc.NATURAL, WIDE)
    assert st[0] == lc.LU_ZERO_PIVOT and q[st[1]] in (17, 18)


# ---- level sets, stages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wide", [("grid", 16), ("random", 8), ("wide narrow wide", 32), ("tridiagonal", 64), ("pairs", 10), ("diagonal", 4)])
def test_levels_and_stages(lib, name, wide):
    S, which = {"grid": (lc.laplacian2d(21), lc.ND), "random": (lc.random_unsymmetric(200, 4, 7), lc.ND), "wide narrow wide": (lc.wide_narrow_wide(32), lc.NATURAL),
                "tridiagonal": (lc.tridiagonal(300), lc.NATURAL), "pairs": (lc.pairs(10), lc.NATURAL), "diagonal": (sp.identity(9, format="csr") * 2.0, lc.ND)}[name]
    n = S.shape[0]
    p = lc.plan(lib, lc.arrays(S), which, wide)
    Us = sp.triu(p["U"], 1).tocsr()
    # the strict triangles come from the stored PATTERN (an entry that is numerically zero still orders its row behind the one it reads)
    Lp = p["L"].copy(); Lp.data[:] = 1.0; Up = Us.copy(); Up.data[:] = 1.0
    lev_base = 0
    stage_at = 0
    for t, (T, lower) in enumerate(((Lp, True), (Up, False))):
        order, starts, stages = lc.levels_and_stages(T, lower, wide)
        assert p["levels"][t] == len(starts) - 1
        assert np.array_equal(p["rows"][t * n:(t + 1) * n], order)
        assert np.array_equal(p["lev"][lev_base:lev_base + len(starts)], t * n + starts)
        got = p["stages"][stage_at:stage_at + p["nstage"][t]]
        assert got == [(lev_base + a, b, c) for a, b, c in stages], (t, got, stages)
        # the rows' entries in level order: contiguous, ascending columns, the values of the factor
        Tv = p["L"] if t == 0 else Us
        for pos in range(n):
            r = order[pos]; e = slice(p["rp"][t * n + pos], p["rp"][t * n + pos + 1])
            assert np.array_equal(p["col"][e], Tv.indices[Tv.indptr[r]:Tv.indptr[r + 1]]) and np.array_equal(p["val"][e], Tv.data[Tv.indptr[r]:Tv.indptr[r + 1]])
        lev_base += len(starts) - 1; stage_at += p["nstage"][t]
    assert np.array_equal(p["dinv"], 1.0 / p["U"].diagonal()[p["rows"][n:]])
    assert set(p["lanes"]) <= {1, 8, 64}
    for a, b, c in p["stages"]:
        if not c:
            assert np.all(p["lanes"][a:a + b] == 64)               # a narrow stage sums a row with a whole wave
    if name == "tridiagonal":
        assert p["nstage"] == (1, 1) and lc.launches(p["stages"]) == (0, 2) and p["levels"] == (n, n)
        assert p["nstage_t"] == (1, 1) and p["levels_t"] == (n, n)
    if name == "pairs":
        assert p["levels"] == (2, 1) and p["stages"] == [(0, 2, 1), (2, 1, 1)]
    if name == "wide narrow wide":
        assert [s[2] for s in p["stages"][:p["nstage"][0]]] == [1, 0, 1] and p["stages"][1][1] == 3
    if name == "diagonal":
        assert p["levels"] == (1, 1) and p["nnz_l"] == 0 and p["nnz_u"] == n


@pytest.mark.parametrize("name", ["laplacian 15x15 in its spectrum", "pencil", "arrow 200", "random wide levels"])
def test_host_applies_with_every_lane_count(lib, name):
    """The bound for the forward and the transposed host apply, at a threshold low enough that the wide levels use 1, 8 and 64 lanes per row."""
    S, which, wide = {"laplacian 15x15 in its spectrum": (lc.shifted(lc.laplacian2d(15), 2.3), lc.ND, 4), "pencil": (lc.shifted(lc.line_pencil(12, 9)[0], 0.4), lc.ND, 2),
                      "arrow 200": (lc.arrow_last_row(200), lc.NATURAL, 1), "random wide levels": (lc.random_unsymmetric(260, 3, 8), lc.NATURAL, 1)}[name]
    n = S.shape[0]
    x = np.random.default_rng(9).standard_normal(n)
    p = lc.plan(lib, lc.arrays(S), which, wide, x)
    ref = lc.Reference(S, p["perm"])
    ref.check(x, p["y"], name)
    ref.check(x, p["yt"], name, transpose=True)
    print(name, "lanes used:", sorted(set(p["lanes"])))
    # the threshold changes the schedule and the lanes of a row, not the factors
    q = lc.plan(lib, lc.arrays(S), which, 1 << 30, x)
    assert np.array_equal(q["L"].data, p["L"].data) and np.array_equal(q["U"].data, p["U"].data) and np.array_equal(q["perm"], p["perm"])
    assert lc.launches(q["stages"]) == (0, 2)
    ref.check(x, q["y"], name + ", all narrow")


# ---- sanitizers --------------------------------------------------------------------------------------------------------------------------
def test_plan_and_host_applies_under_asan_ubsan(tmp_path):
    """tests/host/lu_plan.cpp, a program of its own built together with ks_csr.cpp with -fsanitize=address,undefined: plans and host applies of three
    small matrices. Nothing is preloaded and nothing is loaded into Python."""
    exe = str(tmp_path / "lu_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", os.path.join(ROOT, "tests", "host", "lu_plan.cpp"),
                           os.path.join(ROOT, "slepc_amd", "csrc", "ks_csr.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    for name in ("laplacian 9x9, nd", "random unsymmetric 70, nd", "arrow 130, natural", "zero pivot", "n = 0 and n = 1"):
        assert any(line.startswith("ok " + name) for line in lines), (name, lines)
    assert lines[-1] == "all ok"
