"""Sparse LU with fill on the ST's KSP (KS_PC_LU, KS_KSP_PREONLY; k_lu_level and k_lu_narrow in slepc_amd/csrc/ks_pc_lu.hip).

The kernels are checked through PCApply against a numpy elimination without pivoting under the library's own permutation (tests/lu_cases.py)
with the componentwise bound  |L U (Q y) - Q x| <= 8 (k + 1) 2^-53 |L||U||Q y|,  k the longest row of the factors - no tuned tolerance. The
threshold between wide and narrow levels is read from PCLUGetInfo, so the cases on both sides of it follow the library's constant.
Unless a test says otherwise: sinvert with one matrix, shell mode."""
import numpy as np
import pytest
import scipy.sparse as sp

import golden_inputs as gi
import lu_cases as lc
import nhep_cases as nc
import twosided_cases as TS
from oracle import oracle as O
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
SUP, ORDER, OUTOFRANGE, ZRPVT = 56, 58, 63, 71


def _mat(ctx, S, keep=True):
    import slepc_amd as ks
    rp, col, val = S if isinstance(S, tuple) else lc.arrays(S)
    return ks.Mat.from_csr(ctx, rp, col, val, keep_csr=keep)


def _st(ctx, A, sigma=0.0, B=None, kind="sinvert", mode="shell", ordering="nd", ksp=None, transpose=False):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(A, B); st.SetMatMode(mode); st.SetPC("lu"); st.PCLUSetOrdering(ordering)
    if ksp:
        st.SetKSPType(ksp)
    if transpose:
        st.SetTransposeSolves(True)
    return st


def _x(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _case(ctx, S, seed, what, ordering="nd", sigma=0.0):
    """PCApply on P = S - sigma I against the reference; returns (st, reference, x, y, info)."""
    st = _st(ctx, _mat(ctx, S), sigma=sigma, ordering=ordering)
    x = _x(S.shape[0], seed)
    y = st.PCApply(x)
    perm = st.PCLUGetPermutation()
    if ordering == "natural":
        assert np.array_equal(perm, np.arange(S.shape[0]))
    ref = lc.Reference(lc.shifted(S, sigma) if sigma != 0.0 else S, perm)
    ref.check(x, y, what)
    return st, ref, x, y, st.PCLUGetInfo()


def _expected_launches(ref, wide):
    Ls = sp.tril(ref.L, -1).tocsr(); Us = sp.triu(ref.U, 1).tocsr()
    a = lc.launches(lc.levels_and_stages(Ls, True, wide)[2]); b = lc.launches(lc.levels_and_stages(Us, False, wide)[2])
    return a[0] + b[0], a[1] + b[1]


# ---- 1: row lengths of a narrow stage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 127, 128, 129, 1000])
def test_narrow_stage_row_lengths(ctx, m):
    """Identity plus a last row coupled to all m others, natural ordering: one row of m entries, summed by one wave - the strides of 64 lanes on both
    sides of their boundaries, and a row longer than the workgroup."""
    st, ref, x, y, info = _case(ctx, lc.arrow_last_row(m), m, "arrow %d" % m, ordering="natural")
    assert info["n"] == m + 1 and info["nnz_l"] == m and info["nnz_u"] == m + 1
    assert info["levels_l"] == (2 if m else 1) and info["levels_u"] == 1
    assert (info["wide_launches"], info["narrow_launches"]) == _expected_launches(ref, info["wide"])


# ---- 2: both sides of the threshold ------------------------------------------------------------------------------------------------------
def _wide(ctx):
    return _st(ctx, _mat(ctx, sp.identity(2, format="csr") * 2.0), ordering="natural").PCLUGetInfo()["wide"]


@pytest.mark.parametrize("side", ["below", "at"])
def test_pairs_on_both_sides_of_the_threshold(ctx, side):
    W = _wide(ctx)
    assert W >= 2
    m = W - 1 if side == "below" else W
    st, ref, x, y, info = _case(ctx, lc.pairs(m), 20, "pairs m = %d" % m, ordering="natural")
    assert info["levels_l"] == 2 and info["levels_u"] == 1
    # L: two levels of m rows - one narrow launch below the threshold, two wide launches at it; U: one level of 2 m rows (wide from m = W / 2 on)
    l_wide, l_narrow = (0, 1) if side == "below" else (2, 0)
    u_wide = 1 if 2 * m >= W else 0
    assert (info["wide_launches"], info["narrow_launches"]) == (l_wide + u_wide, l_narrow + 1 - u_wide)
    assert np.array_equal(st.PCApply(x), y)


def test_wide_narrow_wide_schedule(ctx):
    W = _wide(ctx)
    st, ref, x, y, info = _case(ctx, lc.wide_narrow_wide(W), 21, "wide narrow wide", ordering="natural")
    assert info["levels_l"] == 6
    assert (info["wide_launches"], info["narrow_launches"]) == (3 + 1, 1)                 # L: 2 wide levels, a narrow stage of 3, 1 wide level; U: one wide level
    assert (info["wide_launches"], info["narrow_launches"]) == _expected_launches(ref, W)
    # the same through the transposed plan: the roles of the triangles swap
    st2 = _st(ctx, _mat(ctx, lc.wide_narrow_wide(W)), ordering="natural", transpose=True)
    ref.check(x, st2.PCApplyTranspose(x), "wide narrow wide", transpose=True)


@pytest.mark.parametrize("name", ["n = 1", "diagonal", "tridiagonal"])
def test_degenerate_schedules(ctx, name):
    S = {"n = 1": sp.csr_matrix(np.array([[-3.0]])), "diagonal": sp.diags([2.0 + np.cos(np.arange(777))], [0]).tocsr(), "tridiagonal": lc.tridiagonal(1000)}[name]
    for ordering in ("natural", "nd"):
        st, ref, x, y, info = _case(ctx, S, 22, "%s, %s" % (name, ordering), ordering=ordering)
        if name == "diagonal":
            assert info["nnz_l"] == 0 and info["nnz_u"] == 777 and info["levels_l"] == 1 and info["levels_u"] == 1
            assert np.array_equal(y, x * (1.0 / S.diagonal()))                              # only the permutation and the scaling
        if name == "tridiagonal" and ordering == "natural":
            assert (info["wide_launches"], info["narrow_launches"]) == (0, 2) and info["levels_l"] == 1000 and info["levels_u"] == 1000
        if name == "n = 1":
            assert np.array_equal(y, x * (1.0 / -3.0)) and st.PCLUGetInertia() == (1, 0, 0)


# ---- 3, 4, 5: nested dissection on real patterns, several columns, the transposed side, the two matrix modes -----------------------------------
def _bfw_scipy():
    Sa = O.load_petsc_binary(gi.matrix_path("bfw62a.petsc")).to_scipy().tocsr(); Sb = O.load_petsc_binary(gi.matrix_path("bfw62b.petsc")).to_scipy().tocsr()
    Sa.sort_indices(); Sb.sort_indices()
    return Sa, Sb


def _real_patterns():
    pa, pb = lc.line_pencil(24, 30)
    ba, bb = _bfw_scipy()
    return {"laplacian 40x40 in its spectrum": (lc.laplacian2d(40), None, 2.2), "laplacian 12^3": (lc.laplacian3d(12), None, 0.0),
            "convection pencil 24x30": (pa, pb, -0.5), "bfw62": (ba, bb, -190000.0)}


@pytest.fixture(scope="module", params=list(_real_patterns()))
def real(request, ctx):
    """One set-up and one reference per matrix, shared by the tests below and left unchanged by them."""
    Sa, Sb, sigma = _real_patterns()[request.param]
    A = _mat(ctx, Sa); B = None if Sb is None else _mat(ctx, Sb)
    st = _st(ctx, A, sigma=sigma, B=B, transpose=True)
    P = lc.shifted(Sa, sigma, Sb)
    ref = lc.Reference(P, st.PCLUGetPermutation())
    return request.param, st, ref, P, (A, B, sigma)


def test_real_patterns_bound_and_repeatability(ctx, real):
    name, st, ref, P, _ = real
    n = P.shape[0]
    x = _x(n, 30)
    y = st.PCApply(x)
    ref.check(x, y, name)
    assert np.array_equal(st.PCApply(x), y)
    info = st.PCLUGetInfo()
    print(name, info)
    assert info["n"] == n and info["device_bytes"] >= 12 * (info["nnz_l"] + info["nnz_u"] - n)
    assert info["nnz_l"] >= ref.L.nnz - n and info["nnz_u"] >= ref.U.nnz                # the stored pattern holds every non-zero of the reference
    assert info["narrow_launches"] >= 1 and info["wide_launches"] + info["narrow_launches"] <= info["levels_l"] + info["levels_u"]


def test_real_patterns_several_columns(ctx, real):
    name, st, ref, P, _ = real
    n = P.shape[0]
    assert st.PCMultiColumns() == 8
    X = np.random.default_rng(31).standard_normal((n, 9))
    single = np.stack([st.PCApply(X[:, j]) for j in range(9)], axis=1)
    for k in (1, 7, 8, 9):
        assert np.array_equal(st.PCApplyMulti(X[:, :k]), single[:, :k]), (name, k)


def test_real_patterns_transposed(ctx, real):
    name, st, ref, P, _ = real
    x = _x(P.shape[0], 32)
    y = st.PCApplyTranspose(x)
    ref.check(x, y, name, transpose=True)
    assert np.array_equal(st.PCApplyTranspose(x), y)
    # PREONLY on the transposed side: STMatSolveTranspose is that one application
    A, B, sigma = real[4]
    st2 = _st(ctx, A, sigma=sigma, B=B, ksp="preonly", transpose=True)
    assert np.array_equal(st2.MatSolveTranspose(x), y)


def test_real_patterns_host_applies_are_the_kernels_sums(ctx, real):
    """ksc::lu_apply_host and its transposed sibling restate the kernels' summation order (lanes per row, the order of the DPP sums): the same bits."""
    name, st, ref, P, _ = real
    x = _x(P.shape[0], 34)
    p = lc.plan(lc.load(), lc.arrays(P), lc.ND, st.PCLUGetInfo()["wide"], x)
    assert np.array_equal(p["perm"], st.PCLUGetPermutation())
    assert np.array_equal(st.PCApply(x), p["y"]), name
    assert np.array_equal(st.PCApplyTranspose(x), p["yt"]), name


def test_transposed_is_refused_without_the_switch(ctx):
    import slepc_amd as ks
    st = _st(ctx, _mat(ctx, lc.laplacian2d(6)))
    with pytest.raises(ks.KsError) as e:
        st.PCApplyTranspose(np.ones(36))
    assert e.value.rc == SUP and "ks_st_set_transpose_solves" in str(e.value)


def test_modes_and_transformations(ctx, real):
    """Shell and copy mode factor the same arrays: identical bits. Cayley has the P of sinvert; a shift with two matrices has P = B."""
    name, st, ref, P, (A, B, sigma) = real
    x = _x(P.shape[0], 33)
    y = st.PCApply(x)
    assert np.array_equal(_st(ctx, A, sigma=sigma, B=B, mode="copy").PCApply(x), y)
    sc = _st(ctx, A, sigma=sigma, B=B, kind="cayley"); sc.CayleySetAntishift(1.5)
    assert np.array_equal(sc.PCApply(x), y)
    if B is not None and name != "bfw62":                                                   # (bfw62b is indefinite with small pivots: the pencil's B is the case)
        Sb = _real_patterns()[name][1]
        s2 = _st(ctx, A, sigma=0.3, B=B, kind="shift")
        lc.Reference(Sb, s2.PCLUGetPermutation()).check(x, s2.PCApply(x), name + ", P = B")


# ---- 6: PREONLY --------------------------------------------------------------------------------------------------------------------------
def test_preonly(ctx):
    Sa, Sb = lc.line_pencil(12, 10)
    A = _mat(ctx, Sa); B = _mat(ctx, Sb)
    n = Sa.shape[0]
    x = _x(n, 40)
    # one matrix: STApply is PCApply
    st = _st(ctx, A, sigma=0.7, ksp="preonly")
    assert st.GetKSPStats()["solves"] == 0
    before = st.GetKSPStats()["last_rnorm"]
    y = st.Apply(x)
    assert np.array_equal(y, st.PCApply(x))
    # two matrices: the B product first
    sb = _st(ctx, A, sigma=0.7, B=B, ksp="preonly")
    assert np.array_equal(sb.Apply(x), sb.PCApply(B.mult(x)))
    for _ in range(2):
        st.Apply(x)
    stats = st.GetKSPStats()
    assert (stats["solves"], stats["iterations"]) == (3, 3) and stats["last_rnorm"] == before
    # an exact solve: the residual of P y = x at the level of the factorisation's backward error
    P = lc.shifted(Sa, 0.7)
    assert np.linalg.norm(P @ y - x) <= 1e-12 * np.linalg.norm(x)
    # PREONLY with point Jacobi is one Jacobi application
    st.SetPC("jacobi")
    yj = st.Apply(x)
    assert np.array_equal(yj, st.PCApply(x))
    assert np.allclose(yj, x / P.diagonal(), rtol=4 * 2.0 ** -52, atol=0)
    assert st.GetKSPStats()["solves"] == 4
    # GMRES behind LU converges in one iteration (the preconditioned operator is the identity to rounding)
    sg = _st(ctx, A, sigma=0.7)
    yg = sg.Apply(x)
    assert sg.GetKSPStats()["iterations"] <= 2 and np.linalg.norm(yg - y) <= 1e-10 * np.linalg.norm(y)


# ---- 7: inertia --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["below", "inside", "above"])
def test_inertia_of_the_shifted_laplacian(ctx, where):
    lam = lc.laplacian2d_eigenvalues(20)
    n = lam.size
    inside = next(i for i in range(130, n) if lam[i] - lam[i - 1] > 1e-3)          # a gap between two distinct eigenvalues: `inside` of them lie below it
    sigma = {"below": -0.5, "inside": 0.5 * (lam[inside - 1] + lam[inside]), "above": lam[-1] + 0.5}[where]
    st = _st(ctx, _mat(ctx, lc.laplacian2d(20)), sigma=sigma)
    neg, zero, pos = st.PCLUGetInertia()
    assert zero == 0 and neg + pos == n
    assert neg == int((lam < sigma).sum()) == {"below": 0, "inside": inside, "above": n}[where]


# ---- 8: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import slepc_amd as ks
    S = lc.random_unsymmetric(100, 5, 50)
    A = _mat(ctx, S)
    st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A)
    for bs in (1, 64):
        with pytest.raises(ks.KsError) as e:
            st.SetPC("lu", bs)
        assert e.value.rc == SUP
    with pytest.raises(ks.KsError) as e:
        st.PCLUSetOrdering(2)
    assert e.value.rc == OUTOFRANGE
    with pytest.raises(ks.KsError) as e:
        st.SetKSPType(3)
    assert e.value.rc == SUP
    with pytest.raises(ks.KsError) as e:
        st.PCLUGetInfo()                                            # the PC is still point Jacobi
    assert e.value.rc == ORDER
    assert st.PCLUGetOrdering() == "nd"
    # matrices that did not keep their CSR arrays
    s2 = _st(ctx, _mat(ctx, S, keep=False))
    with pytest.raises(ks.KsError) as e:
        s2.SetUp()
    assert e.value.rc == ORDER
    # a zero pivot under the natural ordering: [[0, 1], [1, 0]] at rows 40, 41 (P = B of a two-matrix shift, so that no shift touches it)
    Z = sp.lil_matrix(S); Z[40, :] = 0.0; Z[41, :] = 0.0; Z[40, 41] = 1.0; Z[41, 40] = 1.0
    Z = Z.tocsr(); Z.eliminate_zeros()
    s3 = _st(ctx, A, sigma=0.1, B=_mat(ctx, Z), kind="shift", ordering="natural")
    with pytest.raises(ks.KsError) as e:
        s3.SetUp()
    assert e.value.rc == ZRPVT and "row 40" in str(e.value)
    with pytest.raises(ks.KsError) as e:
        s3.PCApply(np.ones(100))                                    # still not set up: the same error, nothing half-built
    assert e.value.rc == ZRPVT
    s3.SetPC("jacobi")                                              # and usable again (diag(B) has two zeros, which point Jacobi leaves unscaled)
    assert np.all(np.isfinite(s3.PCApply(np.ones(100))))
    # a new ordering clears the set-up and gives other factors for the same solve
    s4 = _st(ctx, A)
    x = _x(100, 51)
    y_nd = s4.PCApply(x)
    p_nd = s4.PCLUGetPermutation()
    s4.PCLUSetOrdering("natural")
    assert np.array_equal(s4.PCLUGetPermutation(), np.arange(100)) and not np.array_equal(p_nd, np.arange(100))
    lc.Reference(S, np.arange(100)).check(x, s4.PCApply(x), "natural after nd")
    assert np.allclose(s4.PCApply(x), y_nd, rtol=1e-10, atol=1e-12)


def test_two_ranks_are_refused():
    """PETSc's built-in LU is sequential: KS_PC_LU on a two-rank communicator fails at set-up with KS_ERR_SUP on every rank."""
    N = 40
    S = lc.tridiagonal(N)
    split = [(0, 24), (24, N)]

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            r0, r1 = split[rank]
            L = S[r0:r1].tocsr()
            A = ks.Mat.from_csr(ctx, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data, row_start=r0, n_global=N, keep_csr=True)
            st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A); st.SetPC("lu")
            try:
                st.SetUp()
            except ks.KsError as e:
                return e.rc
            return 0
        finally:
            ctx.close()

    assert run_ranks(ThreadComm(2, pairwise=True, timeout=60), fn, join_timeout=120) == [SUP, SUP]


def test_new_exports():
    from slepc_amd import _lib
    L = _lib.lib()
    for name in ("ks_st_pc_lu_set_ordering", "ks_st_pc_lu_get_ordering_type", "ks_st_pc_lu_get_permutation", "ks_st_pc_lu_get_info", "ks_st_pc_lu_get_inertia"):
        assert hasattr(L, name) and name in _lib.header_symbols() and name in _lib._SIG
    import slepc_amd as ks
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define KS_PC_LU 4" in hdr and "KS_KSP_PREONLY = 2" in hdr and "#define KS_ORDERING_ND      0" in hdr and "#define KS_ORDERING_NATURAL 1" in hdr
    assert all(hasattr(ks.ST, m) for m in ("PCLUSetOrdering", "PCLUGetPermutation", "PCLUGetInfo", "PCLUGetInertia"))


# ---- 9: whole solves in the reference's own configuration: -st_ksp_type preonly -st_pc_type lu -----------------------------------------------
def _lu_preonly(eps, kind, transpose=False):
    st = eps.GetST(); st.SetType(kind); st.SetPC("lu"); st.SetKSPType("preonly")
    if transpose:
        st.SetTransposeSolves(True)
    return st


@pytest.mark.parametrize("kind", ["sinvert", "cayley"])
def test_eps_test1_target_22_golden(ctx, kind):
    """test1_1_ks_sinvert / test1_1_ks_cayley: -eps_target 22 on the GHEP of test1 reprints test1_1.out; A - 22 B is indefinite and is solved exactly.
    The restart counts are the oracle's, whose ST solves exactly as well."""
    import slepc_amd as ks
    from test_gpu_ghep import _test1_pencil
    Ao, Bo = _test1_pencil()
    eps = ks.EPS(ctx)
    eps.SetOperators(ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True), ks.Mat.from_csr(ctx, Bo.rowptr, Bo.col, Bo.val, keep_csr=True))
    eps.SetProblemType(ks.EPS_GHEP); eps.SetDimensions(4); eps.SetTolerances(0.0, 1500); eps.SetConvergenceTest("norm"); eps.SetTarget(22.0)
    st = _lu_preonly(eps, kind)
    eps.Solve()
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(eps.GetConverged())])
    r = O.eps_krylovschur_hep(Ao, 4, max_it=1500, which=O.which_target_magnitude(22.0), st=O.ST(Ao, Bo, kind, 22.0), B=Bo, conv="norm")
    print(kind, "restarts", eps.GetIterationNumber(), "oracle", r.its, "converged", eps.GetConverged(), r.nconv, st.GetKSPStats())
    assert np.allclose(np.sort(np.round(lam[:4], 5)), np.sort(gi.eigenvalues_line(gi.read("eps/eps_test1_1.out"))), atol=1.5e-5)
    assert eps.GetConverged() == r.nconv and eps.GetIterationNumber() == r.its       # (the GMRES version of this test makes the comparison for Cayley)
    assert np.allclose(lam[:4], r.eigr[r.perm][:4], rtol=1e-8)
    for i in range(4):
        assert eps.ComputeError(i) < 1e-6
    ksp = st.GetKSPStats()
    assert ksp["solves"] == ksp["iterations"] > 0
    assert st.PCLUGetInertia()[0] == int((np.linalg.eigvalsh(np.diag(Bo.val ** -0.5) @ Ao.to_scipy().toarray() @ np.diag(Bo.val ** -0.5)) < 22.0).sum())


def test_eps_test11_sinvert_golden(ctx):
    """test11 -eps_nev 4 -st_type sinvert: the shift 0.5 lies inside the spectrum of the Markov matrix."""
    import slepc_amd as ks
    Ao = O.markov_matrix(15)
    eps = ks.EPS(ctx)
    eps.SetOperators(ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4); eps.SetTolerances(1e-10, 0)
    eps.SetEigenvalueComparison(nc.right_of(0.5)); eps.SetInitialVector(np.ones(Ao.n))
    st = _lu_preonly(eps, "sinvert"); st.SetShift(0.5)
    eps.Solve()
    r = O.eps_krylovschur_nhep(Ao, 4, tol=1e-10, which=nc.right_of(0.5), st=O.ST(Ao, None, "sinvert", 0.5), v0=np.ones(Ao.n))
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(np.round(lam, 5), gi.eigenvalues_line(gi.read("eps/eps_test11_1.out")), atol=1.5e-5)
    assert eps.GetConverged() == r.nconv and eps.GetIterationNumber() == r.its
    assert np.allclose(lam, r.eigr[r.perm][:4], rtol=1e-9)


def test_eps_test29_sinvert_golden(ctx):
    import slepc_amd as ks
    Sa, Sb = _bfw_scipy()
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, Sa), _mat(ctx, Sb)); eps.SetProblemType(ks.EPS_GNHEP); eps.SetDimensions(4); eps.SetTarget(-190000.0)
    st = _lu_preonly(eps, "sinvert")
    eps.Solve()
    ref = gi.table_first_column(gi.read("eps/eps_test29_1.out"))
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam, ref, rtol=1e-10)
    assert st.GetShift() == -190000.0


def _outer_iterations(ctx, solver, pc, bs):
    import slepc_amd as ks
    S = lc.laplacian2d(12, 9)
    exact = np.linalg.eigvalsh(S.toarray())
    eps = ks.EPS(ctx)
    eps.SetOperators(_mat(ctx, S)); eps.SetProblemType(ks.EPS_HEP); eps.SetType(solver); eps.SetTolerances(1e-8, 2000)
    if solver == "gd":
        eps.SetDimensions(3); eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(1.0)
        want = np.array(sorted(exact, key=lambda v: abs(v - 1.0)))[:3]
    else:
        eps.SetDimensions(4); eps.LOBPCGSetBlockSize(4); eps.GetST().SetShift(-0.1)
        want = exact[:4]
    eps.GetST().SetPC(pc, bs)
    eps.Solve()
    assert eps.GetConverged() >= want.size
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(want.size)])
    assert np.allclose(np.sort(lam), np.sort(want), rtol=0, atol=1e-7 * exact[-1])
    return eps.GetIterationNumber()


@pytest.mark.parametrize("solver", ["gd", "lobpcg"])
def test_stprecond_with_lu_needs_no_more_outer_iterations_than_ilu(ctx, solver):
    """GD at the target 1.0 and LOBPCG with K = A + 0.1 I on the 12 x 9 Laplacian: the exact K^-1 against ILU(0) of two blocks of K."""
    its_lu = _outer_iterations(ctx, solver, "lu", 0)
    its_ilu = _outer_iterations(ctx, solver, "bjacobi-ilu", 64)
    print("%s: outer iterations with lu %d, with bjacobi-ilu %d" % (solver, its_lu, its_ilu))
    assert its_lu <= its_ilu


def test_two_sided_sinvert_with_lu_on_the_transposed_side(ctx):
    """ex41 behind sinvert (markov(15), target 1.1, two-sided Krylov-Schur): the left basis is expanded through y = Q^T L^-T U^-T Q x."""
    import slepc_amd as ks
    from test_gpu_twosided_solves import TOL, _check_pairs
    Ao = O.markov_matrix(15)
    A = ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val, keep_csr=True)
    v0, w0 = TS.ex41_start_vectors(Ao.n)
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ks.EPS_NHEP); eps.SetDimensions(4); eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(1.1)
    eps.SetTwoSided(True); eps.SetInitialSpace(v0[:, None]); eps.SetLeftInitialSpace(w0[:, None])
    st = _lu_preonly(eps, "sinvert", transpose=True)
    eps.Solve()
    assert eps.GetConverged() >= 4 and eps.GetConvergedReason() == 1
    lam = np.array([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam, gi.table_first_column(gi.read("eps/ex41_1.out"))[:4], atol=0.6e-6)
    S = Ao.to_scipy().tocsr(); I = sp.identity(Ao.n, format="csr")
    _check_pairs(eps, S, I, 4, 2.0 * np.linalg.norm((S - 1.1 * I).toarray(), 2) * TOL, "ex41 sinvert lu")
    ksp = st.GetKSPStats()
    assert ksp["solves"] == ksp["iterations"] > 0
