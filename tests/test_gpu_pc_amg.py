"""Smoothed-aggregation multigrid on the ST's KSP (KS_PC_AMG; k_amg_cheby and k_amg_transfer in slepc_amd/csrc/ks_pc_amg.hip, the hierarchy of
ksc::amg_plan in ks_csr.cpp).

The transfer kernels are checked alone through a test hook with small integers, where every summation order gives the same double: bit equality with
numpy. The cycle is checked against its restatement (tests/amg_cases.py), rebuilt in the test from the hierarchy the library exports and evaluated once
in float64 and once in longdouble:  ||y_dev - y_ld|| <= 8 ||y_64 - y_ld||  - another summation order changes rounding errors by small factors, a wrong
coefficient or a missing term shows at 1e-3 and above. Whole solves compare iteration counts with the restatement's and with point Jacobi.
Unless a test says otherwise: sinvert at sigma = 0 with one matrix, shell mode, coarse limit 8 (four levels)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as ac
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
SUP, ORDER, OUTOFRANGE, WRONGSTATE = 56, 58, 63, 73
LD = np.longdouble


def _mat(ctx, S, keep=True):
    import slepc_amd as ks
    rp, col, val = S if isinstance(S, tuple) else ac.arrays(S)
    return ks.Mat.from_csr(ctx, rp, col, val, keep_csr=keep)


def _st(ctx, A, sigma=0.0, B=None, kind="sinvert", mode="shell", coarse=8, levels=10, degree=2, smooth=True, theta=0.0, ksp=None, pc="amg"):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(sigma); st.SetMatrices(A, B); st.SetMatMode(mode); st.SetPC(pc)
    if pc == "amg":
        st.PCAMGSetCoarse(coarse, levels); st.PCAMGSetSmoother(degree); st.PCAMGSetProlongatorSmoothing(smooth); st.PCAMGSetThreshold(theta)
    if ksp:
        st.SetKSPType(ksp)
    return st


def _exported(st):
    """The library's hierarchy as the level dicts of amg_cases.cycle."""
    info = st.PCAMGGetInfo()
    out = []
    for l in range(info["levels"]):
        A, P, agg = st.PCAMGGetLevel(l)
        assert A.shape[0] == info["rows"][l] and A.nnz == info["nnz"][l]
        lev = {"A": A, "n": A.shape[0], "rho": info["rho"][l]}
        if l + 1 < info["levels"]:
            assert P.shape == (A.shape[0], info["rows"][l + 1])
            lev.update(P=P, d=A.diagonal(), agg=agg)
        out.append(lev)
    return out, info


def _ratio(levels, degree, x, y):
    y64 = ac.cycle(levels, x, degree, np.float64); yld = ac.cycle(levels, x, degree, LD)
    own = float(np.linalg.norm((y64.astype(LD) - yld).astype(np.float64)))
    dev = float(np.linalg.norm((np.asarray(y, dtype=LD) - yld).astype(np.float64)))
    assert own > 0.0
    return dev / own, own / float(np.linalg.norm(yld.astype(np.float64)))


def _x(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


# ---- 1: the transfer kernels alone ---------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1000]


def _transfer_matrix(lengths, ncols, seed):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    col = np.concatenate([rng.integers(0, ncols, k) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)      # a column may repeat in a row
    val = rng.integers(-3, 4, col.size).astype(np.float64)
    return rp, col, val


def _run_transfer(ctx, restriction, lanes, rp, col, val, ncols, nvec, seed):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rng = np.random.default_rng(seed)
    nrows = rp.size - 1
    D = np.zeros((nrows, ncols))
    np.add.at(D, (np.repeat(np.arange(nrows), np.diff(rp)), col), val)                       # exact: small integers
    u = np.asfortranarray(rng.integers(-4, 5, (ncols, nvec)).astype(np.float64))
    v = np.asfortranarray(rng.integers(-4, 5, (ncols if restriction else nrows, nvec)).astype(np.float64))
    out = np.asfortranarray(np.full((nrows, nvec), np.nan))
    colp = col if col.size else np.zeros(1, np.int32); valp = val if val.size else np.zeros(1)
    rc = ctx.L.ks_pc_amg_test_transfer(ctx.h, 1 if restriction else 0, lanes, nrows, ncols, rp.ctypes.data_as(ip), colp.ctypes.data_as(ip), valp.ctypes.data_as(dp),
                                       nvec, u.ctypes.data_as(dp), v.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert rc == 0
    want = D @ (u - v) if restriction else v + D @ u
    assert np.array_equal(out, want), (restriction, lanes, nrows, ncols, nvec)


@pytest.mark.parametrize("lanes", [1, 8, 64, 0])
@pytest.mark.parametrize("restriction", [True, False])
def test_transfer_kernels_row_lengths_and_columns(ctx, lanes, restriction):
    ncols = 1100
    rp, col, val = _transfer_matrix(ROW_LENGTHS, ncols, 100 + lanes)
    for nvec in (1, 7, 8, 9):
        _run_transfer(ctx, restriction, lanes, rp, col, val, ncols, nvec, 7 * nvec + lanes)


@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_transfer_kernels_shapes(ctx, lanes):
    """One row; one column; a last row that ends on a wave boundary, on a workgroup boundary, and one past each."""
    for restriction in (True, False):
        _run_transfer(ctx, restriction, lanes, *_transfer_matrix([37], 50, 1), 50, 3, 2)
        _run_transfer(ctx, restriction, lanes, *_transfer_matrix([0], 5, 1), 5, 1, 3)
        _run_transfer(ctx, restriction, lanes, *_transfer_matrix([0, 1, 5, 70, 1, 1, 0, 3], 1, 4), 1, 9, 5)
        for nrows in (64 // lanes, 64 // lanes + 1, 256 // lanes, 256 // lanes + 1, 3 * 256 // lanes):
            lengths = [ROW_LENGTHS[i % 10] for i in range(nrows)]
            _run_transfer(ctx, restriction, lanes, *_transfer_matrix(lengths, 200, nrows), 200, 2, nrows)


def test_transfer_hook_checks_its_arrays(ctx):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rp = np.array([0, 2], np.int32); col = np.array([0, 5], np.int32); val = np.ones(2); u = np.ones(4); out = np.zeros(1)
    rc = ctx.L.ks_pc_amg_test_transfer(ctx.h, 1, 8, 1, 4, rp.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp), 1, u.ctypes.data_as(dp), u.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert rc == OUTOFRANGE                                            # column 5 of 4: refused on the host, nothing launched
    rc = ctx.L.ks_pc_amg_test_transfer(ctx.h, 1, 16, 1, 6, rp.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp), 1, u.ctypes.data_as(dp), u.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert rc == OUTOFRANGE                                            # 16 lanes per row is not built


# ---- 2: the cycle against its restatement ------------------------------------------------------------------------------------------------
def _matrices():
    return {"grid 45x31": ac.grid2d(45, 31), "12^3": ac.laplacian3d(12), "upwind": ac.upwind(), "two grids and five identity rows": ac.blocks_with_isolated_rows()}


SYMMETRIC = ["grid 45x31", "12^3", "two grids and five identity rows"]


@pytest.fixture(scope="module")
def mats(ctx):
    """The device matrices, shared and left unchanged."""
    return {name: (S, _mat(ctx, S)) for name, S in _matrices().items()}


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name", list(_matrices()))
def test_cycle_against_the_restatement(ctx, mats, name, degree, smooth):
    S, A = mats[name]
    n = S.shape[0]
    st = _st(ctx, A, degree=degree, smooth=smooth)
    x = _x(n, 11)
    y = st.PCApply(x)
    levels, info = _exported(st)
    assert info["levels"] == 4 and np.all(np.isfinite(y)), (name, info)
    assert np.array_equal(levels[0]["A"].toarray(), S.toarray())
    # the library's hierarchy is the restatement's (the host tests compare them entry by entry; here: same levels and aggregates)
    ref = ac.hierarchy(S, coarse_limit=8, smooth=smooth)
    assert [l["n"] for l in ref] == info["rows"] and all(np.array_equal(levels[l]["agg"], ref[l]["agg"]) for l in range(3))
    ratio, own = _ratio(levels, degree, x, y)
    print("%s, degree %d, smoothing %s: ||y_dev - y_ld|| / ||y_64 - y_ld|| = %.3f (float64's own relative error %.2e)" % (name, degree, smooth, ratio, own))
    assert ratio <= 8.0, (name, degree, smooth, ratio)
    assert np.array_equal(st.PCApply(x), y)                                                  # the same bits on a second run
    assert info["launches"] >= 3 * (4 * degree + 2) + 1 and info["complexity"] > 1.0 and info["device_bytes"] > 12 * sum(info["nnz"][:-1])


@pytest.mark.parametrize("name", list(_matrices()))
def test_several_columns_are_the_single_column_bits(ctx, mats, name):
    S, A = mats[name]
    st = _st(ctx, A)
    assert st.PCMultiColumns() == 8
    X = np.random.default_rng(12).standard_normal((S.shape[0], 9))
    single = np.stack([st.PCApply(X[:, j]) for j in range(9)], axis=1)
    for k in (1, 7, 8, 9):
        assert np.array_equal(st.PCApplyMulti(X[:, :k]), single[:, :k]), (name, k)


def test_modes_and_transformations(ctx, mats):
    """Shell and copy mode build the hierarchy from the same arrays: identical bits. Cayley has the P of sinvert; a shift with two matrices has P = B."""
    S, A = mats["grid 45x31"]
    n = S.shape[0]
    x = _x(n, 13)
    sigma = -0.3
    y = _st(ctx, A, sigma=sigma).PCApply(x)
    assert np.array_equal(_st(ctx, A, sigma=sigma, mode="copy").PCApply(x), y)
    sc = _st(ctx, A, sigma=sigma, kind="cayley"); sc.CayleySetAntishift(1.5)
    assert np.array_equal(sc.PCApply(x), y)
    Sb = (S + sp.diags([1.0 + 0.1 * np.cos(np.arange(n))], [0])).tocsr(); Sb.sort_indices()
    s2 = _st(ctx, A, sigma=0.3, B=_mat(ctx, Sb), kind="shift")
    y2 = s2.PCApply(x)
    levels, info = _exported(s2)
    assert np.array_equal(levels[0]["A"].toarray(), Sb.toarray()) and info["levels"] == 4
    ratio, _ = _ratio(levels, 2, x, y2)
    print("P = B: ratio %.3f" % ratio)
    assert ratio <= 8.0


@pytest.mark.parametrize("name", SYMMETRIC)
def test_cycle_is_symmetric(ctx, mats, name):
    S, A = mats[name]
    st = _st(ctx, A)
    rng = np.random.default_rng(14)
    u, v = rng.standard_normal(S.shape[0]), rng.standard_normal(S.shape[0])
    a, b = float(u @ st.PCApply(v)), float(v @ st.PCApply(u))
    print("%s: |u.Mv - v.Mu| / |u.Mv| = %.2e" % (name, abs(a - b) / abs(a)))
    assert abs(a - b) <= 1e-10 * abs(a)


# ---- 3: degenerate hierarchies ---------------------------------------------------------------------------------------------------------------
def test_degenerate_hierarchies(ctx):
    x1 = np.array([0.7])
    st = _st(ctx, _mat(ctx, sp.csr_matrix(np.array([[-3.0]]))))
    assert np.array_equal(st.PCApply(x1), x1 * (1.0 / -3.0)) and st.PCAMGGetInfo()["levels"] == 1
    D = sp.diags([2.0 + np.cos(np.arange(777))], [0]).tocsr()
    sd = _st(ctx, _mat(ctx, D))
    x = _x(777, 15)
    assert np.array_equal(sd.PCApply(x), x * (1.0 / D.diagonal())) and sd.PCAMGGetInfo()["levels"] == 1            # no aggregate: one level, the exact solve
    A_, P_, agg = sd.PCAMGGetLevel(0)
    assert np.all(agg == -1) and P_.shape == (777, 0)
    # n <= coarse_limit, and max_levels = 1: the factors of KS_PC_LU, bit for bit
    S = ac.grid2d(12, 9)
    A = _mat(ctx, S)
    xs = _x(108, 16)
    ylu = _st(ctx, A, pc="lu").PCApply(xs)
    assert np.array_equal(_st(ctx, A, coarse=200).PCApply(xs), ylu)
    assert np.array_equal(_st(ctx, A, coarse=8, levels=1).PCApply(xs), ylu)
    two = _st(ctx, A, coarse=8, levels=2)
    assert two.PCAMGGetInfo()["levels"] == 2 and not np.array_equal(two.PCApply(xs), ylu)
    X = np.random.default_rng(17).standard_normal((108, 9))
    one = _st(ctx, A, coarse=200)
    assert np.array_equal(one.PCApplyMulti(X), np.stack([one.PCApply(X[:, j]) for j in range(9)], axis=1))


# ---- 4: errors and options ------------------------------------------------------------------------------------------------------------------
def test_errors_and_options(ctx):
    import slepc_amd as ks
    S = ac.grid2d(17, 9)
    A = _mat(ctx, S)
    st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A)
    for bs in (1, 64):
        with pytest.raises(ks.KsError) as e:
            st.SetPC("amg", bs)
        assert e.value.rc == SUP
    with pytest.raises(ks.KsError) as e:
        st.PCAMGGetInfo()                                           # the PC is still point Jacobi
    assert e.value.rc == ORDER
    assert (st.PCAMGGetThreshold(), st.PCAMGGetSmoother(), st.PCAMGGetCoarse(), st.PCAMGGetProlongatorSmoothing()) == (0.0, 2, (200, 10), True)
    for call, bad in ((st.PCAMGSetThreshold, (-0.1,)), (st.PCAMGSetThreshold, (1.0,)), (st.PCAMGSetSmoother, (0,)), (st.PCAMGSetSmoother, (5,)),
                      (st.PCAMGSetCoarse, (0, 10)), (st.PCAMGSetCoarse, (8, 0)), (st.PCAMGSetCoarse, (8, 17))):
        with pytest.raises(ks.KsError) as e:
            call(*bad)
        assert e.value.rc == OUTOFRANGE, (call, bad)
    st.SetPC("gamg"); st.PCAMGSetThreshold(0.5); st.PCAMGSetSmoother(4); st.PCAMGSetCoarse(1, 16); st.PCAMGSetProlongatorSmoothing(False)
    assert (st.PCAMGGetThreshold(), st.PCAMGGetSmoother(), st.PCAMGGetCoarse(), st.PCAMGGetProlongatorSmoothing()) == (0.5, 4, (1, 16), False)
    # every setter clears the set-up: another hierarchy for the same solve
    s4 = _st(ctx, A)
    x = _x(153, 18)
    y = s4.PCApply(x)
    assert s4.PCAMGGetInfo()["rows"] == [l["n"] for l in ac.hierarchy(S, coarse_limit=8)]
    s4.PCAMGSetCoarse(8, 2)
    assert s4.PCAMGGetInfo()["levels"] == 2 and not np.array_equal(s4.PCApply(x), y)
    s4.PCAMGSetCoarse(8, 10); s4.PCAMGSetSmoother(3)
    assert not np.array_equal(s4.PCApply(x), y)
    s4.PCAMGSetSmoother(2); s4.PCAMGSetProlongatorSmoothing(False)
    assert not np.array_equal(s4.PCApply(x), y)
    s4.PCAMGSetProlongatorSmoothing(True); s4.PCAMGSetThreshold(0.2)
    s4.PCApply(x)
    s4.PCAMGSetThreshold(0.0)
    assert np.array_equal(s4.PCApply(x), y)
    # matrices that did not keep their CSR arrays
    s2 = _st(ctx, _mat(ctx, S, keep=False))
    with pytest.raises(ks.KsError) as e:
        s2.SetUp()
    assert e.value.rc == ORDER
    # no transposed cycle
    s5 = _st(ctx, A)
    with pytest.raises(ks.KsError) as e:
        s5.PCApplyTranspose(x)
    assert e.value.rc == SUP
    s5.SetTransposeSolves(True)
    with pytest.raises(ks.KsError) as e:
        s5.SetUp()
    assert e.value.rc == SUP and "transposed" in str(e.value)
    with pytest.raises(ks.KsError) as e:
        s5.PCApplyTranspose(x)
    assert e.value.rc == SUP
    s5.SetTransposeSolves(False)
    assert np.array_equal(s5.PCApply(x), y)                         # and usable again
    # a zero diagonal entry names its row; nothing is left half-built
    Z = S.tolil(); Z[40, 40] = 0.0; Z = Z.tocsr()
    s6 = _st(ctx, A, sigma=0.1, B=_mat(ctx, Z), kind="shift")
    for _ in range(2):
        with pytest.raises(ks.KsError) as e:
            s6.PCApply(x)
        assert e.value.rc == WRONGSTATE and "row 40" in str(e.value)
    s6.SetPC("jacobi")
    assert np.all(np.isfinite(s6.PCApply(x)))


def test_two_ranks_are_refused():
    """The aggregation of a row-sharded matrix is not built: KS_PC_AMG on a two-rank communicator fails at set-up with KS_ERR_SUP on every rank."""
    N = 40
    S = sp.diags([np.full(N - 1, -1.0), np.full(N, 2.5), np.full(N - 1, -0.8)], [-1, 0, 1]).tocsr()
    split = [(0, 24), (24, N)]

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            r0, r1 = split[rank]
            L = S[r0:r1].tocsr()
            A = ks.Mat.from_csr(ctx, L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data, row_start=r0, n_global=N, keep_csr=True)
            st = ks.ST(ctx); st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A); st.SetPC("amg")
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
    for name in ("ks_st_pc_amg_set_threshold", "ks_st_pc_amg_get_threshold", "ks_st_pc_amg_set_smoother", "ks_st_pc_amg_get_smoother", "ks_st_pc_amg_set_coarse",
                 "ks_st_pc_amg_get_coarse", "ks_st_pc_amg_set_prolongator_smoothing", "ks_st_pc_amg_get_prolongator_smoothing", "ks_st_pc_amg_get_info",
                 "ks_st_pc_amg_get_level", "ks_pc_amg_test_transfer"):
        assert hasattr(L, name) and name in _lib.header_symbols() and name in _lib._SIG
    assert "#define KS_PC_AMG 5" in open(_lib.HEADER_PATH).read()


# ---- 5: whole solves -------------------------------------------------------------------------------------------------------------------------
def _inner_iterations(st, b):
    before = st.GetKSPStats()
    y = st.Apply(b)
    after = st.GetKSPStats()
    assert after["solves"] == before["solves"] + 1
    return after["iterations"] - before["iterations"], y


@pytest.mark.parametrize("name", ["grid 45x31", "12^3"])
def test_sinvert_with_gmres_and_amg(ctx, mats, name):
    """Shift-and-invert at sigma = 0: the analytic eigenvalues, and inner iterations at most the restatement's GMRES count + 2 (point Jacobi: 202 and 59)."""
    import slepc_amd as ks
    S, A = mats[name]
    n = S.shape[0]
    exact = ac.laplacian2d_eigenvalues(45, 31) if name == "grid 45x31" else ac.laplacian3d_eigenvalues(12)
    ref = ac.hierarchy(S, coarse_limit=8)
    b = _x(n, 19)
    its_ref = ac.gmres_iterations(S, lambda r: ac.cycle(ref, r), b)
    st = _st(ctx, A)
    its, y = _inner_iterations(st, b)
    print("%s: GMRES iterations %d with the library's cycle, %d with the restatement's" % (name, its, its_ref))
    assert its <= its_ref + 2
    assert np.linalg.norm(S @ y - b) <= 1e-6 * np.linalg.norm(b)
    tol = 1e-8
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetDimensions(4); eps.SetTolerances(tol, 200)
    eps.SetWhichEigenpairs("target_magnitude"); eps.SetTarget(0.0)
    es = eps.GetST(); es.SetType("sinvert"); es.SetPC("amg"); es.PCAMGSetCoarse(8, 10)
    eps.Solve()
    assert eps.GetConverged() >= 4
    lam = np.sort([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam, exact[:4], rtol=0, atol=10 * tol * exact[3]), (lam, exact[:4])
    ksp = es.GetKSPStats()
    print("%s: %d solves, %d inner iterations" % (name, ksp["solves"], ksp["iterations"]))
    assert ksp["solves"] > 0 and ksp["iterations"] <= (its_ref + 2) * ksp["solves"]


def test_upwind_gmres_needs_fewer_iterations_than_jacobi(ctx, mats):
    S, A = mats["upwind"]
    b = _x(S.shape[0], 20)
    amg, y = _inner_iterations(_st(ctx, A), b)
    jac, _ = _inner_iterations(_st(ctx, A, pc="jacobi"), b)
    bcgs, yb = _inner_iterations(_st(ctx, A, ksp="bcgs"), b)
    print("upwind 40x40: GMRES iterations %d with AMG, %d with point Jacobi; BiCGStab with AMG %d" % (amg, jac, bcgs))
    assert amg < jac and amg <= 14 and bcgs <= 14
    assert np.linalg.norm(S @ y - b) <= 1e-6 * np.linalg.norm(b) and np.linalg.norm(S @ yb - b) <= 1e-5 * np.linalg.norm(b)


def test_anisotropic_threshold_needs_fewer_iterations(ctx):
    S = ac.anisotropic(40, 0.01)
    A = _mat(ctx, S)
    b = _x(1600, 21)
    strong, _ = _inner_iterations(_st(ctx, A, coarse=200, theta=0.25), b)
    weak, _ = _inner_iterations(_st(ctx, A, coarse=200, theta=0.0), b)
    print("anisotropic 40x40: GMRES iterations %d with theta 0.25, %d with theta 0" % (strong, weak))
    assert strong < weak


def _outer(ctx, A, solver, pc, exact):
    import slepc_amd as ks
    eps = ks.EPS(ctx)
    eps.SetOperators(A); eps.SetProblemType(ks.EPS_HEP); eps.SetType(solver); eps.SetTolerances(1e-8, 3000); eps.SetDimensions(4)
    eps.SetWhichEigenpairs("smallest_real")
    if solver == "lobpcg":
        eps.LOBPCGSetBlockSize(4)
    st = eps.GetST(); st.SetShift(0.0); st.SetPC(pc)
    if pc == "amg":
        st.PCAMGSetCoarse(8, 10)
    eps.Solve()
    assert eps.GetConverged() >= 4, (solver, pc, eps.GetConverged())
    lam = np.sort([eps.GetEigenvalue(i)[0] for i in range(4)])
    assert np.allclose(lam, exact[:4], rtol=0, atol=1e-7 * exact[-1]), (solver, pc, lam)
    return eps.GetIterationNumber()


@pytest.mark.parametrize("solver", ["lobpcg", "gd"])
def test_preconditioned_eigensolvers_with_amg(ctx, mats, solver):
    """12^3, nev 4, smallest, STPRECOND with K = A: the eigenvalues point Jacobi gives, in fewer outer iterations."""
    S, A = mats["12^3"]
    exact = ac.laplacian3d_eigenvalues(12)
    amg = _outer(ctx, A, solver, "amg", exact)
    jac = _outer(ctx, A, solver, "jacobi", exact)
    print("%s: outer iterations %d with amg, %d with point Jacobi" % (solver, amg, jac))
    assert amg < jac


def test_jacobi_davidson_with_amg_as_k(ctx, mats):
    """JD once with the cycle as K, on the 45 x 31 grid: its eigenvalues are simple (a single-vector JD finds one copy of a multiple eigenvalue at a time,
    whatever the preconditioner, so the cube's triple second eigenvalue is no case for it)."""
    S, A = mats["grid 45x31"]
    its = _outer(ctx, A, "jd", "amg", ac.laplacian2d_eigenvalues(45, 31))
    print("jd: outer iterations %d with amg" % its)
