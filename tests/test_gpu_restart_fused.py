"""The end of a restart cycle in one launch: the deferred final Gram-Schmidt update of a Krylov run's last column, the restart product
and the copy of the residual column (k_restart_fused, BV.SetDeferFinal / BV.Restart) against the three launches they replace
(KS_DEBUG_NO_RESTART_FUSION). The update is a per-row fma chain and the product a per-row MFMA sequence, neither has a sum across rows:
every comparison here is bit for bit - basis storage, coefficient buffer, projected matrix, pass counts, eigenvalues, error estimates.
Both load forms of the kernel (k_restart_fused<true> on a resident basis, <false> on one whose leading dimension makes it stream) and a second and
third tile per wave (restart_cases.TWO_ROUNDS); which form ran is read from the library's counters (Context.basis_load_counts)."""
import numpy as np
import pytest

import nhep_cases as nc_
import restart_cases as rc
import stream_cases as sc

pytestmark = pytest.mark.gpu


def _matrix(ctx, kind, n):
    import slepc_amd as ks
    if kind == "laplacian":
        return ks.Mat.laplacian2d(ctx, *rc.laplacian_rows(n))
    return ks.Mat.from_csr(ctx, *rc.random_csr(n))


def _collect(bv, extra):
    out = dict(extra)
    out.update({"V": np.stack([bv.column(j) for j in range(-bv.nc, bv.m)], axis=1), "buffer": bv.buffer(), "passes": bv.gs_passes()})
    return out


def _raw_columns(ctx, base, ld, n, count):
    """The first `count` columns of a BV's storage read straight from the device (BV.column would apply a pending update first)."""
    out = np.empty((n, count))
    col = np.empty(n)
    for j in range(count):
        ctx.memcpy_d2h(col, base + 8 * j * ld)
        out[:, j] = col
    return out


def _run(ctx, debug, fused, A, n, k, *, window=None, nc=0, ld=0, arnoldi=False, action="restart", refine=None, v0=None, spare=0):
    """A Krylov run to last column k with the final update deferred, then `action` on the basis; everything the run and the action left behind.
    fused False: the same calls under KS_DEBUG_NO_RESTART_FUSION."""
    import slepc_amd as ks
    debug("no_restart_fusion", 0 if fused else 1)
    m = k + 1 + spare
    bv = ks.BV(ctx, n, m + nc, ld=ld)
    if nc:
        kept = bv.InsertConstraints(np.random.default_rng(17).standard_normal((n, nc)))
        assert kept == nc
    if refine is not None:
        bv.SetOrthogonalization(ks.CGS, refine, 0.7071)
    bv.set_column(0, rc.start_vector(n) if v0 is None else v0)
    base = bv.column_ptr(-nc)                          # (taken before the run: asking for a column later would apply the pending update)
    bv.SetDeferFinal(True)
    s, e = window if window else (0, min(k, 15))
    T = np.zeros((m, m), order="F") if arnoldi else np.zeros((m, 3), order="F")
    res = bv.MatArnoldi(A, T, 0, k) if arnoldi else bv.MatLanczos(A, T, 0, k)
    st0 = bv.restart_stats()
    # what the run left before the action: the constraints and the columns before the last one (the last one still waits for its update when deferred)
    Vpre = _raw_columns(ctx, base, bv.ld, n, nc + k)
    bv.SetActiveColumns(s, k)
    Q = rc.restart_q(m, s, k)
    ret = None
    if action == "restart":
        bv.Restart(Q, s, e, k, e)
    elif action == "column":
        ret = bv.column(k)
    elif action == "dotcolumn":
        ret = bv.DotColumn(k)
    elif action == "normcolumn":
        ret = np.array([bv.NormColumn(k)])
    elif action == "scalecolumn":
        bv.ScaleColumn(k, 0.75)
    elif action == "multinplace":
        bv.MultInPlace(Q, s, e)
    elif action == "copycolumn":
        bv.CopyColumn(k, e)
    elif action == "lanczos":
        bv.SetActiveColumns(0, k)
        T2 = np.zeros((m, 3), order="F")
        ret = np.array(bv.MatLanczos(A, T2, k - 1, k)[:2] + (0.0,)) if k > 1 else None
    else:
        raise AssertionError(action)
    st1 = bv.restart_stats()
    out = _collect(bv, {"Vpre": Vpre, "T": T, "res": (res[0], res[2]), "beta": np.array([res[1]])})
    if ret is not None:
        out["ret"] = np.asarray(ret, dtype=np.float64)
    out["stages"] = rc.restart_stages(Vpre, out["V"], Q, nc, s, e, k) if action == "restart" and not res[2] else ()
    bv.destroy()
    return out, st0, st1


def _both(ctx, debug, *args, **kw):
    """The deferred run and the run under no_restart_fusion. The first entry that differs names the stage: Vpre, T, res, beta are the Krylov run's
    (before the restart), V, buffer, passes what the restart left."""
    a, sa0, sa1 = _run(ctx, debug, True, *args, **kw)
    b, sb0, sb1 = _run(ctx, debug, False, *args, **kw)
    assert not sb0["pending"] and sb1["fused"] == 0 and sb1["flushes"] == 0, (sb0, sb1)        # the hook keeps today's launches
    _both.last = a                                   # (what the deferred run left, for a test that looks at more than the difference)
    # each run against its own state before the restart: a failure names the run and the stage, whatever the other run did
    assert a["stages"] == () and b["stages"] == (), ("fused", a["stages"], "unfused", b["stages"])
    diff = rc.first_difference(a, b)
    _both.detail = rc.describe_difference(a, b) if diff is not None else None       # (for the message of a failure)
    return diff, sa0, sa1


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["laplacian", "csr"])
@pytest.mark.parametrize("n", rc.SIZES)
def test_restart_row_counts(ctx, debug, kind, n):
    """Every row count: one row group, partial last 32-row group, partial last 128-row tile, several workgroups, a second and a third tile per wave;
    short and full-width bases. A basis of these sizes is resident: every launch that chooses a load form reports plain loads."""
    import slepc_amd as ks
    num_cu = ctx.device_info()["num_cu"]
    two_rounds = n == rc.TWO_ROUNDS
    n = rc.rows(n, num_cu)
    if two_rounds:
        tiles = -(-n // sc.RESTART_TILE); waves = sc.RESTART_WAVES * min(-(-tiles // sc.RESTART_WAVES), num_cu)
        assert tiles > 2 * waves and n % 32 == 2, (n, tiles, waves)
    ctx.basis_load_counts(reset=True)
    A = _matrix(ctx, kind, n)
    for k in (1, 5, 30):
        if k >= n:
            continue
        for refine in (ks.REFINE_IFNEEDED, ks.REFINE_ALWAYS):
            diff, st0, st1 = _both(ctx, debug, A, n, k, window=(0, max(1, min(k - 1, 15))), refine=refine)
            assert diff is None, (kind, n, k, refine, diff, _both.detail)
            if n >= 510 and refine == ks.REFINE_ALWAYS:
                assert st0["pending"], (kind, n, k, st0)      # two passes by policy: the update of the last column waits
            if st0["pending"]:
                assert (st1["fused"], st1["flushes"]) == ((1, 0) if k > 1 else (0, 1)), (kind, n, k, refine, st1)
    plain, streaming = ctx.basis_load_counts(reset=True)
    assert plain > 0 and streaming == 0, (plain, streaming)


@pytest.mark.parametrize("n", [514, 4098, rc.TWO_ROUNDS])
def test_restart_streaming_loads(ctx, debug, n):
    """k_restart_fused<false>: the same runs on a basis whose leading dimension puts its storage above the size at which the library streams it
    (stream_cases.streaming_ld asks the library; the rows n .. ld - 1 are never touched). The reference is the three launches under
    no_restart_fusion as before - streaming forms of k_gs_update and the panel product, which tests/test_gpu_sweep_variants.py holds to numpy.
    No launch of either run may report plain loads, and the deferred run must have taken the one-launch form."""
    import slepc_amd as ks
    num_cu = ctx.device_info()["num_cu"]
    kind = "laplacian" if n == rc.TWO_ROUNDS else "csr"
    n = rc.rows(n, num_cu)
    A = _matrix(ctx, kind, n)
    for k, nc in ((5, 0), (30, 0), (16, 1)):
        ld = sc.streaming_ld(ctx, n, nc + k + 1)
        ctx.basis_load_counts(reset=True)
        diff, st0, st1 = _both(ctx, debug, A, n, k, window=(0, max(1, min(k - 1, 15))), nc=nc, ld=ld, refine=ks.REFINE_ALWAYS)
        plain, streaming = ctx.basis_load_counts(reset=True)
        assert diff is None, (n, k, nc, diff, _both.detail)
        assert st0["pending"] and (st1["fused"], st1["flushes"]) == (1, 0), (n, k, nc, st0, st1)
        assert streaming > 0 and plain == 0, (n, k, nc, plain, streaming)


@pytest.mark.parametrize("k", rc.LAST_COLUMNS)
def test_restart_widths_and_windows(ctx, debug, k):
    """Every last column (4 and 8 k-steps, odd and even chains) with every window start and width; Lanczos and Arnoldi."""
    n = 514
    A = _matrix(ctx, "csr", n)
    import slepc_amd as ks
    ran = 0
    for window in rc.windows(k):
        for arnoldi, refine in ((False, ks.REFINE_ALWAYS), (True, ks.REFINE_ALWAYS), (False, ks.REFINE_IFNEEDED)):
            diff, st0, st1 = _both(ctx, debug, A, n, k, window=window, arnoldi=arnoldi, refine=refine)
            assert diff is None, (k, window, arnoldi, refine, diff)
            if refine == ks.REFINE_ALWAYS:
                assert st0["pending"], (k, window, st0)
            s, e = window
            if st0["pending"]:
                # the one-launch form unless the copy's target is the residual's own column
                assert (st1["fused"], st1["flushes"]) == ((1, 0) if e < k else (0, 1)), (k, window, st1)
            ran += 1
    assert ran >= 3


@pytest.mark.parametrize("nc,k,fuses", [(1, 16, True), (1, 30, True), (2, 30, True), (3, 30, False)])
def test_restart_with_constraints(ctx, debug, nc, k, fuses):
    """Constraint columns take part in the update and not in the product; nc + k = 32 is the widest basis the kernel takes, 33 falls back."""
    n = 4098
    A = _matrix(ctx, "laplacian", n)
    import slepc_amd as ks
    diff, st0, st1 = _both(ctx, debug, A, n, k, window=(2, min(17, k - 1)), nc=nc, refine=ks.REFINE_ALWAYS)
    assert diff is None, (nc, k, diff)
    assert st0["pending"] == fuses and st1["fused"] == (1 if fuses else 0) and st1["flushes"] == 0, (st0, st1)


def test_restart_odd_leading_dimension_falls_back(ctx, debug):
    """Odd n with an odd user ld: columns are not 16-byte aligned, nothing is deferred and the separate launches run."""
    n = 511
    A = _matrix(ctx, "csr", n)
    diff, st0, st1 = _both(ctx, debug, A, n, 17, window=(0, 15), ld=513)
    assert diff is None, diff
    assert not st0["pending"] and st1["fused"] == 0


@pytest.mark.parametrize("action", ["column", "dotcolumn", "normcolumn", "scalecolumn", "multinplace", "copycolumn", "lanczos"])
def test_pending_update_consumed_elsewhere(ctx, debug, action):
    """With the update waiting, anything else that touches the basis applies it first, exactly once, and sees today's data."""
    n = 4098
    A = _matrix(ctx, "laplacian", n)
    import slepc_amd as ks
    diff, st0, st1 = _both(ctx, debug, A, n, 17, window=(2, 17) if action != "copycolumn" else (2, 10), action=action, spare=1, refine=ks.REFINE_ALWAYS)
    assert diff is None, (action, diff)
    # (a second run applies the first run's update as it starts and leaves one of its own waiting)
    assert st0["pending"] and st1["pending"] == (action == "lanczos") and st1["flushes"] == 1 and st1["fused"] == 0, (action, st0, st1)


@pytest.mark.parametrize("case", ["third_pass", "breakdown", "never", "always"])
def test_columns_beyond_the_optimistic_program(ctx, debug, case):
    """A last column that needs a third pass, or breaks down with a zero residual (invariant subspace of dimension 3 of a diagonal matrix,
    with and without a 1e-20 leak into the other directions), and the refinement policies NEVER and ALWAYS: results and pass counts of
    the separate launches."""
    import slepc_amd as ks
    if case in ("third_pass", "breakdown"):
        n = 600
        d = 1.0 + np.arange(n, dtype=float) / n
        A = ks.Mat.from_csr(ctx, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)
        v = np.full(n, 1e-20 if case == "third_pass" else 0.0); v[[1, n // 2, n - 7]] = [1.0, 2.0, -1.0]; v /= np.linalg.norm(v)
        diff, st0, st1 = _both(ctx, debug, A, n, 3, window=(0, 2), v0=v)
        assert diff is None, (case, diff)
        assert not st0["pending"] and st0["flushes"] == 1 and st1["fused"] == 0, (case, st0, st1)     # applied where the run noticed, as today
        if case == "third_pass":
            assert _both.last["passes"] == (7, 3) and _both.last["res"] == (3, False), _both.last["passes"]      # 2 + 2 + 3 passes, no breakdown
        else:
            assert _both.last["res"] == (3, True), _both.last["res"]
    else:
        n = 514
        A = _matrix(ctx, "csr", n)
        refine = ks.REFINE_NEVER if case == "never" else ks.REFINE_ALWAYS
        diff, st0, st1 = _both(ctx, debug, A, n, 17, window=(0, 15), refine=refine)
        assert diff is None, (case, diff)
        assert st0["pending"] == (case == "always"), (case, st0)


# ---- solver level ---------------------------------------------------------------------------------------------------------------------------
def _solve(ctx, debug, fused, make, configure, snap):
    import slepc_amd as ks
    debug("no_restart_fusion", 0 if fused else 1)
    A = make()
    eps = ks.EPS(ctx)
    eps.SetOperators(A)
    snaps = []
    configure(eps, snaps if snap else None)
    eps.Solve()
    nconv = eps.GetConverged()
    bv = eps.GetBV()
    out = {"nconv": nconv, "its": eps.GetIterationNumber(), "stats": tuple(sorted(eps.GetStats().items())),
           "eig": np.array([eps.GetEigenvalue(i) for i in range(nconv)]).reshape(-1),
           "errest": np.array([eps.GetErrorEstimate(i) for i in range(nconv)]),
           "V": np.stack([bv.column(j) for j in range(bv.m)], axis=1), "nsnaps": len(snaps)}
    if snaps:
        out["snaps"] = np.stack(snaps, axis=1)
    return out, bv.restart_stats()


def _snapshot_stop(eps, snaps):
    def stop(its, max_it, nconv, nev):
        bv = eps.GetBV()
        snaps.append(bv.column(bv.k))          # the residual column of this restart
        return eps.StoppingBasic(its, max_it, nconv, nev)
    eps.SetStoppingTestFunction(stop)


HEP_SHAPES = [(12, 12, 12), (17, 13, 11)]
OPTIONS = ["plain", "lock_off", "harmonic", "trueres", "snapshot"]


def _configure(problem, option):
    import slepc_amd as ks

    def configure(eps, snaps):
        eps.SetProblemType(ks.EPS_HEP if problem == "hep" else ks.EPS_NHEP)
        eps.SetDimensions(4, 12)
        eps.SetTolerances(1e-9, 400)
        if option == "lock_off":
            eps.KrylovSchurSetLocking(False)
        elif option == "harmonic":
            eps.SetTarget(0.9 if problem == "nhep" else 11.0)
            eps.SetWhichEigenpairs("target_magnitude")
            eps.SetExtraction("harmonic")
        elif option == "trueres":
            eps.SetTrueResidual(True)
        elif option == "snapshot":
            _snapshot_stop(eps, snaps)
    return configure


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("shape", HEP_SHAPES)
def test_hep_solves_identical(ctx, debug, shape, option):
    import slepc_amd as ks
    make = lambda: ks.Mat.laplacian3d(ctx, *shape)
    a, sa = _solve(ctx, debug, True, make, _configure("hep", option), option == "snapshot")
    b, sb = _solve(ctx, debug, False, make, _configure("hep", option), option == "snapshot")
    assert rc.first_difference(a, b) is None, (shape, option, rc.first_difference(a, b))
    assert sb["fused"] == 0 and sb["flushes"] == 0 and not sa["pending"], (sa, sb)
    if option in ("plain", "lock_off"):
        assert sa["fused"] > 0, sa                # restarts of the plain loop take the one-launch form
    if option in ("harmonic", "snapshot"):
        assert sa["fused"] == 0 and sa["flushes"] > 0, sa      # these look at the residual column before the restart: applied on its own
    assert a["its"] > 2, a["its"]
    if option == "plain":
        assert a["nconv"] >= 4, a["nconv"]
    if option == "snapshot":
        assert a["nsnaps"] == a["its"]


@pytest.mark.parametrize("option", OPTIONS)
def test_nhep_solves_identical(ctx, debug, option):
    import slepc_amd as ks
    Ao = nc_.random_nonsymmetric(400)
    make = lambda: ks.Mat.from_csr(ctx, Ao.rowptr, Ao.col, Ao.val)
    a, sa = _solve(ctx, debug, True, make, _configure("nhep", option), option == "snapshot")
    b, sb = _solve(ctx, debug, False, make, _configure("nhep", option), option == "snapshot")
    assert rc.first_difference(a, b) is None, (option, rc.first_difference(a, b))
    assert sb["fused"] == 0 and sb["flushes"] == 0 and not sa["pending"], (sa, sb)
    assert a["its"] > 2, a["its"]
