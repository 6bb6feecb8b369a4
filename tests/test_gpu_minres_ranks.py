"""KS_KSP_MINRES on row-sharded matrices: ranks are threads of one process (tests/thread_comm.py), at most four at a time, each with a context of its
own that it closes. On more than one rank a sweep's partials go through a one-workgroup finish kernel and the allreduce on the device buffer, in
stream order, two collectives per iteration; a rank without rows writes zero partials and takes part in every collective. The systems are
ikron(9, 57) (n = 513, I (x) T, indefinite) and lap(33, 31) under sinvert at 1.5 (n = 1023, four negative eigenvalues) of tests/minres_cases.py with
Jacobi-abs, on the row splits

    two ranks           one tile exactly and the rest
    four ranks          rank 0 empty; 5 and 63 rows (less than a tile)
    four ranks          an empty rank in the middle, a last rank of one row

and once with the force_multi hook on one rank, which takes the same path without threads. The counts are the pinned ones of
tests/test_minres_cases_host.py; the solutions agree with the one-rank restatement within the true-residual bound of tests/test_gpu_minres.py."""
import math

import numpy as np
import pytest

import minres_cases as mc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
SPLITS = {"kron": [[512, 1], [0, 5, 63, 445], [65, 0, 447, 1]], "lap": [[512, 511], [0, 5, 63, 955], [65, 0, 957, 1]]}


def _system(which, pc="jacobi-abs"):
    if which == "kron":
        case, ref = mc.kron_reference(9, 57, pc)
        return case, case.P, 0.0, 1e-8, ref
    case, P, rtol, ref, _, _ = mc.lap_reference(0, pc)
    return case, P, mc.LAP[0][1], rtol, ref


def _solve(ks, ctx, case, r0, r1, sigma, pc, rtol):
    from slepc_amd import partition as P
    import ctypes as C
    A = ks.Mat.from_csr(ctx, *P.local_block(case.rowptr, case.col, case.val, r0, r1), row_start=r0, n_global=case.n)
    st = ks.ST(ctx)
    W = ks.BV(ctx, r1 - r0, 2, N=case.n, row_start=r0)
    try:
        st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetKSPType("minres"); st.SetKSP(rtol=rtol)
        if pc == "jacobi-abs":
            st.SetPC("jacobi"); st.PCJacobiSetUseAbs(True)
        else:
            st.SetPC(pc)
        W.set_column(0, case.b[r0:r1])
        ks._lib.check(ctx.L.ks_st_apply(st.h, C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1))))
        return {"y": W.column(1), "ksp": st.GetKSPStats(), "mr": st.GetMINRESStats()}
    finally:
        W.destroy(); st.destroy(); A.destroy()


def _check(out, case, P, ref, pc):
    minv = mc.minv_of(P, pc)
    y = np.concatenate([o["y"] for o in out])
    res = mc.mnorm(minv, case.b - P @ y)
    diff = mc.mnorm(minv, P @ (y - ref.y))
    print("its %s (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, P (y - y_ref) %.3e, gap %.2e, %s" % ([o["ksp"]["iterations"] for o in out], ref.its, out[0]["ksp"]["last_rnorm"], ref.tol, res, diff, ref.gap, out[0]["mr"]))
    for o in out:
        assert o["ksp"] == out[0]["ksp"]                                     # count and residual norm: the same bits on every rank
        assert o["ksp"]["iterations"] == ref.its and o["ksp"]["solves"] == 1 and o["ksp"]["last_rnorm"] <= ref.tol
        assert o["mr"]["host_waits"] == math.ceil(ref.its / 8) and o["mr"]["gated_iterations"] == 8 * math.ceil(ref.its / 8) - ref.its
    assert res <= ref.tol + 8 * ref.gap
    assert diff <= ref.tol + 8 * ref.gap


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which,split", [(w, i) for w in ("kron", "lap") for i in range(3)], ids=["%s-%s" % (w, "-".join(map(str, SPLITS[w][i]))) for w in ("kron", "lap") for i in range(3)])
def test_sharded_counts_and_solutions(which, split):
    case, P, sigma, rtol, ref = _system(which)
    counts = SPLITS[which][split]
    starts = np.concatenate([[0], np.cumsum(counts)])
    assert starts[-1] == case.n

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            return _solve(ks, ctx, case, int(starts[rank]), int(starts[rank + 1]), sigma, "jacobi-abs", rtol)
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(len(counts), pairwise=True, timeout=60), fn, join_timeout=120)      # pairwise: a rank without rows has no neighbour to exchange with
    _check(out, case, P, ref, "jacobi-abs")


def test_collective_path_on_one_rank():
    """force_multi: the finish kernels and the allreduces on a communicator of one rank, without threads, with and without a preconditioner (the
    communicator is the caller-supplied one of tests/thread_comm.py at size 1, as in tests/test_gpu_cg_ranks.py)."""
    import slepc_amd as ks
    ctx = ks.Context(0)
    out = {}
    try:
        ctx.set_debug("force_multi")
        ThreadComm(1, timeout=60).install(ctx, 0)
        for which, pc in (("kron", "jacobi-abs"), ("kron", "none"), ("lap", "jacobi-abs")):
            case, P, sigma, rtol, ref = _system(which, pc)
            out[which, pc] = [_solve(ks, ctx, case, 0, case.n, sigma, pc, rtol)]
    finally:
        ctx.close()
    for (which, pc), o in out.items():
        case, P, sigma, rtol, ref = _system(which, pc)
        _check(o, case, P, ref, pc)
