"""KS_KSP_CG on row-sharded matrices: ranks are threads of one process (tests/thread_comm.py), at most four at a time, each with a context of its
own that it closes. On more than one rank the sweeps' partials go through a one-workgroup finish kernel and ks_comm_allreduce_sum on the device
buffer, in stream order; a rank without rows writes zero partials and takes part in every collective. The system is lap(33, 31) of tests/cg_cases.py
(n = 1023) under sinvert at sigma = 0, the tolerance derived from the reference history as in tests/test_gpu_cg.py, on the row splits

    [512, 511]          one tile exactly, and a tile less one row
    [0, 5, 63, 955]     rank 0 empty; 5 and 63 rows (less than a tile)
    [65, 0, 957, 1]     an empty rank in the middle, a last rank of one row

and once with the force_multi hook on one rank, which takes the same path without threads."""
import math

import numpy as np
import pytest

import cg_cases as cc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
SPLITS = [[512, 511], [0, 5, 63, 955], [65, 0, 957, 1]]


def _solve(ks, ctx, case, r0, r1, pc, rtol):
    from slepc_amd import partition as P
    import ctypes as C
    A = ks.Mat.from_csr(ctx, *P.local_block(case.rowptr, case.col, case.val, r0, r1), row_start=r0, n_global=case.n)
    st = ks.ST(ctx)
    W = ks.BV(ctx, r1 - r0, 2, N=case.n, row_start=r0)
    try:
        st.SetType("sinvert"); st.SetShift(0.0); st.SetMatrices(A); st.SetKSPType("cg"); st.SetPC(pc); st.SetKSP(rtol=rtol)
        W.set_column(0, case.b[r0:r1])
        ks._lib.check(ctx.L.ks_st_apply(st.h, C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1))))
        return {"y": W.column(1), "ksp": st.GetKSPStats(), "cg": st.GetCGStats()}
    finally:
        W.destroy(); st.destroy(); A.destroy()


def _check(out, case, P, ref, pc):
    minv = cc.jacobi(P) if pc == "jacobi" else (lambda r: r)
    y = np.concatenate([o["y"] for o in out])
    res = float(np.linalg.norm(minv(case.b - P @ y)))
    print("its %s (reference %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e, %s" % ([o["ksp"]["iterations"] for o in out], ref.its, out[0]["ksp"]["last_rnorm"], ref.tol, res, ref.gap, out[0]["cg"]))
    for o in out:
        assert o["ksp"] == out[0]["ksp"]                                     # count and residual norm: the same bits on every rank
        assert o["ksp"]["iterations"] == ref.its and o["ksp"]["solves"] == 1 and o["ksp"]["last_rnorm"] <= ref.tol
        assert o["cg"]["host_waits"] <= math.ceil(ref.its / 8) + 2
    assert res <= ref.tol + 8 * ref.gap


@pytest.mark.timeout(300)
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("counts", SPLITS, ids=["-".join(map(str, s)) for s in SPLITS])
def test_sharded_counts_and_solutions(counts, pc):
    case, P, rtol, ref, _ = cc.lap_reference(0, pc, 0.0, 1e-8)
    starts = np.concatenate([[0], np.cumsum(counts)])
    assert starts[-1] == case.n

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            return _solve(ks, ctx, case, int(starts[rank]), int(starts[rank + 1]), pc, rtol)
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(len(counts), pairwise=True, timeout=60), fn, join_timeout=120)      # pairwise: a rank without rows has no neighbour to exchange with
    _check(out, case, P, ref, pc)


def test_collective_path_on_one_rank():
    """force_multi: the finish kernels and the allreduces on a communicator of one rank, without threads. The communicator is the caller-supplied one of
    tests/thread_comm.py at size 1, not the native RCCL provider: that one would map the system's librccl into the test process ahead of the torch that
    later test modules import with a librccl of its own (tests/test_gpu_multirank.py keeps RCCL in a child process for the same reason)."""
    import slepc_amd as ks
    ctx = ks.Context(0)
    out = {}
    try:
        ctx.set_debug("force_multi")
        ThreadComm(1, timeout=60).install(ctx, 0)
        for pc in ("jacobi", "none"):
            case, P, rtol, ref, _ = cc.lap_reference(0, pc, 0.0, 1e-8)
            out[pc] = [_solve(ks, ctx, case, 0, case.n, pc, rtol)]
    finally:
        ctx.close()
    for pc in ("jacobi", "none"):
        case, P, rtol, ref, _ = cc.lap_reference(0, pc, 0.0, 1e-8)
        _check(out[pc], case, P, ref, pc)
