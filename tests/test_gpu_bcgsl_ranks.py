"""KS_KSP_BCGSL on row-sharded matrices: ranks are threads of one process (tests/thread_comm.py), at most four at a time, each with a context of its
own that it closes. On more than one rank every sweep's sums (one, two, or the Gram matrix's (l + 1)(l + 2) / 2) go through a one-workgroup finish
kernel and ks_comm_allreduce_sum on the device buffer, in stream order; a rank without rows writes zero partials and takes part in every
collective. Two systems of tests/bcgsl_cases.py under sinvert with point Jacobi: the I (x) T system of n = 1208 at rtol 1e-12 with its pinned
counts (l = 2 and l = 3), and the 45 x 31 convection-diffusion system at c = 8 with the bounds of tests/test_gpu_bcgsl.py (l = 2, the count not
pinned), on three ragged row splits each, and once with the force_multi hook on one rank, which takes the same path without threads."""
import math

import numpy as np
import pytest

import bcgsl_cases as bc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
SPLITS = {"kron": [[512, 696], [0, 5, 63, 1140], [65, 0, 1142, 1]], "convdiff": [[512, 883], [0, 5, 63, 1327], [65, 0, 1329, 1]]}
CASES = [("kron", 2), ("kron", 3), ("convdiff", 2)]


def _system(which, ell):
    if which == "kron":
        case, pc, ref = bc.kron_reference(0, ell)
        return case, case.P, 0.0, 1e-12, ref
    case, P, sigma, ref = bc.convdiff_reference(1, ell)
    return case, P, sigma, 1e-8, ref


def _solve(ks, ctx, case, r0, r1, sigma, ell, rtol, max_it):
    from slepc_amd import partition as P
    import ctypes as C
    A = ks.Mat.from_csr(ctx, *P.local_block(case.rowptr, case.col, case.val, r0, r1), row_start=r0, n_global=case.n)
    st = ks.ST(ctx)
    W = ks.BV(ctx, r1 - r0, 2, N=case.n, row_start=r0)
    try:
        st.SetType("sinvert"); st.SetShift(sigma); st.SetMatrices(A); st.SetKSPType("bcgsl"); st.BCGSLSetEll(ell); st.SetPC("jacobi"); st.SetKSP(rtol=rtol, max_it=max_it)
        W.set_column(0, case.b[r0:r1])
        ks._lib.check(ctx.L.ks_st_apply(st.h, C.c_void_p(W.column_ptr(0)), C.c_void_p(W.column_ptr(1))))
        return {"y": W.column(1), "ksp": st.GetKSPStats(), "bl": st.GetBCGSLStats()}
    finally:
        W.destroy(); st.destroy(); A.destroy()


def _check(out, which, ell, case, P, ref):
    minv = bc.jacobi(P)
    y = np.concatenate([o["y"] for o in out])
    res = float(np.linalg.norm(minv(case.b - P @ y)))
    print("its %s (restatement %d), last_rnorm %.3e, tol %.3e, true residual %.3e, gap %.2e, %s" % ([o["ksp"]["iterations"] for o in out], ref.its, out[0]["ksp"]["last_rnorm"], ref.tol, res, ref.gap, out[0]["bl"]))
    for o in out:
        assert o["ksp"] == out[0]["ksp"]                                     # count and residual norm: the same bits on every rank
        assert o["ksp"]["solves"] == 1 and o["ksp"]["last_rnorm"] <= ref.tol
        its = o["ksp"]["iterations"]
        if which == "kron":
            assert its == ref.its
        else:
            assert 0 < its <= 2 * ref.its + 1
        k = its // ell
        assert o["bl"]["host_waits"] == math.ceil((k + 1) / 4) and o["bl"]["gated_iterations"] == 4 * math.ceil((k + 1) / 4) - (k + 1)
    assert res <= ref.tol + 8 * ref.gap


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which,ell,split", [(w, l, i) for w, l in CASES for i in range(3)], ids=["%s-l%d-%s" % (w, l, "-".join(map(str, SPLITS[w][i]))) for w, l in CASES for i in range(3)])
def test_sharded_counts_and_solutions(which, ell, split):
    case, P, sigma, rtol, ref = _system(which, ell)
    assert ref.reason == "converged"
    counts = SPLITS[which][split]
    starts = np.concatenate([[0], np.cumsum(counts)])
    assert starts[-1] == case.n

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        try:
            comm.install(ctx, rank)
            return _solve(ks, ctx, case, int(starts[rank]), int(starts[rank + 1]), sigma, ell, rtol, 2 * ref.its)
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(len(counts), pairwise=True, timeout=60), fn, join_timeout=120)      # pairwise: a rank without rows has no neighbour to exchange with
    _check(out, which, ell, case, P, ref)


def test_collective_path_on_one_rank():
    """force_multi: the finish kernels and the allreduces on a communicator of one rank, without threads (the communicator is the caller-supplied one of
    tests/thread_comm.py at size 1, as in tests/test_gpu_cg_ranks.py). l = 4 has the widest finish kernel, 15 sums."""
    import slepc_amd as ks
    ctx = ks.Context(0)
    out = {}
    cases = CASES + [("kron", 1), ("kron", 4)]
    try:
        ctx.set_debug("force_multi")
        ThreadComm(1, timeout=60).install(ctx, 0)
        for which, ell in cases:
            case, P, sigma, rtol, ref = _system(which, ell)
            out[which, ell] = [_solve(ks, ctx, case, 0, case.n, sigma, ell, rtol, 2 * ref.its)]
    finally:
        ctx.close()
    for (which, ell), o in out.items():
        case, P, sigma, rtol, ref = _system(which, ell)
        _check(o, which, ell, case, P, ref)
