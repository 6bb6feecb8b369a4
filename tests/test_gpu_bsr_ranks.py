"""Block CSR matrices sharded by block rows: ranks are threads of one process (tests/thread_comm.py), each with a context of its own that it closes.
The diagonal block of every rank is block CSR; the ghost block, the halo plan and both halo kinds are the existing code on the expansion. The matrix
is bsr_cases.small at bs = 3 (integer data: every sum is exact, so the sharded product - diagonal block, then the ghost rows added - has the bits of
the one-rank product, which is the exact product of the expansion); the splits are in block rows, [half, rest] and [a, 0, b] with a rank that owns
nothing. The provider halo runs with ranks as threads; the peer-mapped halo between two processes (gloo for the collectives), as everywhere else in
the suite: its kernels wait for the neighbour's kernels, and the streams of one process share its few hardware queues, where a waiting kernel can
stand in front of the kernel it waits for until the halo's bounded wait gives up - ranks as threads are no place for it."""
import functools
import os
import sys
import time

import numpy as np
import pytest

import bsr_cases as bc
import layout_cases as lc
from thread_comm import ThreadComm, run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 3
KS_ERR_ARG_SIZ = 60


@functools.lru_cache(maxsize=None)
def world_case():
    """The matrix, its expansion, two vectors and a block of 11 columns with their exact products, and the one-rank GPU results."""
    import slepc_amd as ks
    ctx = ks.Context(0)
    try:
        P = ks.Mat.from_bsr(ctx, [0, 1], [0], np.ones((1, BS, BS)))
        i = P.bsr_info(); P.destroy()
        a = bc.small(BS, i["group_block_rows"], i["chunk_entries"])
        e = bc.expand(*a)
        n = len(e[0]) - 1
        xs = [lc.int_vector(n, 11), lc.int_vector(n, 12)]
        X = lc.int_vector(n, 13, cols=11)
        A = ks.Mat.from_bsr(ctx, *a)
        assert A.layout() == "bsr"
        one = {"y": [A.mult(x) for x in xs], "Y": A.mult_multi(X), "diag": A.get_diagonal(), "norm": A.norm_inf()}
        A.destroy()
    finally:
        ctx.close()
    ys = [lc.exact_product(*e, x) for x in xs]
    assert all(np.array_equal(u, v) for u, v in zip(one["y"], ys)) and np.array_equal(one["Y"], lc.exact_product(*e, X))
    return a, e, xs, X, one


def local_blocks(a, I0, I1):
    brp, bcol, blocks = a
    k0, k1 = int(brp[I0]), int(brp[I1])
    return (brp[I0:I1 + 1] - brp[I0]).astype(np.int32), bcol[k0:k1], blocks[k0:k1]


def splits(nb):
    return {2: [nb // 2, nb - nb // 2], 3: [nb // 3 + 1, 0, nb - nb // 3 - 1]}


def rank_body(ks, ctx, a, xs, X, starts, rank, N, halo, in_step):
    """One rank: the matrix from its block rows, two products back to back, the block product on 11 columns, diagonal and norm. in_step() keeps the
    ranks of a thread world together (a rank without rows would be done long before the others)."""
    I0, I1 = int(starts[rank]), int(starts[rank + 1])
    r0, r1 = I0 * BS, I1 * BS
    A = ks.Mat.from_bsr(ctx, *local_blocks(a, I0, I1), row_start=r0, n_global=N)
    res = {"layout": A.layout(), "info": A.bsr_info(), "sizes": (A.n, A.N, A.nnz), "halo": A.set_halo(halo)}
    B = ks.BV(ctx, A.n, 4, N=N)
    for j, x in enumerate(xs):
        B.set_column(j, x[r0:r1])
    for j in range(2):                                   # back to back, no host wait in between
        A.mult_dev(B.column_ptr(j), B.column_ptr(2 + j))
    res["y"] = [B.column(2 + j) for j in range(2)]
    in_step()
    XB, YB = ks.BV(ctx, A.n, 11, N=N), ks.BV(ctx, A.n, 11, N=N)
    XB.set_dense(X[r0:r1])
    A.mult_multi_dev(XB.column_ptr(0), XB.ld, YB.column_ptr(0), YB.ld, 11)
    res["Y"] = YB.dense()
    in_step()
    res["diag"] = A.get_diagonal()
    res["norm"] = A.norm_inf()
    ctx.synchronize()                                    # raises if a bounded wait of the peer halo gave up
    in_step()
    if halo == "peer":
        A.set_halo("provider")
    for M in (B, XB, YB, A):
        M.destroy()
    return res


def check_ranks(out, a, one, starts, N, halo):
    for rank in range(len(starts) - 1):
        I0, I1 = int(starts[rank]), int(starts[rank + 1])
        r0, r1 = I0 * BS, I1 * BS
        o = out[rank]
        lb = local_blocks(a, I0, I1)
        own = (lb[1] >= I0) & (lb[1] < I1)
        assert o["layout"] == "bsr" and o["halo"] == halo, (rank, o["layout"], o["halo"])
        assert o["info"]["bs"] == BS and o["info"]["block_rows"] == I1 - I0 and o["info"]["blocks"] == int(own.sum())      # the diagonal block alone
        assert o["info"]["index_bytes"] == 4 * int(own.sum()) + 4 * (I1 - I0 + 1)
        assert o["sizes"] == (r1 - r0, N, int(lb[0][-1]) * BS * BS)
        for j in range(2):
            assert np.array_equal(o["y"][j], one["y"][j][r0:r1]), (rank, j)
        assert np.array_equal(o["Y"], one["Y"][r0:r1])
        assert np.array_equal(o["diag"], one["diag"][r0:r1]) and o["norm"] == one["norm"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_bsr_sharded_products_have_the_one_rank_bits(world):
    halo = "provider"
    a, e, xs, X, one = world_case()
    nb = len(a[0]) - 1
    starts = np.concatenate([[0], np.cumsum(splits(nb)[world])])
    N = nb * BS

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        comm.install(ctx, rank)
        try:
            return rank_body(ks, ctx, a, xs, X, starts, rank, N, halo, comm.bar.wait)
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(world, pairwise=True, timeout=60), fn, join_timeout=120)
    check_ranks(out, a, one, starts, N, halo)
    assert any(int(starts[r + 1]) == int(starts[r]) for r in range(world)) == (world == 3)      # the rank without rows took part in everything


def _peer_worker(rank, world, port, q, a, xs, X, starts, N):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import slepc_amd as ks
        from slepc_amd import gloo_provider
        ctx = ks.Context(0)
        gloo_provider.install(ctx, dist, torch, rank, world)
        res = rank_body(ks, ctx, a, xs, X, starts, rank, N, "peer", dist.barrier)
        dist.barrier()
        ctx.close()
        q.put((rank, res))
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_bsr_sharded_products_peer_halo_between_processes():
    """Two processes on one GPU, boundary entries stored straight into the neighbour's ghost mailbox: the same bits as one rank."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _collect, _free_port
    a, e, xs, X, one = world_case()
    nb = len(a[0]) - 1
    starts = np.concatenate([[0], np.cumsum(splits(nb)[2])])
    N = nb * BS
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_peer_worker, args=(r, 2, port, q, a, xs, X, starts, N)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(_collect(q, procs, 2))
    for r in range(2):
        assert "error" not in out[r], out[r].get("error")
    check_ranks(out, a, one, starts, N, "peer")


@pytest.mark.timeout(120)
def test_bsr_sharded_size_not_a_multiple_is_refused_before_any_collective():
    """n_global = 3 nb + 1 on every rank: KS_ERR_ARG_SIZ at once, nobody waits in a collective for a rank that has left."""
    a = bc.small(BS, 8, 7 * BS * BS)
    nb = len(a[0]) - 1
    starts = [0, nb // 2, nb]
    timeout = 40

    def fn(rank, comm):
        import slepc_amd as ks
        ctx = ks.Context(0)
        comm.install(ctx, rank)
        try:
            brp, bcol, blocks = local_blocks(a, starts[rank], starts[rank + 1])
            t0 = time.perf_counter()
            try:
                ks.Mat.from_bsr(ctx, brp, bcol, blocks, row_start=starts[rank] * BS, n_global=nb * BS + 1)
                return None, 0.0
            except ks.KsError as err:
                return err.rc, time.perf_counter() - t0
        finally:
            ctx.close()
    out = run_ranks(ThreadComm(2, pairwise=True, timeout=timeout), fn, join_timeout=2 * timeout)
    for rank in range(2):
        assert out[rank][0] == KS_ERR_ARG_SIZ, out[rank]
        assert out[rank][1] < timeout / 4
