"""Ranks as THREADS of one process: a communicator provider for libksgpu (ks_comm_set_ops) and the runner of a rank function.

A GPU box admits only a few processes on its card, so tests with more ranks than that - or with many short cases - run every rank as a thread
with its own libksgpu context (own streams). allreduce (fixed rank order: identical bits on every rank) and allgather meet all ranks at a
threading.Barrier. The neighbour exchange has two modes:

  collective (default)  every rank of the communicator enters every exchange: the slab matrices, where every rank has a neighbour.
  pairwise              one queue.Queue per ordered (src, dst) pair: only the ranks named in a halo plan take part, so a rank whose matrix has
                        no peers - and therefore never calls the exchange - does not leave the others waiting at a barrier.

Nothing waits forever: the barrier and every queue read have a time limit, and a rank that fails calls abort(), which breaks the barrier and
poisons the queues, so that the other ranks end at once with an error of their own."""
import ctypes
import queue
import threading
import traceback

import numpy as np

_POISON = object()


class ThreadComm:
    def __init__(self, size, pairwise=False, timeout=240):
        self.size = size
        self.pairwise = pairwise
        self.timeout = timeout
        self.bar = threading.Barrier(size, timeout=timeout)
        self.slots = [None] * size
        self.mail = {}
        self.queues = {(s, d): queue.Queue() for s in range(size) for d in range(size) if s != d} if pairwise else {}

    def abort(self):
        """A rank failed: no other rank may go on waiting for it."""
        try:
            self.bar.abort()
        except Exception:      # noqa: BLE001
            pass
        for q in self.queues.values():
            q.put(_POISON)

    def install(self, ctx, rank):
        size, bar, slots, mail, queues, timeout = self.size, self.bar, self.slots, self.mail, self.queues, self.timeout

        def allreduce_sum(ptr, count, stream):
            h = np.empty(count)
            ctx.memcpy_d2h(h, ptr, stream)
            slots[rank] = h
            bar.wait()
            tot = slots[0].copy()
            for r in range(1, size):
                tot += slots[r]                      # fixed rank order: identical bits on every rank
            bar.wait()
            ctx.memcpy_h2d(ptr, tot, stream)
            return 0

        def allgather_host(send, nbytes, recv):
            slots[rank] = ctypes.string_at(send, nbytes)
            bar.wait()
            ctypes.memmove(recv, b"".join(slots[r] for r in range(size)), nbytes * size)
            bar.wait()
            return 0

        def exchange(peers, dsend, soff, scnt, drecv, roff, rcnt, eb, stream):
            for i, p in enumerate(peers):
                if scnt[i]:
                    h = np.empty(scnt[i] * eb, dtype=np.uint8)
                    ctx.memcpy_d2h(h, dsend + soff[i] * eb, stream)
                    mail[(rank, p)] = h
            bar.wait()
            for i, p in enumerate(peers):
                if rcnt[i]:
                    ctx.memcpy_h2d(drecv + roff[i] * eb, mail[(p, rank)], stream)
            bar.wait()
            return 0

        def exchange_pairwise(peers, dsend, soff, scnt, drecv, roff, rcnt, eb, stream):
            # one message per (src, dst) pair and exchange, in the order of the calls: a queue keeps back-to-back products apart
            for i, p in enumerate(peers):
                if scnt[i]:
                    h = np.empty(scnt[i] * eb, dtype=np.uint8)
                    ctx.memcpy_d2h(h, dsend + soff[i] * eb, stream)
                    queues[(rank, p)].put(h)
            for i, p in enumerate(peers):
                if rcnt[i]:
                    h = queues[(p, rank)].get(timeout=timeout)          # queue.Empty after the time limit: never a hang
                    if h is _POISON:
                        queues[(p, rank)].put(_POISON)
                        raise RuntimeError("rank %d: the exchange was aborted by a failing rank" % rank)
                    if h.size != rcnt[i] * eb:
                        raise RuntimeError("rank %d expected %d bytes from rank %d and got %d" % (rank, rcnt[i] * eb, p, h.size))
                    ctx.memcpy_h2d(drecv + roff[i] * eb, h, stream)
            return 0

        ctx.set_comm_ops(rank, size, allreduce_sum, allgather_host, exchange_pairwise if self.pairwise else exchange)


def run_ranks(comm, fn, join_timeout=300):
    """fn(rank, comm) on one thread per rank; the list of their results. A rank that raises aborts the communicator (the others end at once)
    and its traceback fails the calling test."""
    world = comm.size
    out = [None] * world

    def body(rank):
        try:
            out[rank] = {"ok": fn(rank, comm)}
        except BaseException:      # noqa: BLE001
            out[rank] = {"error": traceback.format_exc()}
            comm.abort()

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(join_timeout)
    alive = [r for r, t in enumerate(th) if t.is_alive()]
    if alive:
        comm.abort()
        for t in th:
            t.join(30)
    assert not alive, "ranks %s did not finish within %d s" % (alive, join_timeout)
    errors = ["rank %d:\n%s" % (r, o["error"]) for r, o in enumerate(out) if o is not None and "error" in o]
    assert not errors and None not in out, "\n".join(errors)     # (all of them: the first to fail made the others fail at their next wait)
    return [o["ok"] for o in out]
