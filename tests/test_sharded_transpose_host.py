"""The host plan of the transposed product of a row-sharded matrix (ksc::sharded_transpose_plan, slepc_amd/csrc/ks_csr.cpp) and its host walk.
CPU only: every rank's plan is built through the ksc_* hooks of libksgpu.so, the walk of each rank runs on the host and the reverse exchange
between the ranks is simulated in numpy. Matrix values and vectors are small integers (tests/sharded_cases.py), so A^T x is exact in any order and
the result is compared with the integer product by np.array_equal."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import sharded_cases as sc
import slepc_amd._lib as L

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LP = C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_sharded_transpose_plan.argtypes = [C.c_int, C.c_int, IP, IP, DP, C.c_int, IP, C.c_int, IP, IP, IP, DP, IP, IP, DP, IP, IP, IP, LP]
    lib.ksc_sharded_transpose_plan.restype = None
    lib.ksc_sharded_transpose_local.argtypes = [C.c_int, C.c_int, IP, IP, DP, C.c_int, IP, DP, DP, DP]
    lib.ksc_sharded_transpose_local.restype = None
    lib.ksc_sharded_transpose_add.argtypes = [C.c_int, C.c_int, IP, DP, DP]
    lib.ksc_sharded_transpose_add.restype = None
    return lib


def _i(a):
    return a.ctypes.data_as(IP)


def _d(a):
    return a.ctypes.data_as(DP)


@functools.lru_cache(maxsize=None)
def case(name, world):
    return {"far": lambda: sc.far(world), "islands": sc.islands, "bighalo": lambda: sc.bighalo(world)}[name]()


def build_plan(lib, c, rank, fp):
    rp, col, val = (np.ascontiguousarray(a) for a in c.block(rank))
    r0, r1 = c.range(rank)
    n, nnz, ng, ns = r1 - r0, len(col), len(fp["ghosts"]), len(fp["send_idx"])
    out = {"d_rp": np.zeros(n + 1, np.int32), "d_col": np.zeros(max(nnz, 1), np.int32), "d_val": np.zeros(max(nnz, 1)),
           "o_rp": np.zeros(ng + 1, np.int32), "o_row": np.zeros(max(nnz, 1), np.int32), "o_val": np.zeros(max(nnz, 1)),
           "acc_rows": np.zeros(max(ns, 1), np.int32), "acc_ptr": np.zeros(ns + 1, np.int32), "acc_pos": np.zeros(max(ns, 1), np.int32)}
    info = np.zeros(3, np.int64)
    lib.ksc_sharded_transpose_plan(n, r0, _i(rp), _i(col), _d(val), ng, _i(fp["ghosts"]), ns, _i(fp["send_idx"]),
                                   _i(out["d_rp"]), _i(out["d_col"]), _d(out["d_val"]), _i(out["o_rp"]), _i(out["o_row"]), _d(out["o_val"]),
                                   _i(out["acc_rows"]), _i(out["acc_ptr"]), _i(out["acc_pos"]), info.ctypes.data_as(LP))
    nd, no, na = (int(v) for v in info)
    for k in ("d_col", "d_val"):
        out[k] = out[k][:nd]
    for k in ("o_row", "o_val"):
        out[k] = out[k][:no]
    out["acc_rows"] = out["acc_rows"][:na]; out["acc_ptr"] = out["acc_ptr"][:na + 1]; out["acc_pos"] = out["acc_pos"][:ns]
    return out


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,world", [("far", 4), ("far", 8), ("islands", 4), ("bighalo", 2), ("bighalo", 4)])
def test_sharded_transpose_plan_and_host_walk(lib, name, world):
    c = case(name, world)
    fps = sc.forward_plan(c)
    needs, nghost, nsend = sc.halo_plan(c)
    x = sc.int_vectors(c.N, 1, seed=100 + c.N % 97)[0]
    ref = (c.int_matrix().T @ x.astype(np.int64)) / float(c.scale)
    assert np.abs(ref).max() * c.scale < 2.0 ** 53
    rsend, y = [], []
    for rank in range(world):
        fp = fps[rank]
        r0, r1 = c.range(rank)
        n = r1 - r0
        assert len(fp["ghosts"]) == nghost[rank] and len(fp["send_idx"]) == nsend[rank]
        rp, col, val = (np.ascontiguousarray(a) for a in c.block(rank))
        keep = {"ghosts": fp["ghosts"].copy(), "send_idx": fp["send_idx"].copy(), "rp": rp.copy(), "col": col.copy(), "val": val.copy()}
        pl = build_plan(lib, c, rank, fp)
        # the forward arrays are inputs only
        assert np.array_equal(keep["ghosts"], fp["ghosts"]) and np.array_equal(keep["send_idx"], fp["send_idx"])
        assert np.array_equal(keep["rp"], rp) and np.array_equal(keep["col"], col) and np.array_equal(keep["val"], val)
        ns = len(fp["send_idx"])
        # acc_pos: a permutation of 0 .. nsend-1, grouped by row (ascending rows), ascending inside a row
        assert np.array_equal(np.sort(pl["acc_pos"]), np.arange(ns))
        assert pl["acc_ptr"][0] == 0 and pl["acc_ptr"][-1] == ns and np.all(np.diff(pl["acc_ptr"]) >= 1)
        assert np.all(np.diff(pl["acc_rows"]) > 0) and np.array_equal(pl["acc_rows"], np.unique(fp["send_idx"]))
        for i, r in enumerate(pl["acc_rows"]):
            pos = pl["acc_pos"][pl["acc_ptr"][i]:pl["acc_ptr"][i + 1]]
            assert np.all(np.diff(pos) > 0) and np.all(fp["send_idx"][pos] == r)
        # the two transposed blocks: every entry of the rank once; rows of original rows ascending (stable)
        loc = (col >= r0) & (col < r1)
        assert len(pl["d_col"]) == np.count_nonzero(loc) and len(pl["o_row"]) == np.count_nonzero(~loc)
        assert pl["o_rp"][-1] == len(pl["o_row"]) and np.all(np.diff(pl["o_rp"]) >= 1)        # every ghost has at least one entry
        rows = np.repeat(np.arange(n), np.diff(rp))
        for blk_rp, blk_row, blk_val, key in ((pl["d_rp"], pl["d_col"], pl["d_val"], col[loc] - r0),
                                              (pl["o_rp"], pl["o_row"], pl["o_val"], np.searchsorted(fp["ghosts"], col[~loc]))):
            sel = loc if blk_rp is pl["d_rp"] else ~loc
            order = np.argsort(key, kind="stable")
            assert np.array_equal(blk_row, rows[sel][order]) and np.array_equal(blk_val, val[sel][order])
            assert np.array_equal(blk_rp, np.concatenate([[0], np.cumsum(np.bincount(key, minlength=len(blk_rp) - 1))]))
        # one rank's share on the host
        xs = np.ascontiguousarray(x[r0:r1])
        rs = np.zeros(max(len(fp["ghosts"]), 1)); yl = np.zeros(max(n, 1))
        lib.ksc_sharded_transpose_local(n, r0, _i(rp), _i(col), _d(val), len(fp["ghosts"]), _i(fp["ghosts"]), _d(xs), _d(rs), _d(yl))
        rsend.append(rs); y.append(yl)
    # the reverse exchange: what rank p sends forward to q (send segment) it now receives from q (q's receive segment for p)
    for rank in range(world):
        fp = fps[rank]
        rrecv = np.zeros(max(len(fp["send_idx"]), 1))
        for i, q in enumerate(fp["peers"]):
            fq = fps[q]
            j = fq["peers"].index(rank)
            assert fq["rcnt"][j] == fp["scnt"][i]
            rrecv[fp["soff"][i]:fp["soff"][i] + fp["scnt"][i]] = rsend[q][fq["roff"][j]:fq["roff"][j] + fq["rcnt"][j]]
        r0, r1 = c.range(rank)
        lib.ksc_sharded_transpose_add(r1 - r0, len(fp["send_idx"]), _i(fp["send_idx"]), _d(rrecv), _d(y[rank]))
        assert np.array_equal(y[rank][:r1 - r0], ref[r0:r1]), (name, world, rank)
