"""ctypes wrappers of the assembly planners of slepc_amd/csrc/ks_csr.cpp (the ksc_* hooks of libksgpu.so; CPU only): the diagonal / ghost split of a
row block, the three host steps of the halo plan, the binned layout. Shared by tests/test_assembly_host.py and the worker of tests/test_dist_cpu.py."""
import ctypes as C
import os

import numpy as np

import slepc_amd._lib as L

IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)
LP = C.POINTER(C.c_longlong)
HP = C.POINTER(C.c_ushort)

SPLIT_ROWPTR, SPLIT_COLUMN = 1, 2
HALO_UNORDERED, HALO_SELF, HALO_NOT_OWNED = 1, 2, 3
BINNED_16BIT, BINNED_32BIT = 1, 2
BN_CS_MAX, BN_SEG_PAD = 9984, 8            # ksgpu_internal.h


def load():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_split_block.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, DP, IP, IP, DP, IP, IP, DP, IP, LP]
    lib.ksc_halo_recv_counts.argtypes = [C.c_int, IP, C.c_int, IP, C.c_int, IP]
    lib.ksc_halo_peers.argtypes = [C.c_int, C.c_int, IP, IP, IP, IP, IP, IP, IP, IP]
    lib.ksc_halo_localize_send_idx.argtypes = [C.c_int, C.c_int, C.c_int, IP]
    lib.ksc_binned_geometry.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, IP]
    lib.ksc_binned_plan.argtypes = [C.c_int, IP, IP, DP, C.c_int, C.c_int, C.c_int, LP, HP, HP, DP, IP, IP, IP, LP, IP, IP, DP, DP]
    for f in (lib.ksc_split_block, lib.ksc_halo_recv_counts, lib.ksc_halo_peers, lib.ksc_halo_localize_send_idx, lib.ksc_binned_geometry, lib.ksc_binned_plan):
        f.restype = C.c_int
    return lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t=IP):
    return a.ctypes.data_as(t)


def split_block(lib, n_local, row_start, n_global, rowptr, col, val):
    """-> dict(status, bad_row, bad_col) on a rejection, else also rp_d, col_d, val_d, rp_o, col_o, val_o, garray."""
    rowptr, col, val = _i32(rowptr), _i32(col), np.ascontiguousarray(val, dtype=np.float64)
    cap = max(int(rowptr[n_local]), 1)
    o = {"rp_d": np.zeros(n_local + 1, np.int32), "col_d": np.zeros(cap, np.int32), "val_d": np.zeros(cap),
         "rp_o": np.zeros(n_local + 1, np.int32), "col_o": np.zeros(cap, np.int32), "val_o": np.zeros(cap), "garray": np.zeros(cap, np.int32)}
    info = np.zeros(6, np.int64)
    st = lib.ksc_split_block(n_local, row_start, n_global, _p(rowptr), _p(col), _p(val, DP), _p(o["rp_d"]), _p(o["col_d"]), _p(o["val_d"], DP),
                             _p(o["rp_o"]), _p(o["col_o"]), _p(o["val_o"], DP), _p(o["garray"]), _p(info, LP))
    assert st == info[0]
    if st:
        return {"status": st, "bad_row": int(info[1]), "bad_col": int(info[2])}
    nd, no, ng = (int(v) for v in info[3:])
    for k in ("col_d", "val_d"):
        o[k] = o[k][:nd]
    for k in ("col_o", "val_o"):
        o[k] = o[k][:no]
    o["garray"] = o["garray"][:ng]
    o["status"] = 0
    return o


def halo_recv_counts(lib, garray, starts, rank):
    """starts: world + 1 row starts. -> (status, recv_cnt[world])"""
    garray, starts = _i32(garray), _i32(starts)
    cnt = np.zeros(len(starts) - 1, np.int32)
    st = lib.ksc_halo_recv_counts(len(garray), _p(garray), len(starts) - 1, _p(starts), rank, _p(cnt))
    return st, cnt


def halo_peers(lib, rank, recv_cnt, all_cnt):
    """all_cnt: world x world, row p = rank p's recv_cnt. -> dict(peers, rcnt, scnt, roff, soff, nsend)"""
    recv_cnt, all_cnt = _i32(recv_cnt), _i32(all_cnt)
    world = len(recv_cnt)
    assert all_cnt.shape == (world, world)
    a = [np.zeros(world, np.int32) for _ in range(5)]
    nsend = C.c_int(-1)
    k = lib.ksc_halo_peers(rank, world, _p(recv_cnt), _p(all_cnt), *[_p(x) for x in a], C.cast(C.byref(nsend), IP))
    out = {name: x[:k] for name, x in zip(("peers", "rcnt", "scnt", "roff", "soff"), a)}
    out["nsend"] = nsend.value
    return out


def halo_localize_send_idx(lib, row_start, n, ids):
    """ids: the global row ids the peers asked for. -> (status, local rows)"""
    sidx = _i32(ids).copy()
    st = lib.ksc_halo_localize_send_idx(row_start, n, len(sidx), _p(sidx))
    return st, sidx


def binned_geometry(lib, n, nnz, ncu, cs_max=BN_CS_MAX, seg_pad=BN_SEG_PAD):
    geo = np.zeros(4, np.int32)
    st = lib.ksc_binned_geometry(n, nnz, ncu, cs_max, seg_pad, _p(geo))
    return st, dict(zip(("ns", "cs", "wb", "wr"), (int(v) for v in geo)))


def binned_plan(lib, n, rowptr, col, val, ncu, x=None, cs_max=BN_CS_MAX, seg_pad=BN_SEG_PAD):
    """-> dict: ns, cs, wb, wr, nwin, entries, the nine arrays of the plan (2-D where the plan is) and, with x, y = the host walk of the plan."""
    rowptr, col, val = _i32(rowptr), _i32(col), np.ascontiguousarray(val, dtype=np.float64)
    info = np.zeros(8, np.int64)
    args = (n, _p(rowptr), _p(col), _p(val, DP), ncu, cs_max, seg_pad, _p(info, LP))
    assert lib.ksc_binned_plan(*args, None, None, None, None, None, None, None, None, None, None, None) == 0, info
    _, ns, cs, wb, wr, _, nwin, entries = (int(v) for v in info)
    o = {"ns": ns, "cs": cs, "wb": wb, "wr": wr, "nwin": nwin, "entries": entries,
         "col16": np.zeros(entries, np.uint16), "row16": np.zeros(entries, np.uint16), "val2": np.zeros(entries),
         "off1": np.zeros((ns, wb + 1), np.int32), "off2t": np.zeros((ns, wb), np.int32), "wseg": np.zeros((ns, nwin), np.int32),
         "sbase": np.zeros(ns + 1, np.int64), "off2": np.zeros((wb, ns), np.int32), "log2": np.zeros((wb, ns + 1), np.int32)}
    xx = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    y = None if x is None else np.full(n, np.nan)
    assert lib.ksc_binned_plan(*args, _p(o["col16"], HP), _p(o["row16"], HP), _p(o["val2"], DP), _p(o["off1"]), _p(o["off2t"]), _p(o["wseg"]),
                               _p(o["sbase"], LP), _p(o["off2"]), _p(o["log2"]), None if x is None else _p(xx, DP), None if x is None else _p(y, DP)) == 0
    o["y"] = y
    return o
