"""Block CSR (BAIJ) input on the host (slepc_amd/csrc/ks_csr.cpp: bsr_expand, bsr_diag, bsr_plan, bsr_apply_host). CPU only.

tests/host/bsr_plan.cpp, a program of its own built together with ks_csr.cpp with -fsanitize=address,undefined, checks the expansion against brute
force for block sizes 1 .. 9, the host walk of the device image against a plain CSR product of the expansion for block sizes 2 .. 8 (one rank, and
the middle rank of three) with exact integer data, and every rejection. One build and one run.

The other tests pin tests/bsr_cases.py, which the GPU tests rest on: its numpy expansion against the library's (the ksc_bsr_expand hook of
libksgpu.so), the premise of its exact sums, and the shapes its generators promise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bsr_cases as bc
import layout_cases as lc
import slepc_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, DP, LLP = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_longlong)

CHECKS = ["expansion bs %d" % bs for bs in range(1, 10)] + \
         ["product bs %d %s" % (bs, w) for bs in range(2, 9) for w in ("one rank", "middle rank of three")] + ["rejections"]


def constants(bs):
    """Any constants a kernel could have: a group of four waves' worth of block rows, a chunk of whole blocks (the GPU tests read the real ones)."""
    return 4 * (64 // bs), 7 * bs * bs


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bsr_plan") / "bsr_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wno-unknown-pragmas", "-pthread", os.path.join(ROOT, "tests", "host", "bsr_plan.cpp"),
                           os.path.join(ROOT, "slepc_amd", "csrc", "ks_csr.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", CHECKS)
def test_bsr_planners_under_asan_ubsan(report, name):
    assert any(line == "ok " + name or line.startswith("ok " + name + ":") for line in report), (name, report)
    assert report[-1] == "all ok"


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(os.environ.get("KS_HOST_HOOKS_LIB") or L.LIB_PATH)
    lib.ksc_bsr_expand.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, DP, IP, IP, DP, LLP]
    lib.ksc_bsr_expand.restype = C.c_int
    lib.ksc_bsr_plan.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, DP, C.c_int, C.c_int, DP, DP, DP, LLP]
    lib.ksc_bsr_plan.restype = None
    return lib


def _colmajor(blocks):
    return np.ascontiguousarray(blocks.transpose(0, 2, 1)).reshape(-1)


@pytest.mark.parametrize("bs", range(2, 9))
def test_cases_expansion_is_the_librarys(lib, bs):
    G, chunk = constants(bs)
    brp, bcol, blocks = bc.small(bs, G, chunk)
    rp, col, val = bc.expand(brp, bcol, blocks)
    nb, nnz = len(brp) - 1, int(brp[-1]) * bs * bs
    bval = _colmajor(blocks)
    rp2, col2, val2 = np.zeros(nb * bs + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
    info = (C.c_longlong * 4)()
    st = lib.ksc_bsr_expand(bs, nb, nb, brp.ctypes.data_as(IP), bcol.ctypes.data_as(IP), bval.ctypes.data_as(DP),
                            rp2.ctypes.data_as(IP), col2.ctypes.data_as(IP), val2.ctypes.data_as(DP), info)
    assert st == 0 and info[3] == nnz
    assert np.array_equal(rp, rp2) and np.array_equal(col, col2) and np.array_equal(val, val2)
    # and the host walk of the image gives the exact product of that expansion
    x = lc.int_vector(nb * bs, 3)
    y = np.full(nb * bs, -1.0)
    img = np.zeros(nnz)
    lib.ksc_bsr_plan(bs, nb, 0, brp.ctypes.data_as(IP), bcol.ctypes.data_as(IP), bval.ctypes.data_as(DP), G, chunk // (bs * bs),
                     img.ctypes.data_as(DP), x.ctypes.data_as(DP), y.ctypes.data_as(DP), info)
    assert info[0] == int(brp[-1])
    assert np.array_equal(img.reshape(-1, bs, bs), blocks)                   # the image is row-major blocks
    assert np.array_equal(y, lc.exact_product(rp, col, val, x))


@pytest.mark.parametrize("bs", range(2, 9))
def test_small_shape_and_exactness_premise(bs):
    for G, chunk in (constants(bs), (4 * (64 // bs), min(64, 512 // (bs * bs)) * bs * bs)):
        brp, bcol, blocks = bc.small(bs, G, chunk)
        lens = np.diff(brp)
        assert len(lens) == 5 * G + 3 and np.all(lens[::7] == 0) and (lens == 1).any()
        assert bs * bs * lens.max() > 3 * chunk and lens.max() <= bc.LONG_ROW_BLOCKS_MAX
        assert np.abs(blocks).max() <= 255 and np.array_equal(blocks, np.round(blocks))
        assert lens.max() * bs <= 1600 and bc.longest_row_bound(brp, blocks) < 2 ** 22       # every partial sum is exact in any order
        zeros = (blocks == 0).any(axis=(1, 2)).sum()
        assert abs(zeros - len(bcol) / 5) <= 1
        unsorted = repeated = 0
        for I in range(len(lens)):
            c = bcol[brp[I]:brp[I + 1]]
            unsorted += bool(np.any(np.diff(c) < 0)); repeated += len(np.unique(c)) < len(c)
        assert unsorted > 10 and repeated > 10
        br, bcr, blr = bc.small_real(bs, G, chunk)
        lr = np.diff(br)
        assert len(lr) == 10 * G + 3 and len(lr) * bs >= 2048 and np.all(lr[::7] == 0) and (lr == 1).any() and lr.max() == lens.max()
        assert abs((blr == 0).any(axis=(1, 2)).sum() - len(bcr) / 5) <= 1 and not np.array_equal(blr, np.round(blr))


@pytest.mark.parametrize("symmetric", [True, False])
def test_mesh_blocks(symmetric):
    import scipy.sparse as sp
    brp, bcol, blocks = bc.mesh_blocks(4, 3, 0.8, symmetric=symmetric)
    rp, col, val = bc.expand(brp, bcol, blocks)
    A = sp.csr_matrix((val, col, rp), shape=(192, 192))
    P = sp.csr_matrix((np.ones(len(bcol)), bcol, brp), shape=(64, 64))
    assert (P != P.T).nnz == 0 and P.diagonal().all() and np.diff(brp).max() <= 27
    assert all(np.all(np.diff(bcol[brp[I]:brp[I + 1]]) > 0) for I in range(64))
    assert (abs(A - A.T).max() == 0) == symmetric
    assert predicted_bytes_are_consistent(brp, blocks)


def predicted_bytes_are_consistent(brp, blocks):
    i = bc.predict_info(brp, blocks)
    return bc.layout_bytes(brp, blocks) == 8 * i["bs"] ** 2 * i["blocks"] + i["index_bytes"]
