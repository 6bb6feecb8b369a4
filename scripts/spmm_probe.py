"""The block product (ks_mat_mult_multi, BVMatMult's MAT method) against the column loop (one ks_mat_mult per column): us per column at
ncols in {1, 2, 4, 8, 16, 32} from device events (ks_prof, class spmv_csr: every launch of the product), the layout's compulsory bytes
per call (A_bytes per pass + 16 n per column: the byte model of DESIGN.md section 15) and TB/s, and whether the block's columns are
bit for bit the loop's. CSR matrices are timed with both gather forms (KSGPU_SPMM=direct / interleaved).
Usage: python scripts/spmm_probe.py [only=name,...] [nx=216] [reps=10]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import slepc_amd as ks

args = dict(a.split("=", 1) for a in sys.argv[1:])
only = set(args["only"].split(",")) if "only" in args else None
NX = int(args.get("nx", 216))
REPS = int(args.get("reps", 10))
NCOLS = [1, 2, 4, 8, 16, 32]
ctx = ks.Context(0)


def tri(n):
    return sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])


def banded(n, mean, seed):
    """scripts/csr_probe.py's banded random CSR: Poisson row lengths, every 17th row empty, columns within +-32768 of the diagonal."""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.poisson(mean, n), 0, None); lens[::17] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = (np.repeat(np.arange(n), lens) + rng.integers(-32768, 32768, nnz)).clip(0, n - 1).astype(np.int32)
    # sorted, duplicate-free rows are not needed by the product; keep the generator's entries as they are
    return rowptr, col, rng.uniform(-1, 1, nnz)


def fem3(g):
    """3 degrees of freedom per node of a g^3 grid, 27-point node coupling: rows of 81 entries, random values."""
    P = sp.kron(sp.kron(tri(g), tri(g)), tri(g)).tocsr()
    F = sp.kron(P, np.ones((3, 3))).tocsr(); F.sort_indices()
    return F.indptr.astype(np.int32), F.indices.astype(np.int32), np.random.default_rng(7).standard_normal(F.nnz)


def stencil27(N):
    P = sp.kron(tri(N), sp.kron(tri(N), tri(N))).tocsr(); P.sort_indices()
    n = P.shape[0]
    val = np.full(P.nnz, -1.0); val[P.indices == np.repeat(np.arange(n), np.diff(P.indptr))] = 26.0
    return P.indptr.astype(np.int32), P.indices.astype(np.int32), val


def cases():
    yield "laplacian%d^3" % NX, None, None, lambda: ks.Mat.laplacian3d(ctx, NX, NX, NX)
    yield "laplacian%d^3_sell" % NX, "sell", None, lambda: ks.Mat.laplacian3d(ctx, NX, NX, NX)
    yield "stencil27_128^3", None, None, lambda: ks.Mat.from_csr(ctx, *stencil27(128))
    for form in ("direct", "interleaved"):
        yield "laplacian%d^3_csr_%s" % (NX, form), "csr", form, lambda: ks.Mat.laplacian3d(ctx, NX, NX, NX)
        yield "banded_mean32_csr_" + form, "csr", form, lambda: ks.Mat.from_csr(ctx, *banded(1_000_000, 32, 1))
        yield "banded_mean100_csr_" + form, "csr", form, lambda: ks.Mat.from_csr(ctx, *banded(500_000, 100, 2))
        yield "fem3dof_27pt_64^3_csr_" + form, "csr", form, lambda: ks.Mat.from_csr(ctx, *fem3(64))


def timed(fn, reps):
    fn(); ctx.synchronize()
    ctx.prof_enable(True, classes=["spmv_csr"]); ctx.prof_reset()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    v = ctx.prof_get()["spmv_csr"]; ctx.prof_enable(False)
    return v["ms"] / reps, v["hbm_bytes"] / reps


for name, layout, form, make in cases():
    if only and not any(o in name for o in only):
        continue
    for k, v in (("KSGPU_SPMV", layout), ("KSGPU_SPMM", form)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    A = make()
    n = A.n
    X, Y, Z = (ks.BV(ctx, n, max(NCOLS)) for _ in range(3))
    X.SetRandom(3)
    x0, y0, z0, ld = X.column_ptr(0), Y.column_ptr(0), Z.column_ptr(0), X.ld
    print("%s: n=%d nnz=%d layout=%s gather=%s" % (name, n, A.nnz, A.layout(), form or "-"), flush=True)
    for nc in NCOLS:
        loop_ms, loop_b = timed(lambda: [A.mult_dev(x0 + 8 * j * ld, z0 + 8 * j * ld) for j in range(nc)], REPS)
        blk_ms, blk_b = timed(lambda: A.mult_multi_dev(x0, ld, y0, ld, nc), REPS)
        same = all(np.array_equal(Y.column(j), Z.column(j)) for j in range(nc))
        print("  ncols %2d  loop %8.2f us/col %5.2f TB/s  block %8.2f us/col %5.2f TB/s  block/loop %.3f  bytes/row/col loop %6.1f block %6.1f  bits_equal %s"
              % (nc, 1e3 * loop_ms / nc, loop_b / loop_ms / 1e9, 1e3 * blk_ms / nc, blk_b / blk_ms / 1e9, blk_ms / loop_ms,
                 loop_b / n / nc, blk_b / n / nc, same), flush=True)
    del X, Y, Z
    A.destroy()
