"""The bound of the transposed ILU(0) block solves (tests/test_ilu_transpose_host.py on the host, tests/test_gpu_pc_ilu_transpose.py on the GPU).

PCApplyTranspose uses the factors of tests/ilu_cases.py's reference, M = L U of every block: y = M^-T x = L^-T U^-T x. Componentwise

    |M^T y - x| <= 8 (k + 1) 2^-53 (|U^T| |L^T| |y|)      k = the larger of the block's longest row and longest column

which is ilu_cases' bound with the substitution's row length corrected: a row of a transposed factor is a column of the factor. The left side is
evaluated in extended precision (ilu_cases._mv)."""
import numpy as np

import ilu_cases as ic


def block_k(F, k_row):
    """The larger of the longest row (k_row, as the reference counts it) and the longest column of the block's factors F."""
    return max(int(k_row), int(np.max(np.bincount(F.indices, minlength=F.shape[0]))))


def ratios_t(ref, x, y):
    """max over the rows of |M^T y - x| / (8 (k + 1) u |U^T||L^T||y|), one figure per block (0/0 counts as 0: an exact row)."""
    out = []
    for b0, bl, L, U, k, P, F in ref.blocks:
        Lt, Ut = L.T.tocsr(), U.T.tocsr()
        kk = block_k(F, k)
        yb = y[b0:b0 + bl]
        res = np.abs(ic._mv(Ut, ic._mv(Lt, yb)) - x[b0:b0 + bl].astype(ic.LD))
        bound = 8.0 * (kk + 1) * ic.U53 * ic._mv(abs(Ut), ic._mv(abs(Lt), np.abs(yb)))
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(res == 0, 0.0, res / bound)
        out.append(float(np.max(q)))
    return out


def check_t(ref, x, y, what=""):
    assert np.all(np.isfinite(y)), what
    r = ratios_t(ref, x, y)
    print("%s: largest |M^T y - x| / bound per block: max %.3g over %d blocks" % (what, max(r), len(r)))
    assert max(r) <= 1.0, (what, r)
    return max(r)


def solve_t(ref, x):
    """M^-T x in double with scipy's triangular solves (the CPU restatement, not the bound)."""
    import scipy.sparse.linalg as spl
    y = np.empty(ref.n)
    for b0, bl, L, U, *_ in ref.blocks:
        w = spl.spsolve_triangular(U.T.tocsr(), x[b0:b0 + bl], lower=True)
        y[b0:b0 + bl] = spl.spsolve_triangular(L.T.tocsr(), w, lower=False, unit_diagonal=True)
    return y
