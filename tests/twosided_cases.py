"""Shared inputs and the CPU restatement of the two-sided Krylov-Schur solver (EPSSolve_KrylovSchur_TwoSided, ks-twosided.c:27-241, on
DS NHEPTS, dsnhepts.c) for tests/test_ds_twosided_host.py and tests/test_gpu_twosided.py.

The restatement is built from the oracle's pieces: two oracle.BV bases (the reference's Gram-Schmidt policy, Arnoldi through a callable
operator), two oracle.DSNHEP halves (LAPACK hseqr / trexc / trevc) and, written out here, what DS NHEPTS adds to them: the correspondence
check, the greedy nearest-value permutation and DSSortWithPermutation_NHEP_Private (dsutil.c:177-237). It is the integer-control-flow
reference of the GPU tests: restarts, converged pairs and Arnoldi steps must come out the same."""
import ctypes as C

import numpy as np

from oracle import oracle as O

SQRT_EPS = np.sqrt(np.finfo(float).eps)
LEFT_SEED_XOR = 0x9E3779B97F4A7C15          # the left start vectors draw from their own stream (ks_krylovschur.hip: left_start_vector)


def transpose(A):
    S = A.to_scipy().T.tocsr(); S.sort_indices()
    return O.CSR(A.n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))


def ex41_start_vectors(n):
    """ex41.c:103-114: v0 = e0 + e1 + e2, w0 = 2 e0 + 0.5 e2"""
    v0 = np.zeros(n); v0[:3] = 1.0
    w0 = np.zeros(n); w0[0] = 2.0; w0[2] = 0.5
    return v0, w0


def convection_diffusion(n, px=0.05, py=0.02):
    """n x n grid, centre 4, west / east -(1 +- px), south / north -(1 +- py). Exact eigenvalues: the sums over both directions of
    2 - 2 sqrt(1 - p^2) cos(k pi / (n + 1)), k = 1..n (a tridiagonal Toeplitz matrix tridiag(-(1+p), 2, -(1-p)) per direction)."""
    import scipy.sparse as sp
    Tx = sp.diags([-(1 + px) * np.ones(n - 1), 2.0 * np.ones(n), -(1 - px) * np.ones(n - 1)], [-1, 0, 1])
    Ty = sp.diags([-(1 + py) * np.ones(n - 1), 2.0 * np.ones(n), -(1 - py) * np.ones(n - 1)], [-1, 0, 1])
    I = sp.identity(n)
    S = (sp.kron(I, Tx) + sp.kron(Ty, I)).tocsr(); S.sort_indices()
    k = np.arange(1, n + 1)
    ex = 2 - 2 * np.sqrt(1 - px * px) * np.cos(k * np.pi / (n + 1))
    ey = 2 - 2 * np.sqrt(1 - py * py) * np.cos(k * np.pi / (n + 1))
    exact = np.sort((ex[:, None] + ey[None, :]).ravel())[::-1]
    return O.CSR(n * n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)), exact


def ragged_nonsymmetric(n=3000, seed=11):
    """rows of 1 to 40 entries (mean about 20, more than 16), columns anywhere, values N(0,1): a general CSR matrix"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, n)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    cols = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens])
    vals = rng.standard_normal(rowptr[-1])
    S = sp.csr_matrix((vals, cols, rowptr), shape=(n, n)); S.sort_indices()
    return O.CSR(n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64))


class DSNHEPTS:
    """DS NHEPTS: half `a` (A, Q, X of Op) and half `b` (B, Z, Y of Op^T, own wr2 / wi2). Dimensions and state live in `a` and are
    copied to `b` before every step."""

    def __init__(self, ld, compare):
        self.ld = ld
        self.a = O.DSNHEP(ld, compare); self.b = O.DSNHEP(ld, compare)
        self.wr2 = np.zeros(ld); self.wi2 = np.zeros(ld)
        self.permuted = 0

    def _dims_to_b(self):
        a, b = self.a, self.b
        b.n, b.l, b.k, b.t, b.state = a.n, a.l, a.k, a.t, a.state

    def SetDimensions(self, n, l, k):
        self.a.SetDimensions(n, l, k); self.b.SetDimensions(n, l, k)

    def SetState(self, st):
        self.a.SetState(st); self.b.SetState(st)

    def Solve(self, wr, wi):
        self._dims_to_b()
        self.a.Solve(wr, wi); self.b.Solve(self.wr2, self.wi2)

    def permutation(self, wr, wi):
        """dsnhepts.c:216-229: None when the two halves correspond, else the greedy nearest-value permutation"""
        n = self.a.n
        idx = [i for i in range(n) if np.hypot(self.wr2[i] - wr[i], self.wi2[i] - wi[i]) > SQRT_EPS]
        if not idx:
            return None
        p = -np.ones(n, dtype=np.int64); free = list(idx)
        for i in idx:
            best, t = None, np.finfo(float).max
            for j in free:
                s = np.hypot(self.wr2[j] - wr[i], self.wi2[j] - wi[i])
                if s < t:
                    best, t = j, s
            p[i] = best; free.remove(best)
        for i in range(n):
            if p[i] == -1:
                p[i] = i
        return p

    def sort_with_permutation(self, perm):
        """DSSortWithPermutation_NHEP_Private dsutil.c:177-237 on the second half"""
        b = self.b; n, ld, T, Q = b.n, b.ld, b.A, b.Q
        work = np.zeros(ld); info = C.c_int(0)
        i = b.l
        while i < n - 1:
            pos = int(perm[i])
            inc = 2 if (pos < n - 1 and T[pos + 1, pos] != 0.0) else 1
            if pos != i:
                assert pos > i
                assert (T[pos, pos - 1] == 0.0 or perm[i + 1] == pos - 1) and (pos == n - 1 or T[pos + 1, pos] == 0.0 or perm[i + 1] == pos + 1), "Invalid permutation due to a 2x2 block"
                ifst = C.c_int(pos + 1); ilst = C.c_int(i + 1)
                O._L("dtrexc")(b"V", O._i(n), O._p(T), O._i(ld), O._p(Q), O._i(ld), C.byref(ifst), C.byref(ilst), O._p(work), C.byref(info))
                assert info.value == 0, info.value
                for j in range(i + 1, n):
                    if i <= perm[j] < pos:
                        perm[j] += inc
                perm[i] = i
                if inc == 2:
                    perm[i + 1] = i + 1
            i += inc
        b._eig_from_T(self.wr2, self.wi2, b.l, n)

    def Sort(self, wr, wi):
        self.a.Sort(wr, wi)
        self._dims_to_b()
        self.b.Sort(self.wr2, self.wi2)
        p = self.permutation(wr, wi)
        if p is not None:
            self.permuted += 1
            self.sort_with_permutation(p)
        return p is not None

    def UpdateExtraRow(self):
        self._dims_to_b()
        self.a.UpdateExtraRow(); self.b.UpdateExtraRow()

    def GetTruncateSize(self, l, n, k):
        if self.a.A[l + k, l + k - 1] != 0.0 or self.b.A[l + k, l + k - 1] != 0.0:
            k = k + 1 if l + k < n - 1 else k - 1
        return k

    def Truncate(self, n, trim):
        self._dims_to_b()
        self.a.Truncate(n, trim); self.b.Truncate(n, trim)


class TwoSidedResult:
    pass


def eps_krylovschur_twosided(A, nev, ncv=None, tol=1e-8, max_it=None, which="largest_magnitude", keep=0.5, seed=0x12345678,
                             v0=None, w0=None, lock=True, sigma=0.0):
    """EPSSolve_KrylovSchur_TwoSided (ks-twosided.c:126-241) with EPSTwoSidedRQUpdate1 / 2, the two-sided EPSKrylovConvergence
    (epskrylov.c:241-282, relative test) and the left branch of EPSComputeVectors_Schur (epsdefault.c:141-167). sigma: STSHIFT.
    Result: nconv, its, steps (of both runs), eigr / eigi / perm as the one-sided oracle's, X and Y (columns of the two bases after
    EPSComputeVectors), permuted_at (restarts whose DSSort permuted the second half) and margin, the smallest relative distance from
    tol of any estimate the convergence test looked at."""
    import scipy.linalg as sl
    n = A.n
    At = transpose(A)
    if ncv is None:
        ncv = min(n, max(2 * nev, nev + 15))
    mpd = ncv
    if max_it is None:
        max_it = max(100, 2 * n // ncv)
    compare = which if callable(which) else O.WHICH[which]
    if sigma != 0.0:
        def ds_compare(ar, ai, br, bi):
            return compare(ar + sigma, ai, br + sigma, bi)
    else:
        ds_compare = compare
    op = (lambda x: A.mult(x) - sigma * x) if sigma != 0.0 else (lambda x: A.mult(x))
    opt = (lambda x: At.mult(x) - sigma * x) if sigma != 0.0 else (lambda x: At.mult(x))
    V = O.BV(n, ncv + 1); W = O.BV(n, ncv + 1)
    ds = DSNHEPTS(ncv + 1, ds_compare)
    ld = ncv + 1
    M = np.zeros((ld, ld), order="F")
    eigr = np.zeros(ld); eigi = np.zeros(ld); errest = np.zeros(ld)

    def start_vector(bv, i, first, sd):
        if first is not None and i == 0:
            bv.set_column(0, first)
        else:
            bv.SetRandomColumn(i, sd)
        _, norm, lindep = bv.OrthogonalizeColumn(i)
        if not (lindep or norm == 0.0):
            bv.ScaleColumn(i, 1.0 / norm)
        return lindep or norm == 0.0

    V.SetActiveColumns(0, ncv + 1); W.SetActiveColumns(0, ncv + 1)
    assert not start_vector(V, 0, v0, seed)
    assert not start_vector(W, 0, w0, (seed ^ LEFT_SEED_XOR) & 0xFFFFFFFFFFFFFFFF)
    l = 0; nconv = 0; its = 0; reason = 0; steps = 0
    permuted_at = []; margin = np.inf
    while reason == 0:
        its += 1
        nv = min(nconv + mpd, ncv)
        k0 = nconv + l
        ds.SetDimensions(nv, nconv, k0)
        Hs = np.asfortranarray(ds.a.A)
        nv, beta, breakdown = V.MatArnoldiOp(op, Hs, k0, nv)
        ds.a.A[:, :] = Hs
        Hs = np.asfortranarray(ds.b.A)
        nvt, betat, breakdownt = W.MatArnoldiOp(opt, Hs, k0, nv)
        ds.b.A[:, :] = Hs
        steps += (nv - k0) + (nvt - k0)
        nv = min(nv, nvt)
        ds.SetDimensions(nv, nconv, k0)
        ds.SetState(O.DS_STATE_RAW if l else O.DS_STATE_INTERMEDIATE)
        breakdown = breakdown or breakdownt
        # L-shaped BVMatProject(V,NULL,W,M): everything but the leading k0 x k0 block
        Vd, Wd = V.dense(), W.dense()
        M[:k0, k0:nv] = Wd[:, :k0].T @ Vd[:, k0:nv]
        M[k0:nv, :nv] = Wd[:, k0:nv].T @ Vd[:, :nv]
        # EPSTwoSidedRQUpdate1
        V.SetActiveColumns(0, nv); W.SetActiveColumns(0, nv)
        lu = sl.lu_factor(np.array(M[:nv, :nv]), check_finite=False)
        w = W.DotVec(np.array(V.column(nv)))
        w = sl.lu_solve(lu, w, trans=0, check_finite=False)
        V.MultColumn(-1.0, 1.0, nv, w)
        ds.a.A[:nv, nv - 1] += beta * w
        w = V.DotVec(np.array(W.column(nv)))
        w = sl.lu_solve(lu, w, trans=1, check_finite=False)
        W.MultColumn(-1.0, 1.0, nv, w)
        ds.b.A[:nv, nv - 1] += betat * w
        V.SetActiveColumns(k0, nv); W.SetActiveColumns(k0, nv)
        # projected problem
        ds.Solve(eigr, eigi)
        if ds.Sort(eigr, eigi):
            permuted_at.append(its)
        ds.UpdateExtraRow()
        norm = V.NormColumn(nv); norm2 = W.NormColumn(nv)
        marker = -1
        k = nconv
        while k < nv:
            re, im = eigr[k] + sigma, eigi[k]            # STSHIFT: the estimate is taken on the back-transformed value (epskrylov.c:245)
            newk, resnorm = ds.a.Vectors(k)
            errest[k] = O._converged("rel", re, im, resnorm * beta * norm)
            margin = min(margin, abs(errest[k] - tol) / tol)
            if marker == -1 and errest[k] >= tol:
                marker = k
            ds._dims_to_b()
            _, lres = ds.b.Vectors(k)
            lerrest = O._converged("rel", re, im, lres * betat * norm2)
            margin = min(margin, abs(lerrest - tol) / tol)
            errest[k] = max(errest[k], lerrest)
            if marker == -1 and lerrest >= tol:
                marker = k
            if newk == k + 1:
                errest[k + 1] = errest[k]; k += 1
            if marker != -1:
                break
            k += 1
        k = marker if marker != -1 else nv
        if k >= nev:
            reason = 1
        elif its >= max_it:
            reason = -1
        if reason != 0 or breakdown or k == nv:
            l = 0
        else:
            l = max(1, int((nv - k) * keep))
            l = ds.GetTruncateSize(k, nv, l)
        if not lock and l > 0:
            l += k; k = 0
        V.SetActiveColumns(nconv, nv); W.SetActiveColumns(nconv, nv)
        V.MultInPlace(ds.a.Q[:nv, :nv], nconv, k + l)
        W.MultInPlace(ds.b.Q[:nv, :nv], nconv, k + l)
        if reason == 0 and not breakdown:
            V.CopyColumn(nv, k + l); W.CopyColumn(nv, k + l)
        if reason == 0:
            if breakdown or k == nv:
                if k < nev:
                    b1 = start_vector(V, k, None, seed); b2 = start_vector(W, k, None, (seed ^ LEFT_SEED_XOR) & 0xFFFFFFFFFFFFFFFF)
                    if b1 or b2:
                        reason = -2
            else:
                ds.SetDimensions(ds.a.n, k, ds.a.k)
                ds.Truncate(k + l, False)
            # EPSTwoSidedRQUpdate2 with the column loop from the old nconv
            kk = k + l
            V.SetActiveColumns(0, nv); W.SetActiveColumns(0, nv)
            for bv, h in ((V, ds.a), (W, ds.b)):
                c, nrm, _ = bv.OrthogonalizeColumn(kk)
                bv.ScaleColumn(kk, 1.0 / nrm)
                for j in range(nconv, kk):
                    h.A[:kk, j] += c[:kk] * h.A[kk, j]
                    h.A[kk, j] *= nrm
            M[:nv, :nv] = ds.b.Q[:nv, :nv].T @ (M[:nv, :nv] @ ds.a.Q[:nv, :nv])
            V.SetActiveColumns(nconv, nv); W.SetActiveColumns(nconv, nv)
        nconv = k
    ds.Truncate(nconv, True)
    # EPSComputeVectors_Schur, both sides: eigenvectors of the trimmed T and S without back-transformation
    V.SetActiveColumns(0, nconv); W.SetActiveColumns(0, nconv)
    for bv, h in ((V, ds.a), (W, ds.b)):
        h.state = O.DS_STATE_RAW
        Qsave = h.Q.copy(); h.Q[:, :] = np.eye(h.ld)
        Z = np.asfortranarray(h.VectorsAll().copy()) if nconv else None
        h.Q[:, :] = Qsave
        if nconv:
            bv.MultInPlace(Z, 0, nconv)
    eigr[:nconv] += sigma
    X = V.dense()[:, :nconv].copy(); Y = W.dense()[:, :nconv].copy()
    i = 0
    while i < nconv:                                   # BVNormalize(W, eigi), then y = wr - i wi for a pair (epsdefault.c:158-166)
        if eigi[i] != 0.0 and i + 1 < nconv:
            nrm = np.hypot(np.linalg.norm(Y[:, i]), np.linalg.norm(Y[:, i + 1]))
            Y[:, i] /= nrm; Y[:, i + 1] /= nrm
            if eigi[i] > 0.0:
                Y[:, i + 1] *= -1.0
            i += 2
        else:
            Y[:, i] /= np.linalg.norm(Y[:, i]); i += 1
    # final sort keeping pairs together (slepcsc.c:89-140); STSHIFT keeps the positive imaginary part first
    perm = list(range(nconv))
    i = nconv - 1
    while i >= 0:
        re = eigr[perm[i]]; im = eigi[perm[i]]
        j = i + 1
        if im != 0:
            i -= 1
            im = eigi[perm[i]]
        while j < nconv:
            if compare(re, im, eigr[perm[j]], eigi[perm[j]]) <= 0:
                break
            if not im:
                if eigi[perm[j]] == 0.0:
                    perm[j - 1], perm[j] = perm[j], perm[j - 1]; j += 1
                else:
                    tmp = perm[j - 1]; perm[j - 1] = perm[j]; perm[j] = perm[j + 1]; perm[j + 1] = tmp; j += 2
            else:
                if eigi[perm[j]] == 0.0:
                    tmp = perm[j - 2]; perm[j - 2] = perm[j]; perm[j] = perm[j - 1]; perm[j - 1] = tmp; j += 1
                else:
                    perm[j - 2], perm[j] = perm[j], perm[j - 2]
                    perm[j - 1], perm[j + 1] = perm[j + 1], perm[j - 1]; j += 2
        i -= 1
    res = TwoSidedResult()
    res.nconv = nconv; res.its = its; res.reason = reason; res.steps = steps; res.ncv = ncv
    res.eigr = eigr[:nconv].copy(); res.eigi = eigi[:nconv].copy(); res.perm = np.array(perm, dtype=np.int64)
    res.X, res.Y = X, Y
    res.permuted_at = permuted_at; res.margin = margin
    res.passes = V.passes_total() + W.passes_total()
    return res


def residuals(S, kr, ki, xr, xi, left=False):
    """ComputeResidualNorm of ex41.c:239-271, with the transposed product for the left vector. For a conjugate pair the left vector the
    solver returns satisfies y^H A = k y^H, that is A^T conj(y) = k conj(y): ex41's formula is applied to conj(y) = yr - i yi (what
    EPSComputeResidualNorm_Private does with its -ki, epssolve.c:705,711). ex41 itself only meets real eigenvalues."""
    Sm = S.T if left else S
    if ki == 0 or abs(ki) < abs(kr * np.finfo(float).eps):
        return np.linalg.norm(Sm @ xr - kr * xr)
    if left:
        xi = -xi
    nr = np.linalg.norm(Sm @ xr - kr * xr + ki * xi)
    ni = np.linalg.norm(Sm @ xi - kr * xi - ki * xr)
    return np.hypot(nr, ni)
