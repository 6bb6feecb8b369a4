"""Transposed ST solves (ks_st_set_transpose_solves): STMatSolveTranspose and STApplyTranspose for every transformation with a solve, both KSPs on
their transposed side, all three preconditioners, both matrix modes.

The pencil is the 24 x 30 convection pencil at sigma = -0.5 of tests/test_gpu_pc_ilu.py (B its diagonal mass matrix), the KSP tolerance 1e-12. The
reference is STApplyTranspose_Generic (stsolve.c:107-116) restated with scipy's sparse LU of P^T:
    sinvert  y = B^T P^-T x      cayley  y = (A + nu B)^T P^-T x      shift, two matrices  y = (A - sigma B)^T B^-T x
and the bound 1e-9 ||ref||, the forward test's bound at the same rtol on the same pencil."""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

import ilu_cases as ic
import ilu_transpose_cases as itc

pytestmark = pytest.mark.gpu
NX, NY, SIGMA, NU = 24, 30, -0.5, 2.0
PCS = [("jacobi", 0, "shell"), ("bjacobi", 4, "shell"), ("bjacobi-ilu", 4 * NX, "shell"), ("bjacobi-ilu", 64, "copy")]


class Pencil:
    def __init__(self):
        self.Sa, self.Sb = ic.line_pencil(NX, NY)
        self.n = NX * NY
        rng = np.random.default_rng(21)
        self.x = rng.standard_normal(self.n); self.y = rng.standard_normal(self.n)
        self.P = {"sinvert": ic.shifted(self.Sa, SIGMA, self.Sb), "cayley": ic.shifted(self.Sa, SIGMA, self.Sb), "shift": self.Sb.tocsr()}
        self.M = {"sinvert": self.Sb, "cayley": (self.Sa + NU * self.Sb).tocsr(), "shift": ic.shifted(self.Sa, SIGMA, self.Sb)}
        self.lu_t = {k: spl.splu(P.T.tocsc()) for k, P in self.P.items()}
        self.lu = {k: spl.splu(P.tocsc()) for k, P in self.P.items()}

    def solve_t(self, kind, b):
        return self.lu_t[kind].solve(b)

    def op_t(self, kind, x):
        return self.M[kind].T @ self.solve_t(kind, x)

    def op(self, kind, x):
        return self.lu[kind].solve(self.M[kind] @ x)


@pytest.fixture(scope="module")
def pencil():
    return Pencil()


@pytest.fixture(scope="module")
def mats(ctx, pencil):
    import slepc_amd as ks
    return (ks.Mat.from_csr(ctx, *ic.arrays(pencil.Sa), keep_csr=True), ks.Mat.from_csr(ctx, *ic.arrays(pencil.Sb), keep_csr=True))


def _st(ctx, mats, kind, ksp, pc, bs, mode, transpose=True):
    import slepc_amd as ks
    st = ks.ST(ctx)
    st.SetType(kind); st.SetShift(SIGMA); st.SetMatrices(*mats); st.SetMatMode(mode); st.SetPC(pc, bs); st.SetKSPType(ksp)
    if kind == "cayley":
        st.CayleySetAntishift(NU)
    st.SetKSP(rtol=1e-12); st.SetTransposeSolves(transpose)
    return st


@pytest.mark.parametrize("pc,bs,mode", PCS)
@pytest.mark.parametrize("ksp", ["gmres", "bcgs"])
@pytest.mark.parametrize("kind", ["sinvert", "cayley", "shift"])
def test_transposed_operator_and_solve_agree_with_the_lu_of_the_transpose(ctx, pencil, mats, kind, ksp, pc, bs, mode):
    st = _st(ctx, mats, kind, ksp, pc, bs, mode)
    x, y = pencil.x, pencil.y
    ref = pencil.op_t(kind, x)
    got = st.ApplyTranspose(x)
    print("%s %s %s/%d %s: ||Op^T x - ref|| / ||ref|| = %.2e" % (kind, ksp, pc, bs, mode, np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    assert np.linalg.norm(got - ref) <= 1e-9 * np.linalg.norm(ref)
    s0 = st.GetKSPStats()
    sol = pencil.solve_t(kind, x)
    assert np.linalg.norm(st.MatSolveTranspose(x) - sol) <= 1e-9 * np.linalg.norm(sol)
    s1 = st.GetKSPStats()
    assert s1["solves"] == s0["solves"] + 1 and s1["iterations"] > s0["iterations"]          # the statistics count both sides
    # y . (Op x) = (Op^T y) . x: a transposed factor applied in the wrong order passes no such test
    lhs = float(y @ st.Apply(x)); rhs = float(st.ApplyTranspose(y) @ x)
    assert abs(lhs - rhs) <= 1e-9 * np.linalg.norm(x) * np.linalg.norm(y), (lhs, rhs)
    fwd = pencil.op(kind, x)
    assert np.linalg.norm(st.Apply(x) - fwd) <= 1e-9 * np.linalg.norm(fwd)                  # the forward side beside it


def test_the_switch_off_refuses_as_before(ctx, pencil, mats):
    import slepc_amd as ks
    for kind in ("sinvert", "cayley", "shift"):
        st = _st(ctx, mats, kind, "gmres", "jacobi", 0, "shell", transpose=False)
        with pytest.raises(ks.KsError) as e:
            st.ApplyTranspose(pencil.x)
        assert e.value.rc == 56 and "ks_st_set_transpose_solves" in str(e.value)
        fwd = pencil.op(kind, pencil.x)
        assert np.linalg.norm(st.Apply(pencil.x) - fwd) <= 1e-9 * np.linalg.norm(fwd)
    # switching on clears the set-up; switching off again refuses again
    st.SetTransposeSolves(True)
    ref = pencil.op_t("shift", pencil.x)
    assert np.linalg.norm(st.ApplyTranspose(pencil.x) - ref) <= 1e-9 * np.linalg.norm(ref)
    st.SetTransposeSolves(False)
    with pytest.raises(ks.KsError) as e:
        st.ApplyTranspose(pencil.x)
    assert e.value.rc == 56


def test_one_matrix(ctx, pencil):
    """sinvert: y = P^-T x; cayley with B = I: y = (A + nu I)^T P^-T x"""
    import scipy.sparse as sp
    import slepc_amd as ks
    A = ks.Mat.from_csr(ctx, *ic.arrays(pencil.Sa), keep_csr=True)
    P = ic.shifted(pencil.Sa, SIGMA)
    lu_t = spl.splu(P.T.tocsc())
    for kind, M in (("sinvert", sp.identity(pencil.n)), ("cayley", pencil.Sa + NU * sp.identity(pencil.n))):
        st = _st(ctx, (A, None), kind, "gmres", "bjacobi-ilu", 96, "shell")
        ref = M.T @ lu_t.solve(pencil.x)
        assert np.linalg.norm(st.ApplyTranspose(pencil.x) - ref) <= 1e-9 * np.linalg.norm(ref), kind


def _cpu_gmres_iterations(Pt, minv_t, b, rtol, restart=30):
    """The transposed inner solve restated with scipy: GMRES(30) on M^-T P^T y = M^-T b, zero guess, relative tolerance on the preconditioned residual."""
    n = Pt.shape[0]
    its = [0]

    def count(_):
        its[0] += 1
    _, info = spl.gmres(spl.LinearOperator((n, n), matvec=lambda v: minv_t(Pt @ v)), minv_t(b), rtol=rtol, atol=0.0, restart=restart, maxiter=1000,
                        callback=count, callback_type="pr_norm")
    assert info == 0
    return its[0]


def test_ilu_blocks_take_fewer_iterations_than_point_jacobi_on_the_transposed_side(ctx, pencil, mats):
    """Restated on the CPU with scipy's GMRES(30) on the transposed system, point Jacobi takes 26 iterations and the ILU(0) blocks of four grid
    lines 10: a gap far above the 1.5 below which the comparison on the device would not be asserted."""
    P = pencil.P["sinvert"]
    Pt = P.T.tocsr()
    d = P.diagonal()
    ref = ic.Reference.of(P, 4 * NX)
    cpu = {"jacobi": _cpu_gmres_iterations(Pt, lambda v: v / d, pencil.x, 1e-12), "ilu": _cpu_gmres_iterations(Pt, lambda v: itc.solve_t(ref, v), pencil.x, 1e-12)}
    print("CPU restatement:", cpu)
    assert cpu["jacobi"] >= 1.5 * cpu["ilu"], cpu
    sol = pencil.solve_t("sinvert", pencil.x)
    its = {}
    for label, pc, bs in (("jacobi", "jacobi", 0), ("ilu", "bjacobi-ilu", 4 * NX)):
        st = _st(ctx, mats, "sinvert", "gmres", pc, bs, "shell")
        y = st.MatSolveTranspose(pencil.x)
        assert np.linalg.norm(y - sol) <= 1e-9 * np.linalg.norm(sol)
        its[label] = st.GetKSPStats()["iterations"]
    print("GPU:", its)
    assert its["ilu"] < its["jacobi"], (its, cpu)
