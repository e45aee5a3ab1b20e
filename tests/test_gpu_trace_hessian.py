"""GPU: termTraceHessian (one launch of curv_kernel's HJ_CURV_TRACE mode, csrc/hj_curv.h) and termDiscount against the NumPy
restatement of tests/trace_hess_ref.py, and by behaviour: the heat equation, anisotropic covariance growth, discounted decay.

Tolerances follow test_gpu_curvature.py.  fp64: the kernel evaluates the restatement's expressions in its order with
contraction off -- checked at 1e-12 x max|out|.  fp32: the kernel's arithmetic in single precision against the fp64 restatement
of the SAME fp32-rounded input and matrices; ydot sums products of a second derivative with an entry of L and one of R, so the
second-derivative bound of that file (1e-5 x max|out| + 16 eps32 max|phi| sum_i dx_i^-2) is scaled by sum_ikm |L_im| |R_ki|."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trace_hess_ref as TR              # noqa: E402
import levelsetpy_amd as L               # noqa: E402
from oracle import hj_oracle as O        # noqa: E402
from test_gpu_curvature import CASES, EPS32, _grids, _phi, _np, _close64, _dx_sum   # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dense(nd, shift):
    """A fixed non-symmetric nd x nd matrix."""
    return np.array([[(1.0 + 0.1 * i) if i == j else 0.15 * (i - j) + 0.05 * shift * (i + 2 * j + 1) for j in range(nd)]
                     for i in range(nd)])


def _mixed_cells(og):
    """L and R as cell matrices mixing array, scalar and zero entries."""
    nd = og.dim
    x = og.xs
    Lc = [[(1 + 0.3 * np.sin(x[i] + j)) if (i + j) % 2 == 0 else (0.0 if i < j else 0.4) for j in range(nd)] for i in range(nd)]
    Rc = [[(0.8 + 0.2 * np.cos(x[j] * (i + 1))) if i == j else (-0.25 if i > j else 0.1 * x[0]) for j in range(nd)]
          for i in range(nd)]
    return Lc, Rc


def _to_tensor_cells(M):
    return [[torch.as_tensor(e, device="cuda") if isinstance(e, np.ndarray) else e for e in row] for row in M]


def _forms(og):
    """(name, L, R for termTraceHessian, L, R for the restatement, every entry scalar?)."""
    nd = og.dim
    Ld, Rd = _dense(nd, 1), _dense(nd, -1)
    Lc, Rc = _mixed_cells(og)
    return [("dense", Ld, Rd, Ld, Rd, True),
            ("cell", Lc, Rc, Lc, Rc, False),
            ("callable", lambda t, d, sd: Ld * (1 + t), lambda t, d, sd: Rc, Ld * 1.5, Rc, False),
            ("tensor entries", _to_tensor_cells(Lc), _to_tensor_cells(Rc), Lc, Rc, False)]


def _sd(g, Lm, Rm, hessianFunc=None):
    return L.Bundle(dict(grid=g, hessianFunc=hessianFunc or L.hessianSecond, L=Lm, R=Rm))


@pytest.mark.parametrize("N,periodic,tz", CASES)
def test_trace_hessian_matches_restatement_fp64(N, periodic, tz):
    g, og = _grids(N, periodic, tz)
    phi = _phi(og)
    for name, Lg, Rg, Lw, Rw, _ in _forms(og):
        want, sb_want = TR.term_trace_hessian(og, phi, Lw, Rw)
        # NumPy data and device data (NumPy entries with tensor data included)
        for y in (phi.reshape(-1, 1), torch.as_tensor(phi.reshape(-1, 1), device="cuda")):
            sd = _sd(g, Lg, Rg)
            ydot, sb, sd2 = L.termTraceHessian(0.5, y, sd)
            assert sd2 is sd and type(ydot) is type(y) and tuple(ydot.shape) == want.shape, name
            _close64(ydot, want)
            assert abs(sb - sb_want) <= 1e-12 * sb_want, (name, sb, sb_want)


def _round32(M, scalars):
    """The entries the fp32 launch reads: arrays in fp32; scalar entries too when some entry is an array (the launch then
    forms the bound's trace in double from the fp32 entries; with every entry a scalar the host forms it from the doubles)."""
    return [[np.asarray(e, dtype=np.float32).astype(np.float64) if isinstance(e, np.ndarray) or scalars else e for e in row]
            for row in M]


def _abs_scale(Lw, Rw):
    Lm = [[float(np.max(np.abs(e))) for e in row] for row in Lw]
    Rm = [[float(np.max(np.abs(e))) for e in row] for row in Rw]
    n = len(Lm)
    return sum(Lm[i][m] * Rm[k][i] for i in range(n) for k in range(n) for m in range(n))


@pytest.mark.parametrize("N,periodic,tz", [CASES[0], CASES[5], CASES[9], CASES[12]])
def test_trace_hessian_matches_restatement_fp32(N, periodic, tz):
    g, og = _grids(N, periodic, tz)
    phi = _phi(og).astype(np.float32).astype(np.float64)
    y = torch.as_tensor(phi.reshape(-1, 1), device="cuda", dtype=torch.float32)
    for name, Lg, Rg, Lw, Rw, all_scalar in _forms(og)[:2]:
        Lw, Rw = _round32(Lw, not all_scalar), _round32(Rw, not all_scalar)
        want, sb_want = TR.term_trace_hessian(og, phi, Lw, Rw)
        ydot, sb, _ = L.termTraceHessian(0.0, y, _sd(g, Lg, Rg))
        assert ydot.dtype == torch.float32
        tol = 1e-5 * float(np.abs(want).max()) + 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) * _abs_scale(Lw, Rw)
        err = float(np.abs(_np(ydot).astype(np.float64) - want).max())
        assert err <= tol, (name, err, tol)
        assert abs(sb - sb_want) <= 1e-12 * sb_want, (name, sb, sb_want)


def test_identity_matrices_give_the_laplacian():
    for N, periodic, tz in (CASES[1], CASES[6], CASES[10], CASES[12]):
        g, og = _grids(N, periodic, tz)
        y = torch.as_tensor(_phi(og), device="cuda")
        ident = np.eye(len(N))
        ydot, _, _ = L.termTraceHessian(0.0, y.reshape(-1, 1), _sd(g, ident, ident))
        lap = L.laplacianSecond(g, y)
        assert float((ydot.reshape(lap.shape) - lap).abs().max()) <= 1e-12 * float(lap.abs().max())


def test_one_launch_equals_the_array_path_on_tensors():
    g, og = _grids((21, 23, 25), (1,), (2,))
    y = torch.as_tensor(_phi(og).reshape(-1, 1), device="cuda")
    Lc, Rc = _mixed_cells(og)
    Lt, Rt = _to_tensor_cells(Lc), _to_tensor_cells(Rc)

    def wrapped(grid, data):                 # not hessianSecond itself: the array path
        return L.hessianSecond(grid, data)
    a, sa, _ = L.termTraceHessian(0.0, y, _sd(g, Lt, Rt))
    b, sb, _ = L.termTraceHessian(0.0, y, _sd(g, Lt, Rt, hessianFunc=wrapped))
    assert torch.is_tensor(b) and b.is_cuda
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert abs(sa - sb) <= 1e-12 * sb


def _heat(nd, n, s, tf, lam=None, numpy=False):
    """phi_t = Laplacian(phi) (- lam phi) from a Gaussian on [-2, 2]^nd under odeCFL3: (grid, phi(tf), t)."""
    lo, hi = [-2.0] * nd, [2.0] * nd
    g = L.createGrid(np.array(lo).reshape(-1, 1), np.array(hi).reshape(-1, 1), n * np.ones((nd, 1), dtype=np.int64))
    og = O.Grid(lo, hi, [n] * nd)
    y0 = np.exp(-sum(x ** 2 for x in og.xs) / (2 * s * s)).reshape(-1, 1)
    ident = np.eye(nd)
    sdT = _sd(g, ident, ident)
    if lam is None:
        f, sd = L.termTraceHessian, sdT
    else:
        f = L.termSum
        sd = L.Bundle(dict(innerFunc=[L.termTraceHessian, L.termDiscount], innerData=[sdT, L.Bundle(dict(grid=g, lambder=lam))]))
    op = L.odeCFLset(L.Bundle(dict(factorCFL=0.5)))
    t, y, _ = L.odeCFL3(f, [0.0, tf], y0 if numpy else torch.as_tensor(y0, device="cuda"), op, sd)
    return og, y, t


def _gauss(og, s, t):
    v = s * s + 2 * t
    return (s * s / v) ** (og.dim / 2) * np.exp(-sum(x ** 2 for x in og.xs) / (2 * v))


@pytest.mark.parametrize("nd,ns,s", [(2, (41, 81), 0.3), (3, (21, 41), 0.4)])
def test_heat_equation_converges(nd, ns, s):
    """A Gaussian under phi_t = trace(I D^2phi I): the max error against the exact solution drops ~4x (second order) when
    N - 1 doubles; at least 3x is required (the restatement integrated the same way drops 4.04x / 4.07x)."""
    tf = 0.05
    errs = []
    for n in ns:
        og, y, t = _heat(nd, n, s, tf)
        assert torch.is_tensor(y) and y.is_cuda and abs(t - tf) < 1e-12
        errs.append(float(np.abs(_np(y).reshape(og.shape) - _gauss(og, s, tf)).max()))
    assert errs[0] / errs[1] >= 3.0, errs


def test_anisotropic_diffusion_grows_the_covariance():
    """L = sigma, R = sigma^T: phi_t = sum_ij (sigma^T sigma)_ij phi_ij, so a normalised Gaussian's covariance grows as
    Sigma(t) = Sigma0 + 2 sigma^T sigma t.  Centred differences conserve the second moments exactly in the interior; the
    restatement integrated the same way lands within 5e-8."""
    sig = np.array([[0.6, 0.2], [-0.1, 0.4]])
    S0 = np.array([[0.2, 0.05], [0.05, 0.12]])
    n, tf = 121, 0.1
    g = L.createGrid(-3 * np.ones((2, 1)), 3 * np.ones((2, 1)), n * np.ones((2, 1), dtype=np.int64))
    og = O.Grid([-3.0] * 2, [3.0] * 2, [n] * 2)
    X = np.stack(og.xs).reshape(2, -1)
    y0 = np.exp(-0.5 * np.einsum('ik,ij,jk->k', X, np.linalg.inv(S0), X)).reshape(-1, 1)
    op = L.odeCFLset(L.Bundle(dict(factorCFL=0.5)))
    t, y, _ = L.odeCFL3(L.termTraceHessian, [0.0, tf], torch.as_tensor(y0, device="cuda"), op, _sd(g, sig, sig.T))
    assert torch.is_tensor(y) and abs(t - tf) < 1e-12
    w = _np(y).ravel()
    mu = X @ w / w.sum()
    cov = (X * w) @ X.T / w.sum() - np.outer(mu, mu)
    assert np.abs(cov - (S0 + 2 * sig.T @ sig * tf)).max() <= 1e-6, cov


def test_discount_scales_the_heat_solution():
    """termSum(termTraceHessian, termDiscount(lambda)): phi_t = Laplacian(phi) - lambda phi is e^{-lambda t} times the heat
    solution; on the device, and equal to the NumPy-input run."""
    lam, s, tf = 2.0, 0.3, 0.05
    og, yh, _ = _heat(2, 61, s, tf)
    _, yd, td = _heat(2, 61, s, tf, lam=lam)
    assert torch.is_tensor(yd) and yd.is_cuda and yd.dtype == torch.float64 and abs(td - tf) < 1e-12
    ref = np.exp(-lam * tf) * _np(yh)
    # not to rounding: RK3's stability polynomial of (A - lambda) differs from e^{-lambda dt} times that of A by O(lambda dt)
    # times the highest modes' terms (2.2e-8 of max|phi| here); a discount that is missing or of the wrong sign is off by 10-20 %
    assert float(np.abs(_np(yd) - ref).max()) <= 1e-6 * float(np.abs(ref).max())
    assert float(np.abs(_np(yd).reshape(og.shape) - np.exp(-lam * tf) * _gauss(og, s, tf)).max()) <= 2e-3
    _, yn, tn = _heat(2, 61, s, tf, lam=lam, numpy=True)
    assert abs(tn - td) <= 1e-14
    np.testing.assert_allclose(np.asarray(yn), _np(yd), rtol=0, atol=1e-12)


def test_term_discount_on_the_device():
    g, og = _grids((37, 41), (1,), ())
    phi = _phi(og)
    lam = 0.5 + 0.25 * np.cos(og.xs[0])
    y = torch.as_tensor(phi.reshape(-1, 1), device="cuda")
    for lambder in (0.75, lam, torch.as_tensor(lam, device="cuda"), lambda t, d, sd: lam):
        ydot, sb, _ = L.termDiscount(0.0, y, L.Bundle(dict(grid=g, lambder=lambder)))
        assert torch.is_tensor(ydot) and ydot.is_cuda and tuple(ydot.shape) == (phi.size, 1) and sb == float('inf')
        want, _ = TR.term_discount(phi, 0.75 if isinstance(lambder, float) else lam)
        np.testing.assert_array_equal(_np(ydot), want)


def test_large_grid_per_node_matrices_fp64():
    """201^3 fp64 (8 M cells) with per-node L and R (the in-kernel reduction of the step bound)."""
    n = 201
    g, og = _grids((n, n, n), (2,), ())
    phi = _phi(og)
    x = og.xs
    Lc = [[1 + 0.2 * np.sin(x[0]), 0.0, 0.3], [0.1, 1.0, 0.0], [0.0, -0.2, 0.9 + 0.1 * x[2]]]
    Rc = [[0.8, 0.2 * np.cos(x[1]), 0.0], [0.0, 1.1, 0.0], [0.25, 0.0, 1.0]]
    want, sb_want = TR.term_trace_hessian(og, phi, Lc, Rc)
    y = torch.as_tensor(phi.reshape(-1, 1), device="cuda")
    ydot, sb, _ = L.termTraceHessian(0.0, y, _sd(g, _to_tensor_cells(Lc), _to_tensor_cells(Rc)))
    _close64(ydot, want)
    assert abs(sb - sb_want) <= 1e-12 * sb_want


def test_c_abi_refuses_aliasing_and_null_arguments():
    from levelsetpy_amd.context import device_grid
    g, og = _grids((37, 41), (), ())
    dg = device_grid(g, "float64")
    y = torch.as_tensor(_phi(og), device="cuda")
    a = torch.ones_like(y)
    out = torch.empty_like(y)
    lib = dg.lib
    nn = 4
    ptrs = (C.c_void_p * nn)(a.data_ptr(), None, None, None)
    scal = (C.c_double * nn)(0.0, 0.5, 0.5, 1.0)
    sb = C.c_double()
    call = lambda yp, op, Lp=ptrs, Ls=scal, Rp=None, Rs=scal: lib.hj_term_trace_hessian(  # noqa: E731
        dg.ctx, yp, Lp, Ls, Rp, Rs, op, C.byref(sb))
    assert call(y.data_ptr(), out.data_ptr()) == 0
    assert call(y.data_ptr(), y.data_ptr()) == -1              # ydot aliases y
    assert call(y.data_ptr(), a.data_ptr()) == -1              # ydot aliases an entry of L
    assert call(None, out.data_ptr()) == -1                    # null y
    assert call(y.data_ptr(), None) == -1                      # null ydot
    assert call(y.data_ptr(), out.data_ptr(), Ls=None) == -1   # a scalar entry of L without scalars
    assert lib.hj_term_trace_hessian(None, y.data_ptr(), None, scal, None, scal, out.data_ptr(), C.byref(sb)) == -1
    dg.sync()
