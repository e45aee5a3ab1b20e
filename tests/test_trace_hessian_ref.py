"""CPU: the NumPy restatement of termTraceHessian / termDiscount (tests/trace_hess_ref.py) against closed forms, the array path
of termTraceHessian (a foreign hessianFunc: pure NumPy, no GPU) against the restatement, the cell-matrix helpers, termDiscount
on NumPy arrays, argument errors and the C ABI of the new entry point.  The one-launch path is checked against the
restatement in test_gpu_trace_hessian.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import curvature_ref as CR               # noqa: E402
import trace_hess_ref as TR              # noqa: E402
import levelsetpy_amd as L               # noqa: E402
from levelsetpy_amd import _ffi          # noqa: E402
from oracle import hj_oracle as O        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER = (slice(1, -1),) * 3
Q = np.array([[2.0, -0.6, 0.3], [-0.6, 1.5, 0.4], [0.3, 0.4, 3.0]])
LM = np.array([[1.0, 0.5, 0.0], [-0.3, 2.0, 0.7], [0.2, 0.0, 0.8]])     # not symmetric
RM = np.array([[0.9, 0.0, 0.4], [0.6, 1.1, 0.0], [-0.5, 0.3, 1.2]])     # not L^T


def _grid3():
    return O.Grid([-1, -2, -1.5], [1, 1, 1], [11, 13, 12], pd_dims=[1])


def _quadratic(g):
    x = np.stack(g.xs)
    c = np.array([1.0, -1.0, 0.5])
    return 0.5 * np.einsum('i...,ij,j...->...', x, Q, x) + np.einsum('i,i...->...', c, x)


def _sd(g, Lm, Rm, hessianFunc=CR.hessian_second, **kw):
    return L.Bundle(dict(grid=g, hessianFunc=hessianFunc, L=Lm, R=Rm, **kw))


def test_closed_form_constant_matrices():
    """The centred Hessian of a quadratic is exact in the interior: trace(L D^2phi R) = trace(L Q R) there."""
    g = _grid3()
    ydot, _ = TR.term_trace_hessian(g, _quadratic(g), LM, RM)
    np.testing.assert_allclose(ydot.reshape(g.shape)[INNER], np.trace(LM @ Q @ RM), rtol=0, atol=1e-11)


def test_closed_form_per_node_matrices():
    g = _grid3()
    x, y, z = g.xs
    Lx = [[LM[i, j] * (1 + 0.3 * np.sin(x + j)) for j in range(3)] for i in range(3)]
    Rx = [[RM[i, j] + 0.2 * np.cos(y * (i + 1)) * z for j in range(3)] for i in range(3)]
    ydot, _ = TR.term_trace_hessian(g, _quadratic(g), Lx, Rx)
    Lx_, Rx_ = np.array(Lx), np.array(Rx)           # (3, 3) + grid shape
    want = np.einsum('ik...,kj,ji...->...', Lx_, Q, Rx_)
    np.testing.assert_allclose(ydot.reshape(g.shape)[INNER], want[INNER], rtol=0, atol=1e-11)


def test_order_of_l_and_r_matters():
    """tr(L P R) != tr(R P L) for a non-symmetric L with R != L^T: a swap of L and R is caught."""
    g = _grid3()
    a, b = np.trace(LM @ Q @ RM), np.trace(RM @ Q @ LM)
    assert abs(a - b) > 0.1
    ydot, _ = TR.term_trace_hessian(g, _quadratic(g), LM, RM)
    swapped, _ = TR.term_trace_hessian(g, _quadratic(g), RM, LM)
    np.testing.assert_allclose(swapped.reshape(g.shape)[INNER], b, atol=1e-11)
    got, _, _ = L.termTraceHessian(0.0, _quadratic(g).reshape(-1, 1), _sd(g, LM, RM))
    np.testing.assert_allclose(got.reshape(g.shape)[INNER], a, atol=1e-11)
    assert float(np.abs(got - swapped).max()) > 0.1


def test_step_bound_closed_form():
    g = O.Grid([0, 0], [1, 2], [11, 21])           # dx = 0.1, 0.1
    ident = np.eye(2)
    assert np.isclose(TR.step_bound(g, TR.as_cell(ident, 2), TR.as_cell(ident, 2)), 1 / (2 * 200.0), rtol=1e-14)
    # L = R = diag(s): trace(L D R) = sum_i s_i^2 / dx_i^2
    s = np.diag([2.0, 0.5])
    assert np.isclose(TR.step_bound(g, TR.as_cell(s, 2), TR.as_cell(s, 2)), 1 / (2 * (400.0 + 25.0)), rtol=1e-14)
    zero = np.zeros((2, 2))
    assert TR.step_bound(g, TR.as_cell(zero, 2), TR.as_cell(ident, 2)) == float('inf')


def _rand_cell(rng, n, m, shape):
    return [[rng.standard_normal(shape) for _ in range(m)] for _ in range(n)]


def test_cell_matrix_multiply_and_trace_match_einsum():
    rng = np.random.default_rng(5)
    shape = (4, 5)
    A, B = _rand_cell(rng, 2, 3, shape), _rand_cell(rng, 3, 2, shape)
    Cm = L.cellMatrixMultiply(A, B)
    want = np.einsum('ik...,kj...->ij...', np.array(A), np.array(B))
    assert len(Cm) == 2 and all(len(r) == 2 for r in Cm)
    np.testing.assert_allclose(np.array(Cm), want, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(L.cellMatrixTrace(Cm), np.einsum('ii...->...', want), rtol=1e-14, atol=1e-14)
    # scalar x cell, cell x scalar, array x cell, numeric x numeric
    np.testing.assert_array_equal(np.array(L.cellMatrixMultiply(2.5, A)), 2.5 * np.array(A))
    np.testing.assert_array_equal(np.array(L.cellMatrixMultiply(A, 2.5)), 2.5 * np.array(A))
    w = rng.standard_normal(shape)
    np.testing.assert_array_equal(np.array(L.cellMatrixMultiply(w, A)), w * np.array(A))
    np.testing.assert_array_equal(L.cellMatrixMultiply(w, w), w * w)
    assert L.cellMatrixMultiply(2.0, 3.0) == 6.0
    # mixed numbers and arrays inside a cell matrix
    M = [[1.0, w], [0.0, 2.0]]
    np.testing.assert_array_equal(L.cellMatrixTrace(L.cellMatrixMultiply(M, M)), 1.0 + 0.0 * w + 4.0)
    assert L.cellMatrixTrace(np.array([[1.0, 2.0], [3.0, 4.0]])) == 5.0


def test_cell_matrix_dimension_errors():
    rng = np.random.default_rng(6)
    A, B = _rand_cell(rng, 2, 3, (3,)), _rand_cell(rng, 2, 3, (3,))
    with pytest.raises(ValueError, match="Inner dimensions"):
        L.cellMatrixMultiply(A, B)
    with pytest.raises(ValueError, match="dimension 2"):
        L.cellMatrixMultiply([[1.0, 2.0], [3.0]], A)
    with pytest.raises(ValueError, match="square"):
        L.cellMatrixTrace(A)
    with pytest.raises(ValueError, match="numeric array or a cell"):
        L.cellMatrixMultiply(A, "x")
    with pytest.raises(ValueError, match="numeric array or a cell"):
        L.cellMatrixMultiply("x", A)


def _phi(g):
    r = np.sqrt(sum((x - 0.1 * (d + 1)) ** 2 for d, x in enumerate(g.xs)))
    return r - 0.5 + 0.2 * np.sin(2 * g.xs[0] + 1) * np.cos(3 * g.xs[-1] - 0.5) + 0.3 * g.xs[0] * g.xs[-1]


def _forms(g):
    """(name, L, R as given to termTraceHessian, L, R for the restatement)."""
    x = g.xs
    Lcell = [[1.0, 0.0, x[0] * 0.2 + 1], [0.5, np.cos(x[1]), 0.0], [0.0, -0.3, 2.0]]
    Rcell = [[np.exp(-x[2] ** 2), 0.1, 0.0], [0.0, 1.0, 0.4 * x[0]], [0.2, 0.0, 0.7]]
    return [("dense", LM, RM, LM, RM),
            ("nested list", LM.tolist(), RM.tolist(), LM, RM),
            ("cell", Lcell, Rcell, Lcell, Rcell),
            ("callable", lambda t, d, sd: LM * (1 + t), lambda t, d, sd: Rcell, LM * 1.5, Rcell)]


def test_array_path_equals_restatement_for_every_form():
    g = _grid3()
    phi = _phi(g)
    for name, Lg, Rg, Lw, Rw in _forms(g):
        want, sb_want = TR.term_trace_hessian(g, phi, Lw, Rw)
        sd = _sd(g, Lg, Rg)
        ydot, sb, sd2 = L.termTraceHessian(0.5, phi.reshape(-1, 1), sd)
        assert sd2 is sd and isinstance(ydot, np.ndarray) and ydot.shape == want.shape, name
        np.testing.assert_array_equal(ydot, want)
        assert sb == sb_want, (name, sb, sb_want)


def test_callable_matrices_receive_t_data_and_schemedata_l_first():
    g = _grid3()
    phi = _phi(g)
    calls = []

    def mk(tag, M):
        def f(t, data, sd):
            calls.append((tag, t, data, sd))
            return M
        return f
    sd = _sd(g, mk("L", LM), mk("R", RM), extra=7)
    y = [phi.reshape(-1, 1), np.zeros((phi.size, 1))]          # a vector level set: only y[0] is used
    ydot, _, _ = L.termTraceHessian(0.25, y, [sd, None])
    assert [c[0] for c in calls] == ["L", "R"]
    for _, t, data, s in calls:
        assert t == 0.25 and s is sd and data.shape == g.shape
        np.testing.assert_array_equal(data, phi)
    np.testing.assert_array_equal(ydot, TR.term_trace_hessian(g, phi, LM, RM)[0])


def test_array_path_one_dimension_scalar_matrices():
    g = O.Grid([-1], [1], [41])
    phi = np.sin(3 * g.xs[0]) + g.xs[0] ** 2
    ydot, sb, _ = L.termTraceHessian(0.0, phi.reshape(-1, 1), _sd(g, 0.5, 2.0))
    want, sb_want = TR.term_trace_hessian(g, phi, [[0.5]], [[2.0]])
    np.testing.assert_array_equal(ydot, want)
    assert sb == sb_want == 1 / (2 * float(g.dx[0, 0]) ** -2)


def test_term_discount_on_numpy():
    g = O.Grid([0, 0], [1, 1], [4, 5])
    y = np.arange(20.0).reshape(-1, 1)
    lam = np.linspace(0, 1, 20).reshape(4, 5)
    seen = []

    def lam_f(t, d, sd):
        seen.append((t, d.shape, sd))
        return lam * t
    for lambder, want in [(0.5, -0.5 * y), (lam, -(lam.reshape(-1, 1) * y)), (lam_f, -(lam.reshape(-1, 1) * 2.0 * y))]:
        sd = L.Bundle(dict(grid=g, lambder=lambder))
        ydot, sb, sd2 = L.termDiscount(2.0, y, sd)
        assert ydot.shape == (20, 1) and sb == float('inf') and sd2 is sd
        np.testing.assert_array_equal(ydot, want)
        np.testing.assert_array_equal(ydot, TR.term_discount(y.reshape(4, 5), lambder if not callable(lambder) else lam * 2.0)[0])
    assert seen == [(2.0, (4, 5), sd)]
    # a vector level set: only y[0]
    ydot, _, _ = L.termDiscount(0.0, [y, None], [L.Bundle(dict(grid=g, lambder=0.5))])
    np.testing.assert_array_equal(ydot, -0.5 * y)
    with pytest.raises(ValueError, match="lambder must be"):
        L.termDiscount(0.0, y, L.Bundle(dict(grid=g, lambder="x")))


def test_argument_errors():
    g = _grid3()
    y = _phi(g).reshape(-1, 1)
    for missing, msg in [("grid", "grid not in"), ("hessianFunc", "hessianFunc not in"), ("L", "L is not in"),
                         ("R", "R is not in")]:
        d = dict(grid=g, hessianFunc=CR.hessian_second, L=LM, R=RM)
        del d[missing]
        with pytest.raises(AssertionError, match=msg):
            L.termTraceHessian(0.0, y, L.Bundle(d))
    with pytest.raises(ValueError, match="3 x 3"):
        L.termTraceHessian(0.0, y, _sd(g, np.eye(2), RM))
    with pytest.raises(ValueError, match="3 x 3"):
        L.termTraceHessian(0.0, y, _sd(g, LM, [[1.0, 0.0, 0.0], [0.0, 1.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="Input matrix must be"):
        L.termTraceHessian(0.0, y, _sd(g, "eye", RM))
    with pytest.raises(ValueError, match="size of data"):
        L.termTraceHessian(0.0, y, _sd(g, [[np.ones(5), 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], RM))
    g2 = O.Grid([0, 0], [1, 1], [6, 7])
    with pytest.raises(ValueError, match="1 x 1"):
        L.termTraceHessian(0.0, np.zeros((42, 1)), _sd(g2, 1.0, np.eye(2)))
    for missing, msg in [("grid", "grid not in"), ("lambder", "lambder not in")]:
        d = dict(grid=g2, lambder=1.0)
        del d[missing]
        with pytest.raises(AssertionError, match=msg):
            L.termDiscount(0.0, np.zeros((42, 1)), L.Bundle(d))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "hj_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(hj_[a-z0-9_]+)\s*\(", txt))


def test_new_entry_point_is_in_header_ffi_and_library():
    assert "hj_term_trace_hessian" in _header_symbols()
    assert "hj_term_trace_hessian" in _ffi.SIGNATURES
    assert hasattr(_ffi.lib(), "hj_term_trace_hessian")


def test_new_entry_point_refuses_a_null_context():
    sb = C.c_double()
    assert _ffi.lib().hj_term_trace_hessian(None, None, None, None, None, None, None, C.byref(sb)) == -1


def test_package_exports_the_new_names():
    for name in ("termTraceHessian", "termDiscount", "cellMatrixMultiply", "cellMatrixTrace"):
        assert callable(getattr(L, name)), name
