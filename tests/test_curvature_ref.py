"""CPU: the NumPy restatement of the second-order derivatives (tests/curvature_ref.py) against closed forms, what the
shipped mixed-partial loop bound loses, and the C ABI of the new entry points.  The GPU kernels are checked against this
restatement in test_gpu_curvature.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import curvature_ref as R                # noqa: E402
import levelsetpy_amd as L               # noqa: E402
from levelsetpy_amd import _ffi          # noqa: E402
from oracle import hj_oracle as O        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hj_term_curvature", "hj_curvature_second", "hj_hessian_second", "hj_laplacian_second", "hj_centered_first_second"]


def _radius(g):
    return np.sqrt(sum(x ** 2 for x in g.xs))


def _inv(r):
    return np.divide(1.0, r, out=np.full_like(r, np.inf), where=r > 0)


@pytest.mark.parametrize("n", [101, 201])
def test_circle_curvature_is_one_over_r(n):
    """Every level set of a circle's signed distance is a circle: kappa = 1/r, |grad phi| = 1.  Centred second-order
    differences: the error is C dx^2 with C ~ max 1/r^3 over the band (r >= 0.2: 125), observed ~30 dx^2 at both sizes."""
    g = O.Grid([-1, -1], [1, 1], [n, n])
    r = _radius(g)
    k, m = R.curvature_second(g, r - 0.5)
    band = (r > 0.2) & (r < 0.8)
    dx2 = float(g.dx[0, 0]) ** 2
    assert np.abs(k - _inv(r))[band].max() <= 40 * dx2
    assert np.abs(m - 1)[band].max() <= 10 * dx2


def test_circle_curvature_converges_at_second_order():
    """Max error over the band r in (0.3, 0.8) at n = 101, 201, 401: each halving of dx divides it by ~4."""
    errs = []
    for n in (101, 201, 401):
        g = O.Grid([-1, -1], [1, 1], [n, n])
        r = _radius(g)
        k, _ = R.curvature_second(g, r - 0.5)
        band = (r > 0.3) & (r < 0.8)
        errs.append(np.abs(k - _inv(r))[band].max())
    assert 3.7 < errs[0] / errs[1] < 4.3 and 3.7 < errs[1] / errs[2] < 4.3, errs


def test_sphere_curvature_is_two_over_r():
    g = O.Grid([-1] * 3, [1] * 3, [61] * 3)
    r = _radius(g)
    k, m = R.curvature_second(g, r - 0.5)
    band = (r > 0.3) & (r < 0.8)
    dx2 = float(g.dx[0, 0]) ** 2
    assert np.abs(k - 2 * _inv(r))[band].max() <= 40 * dx2
    assert np.abs(m - 1)[band].max() <= 10 * dx2


def test_quadratic_has_an_exact_hessian():
    """Centred differences are exact on quadratics: in the interior every second partial, mixed ones included, is the
    constant coefficient to rounding, and the first partials are the exact gradient (one axis periodic: only the ghost
    cells differ, and the interior does not read them)."""
    g = O.Grid([-1, -2, -1.5], [1, 1, 1], [11, 13, 12], pd_dims=[1])
    x, y, z = g.xs
    phi = 1.5 * x * x - 0.7 * x * y + 0.3 * y * z + 2 * z * z - 0.4 * x * z + x - y
    s, f = R.hessian_second(g, phi)
    inner = (slice(1, -1),) * 3
    H = [[3.0], [-0.7, 0.0], [-0.4, 0.3, 4.0]]
    for i in range(3):
        for j in range(i + 1):
            np.testing.assert_allclose(s[i][j][inner], H[i][j], atol=1e-12)
        for j in range(i + 1, 3):
            assert s[i][j] is None
    grad = [3 * x - 0.7 * y - 0.4 * z + 1, -0.7 * x + 0.3 * z - 1, 0.3 * y + 4 * z - 0.4 * x]
    for i in range(3):
        np.testing.assert_allclose(f[i][inner], grad[i][inner], atol=1e-12)
    np.testing.assert_allclose(R.laplacian_second(g, phi)[inner], 7.0, atol=1e-12)
    for d in range(3):
        np.testing.assert_allclose(R.centered_first_second(g, phi, d)[inner], grad[d][inner], atol=1e-12)


def _rotated_ellipse(n):
    g = O.Grid([-1, -1], [1, 1], [n, n])
    th = np.pi / 6
    u = np.cos(th) * g.xs[0] + np.sin(th) * g.xs[1]
    v = -np.sin(th) * g.xs[0] + np.cos(th) * g.xs[1]
    return g, (u / 0.8) ** 2 + (v / 0.4) ** 2 - 1


def _exact_kappa_2d(g):
    """O&F eq. 1.8 in 2-D with the exact derivatives of the quadratic form above (centred differences reproduce them)."""
    th = np.pi / 6
    a, b = 1 / 0.8 ** 2, 1 / 0.4 ** 2
    c, s = np.cos(th), np.sin(th)
    hxx, hyy, hxy = 2 * (a * c * c + b * s * s), 2 * (a * s * s + b * c * c), 2 * (a - b) * c * s
    px, py = hxx * g.xs[0] + hxy * g.xs[1], hxy * g.xs[0] + hyy * g.xs[1]
    den = (px ** 2 + py ** 2) ** 1.5
    return (hxx * py ** 2 - 2 * px * py * hxy + hyy * px ** 2) / np.where(den > 0, den, 1.0)


def test_rotated_ellipse_needs_the_mixed_term():
    """The shipped loop bound (j < i - 1, curvature.py:48) drops -2 phi_x phi_y phi_xy in 2-D.  On a rotated ellipse (phi_xy
    != 0) the restatement with j < i matches the exact curvature to rounding in the interior; the shipped bound is off by
    O(1)."""
    g, phi = _rotated_ellipse(81)
    exact = _exact_kappa_2d(g)
    k, _ = R.curvature_second(g, phi)
    ks, _ = R.curvature_second(g, phi, mixed="shipped")
    r = _radius(g)
    band = (r > 0.3) & (r < 0.9)
    band[0, :] = band[-1, :] = band[:, 0] = band[:, -1] = False
    assert np.abs(k - exact)[band].max() <= 1e-10 * np.abs(exact[band]).max()
    assert np.abs(ks - exact)[band].max() >= 0.2 * np.abs(exact[band]).max()


def test_corner_ghosts_follow_the_padding_order():
    """A corner ghost of addGhostAllDims is dimension 1's rule applied to dimension 0's ghost values: with axis 0 periodic and
    axis 1 extrapolated, the (-1, -1) corner is extrapolated along axis 1 from the wrapped row, and the mixed partial of
    the corner cell reads it."""
    g = O.Grid([0, 0], [1, 1], [5, 6], pd_dims=[0])
    rng = np.random.default_rng(3)
    phi = rng.standard_normal(g.shape)
    P = O.add_ghost_all_dims(g, phi, 1)
    edge, inner = phi[-1, 0], phi[-1, 1]
    assert P[0, 0] == edge + 1 * (abs(edge - inner) * np.sign(edge))
    s, f = R.hessian_second(g, phi)
    dxi = [1 / float(v) for v in g.dx.ravel()]
    # second[1][0] at cell (0, 0) (padded index (1, 1)): the centred difference along axis 0 of first[1], which at the
    # axis-0 ghost row reads the corner P[0, 0]
    f1_hi = 0.5 * dxi[1] * (P[2, 2] - P[2, 0])
    f1_lo = 0.5 * dxi[1] * (P[0, 2] - P[0, 0])
    assert s[1][0][0, 0] == 0.5 * dxi[0] * (f1_hi - f1_lo)


def test_term_sum_adds_every_term_and_combines_bounds_harmonically():
    a, b, c = np.full((4, 1), 1.0), np.full((4, 1), 2.0), np.full((4, 1), -0.5)
    ydot, sb = R.term_sum([(a, 2.0), (b, float('inf')), (c, 4.0)])
    np.testing.assert_array_equal(ydot, a + b + c)
    assert sb == 1 / (1 / 2.0 + 1 / 4.0)
    assert R.term_sum([(a, float('inf'))])[1] == float('inf')


def test_step_bound_of_term_curvature():
    g = O.Grid([0, 0], [1, 2], [11, 21])
    assert np.isclose(R.step_bound_curvature(g, 2.0), 1 / (2 * 2.0 * (100.0 + 100.0)), rtol=1e-14, atol=0)
    assert R.step_bound_curvature(g, 0.0) == float('inf')


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "hj_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(hj_[a-z0-9_]+)\s*\(", txt))


def test_new_entry_points_are_in_header_ffi_and_library():
    syms = _header_symbols()
    lib = _ffi.lib()
    for s in NEW:
        assert s in syms, s
        assert s in _ffi.SIGNATURES, s
        assert hasattr(lib, s), s


def test_new_entry_points_refuse_a_null_context():
    lib = _ffi.lib()
    sb = C.c_double()
    assert lib.hj_term_curvature(None, None, None, 1.0, None, C.byref(sb)) == -1
    assert lib.hj_curvature_second(None, None, None, None) == -1
    assert lib.hj_laplacian_second(None, None, None) == -1
    assert lib.hj_centered_first_second(None, 0, None, None) == -1


def test_package_exports_the_new_names():
    for name in ("termSum", "termCurvature", "termForcing", "curvatureSecond", "hessianSecond", "laplacianSecond",
                 "centeredFirstSecond"):
        assert callable(getattr(L, name)), name


def test_term_sum_argument_errors():
    with pytest.raises(ValueError, match="cell vectors"):
        L.termSum(0.0, np.zeros((4, 1)), L.Bundle(dict(innerFunc=L.termForcing, innerData=[None])))
    with pytest.raises(ValueError, match="same len"):
        L.termSum(0.0, np.zeros((4, 1)), L.Bundle(dict(innerFunc=[L.termForcing], innerData=[None, None])))


def test_term_forcing_on_host_arrays():
    g = L.createGrid(np.zeros((2, 1)), np.ones((2, 1)), np.array([[4], [5]]))
    y = np.arange(20.0).reshape(-1, 1)
    f = np.linspace(0, 1, 20).reshape(4, 5)
    for forcing, want in [(2.5, np.full((20, 1), -2.5)), (f, -f.reshape(-1, 1)),
                          (lambda t, d, sd: d * t, -(y * 3.0))]:
        ydot, sb, _ = L.termForcing(3.0, y, L.Bundle(dict(grid=g, forcing=forcing)))
        np.testing.assert_array_equal(ydot, want)
        assert sb == float('inf')
    with pytest.raises(ValueError, match="forcing must be"):
        L.termForcing(0.0, y, L.Bundle(dict(grid=g, forcing="x")))


def test_term_sum_sums_every_inner_term_on_host_arrays():
    """The shipped termSum adds only the last inner term (term_sum.py:96): three forcings must all arrive."""
    g = L.createGrid(np.zeros((2, 1)), np.ones((2, 1)), np.array([[4], [5]]))
    y = np.zeros((20, 1))
    inner = [L.Bundle(dict(grid=g, forcing=v)) for v in (1.0, 2.0, 4.0)]
    sd = L.Bundle(dict(innerFunc=[L.termForcing] * 3, innerData=inner))
    ydot, sb, sd2 = L.termSum(0.0, y, sd)
    np.testing.assert_array_equal(ydot, np.full((20, 1), -7.0))
    assert sb == float('inf') and sd2 is sd and sd.innerData[2] is inner[2]
