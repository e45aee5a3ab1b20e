"""GPU: the second-order derivatives, termCurvature, termSum and termForcing (levelsetpy_amd/curvature.py, csrc/hj_curv.h)
against the NumPy restatement of tests/curvature_ref.py, and motion by mean curvature by behaviour.

Tolerances.  fp64: the kernel evaluates the restatement's expressions in its order with contraction off; what may differ is
|p|^3 (NumPy's pow against two products) and the library's sqrt, each within an ulp or two -- checked at 1e-12 x max|out|.
fp32: the kernel's arithmetic in single precision against the fp64 restatement of the SAME (fp32-rounded) input.  A second
difference cancels: phi(+) - 2 phi + phi(-) carries an absolute rounding error of a few eps32 max|phi|, which dx^-2 scales
up, so a k-th derivative is checked at 1e-5 x max|out| + 16 eps32 max|phi| sum_i dx_i^-k; kappa and ydot divide by
|grad phi| and are checked where |grad phi| >= 0.5 with the second-derivative bound over 0.5."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import curvature_ref as R                # noqa: E402
import levelsetpy_amd as L               # noqa: E402
from oracle import hj_oracle as O        # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
EPS32 = float(np.finfo(np.float32).eps)

# (N, periodic axes, towardZero axes): every boundary rule, and periodic next to extrapolated (the corner-ghost case)
CASES = [
    ((41,), (), ()),
    ((41,), (0,), ()),
    ((41,), (), (0,)),
    ((37, 41), (), ()),
    ((37, 41), (0,), ()),
    ((37, 41), (1,), (0,)),
    ((37, 41), (), (0, 1)),
    ((37, 41), (0, 1), ()),
    ((21, 23, 25), (), ()),
    ((21, 23, 25), (1,), (2,)),
    ((21, 23, 25), (0, 2), ()),
    ((11, 12, 13, 9), (), ()),
    ((11, 12, 13, 9), (2,), (0,)),
]


def _grids(N, periodic, tz):
    nd = len(N)
    lo = [-1.0 - 0.1 * d for d in range(nd)]
    hi = [1.0 + 0.05 * d for d in range(nd)]
    g = L.createGrid(np.array(lo).reshape(-1, 1), np.array(hi).reshape(-1, 1), np.array(N, dtype=np.int64).reshape(-1, 1),
                     list(periodic) if periodic else None)
    if tz:
        g.bdryData = [L.Bundle(dict(towardZero=True)) if d in tz else None for d in range(nd)]
    og = O.Grid(lo, hi, list(N), pd_dims=list(periodic), toward_zero=[d in tz for d in range(nd)])
    return g, og


def _phi(og):
    """A sphere's distance, off-centre, bent by a smooth wave: signs of the edge values vary (towardZero matters) and the
    mixed partials do not vanish."""
    r = np.sqrt(sum((x - 0.1 * (d + 1)) ** 2 for d, x in enumerate(og.xs)))
    wave = 0.2 * np.sin(2 * og.xs[0] + 1) * np.cos(3 * og.xs[-1] - 0.5)
    return r - 0.5 + wave + 0.3 * og.xs[0] * og.xs[-1]


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _close64(got, want):
    got, want = _np(got), np.asarray(want)
    assert got.shape == want.shape
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= 1e-12 * scale, (err, scale)


def _dx_sum(og, k):
    return float(np.sum(np.asarray(og.dx, dtype=np.float64).ravel() ** -k))


def _close32(got, want, phi, og, k, mask=None):
    got, want = _np(got).astype(np.float64), np.asarray(want)
    tol = 1e-5 * float(np.abs(want).max()) + 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, k)
    d = np.abs(got - want)
    if mask is not None:
        d = d[mask]
    assert float(d.max()) <= tol, (float(d.max()), tol)


def _kinds(phi):
    yield phi
    yield torch.as_tensor(phi, device="cuda")


@pytest.mark.parametrize("N,periodic,tz", CASES)
def test_derivatives_match_restatement_fp64(N, periodic, tz):
    g, og = _grids(N, periodic, tz)
    phi = _phi(og)
    nd = len(N)
    k_ref, m_ref = R.curvature_second(og, phi)
    s_ref, f_ref = R.hessian_second(og, phi)
    lap_ref = R.laplacian_second(og, phi)
    for data in _kinds(phi):
        k, m = L.curvatureSecond(g, data)
        assert type(k) is type(data)
        _close64(k, k_ref)
        _close64(m, m_ref)
        s, f = L.hessianSecond(g, data)
        for i in range(nd):
            _close64(f[i], f_ref[i])
            for j in range(nd):
                if j <= i:
                    _close64(s[i][j], s_ref[i][j])
                else:
                    assert s[i][j] is None
        _close64(L.laplacianSecond(g, data), lap_ref)
        for d in range(nd):
            a, b = L.centeredFirstSecond(g, data, d)
            assert a is b
            _close64(a, R.centered_first_second(og, phi, d))


@pytest.mark.parametrize("N,periodic,tz", [CASES[0], CASES[5], CASES[9], CASES[12]])
def test_derivatives_match_restatement_fp32(N, periodic, tz):
    g, og = _grids(N, periodic, tz)
    phi = _phi(og).astype(np.float32).astype(np.float64)        # the fp32 input, exactly, for the fp64 restatement
    nd = len(N)
    data = torch.as_tensor(phi, device="cuda", dtype=torch.float32)
    k_ref, m_ref = R.curvature_second(og, phi)
    s_ref, f_ref = R.hessian_second(og, phi)
    k, m = L.curvatureSecond(g, data)
    assert k.dtype == torch.float32
    band = m_ref >= 0.5
    _close32(m, m_ref, phi, og, 1)
    d = np.abs(_np(k).astype(np.float64) - k_ref)[band]
    tol = 1e-5 * float(np.abs(k_ref[band]).max()) + 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) / 0.5
    assert float(d.max()) <= tol, (float(d.max()), tol)
    s, f = L.hessianSecond(g, data)
    for i in range(nd):
        _close32(f[i], f_ref[i], phi, og, 1)
        for j in range(i + 1):
            _close32(s[i][j], s_ref[i][j], phi, og, 2)
    _close32(L.laplacianSecond(g, data), R.laplacian_second(og, phi), phi, og, 2)
    for dd in range(nd):
        _close32(L.centeredFirstSecond(g, data, dd)[0], R.centered_first_second(og, phi, dd), phi, og, 1)


def _b_variants(og):
    arr = 0.5 + 0.25 * np.cos(og.xs[0])
    return [("scalar", 0.75, 0.75), ("array", arr, arr), ("callable", lambda t, d, sd: arr * (1 + t), arr * 1.5),
            ("tensor", torch.as_tensor(arr, device="cuda"), arr)]


@pytest.mark.parametrize("N,periodic,tz", [CASES[1], CASES[4], CASES[6], CASES[9], CASES[12]])
def test_term_curvature_matches_restatement(N, periodic, tz):
    g, og = _grids(N, periodic, tz)
    phi = _phi(og)
    for name, b, b_ref in _b_variants(og):
        want, sb_want = R.term_curvature(og, phi, b_ref)
        for y in (phi.reshape(-1, 1), torch.as_tensor(phi.reshape(-1, 1), device="cuda")):
            sd = L.Bundle(dict(grid=g, b=b, curvatureFunc=L.curvatureSecond))
            ydot, sb, sd2 = L.termCurvature(0.5, y, sd)
            assert sd2 is sd and type(ydot) is type(y) and tuple(ydot.shape) == want.shape, name
            _close64(ydot, want)
            assert abs(sb - sb_want) <= 1e-13 * sb_want, (name, sb, sb_want)


def test_term_curvature_fp32_and_zero_b():
    g, og = _grids((37, 41), (1,), ())
    phi = _phi(og).astype(np.float32).astype(np.float64)
    y = torch.as_tensor(phi.reshape(-1, 1), device="cuda", dtype=torch.float32)
    ydot, sb, _ = L.termCurvature(0.0, y, L.Bundle(dict(grid=g, b=0.75, curvatureFunc=L.curvatureSecond)))
    want, sb_want = R.term_curvature(og, phi, 0.75)
    _, m_ref = R.curvature_second(og, phi)
    band = (m_ref >= 0.5).reshape(-1, 1)
    d = np.abs(_np(ydot).astype(np.float64) - want)[band]
    # ydot = b kappa |grad phi|: the kappa bound of test_derivatives_match_restatement_fp32 times b and max |grad phi|
    tol = 1e-5 * float(np.abs(want[band]).max()) + 0.75 * float(m_ref.max()) * 16 * EPS32 * float(np.abs(phi).max()) * _dx_sum(og, 2) / 0.5
    assert ydot.dtype == torch.float32 and float(d.max()) <= tol
    assert abs(sb - sb_want) <= 1e-13 * sb_want
    _, sb0, _ = L.termCurvature(0.0, y, L.Bundle(dict(grid=g, b=np.zeros(g.shape), curvatureFunc=L.curvatureSecond)))
    assert sb0 == float('inf')


def test_term_curvature_foreign_curvature_func_takes_the_array_path():
    g, og = _grids((37, 41), (0,), ())
    phi = _phi(og)
    arr = 0.5 + 0.25 * np.cos(og.xs[0])
    foreign = lambda gg, d: R.curvature_second(og, d)       # noqa: E731
    ydot, sb, _ = L.termCurvature(0.0, phi.reshape(-1, 1), L.Bundle(dict(grid=g, b=arr, curvatureFunc=foreign)))
    want, sb_want = R.term_curvature(og, phi, arr)
    _close64(ydot, want)
    assert abs(sb - sb_want) <= 1e-13 * sb_want


def test_large_grid_term_curvature_fp64():
    """201^3 fp64 (8 M cells, above the library's 1 M-cell small-grid switch of the other terms)."""
    n = 201
    g, og = _grids((n, n, n), (2,), ())
    phi = _phi(og)
    arr = 0.5 + 0.25 * np.cos(og.xs[0])
    want, sb_want = R.term_curvature(og, phi, arr)
    y = torch.as_tensor(phi.reshape(-1, 1), device="cuda")
    ydot, sb, _ = L.termCurvature(0.0, y, L.Bundle(dict(grid=g, b=torch.as_tensor(arr, device="cuda"), curvatureFunc=L.curvatureSecond)))
    _close64(ydot, want)
    assert abs(sb - sb_want) <= 1e-13 * sb_want


def _normal_sd(g, speed):
    return L.Bundle(dict(grid=g, speed=speed, derivFunc=L.upwindFirstENO2))


def test_term_sum_is_the_sum_of_its_terms():
    g, og = _grids((37, 41), (1,), ())
    phi = _phi(og)
    for y in (phi.reshape(-1, 1), torch.as_tensor(phi.reshape(-1, 1), device="cuda")):
        sdN = _normal_sd(g, 0.3)
        sdC = L.Bundle(dict(grid=g, b=0.2, curvatureFunc=L.curvatureSecond))
        sdF = L.Bundle(dict(grid=g, forcing=np.full(g.shape, 0.125)))
        uN, bN, _ = L.termNormal(0.0, y, sdN)
        uC, bC, _ = L.termCurvature(0.0, y, sdC)
        uF, bF, _ = L.termForcing(0.0, y, sdF)
        assert bF == float('inf')
        sd = L.Bundle(dict(innerFunc=[L.termNormal, L.termCurvature, L.termForcing], innerData=[sdN, sdC, sdF]))
        ydot, sb, sd2 = L.termSum(0.0, y, sd)
        assert sd2 is sd and type(ydot) is type(y)
        want, sb_want = R.term_sum([(_np(uN), bN), (_np(uC), bC), (_np(uF), bF)])
        _close64(ydot, want)
        assert abs(sb - sb_want) <= 1e-13 * sb_want
        # all three terms arrive (the shipped termSum keeps only the last one)
        assert float(np.abs(_np(ydot) - _np(uF)).max()) > 1e-3


def _radii(y, og):
    """Zero crossing of y along the axes and the diagonals from the centre node (linear interpolation)."""
    n = og.shape[0]
    c = n // 2
    nd = og.dim
    dx = float(og.dx[0, 0])
    out = []
    for dirn in ([1] + [0] * (nd - 1), [-1] + [0] * (nd - 1), [0] * (nd - 1) + [1], [1] * nd, [-1] * nd):
        vals = np.array([y[tuple(c + k * d for d in dirn)] for k in range(c + 1)])
        step = dx * np.sqrt(sum(abs(d) for d in dirn))
        k = int(np.argmax(vals > 0))
        out.append(step * (k - 1) + step * (-vals[k - 1]) / (vals[k] - vals[k - 1]))
    return np.array(out)


@pytest.mark.parametrize("nd,n,R0,tf", [(2, 101, 0.6, 0.1), (3, 41, 0.7, 0.05)])
def test_circle_and_sphere_shrink_under_curvature_motion(nd, n, R0, tf):
    """phi_t = kappa |grad phi| moves a sphere of radius R in R^D inward at speed (D - 1)/R: R(t)^2 = R0^2 - 2 (D - 1) t.
    The zero crossing along axes and diagonals must be within 0.05 dx of that.  The truncation error is O(dx^2): the NumPy
    restatement integrated the same way lands within 0.004 dx (2-D, 101^2, t = 0.1) and 0.0035 dx (3-D, 41^3, t = 0.05);
    a curvature off by its mixed term or by a factor moves the diagonal crossings by O(t), tens of cells here."""
    lo, hi = [-1.0] * nd, [1.0] * nd
    g = L.createGrid(np.array(lo).reshape(-1, 1), np.array(hi).reshape(-1, 1), n * np.ones((nd, 1), dtype=np.int64))
    og = O.Grid(lo, hi, [n] * nd)
    r = np.sqrt(sum(x ** 2 for x in og.xs))
    op = L.odeCFLset(L.Bundle(dict(factorCFL=0.9)))
    sd = L.Bundle(dict(grid=g, b=1.0, curvatureFunc=L.curvatureSecond))
    y0 = torch.as_tensor((r - R0).reshape(-1, 1), device="cuda")
    t, y, _ = L.odeCFL3(L.termCurvature, [0.0, tf], y0, op, sd)
    assert torch.is_tensor(y) and y.is_cuda and abs(t - tf) < 1e-12
    want = np.sqrt(R0 ** 2 - 2 * (nd - 1) * tf)
    got = _radii(_np(y).reshape(og.shape), og)
    assert np.abs(got - want).max() <= 0.05 * float(og.dx[0, 0]), (got, want)


def test_ode_cfl3_over_term_sum_stays_on_the_device():
    g, og = _grids((37, 41), (1,), ())
    phi = _phi(og)

    def sd():
        return L.Bundle(dict(innerFunc=[L.termNormal, L.termCurvature, L.termForcing],
                             innerData=[_normal_sd(g, 0.3), L.Bundle(dict(grid=g, b=0.2, curvatureFunc=L.curvatureSecond)),
                                        L.Bundle(dict(grid=g, forcing=0.05))]))
    op = L.odeCFLset(L.Bundle(dict(factorCFL=0.5)))
    td, yd, _ = L.odeCFL3(L.termSum, [0.0, 0.05], torch.as_tensor(phi.reshape(-1, 1), device="cuda"), op, sd())
    th, yh, _ = L.odeCFL3(L.termSum, [0.0, 0.05], phi.reshape(-1, 1), op, sd())
    assert torch.is_tensor(yd) and yd.is_cuda and yd.dtype == torch.float64
    assert abs(td - th) <= 1e-14
    np.testing.assert_allclose(_np(yd), np.asarray(yh), rtol=0, atol=1e-12 * float(np.abs(phi).max()))


def test_stage_combination_of_a_term_sum_finds_the_inner_grid():
    from levelsetpy_amd import integration
    g, og = _grids((37, 41), (), ())
    y = torch.zeros((37 * 41, 1), device="cuda", dtype=torch.float64)
    sd = L.Bundle(dict(innerFunc=[L.termForcing], innerData=[L.Bundle(dict(grid=g, forcing=1.0))]))
    dg = integration._any_device_grid(sd, y)
    assert dg is not None and dg.shape == (37, 41)


def test_argument_errors():
    g, og = _grids((37, 41), (), ())
    phi = _phi(og)
    with pytest.raises(ValueError, match="b must be"):
        L.termCurvature(0.0, phi.reshape(-1, 1), L.Bundle(dict(grid=g, b="x", curvatureFunc=L.curvatureSecond)))
    with pytest.raises(ValueError, match="agree in array size"):
        L.curvatureSecond(g, phi[:-1])
    with pytest.raises(ValueError, match="Illegal dim"):
        L.centeredFirstSecond(g, phi, 2)
