"""Motion by mean curvature and the second-order half of the toolbox (reference SpatialDerivative/Other/,
ExplicitIntegration/Term/term_{curvature,sum,forcing}.py):

    curvature, gradMag = curvatureSecond(grid, data)              kappa (O&F eq. 1.8) and |grad phi|
    second, first      = hessianSecond(grid, data)                second[i][j], j <= i; first[i] = d data / dx_i
    laplacian          = laplacianSecond(grid, data)
    deriv, deriv       = centeredFirstSecond(grid, data, dim)     (twice, so that it serves as a derivFunc)
    ydot, stepBound, schemeData = termCurvature(t, y, schemeData) ydot = b kappa |grad phi|
    ydot, stepBound, schemeData = termSum(t, y, schemeData)       the sum of schemeData.innerFunc's terms
    ydot, stepBound, schemeData = termForcing(t, y, schemeData)   ydot = -forcing

`data` / `y` and the arrays in schemeData may be NumPy arrays or device tensors; results come back as the same kind.
Each derivative function, and termCurvature with curvatureFunc = curvatureSecond, is ONE native launch (hj_curv.h): the
compact second-order stencil with the ghost cells of addGhostAllDims(grid, data, 1), corner ghosts included.

Deviations from the shipped reference, none of whose second-order functions runs: hessianSecond calls a list and an
array (hessian.py:61,71) and stores arrays into a float matrix (:77), so curvatureSecond and laplacianSecond raise too;
curvatureSecond sums the mixed partials over j < i - 1 (curvature.py:48 and hessian.py:88, MATLAB's j = 1:i-1 mistranslated), which drops
-2 phi_x phi_y phi_xy in 2-D; termSum adds only the LAST inner term (term_sum.py:96, the body dedented out of the loop
of :87).  Implemented here is what their docstrings and ToolboxLS describe: O&F eq. 1.8 with j < i, the sum over every
inner term.  Parity is therefore UNPINNED; checked against the NumPy restatement in tests/curvature_ref.py and by
behaviour (a circle / sphere shrinking under unit curvature motion as R^2 = R0^2 - 2 (D - 1) t).
"""
import ctypes as C

import numpy as np

from . import _ffi
from .context import is_tensor, device_grid, array_dtype_name
from .normal_reinit import _like
from .utilities import isfield, iscell, error

__all__ = ["curvatureSecond", "hessianSecond", "laplacianSecond", "centeredFirstSecond",
           "termCurvature", "termSum", "termForcing"]


def _prep(grid, data):
    """(DeviceGrid, device phi of grid shape) for one launch on `data`'s dtype.  `data` has the grid's shape (a 1-D
    grid's is (N, 1), processGrid's grid.shape, or (N,))."""
    dg = device_grid(grid, array_dtype_name(data))
    if tuple(data.shape) != dg.shape and tuple(data.shape) != tuple(grid.shape):
        error('data parameter does not agree in array size with grid')
    dg.bind_stream()
    return dg, dg.to_device(data).reshape(dg.shape)


def _back(dg, t, proto):
    """`t` as `proto`'s kind and shape: a tensor for a tensor, NumPy for NumPy."""
    return dg.like(t, proto, tuple(proto.shape))


def curvatureSecond(grid, data):
    """SpatialDerivative/Other/curvature.py:4 -- second-order centred curvature and gradient magnitude (hj_curvature_second)."""
    dg, phi = _prep(grid, data)
    kap, mag = dg.empty(), dg.empty()
    _ffi.check(dg.lib.hj_curvature_second(dg.ctx, dg.ptr(phi), dg.ptr(kap), dg.ptr(mag)))
    return _back(dg, kap, data), _back(dg, mag, data)


def hessianSecond(grid, data):
    """SpatialDerivative/Other/hessian.py:4 -- `second` is a dim x dim list of lists: second[i][j] = d^2 data / dx_i dx_j for
    j < i, the pure second partial for j == i and None (ToolboxLS's []) for j > i; first[i] = d data / dx_i (hj_hessian_second)."""
    dg, phi = _prep(grid, data)
    nd = dg.dim
    first = [dg.empty() for _ in range(nd)]
    second = [[dg.empty() if j <= i else None for j in range(nd)] for i in range(nd)]
    sp = (C.c_void_p * (nd * nd))(*[dg.ptr(second[i][j]) if j <= i else C.c_void_p(0) for i in range(nd) for j in range(nd)])
    fp = (C.c_void_p * nd)(*[dg.ptr(f) for f in first])
    _ffi.check(dg.lib.hj_hessian_second(dg.ctx, dg.ptr(phi), sp, fp))
    second = [[_back(dg, s, data) if s is not None else None for s in row] for row in second]
    return second, [_back(dg, f, data) for f in first]


def laplacianSecond(grid, data):
    """SpatialDerivative/Other/laplacian.py:3 -- sum of the pure second partials (hj_laplacian_second)."""
    dg, phi = _prep(grid, data)
    out = dg.empty()
    _ffi.check(dg.lib.hj_laplacian_second(dg.ctx, dg.ptr(phi), dg.ptr(out)))
    return _back(dg, out, data)


def centeredFirstSecond(grid, data, dim):
    """SpatialDerivative/Other/centered.py:3 -- the second-order centred first partial along `dim`, returned twice (left and
    right approximations are the same) so that it serves as a derivFunc (hj_centered_first_second)."""
    if dim < 0 or dim >= grid.dim:
        error('Illegal dim parameter')
    dg, phi = _prep(grid, data)
    out = dg.empty()
    _ffi.check(dg.lib.hj_centered_first_second(dg.ctx, int(dim), dg.ptr(phi), dg.ptr(out)))
    deriv = _back(dg, out, data)
    return deriv, deriv


def _number(a):
    return isinstance(a, (int, float, np.number)) and not isinstance(a, bool)


def _on_grid(a, proto, shape):
    """A scalar or an array of the grid's size as an array of `proto`'s kind with `shape` (a 1-D grid's arrays may be
    (N,) or (N, 1))."""
    if isinstance(a, np.ndarray) and a.ndim > 0:
        a = a.reshape(shape)
    return _like(a, proto, shape)


def _sum_dx_inv2(grid):
    return float(np.sum(np.asarray(grid.dx, dtype=np.float64).ravel() ** -2))


def termCurvature(t, y, schemeData):
    thisSchemeData = schemeData[0] if iscell(schemeData) else schemeData
    assert isfield(thisSchemeData, 'grid'), "grid not in schemeData"
    assert isfield(thisSchemeData, 'b'), "b not in schemeData"
    assert isfield(thisSchemeData, 'curvatureFunc'), "curvatureFunc not in schemeData"
    grid = thisSchemeData.grid
    y0 = y[0] if iscell(y) else y
    data = y0.reshape(grid.shape)
    b = thisSchemeData.b
    if callable(b):
        b = b(t, data, thisSchemeData)                                       # term_curvature.py:113-132
    elif not (_number(b) or is_tensor(b) or isinstance(b, np.ndarray)):
        error('schemeData.b must be a scalar, array or function handle')     # :136-137
    scalar = _number(b) or (isinstance(b, np.ndarray) and b.ndim == 0)
    if thisSchemeData.curvatureFunc is curvatureSecond:
        # the whole term is ONE launch (hj_term_curvature); NumPy data goes over PCIe and comes back as NumPy
        dg, phi = _prep(grid, data)
        arr = None if scalar else dg.to_device(_on_grid(b, data, dg.shape))
        out, sb = dg.empty(), C.c_double()
        _ffi.check(dg.lib.hj_term_curvature(dg.ctx, dg.ptr(phi), dg.ptr(arr), float(b) if scalar else 0.0,
                                            dg.ptr(out), C.byref(sb)))
        return dg.like(out, y0, (-1, 1)), float(sb.value), schemeData
    # a foreign curvatureFunc: its curvature, then array expressions on whatever kind of array it returns
    curvature, gradMag = thisSchemeData.curvatureFunc(grid, data)            # :140
    if not scalar:
        b = _on_grid(b, curvature, tuple(curvature.shape))
    delta = -b * curvature * gradMag                                         # :141  O&F (4.5)
    maxb = float(b) if scalar else float(b.max())
    stepBound = float('inf') if maxb == 0 else 1 / (2 * maxb * _sum_dx_inv2(grid))    # :144  O&F (4.7)
    return (-delta).reshape(-1, 1), stepBound, schemeData                    # :147


def termSum(t, y, schemeData):
    thisSchemeData = schemeData[0] if iscell(schemeData) else schemeData
    assert isfield(thisSchemeData, 'innerFunc'), "innerFunc not in schemeData"
    innerFuncs = thisSchemeData.innerFunc
    innerDatas = thisSchemeData.innerData if isfield(thisSchemeData, 'innerData') else None
    if not iscell(innerFuncs) or not iscell(innerDatas):                     # term_sum.py:76-77
        error('schemeData.innerFunc and schemeData.innerData must be cell vectors')
    if len(innerFuncs) != len(innerDatas):                                   # :81-82
        error('schemeData.innerFunc and schemeData.innerData must be the same len')
    ydot = None
    stepBoundInv = 0.0
    for i in range(len(innerFuncs)):                                         # :87, every term (the shipped body is dedented out)
        if iscell(schemeData):
            innerData = list(schemeData)
            innerData[0] = thisSchemeData.innerData[i]
        else:
            innerData = thisSchemeData.innerData[i]
        updateI, stepBoundI, innerData = innerFuncs[i](t, y, innerData)      # :96
        ydot = updateI if ydot is None else ydot + updateI                   # :97
        stepBoundInv += 1 / stepBoundI                                       # :98  (1 / inf = 0)
        if iscell(schemeData):                                               # :101-104
            thisSchemeData.innerData[i] = innerData[0]
        else:
            thisSchemeData.innerData[i] = innerData
    stepBound = float('inf') if stepBoundInv == 0 else 1 / stepBoundInv      # :107-110
    return ydot, stepBound, schemeData


def termForcing(t, y, schemeData):
    thisSchemeData = schemeData[0] if iscell(schemeData) else schemeData
    assert isfield(thisSchemeData, 'grid'), "grid not in schemeData"
    assert isfield(thisSchemeData, 'forcing'), "forcing not in schemeData"
    grid = thisSchemeData.grid
    y0 = y[0] if iscell(y) else y
    data = y0.reshape(grid.shape)
    forcing = thisSchemeData.forcing
    if callable(forcing):
        forcing = forcing(t, data, thisSchemeData)                           # term_forcing.py:104-127
    elif not (_number(forcing) or is_tensor(forcing) or isinstance(forcing, np.ndarray)):
        error('schemeData.forcing must be a scalar, array or function handle')   # :129-130
    # a scalar forcing is applied at every node (ToolboxLS: -forcing(:) broadcast against the other terms)
    ydot = -_on_grid(forcing, data, tuple(data.shape))                       # :133
    return ydot.reshape(-1, 1), float('inf'), schemeData                     # :136  no derivative, no time step limit
