"""NumPy restatement of the reference's second-order derivatives and of termCurvature / termSum / termForcing -- TEST
INFRASTRUCTURE, NOT PRODUCT (the package never imports it).

The shipped functions raise (hessian.py:61,71,77; see levelsetpy_amd/curvature.py), so there is nothing to pin them to.
What is restated is what their docstrings and ToolboxLS describe, formula by formula in the reference's own order, on the
golden-pinned ghost padding of oracle.hj_oracle.add_ghost_all_dims / add_ghost (addGhostAllDims pads dimension 0 first,
then dimension 1 of the padded array, ...: that is where the corner ghost values come from).  `mixed='shipped'` keeps the
shipped mixed-partial loop bound (j < i - 1, curvature.py:48 / hessian.py:88) for the tests that show what it loses.

Citations are file:line of the reference checkout (SpatialDerivative/Other/, ExplicitIntegration/Term/).
"""
import numpy as np

from oracle import hj_oracle as O


def _dx_inv(grid):
    return [1.0 / float(v) for v in np.asarray(grid.dx, dtype=np.float64).ravel()]    # hessian.py:46 dxInv = 1 / grid.dx


def _sl(nd, d, s, rest):
    """index tuple: `s` along d, `rest` along every other axis."""
    return tuple(s if k == d else rest for k in range(nd))


def hessian_second(grid, data, mixed="intended"):
    """hessian.py:4 -> (second, first); second[i][j] for j <= i (None above the diagonal), all of grid shape."""
    nd = grid.dim
    dxInv = _dx_inv(grid)
    P = O.add_ghost_all_dims(grid, np.asarray(data, dtype=np.float64), 1)      # :52  stencil = 1
    real = [slice(1, n + 1) for n in grid.shape]                               # :56-58  indReal
    full = slice(None)
    # centred first partials on the padded array: ghost cells of the other dimensions kept for the mixed partials (:64-71)
    firstP = []
    for i in range(nd):
        n = grid.shape[i]
        hi = tuple(slice(2, n + 2) if k == i else full for k in range(nd))
        lo = tuple(slice(0, n) if k == i else full for k in range(nd))
        firstP.append(0.5 * dxInv[i] * (P[hi] - P[lo]))
    second = [[None] * nd for _ in range(nd)]
    for i in range(nd):
        n = grid.shape[i]
        hi = tuple(slice(2, n + 2) if k == i else real[k] for k in range(nd))
        lo = tuple(slice(0, n) if k == i else real[k] for k in range(nd))
        second[i][i] = dxInv[i] ** 2 * (P[hi] - 2 * P[tuple(real)] + P[lo])     # :85
        js = range(i) if mixed == "intended" else range(i - 1)                   # :88  (MATLAB j = 1:i-1)
        for j in js:
            m = grid.shape[j]
            # firstP[i] has no ghost cells along i (already differentiated), ghost cells elsewhere (:90-97)
            a = tuple(slice(0, grid.shape[k]) if k == i else (slice(2, m + 2) if k == j else real[k]) for k in range(nd))
            b = tuple(slice(0, grid.shape[k]) if k == i else (slice(0, m) if k == j else real[k]) for k in range(nd))
            second[i][j] = 0.5 * dxInv[j] * (firstP[i][a] - firstP[i][b])      # :99
    first = []
    for i in range(nd):                                                          # :102-107  strip the ghost cells
        first.append(firstP[i][tuple(full if k == i else real[k] for k in range(nd))])
    return second, first


def curvature_second(grid, data, mixed="intended"):
    """curvature.py:4 -> (curvature, gradMag), O&F eq. 1.8."""
    second, first = hessian_second(grid, data, mixed)
    gradMag2 = first[0] ** 2                                                     # :39-41
    for i in range(1, grid.dim):
        gradMag2 = gradMag2 + first[i] ** 2
    gradMag = np.sqrt(gradMag2)                                                  # :43
    curvature = np.zeros(grid.shape)
    for i in range(grid.dim):
        curvature = curvature + second[i][i] * (gradMag2 - first[i] ** 2)        # :47
        js = range(i) if mixed == "intended" else range(i - 1)                   # :48
        for j in js:
            curvature = curvature - 2 * first[i] * first[j] * second[i][j]       # :49
    nz = gradMag > 0                                                             # :54-55  0 where |grad phi| = 0
    curvature[nz] = curvature[nz] / gradMag[nz] ** 3
    return curvature, gradMag


def laplacian_second(grid, data):
    """laplacian.py:3: the sum of the pure second partials (:38-40)."""
    second, _ = hessian_second(grid, data)
    out = second[0][0]
    for i in range(1, grid.dim):
        out = out + second[i][i]
    return out


def centered_first_second(grid, data, dim):
    """centered.py:3: ghost cells of grid.bdry[dim] only (:42), centred difference along dim (:54)."""
    n = grid.shape[dim]
    g = O.add_ghost(grid, np.asarray(data, dtype=np.float64), dim, 1)
    nd = grid.dim
    hi = tuple(slice(2, n + 2) if k == dim else slice(None) for k in range(nd))
    lo = tuple(slice(0, n) if k == dim else slice(None) for k in range(nd))
    return 0.5 * _dx_inv(grid)[dim] * (g[hi] - g[lo])


def step_bound_curvature(grid, b):
    """term_curvature.py:144 (O&F eq. 4.7); inf when max b == 0."""
    mb = float(np.max(b))
    s = float(np.sum(np.asarray(grid.dx, dtype=np.float64).ravel() ** -2))
    return float('inf') if mb == 0 else 1 / (2 * mb * s)


def term_curvature(grid, data, b):
    """term_curvature.py:7 with curvatureSecond: (ydot as an (N, 1) column, stepBound)."""
    curvature, gradMag = curvature_second(grid, data)                            # :140
    delta = -np.asarray(b, dtype=np.float64) * curvature * gradMag               # :141  O&F (4.5)
    return (-delta).reshape(-1, 1), step_bound_curvature(grid, b)               # :144,147


def term_sum(parts):
    """term_sum.py:6 over EVERY inner term: parts = [(ydot_i, stepBound_i)] -> (sum ydot, harmonic stepBound) (:87-110)."""
    ydot = 0
    inv = 0.0
    for u, sb in parts:
        ydot = ydot + u
        inv += 1 / sb
    return ydot, (float('inf') if inv == 0 else 1 / inv)
