"""NumPy restatement of the value-function queries (levelsetpy_amd/query.py) -- TEST INFRASTRUCTURE, NOT PRODUCT
(the package never imports it).

eval_u_ref restates hji_solver._eval_point operation by operation, vectorised over states and stored arrays: the
multilinear interpolant of ValueFuncs/evaluate_u.py:64-117 (scipy's RegularGridInterpolator on the periodically
augmented table), with the state wrapped by whole periods and NaN outside an extrapolated axis.  The same operations
in the same order, so its fp64 results equal the host loop's and the device kernel's bit for bit.

costate_ref is eval_u_ref over the oracle's (reference-pinned) upwind derivatives; proj_ref and augment_ref restate
ValueFuncs/data_proj.py:18 and augment_periodic.py:12 as documented (the shipped functions raise, see query.py).

A grid is an oracle.hj_oracle.Grid (bc strings) or the package's Bundle (bdry functions): both carry dim, N, dx, vs.
"""
import numpy as np


def periodic_axes(grid):
    if hasattr(grid, "bc"):
        return [b == 'periodic' for b in grid.bc]
    return [getattr(f, "__name__", "") == "addGhostPeriodic" for f in grid.bdry]


def _axes(grid):
    N = [int(v) for v in np.asarray(grid.N).ravel()]
    dx = [float(v) for v in np.asarray(grid.dx).ravel()]
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in grid.vs]
    return N, dx, vs, periodic_axes(grid)


def locate(grid, xs):
    """Per axis the lower node index and the weight of the upper node, and the mask of states outside the grid."""
    N, dx, vs, per = _axes(grid)
    xs = np.asarray(xs, dtype=np.float64).reshape(-1, grid.dim)
    outside = np.zeros(xs.shape[0], dtype=bool)
    lo, w = [], []
    for d in range(grid.dim):
        xd = xs[:, d].copy()
        v0 = vs[d][0]
        if per[d]:
            period = N[d] * dx[d]
            xd = v0 + np.mod(xd - v0, period)
            i = np.minimum(np.floor((xd - v0) / dx[d]).astype(np.int64), N[d] - 1)
        else:
            out = (xd < v0) | (xd > vs[d][-1]) | ~np.isfinite(xd)
            outside |= out
            xd[out] = v0
            i = np.minimum(np.floor((xd - v0) / dx[d]).astype(np.int64), N[d] - 2)
        lo.append(i)
        w.append((xd - (v0 + i * dx[d])) / dx[d])
    return lo, w, outside


def eval_u_ref(grid, data, xs):
    """V at the M states `xs` (rows): (M,) for one array, (T, M) for a time-first stack."""
    N, dx, vs, per = _axes(grid)
    data = np.asarray(data)
    stack = data.ndim == grid.dim + 1
    assert stack or data.ndim == grid.dim
    a = data.astype(np.float64).reshape((-1,) + tuple(N))
    lo, w, outside = locate(grid, xs)
    M = lo[0].size
    v = np.zeros((a.shape[0], M))
    with np.errstate(invalid='ignore', over='ignore'):
        for corner in range(1 << grid.dim):
            idx, wt = [], np.ones(M)
            for d in range(grid.dim):
                up = (corner >> d) & 1
                j = lo[d] + up
                if per[d]:
                    j = j % N[d]
                idx.append(j)
                wt = wt * (w[d] if up else (1.0 - w[d]))
            term = wt[None, :] * a[(slice(None),) + tuple(idx)]
            v = np.where((wt != 0.0)[None, :], v + term, v)          # corners of weight exactly 0 are skipped
    v[:, outside] = np.nan
    return v if stack else v[0]


def costate_ref(ogrid, data, xs, scheme='WENO5_ASSHIPPED'):
    """grad V at states: eval_u_ref over the oracle's derivC arrays -> (M, dim).  `ogrid` is an oracle Grid, finite data."""
    from oracle import hj_oracle as O
    derivC = O.compute_gradients(ogrid, np.asarray(data, dtype=np.float64), scheme)
    return np.stack([eval_u_ref(ogrid, derivC[d], xs) for d in range(ogrid.dim)], axis=-1)


def augment_ref(grid, data):
    """(vs, data) with one wrapped node appended along every periodic axis (the data of index 0 ALONG THAT AXIS)."""
    N, dx, vs, per = _axes(grid)
    a = np.array(data)
    lead = a.ndim - grid.dim
    for d in range(grid.dim):
        if per[d]:
            vs[d] = np.concatenate([vs[d], [vs[d][-1] + dx[d]]])
            a = np.concatenate([a, np.take(a, [0], axis=lead + d)], axis=lead + d)
    return vs, a


class _Sub(object):
    """The kept axes of a grid with their own N (the grid a projection lives on)."""

    def __init__(self, grid, keep, N=None):
        Nall, dxall, vsall, per = _axes(grid)
        gmin, gmax = np.asarray(grid.min, dtype=np.float64).ravel(), np.asarray(grid.max, dtype=np.float64).ravel()
        self.dim = len(keep)
        self.bc = ['periodic' if per[i] else 'extrapolate' for i in keep]
        self.min, self.max = gmin[keep], gmax[keep]
        if N is None:
            self.N = np.array([Nall[i] for i in keep])
            self.vs = [vsall[i] for i in keep]
            self.dx = np.array([dxall[i] for i in keep])
        else:
            self.N = np.asarray(N, dtype=np.int64).ravel()
            self.vs = [np.linspace(self.min[k], self.max[k], num=int(self.N[k])) for k in range(self.dim)]   # process_grid.py:204
            self.dx = (self.max - self.min) / (self.N - 1)                                                  # :185


def _grid_states(axes):
    mesh = np.meshgrid(*axes, indexing='ij')
    return np.stack([m.ravel() for m in mesh], axis=1)


def proj_ref(grid, data, dims_to_remove, xs='min', NOut=None):
    """dataOut of data_proj.py:18 as documented: 'min' / 'max' over the removed axes, or the slice at the point `xs` of the
    removed axes; on the kept axes' own nodes, or resampled onto linspace(min, max, NOut) when NOut is given.  Time first."""
    Nall, _, vsall, _ = _axes(grid)
    rem = np.asarray(dims_to_remove).astype(bool).ravel()
    keep = [i for i in range(grid.dim) if not rem[i]]
    gone = [i for i in range(grid.dim) if rem[i]]
    data = np.asarray(data)
    lead = data.ndim - grid.dim
    if NOut is not None:
        NOut = np.asarray(NOut).ravel()
        NOut = np.repeat(NOut, len(keep)) if NOut.size == 1 else NOut
    if isinstance(xs, str):
        red = np.amin if xs == 'min' else np.amax
        out = red(data, axis=tuple(lead + i for i in gone))
        if NOut is None or [int(n) for n in NOut] == [Nall[i] for i in keep]:
            return out
        sub, new = _Sub(grid, keep), _Sub(grid, keep, NOut)
        vals = eval_u_ref(sub, out, _grid_states(new.vs))
        return vals.reshape(out.shape[:lead] + tuple(int(n) for n in new.N))
    resample = NOut is not None and [int(n) for n in NOut] != [Nall[i] for i in keep]
    axes = _Sub(grid, keep, NOut).vs if resample else [vsall[i] for i in keep]
    kept = _grid_states(axes)
    pts = np.empty((kept.shape[0], grid.dim))
    pts[:, keep] = kept
    pts[:, gone] = np.asarray(xs, dtype=np.float64).ravel()
    vals = eval_u_ref(grid, data, pts)
    return vals.reshape(data.shape[:lead] + tuple(a.size for a in axes))


# ------------------------------------------------------------------------------------------ shared test cases
SHAPES = {2: (7, 6), 3: (7, 6, 9), 4: (5, 6, 4, 7)}          # non-cubic: a swapped axis shows


def periodic_sets(nd):
    """none, {0}, {last}, {1,2} (3-D / 4-D), all."""
    sets = [(), (0,), (nd - 1,), tuple(range(nd))]
    if nd >= 3:
        sets.append((1, 2))
    return sets


def grid_bounds(shape, pd):
    """The bounds tests/golden/make_golden_query.py uses: a periodic axis stops one node short of its period."""
    nd = len(shape)
    gmin = np.array([-1.0 - 0.25 * d for d in range(nd)])
    span = np.array([2.5 + 0.5 * d for d in range(nd)])
    gmax = gmin + span
    for d in pd:
        gmax[d] = gmin[d] + span[d] * (1.0 - 1.0 / shape[d])
    return gmin, gmax


def make_grids(shape, pd):
    """(package grid Bundle, oracle Grid) of the same grid."""
    import levelsetpy_amd as L
    from oracle import hj_oracle as O
    gmin, gmax = grid_bounds(shape, pd)
    g = L.createGrid(gmin.reshape(-1, 1), gmax.reshape(-1, 1), np.array(shape, dtype=np.int64).reshape(-1, 1),
                     list(pd) if pd else None)
    return g, O.Grid(gmin, gmax, list(shape), list(pd))


def state_set(grid, M, seed=0):
    """M states (rows).  From M >= 63 on the set starts with the special ones: exact nodes, the first and the last node of
    every axis, points inside the first and the last cell (the costate stencils use ghosts there), points outside an
    extrapolated axis (NaN), points several periods away in both directions, points in the wrap cell between the last
    node and the first node plus a period; random states inside the grid fill the rest.  M = 1: one random state."""
    N, dx, vs, per = _axes(grid)
    nd = grid.dim
    rng = np.random.default_rng(1000 * nd + seed)
    lo = np.array([v[0] for v in vs])
    hi = np.array([v[-1] for v in vs])
    dxa = np.array(dx)
    rand = lambda k: lo + rng.random((k, nd)) * (hi - lo)       # noqa: E731
    if M == 1:
        return rand(1)
    sp = [np.array([v[2] for v in vs]), np.array([v[1] for v in vs]), lo.copy(), hi.copy(),
          lo + 0.3 * dxa, hi - 0.3 * dxa, lo + 1.7 * dxa, hi - 1.2 * dxa]
    for d in range(nd):
        base = rand(4)
        period = N[d] * dx[d]
        if per[d]:
            base[0, d] += 3 * period
            base[1, d] -= 4 * period
            base[2, d] = hi[d] + 0.4 * dx[d]                    # the wrap cell
            base[3, d] = lo[d] - 0.25 * dx[d]                   # the wrap cell, one period below
        else:
            base[0, d] = lo[d] - 0.5 * dx[d]                    # outside: NaN
            base[1, d] = hi[d] + 1e-9
            base[2, d] = lo[d]
            base[3, d] = hi[d]
        sp.extend(base)
    sp = np.array(sp)
    assert len(sp) <= 63
    return np.concatenate([sp, rand(M - len(sp))])
