"""The NumPy oracle on BOXES of a grid (test infrastructure, no GPU).

The oracle evaluates about 3.5e6 cells a second: it cannot restate a launch over 2e9 cells.  But ydot at a cell depends only on the 7-point
stencils through that cell and on the cell's own coordinates (the built-in systems' alpha is per node; only stepBound is a reduction over
the grid), so a result is checked on boxes: cut the index range [lo - m, hi + m) out of every axis, evaluate the oracle on that small array
and compare the inner [lo, hi).  m = 3 is one substep's reach, 9 a whole RK3 step's.

  box(G, lo, hi, m)       -> (index lists per axis, slices of the compared cells within the box)
  box_grid(G, idx)        -> oracle.hj_oracle.Grid of the box: coordinates taken from G by index, dx copied, every face 'extrapolate'
  light_grid(...)         -> what box / box_grid need of a grid too large for meshgrid (no xs)
  gather(t, idx)          -> the box of a (device) torch tensor as a host float64 NumPy array
  ydot / stage / rk3_step -> the oracle on a box

On a periodic axis the range is wrapped modulo N (an axis shorter than the range simply repeats: the whole of a periodic axis is a box too);
on an extrapolated axis it is clipped to the grid, and the box's own extrapolation is then the oracle's at a true boundary.  A cut face is
never periodic, and the cells within m of it are wrong by design: they are the margin that is not compared."""
import numpy as np

from levelsetpy_amd import _ffi
from oracle import hj_oracle as O

M_SUBSTEP, M_RK3 = 3, 9


class LightGrid(object):
    """min / max / N / dx / vs / shape / bc / dim of oracle.hj_oracle.Grid by its own expressions (hj_oracle.py, Grid.__init__), without xs."""

    def __init__(self, gmin, gmax, N, pd_dims=None):
        self.min = np.asarray(gmin, dtype=np.float64).reshape(-1, 1)
        self.max = np.asarray(gmax, dtype=np.float64).reshape(-1, 1)
        self.N = np.asarray(N, dtype=np.int64).reshape(-1, 1)
        self.dim = len(self.min)
        self.dx = np.divide(self.max - self.min, self.N - 1)
        self.vs = [np.expand_dims(np.linspace(self.min[i, 0].item(), self.max[i, 0].item(), num=self.N[i, 0].item()), 1)
                   for i in range(self.dim)]
        self.shape = tuple(int(n) for n in self.N.ravel())
        pd_dims = [] if pd_dims is None else ([pd_dims] if np.isscalar(pd_dims) else list(pd_dims))
        self.bc = ['periodic' if i in pd_dims else 'extrapolate' for i in range(self.dim)]


def light_grid(gmin, gmax, N, pd_dims=None):
    return LightGrid(gmin, gmax, N, pd_dims)


def box(G, lo, hi, m):
    """Index lists of the box [lo - m, hi + m) per axis and the slices of [lo, hi) within it."""
    idx, cmp = [], []
    for d in range(G.dim):
        n, a, b = int(G.shape[d]), int(lo[d]), int(hi[d])
        assert 0 <= a < b <= n, (d, a, b, n)
        if G.bc[d] == 'periodic':
            ids, off = np.arange(a - m, b + m) % n, m
        else:
            a0 = max(a - m, 0)
            ids, off = np.arange(a0, min(b + m, n)), a - a0
        idx.append(ids.astype(np.int64))
        cmp.append(slice(off, off + b - a))
    return idx, tuple(cmp)


def box_grid(G, idx):
    g = O.Grid(G.min, G.max, [len(i) for i in idx], None)
    g.bc = ['extrapolate'] * G.dim              # a cut face is never periodic
    g.dx = G.dx.copy()                          # the global spacing, never recomputed
    g.vs = [np.asarray(G.vs[d]).reshape(-1, 1)[idx[d]].copy() for d in range(G.dim)]
    g.xs = np.meshgrid(*g.vs, indexing='ij')
    g.shape = tuple(len(i) for i in idx)
    g.N = np.asarray(g.shape, dtype=np.int64).reshape(-1, 1)
    return g


def take(a, idx):
    """The box of a NumPy array."""
    return a[np.ix_(*idx)]


def gather(t, idx):
    """The box of a torch tensor (any device), copied to the host as float64.  Contiguous index runs are cut by slicing first, so the
    wrapped axes are indexed on an array that is already small."""
    import torch
    wrapped = []
    for d, ids in enumerate(idx):
        if len(ids) == 1 or np.all(np.diff(ids) == 1):
            t = t.narrow(d, int(ids[0]), len(ids))
        else:
            wrapped.append(d)
    for d in wrapped:
        t = t.index_select(d, torch.as_tensor(idx[d], device=t.device))
    return t.to("cpu", torch.float64).numpy()


def ydot(G, make_sys, scheme, idx, ybox, eps_max=None):
    """termLaxFriedrichs on the box; eps_max: the grid-wide max(D1^2) per dim of the intended WENO5."""
    g = box_grid(G, idx)
    v, _ = O.term_lax_friedrichs(g, make_sys(g), scheme, 0., np.ascontiguousarray(ybox, dtype=np.float64).reshape(-1), None, eps_max)
    return v.reshape(g.shape)


def stage_expr(stage, dt, y, y0, yd):
    """The array expression of one stage, written as tests/test_dist_gloo.py's OracleSlabBackend.substep writes it."""
    if stage == _ffi.STAGE_YDOT:
        return yd
    ye = y + dt * yd
    if stage == _ffi.STAGE_EULER:
        return ye
    if stage == _ffi.STAGE_RK3_HALF:
        return 0.25 * (3 * y0 + ye)
    if stage == _ffi.STAGE_RK3_FULL:
        return (1 / 3) * (y0 + 2 * ye)
    return 0.5 * (y0 + ye)


def stage(G, make_sys, scheme, idx, stage_id, dt, ybox, y0box, eps_max=None):
    return stage_expr(stage_id, dt, ybox, y0box, ydot(G, make_sys, scheme, idx, ybox, eps_max))


def rk3_step(G, make_sys, scheme, idx, ybox, tf, factor_cfl=0.8):
    """One odeCFL3 step over [0, tf] on the box (margin M_RK3).  tf must lie below the GRID's CFL step: the box's own stepBound is no smaller
    than the grid's (its alpha maxima are taken over fewer nodes), so deltaT = tf on both sides."""
    g = box_grid(G, idx)
    s = make_sys(g)
    t, y = O.ode_cfl_3(lambda tt, v: O.term_lax_friedrichs(g, s, scheme, tt, v), [0., tf],
                       np.ascontiguousarray(ybox, dtype=np.float64).reshape(-1), factor_cfl, single_step=True)
    return t, y.reshape(g.shape)
