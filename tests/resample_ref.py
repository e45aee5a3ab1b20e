"""NumPy restatement of the resampling rule of include/hj_resample.h (levelsetpy_amd/resample.py) -- TEST INFRASTRUCTURE, NOT
PRODUCT (the package never imports it).

resample_ref applies the affine map term by term in the header's order, evaluates tests/query_ref.py's eval_u_ref there, folds
the members that are inside with np.minimum / np.maximum and fills the nodes no member brought inside.  The same operations in
the same order as the kernel's, so the fp64 results are equal bit for bit.

A grid is anything with dim, N, dx, vs and bc / bdry: the package's Bundle, an oracle Grid, or RefGrid below.  At the end, the
cases tests/test_resample_ref.py and tests/test_gpu_resample.py share.
"""
import numpy as np

import query_ref as Q


class RefGrid(object):
    """dim, N, min, max, dx, vs, bc of a grid, formed as processGrid forms them (process_grid.py:185, :204)."""

    def __init__(self, gmin, gmax, N, pd=()):
        self.min, self.max = np.asarray(gmin, dtype=np.float64).ravel(), np.asarray(gmax, dtype=np.float64).ravel()
        self.N = np.asarray(N, dtype=np.int64).ravel()
        self.dim = self.N.size
        self.dx = np.divide(self.max - self.min, self.N - 1)
        self.vs = [np.linspace(self.min[d].item(), self.max[d].item(), num=int(self.N[d])) for d in range(self.dim)]
        self.bc = ['periodic' if d in tuple(pd) else 'extrapolate' for d in range(self.dim)]
        self.shape = tuple(int(n) for n in self.N)


def shape_of(grid):
    return tuple(int(v) for v in np.asarray(grid.N).ravel())


def node_states(grid):
    """The (M, dim) coordinates of a grid's nodes in C order, from its coordinate vectors."""
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in grid.vs]
    mesh = np.meshgrid(*vs, indexing='ij')
    return np.stack([m.ravel() for m in mesh], axis=1)


def apply_map(xs, A, b):
    """y_i = (((A_i0 x_0) + (A_i1 x_1)) + ...) + b_i for every row of xs: every product taken, left to right."""
    D = xs.shape[1]
    y = np.empty_like(xs)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(D):
            e = A[i, 0] * xs[:, 0]
            for d in range(1, D):
                q = A[i, d] * xs[:, d]
                e = e + q
            y[:, i] = e + b[i]
    return y


def map_table(D, A, b):
    """(list of (A, b) or None for the identity, whether a map was batched): the front end's broadcasting."""
    if A is None and b is None:
        return None, False
    A = np.eye(D) if A is None else np.asarray(A, dtype=np.float64)
    b = np.zeros(D) if b is None else np.asarray(b, dtype=np.float64)
    batched = A.ndim == 3 or b.ndim == 2
    K = A.shape[0] if A.ndim == 3 else (b.shape[0] if b.ndim == 2 else 1)
    A3 = np.broadcast_to(A.reshape(-1, D, D), (K, D, D))
    b2 = np.broadcast_to(b.reshape(-1, D), (K, D))
    return [(A3[k], b2[k]) for k in range(K)], batched


def members_ref(gOld, data, gNew, A=None, b=None):
    """Per member k: v (K, S, M) the interpolant at the image of gNew's nodes, inside (K, M) the mask of nodes member k brings
    inside gOld.  S = 1 for one array.  Also whether a map was batched and whether the data is a stack."""
    D = gOld.dim
    N = shape_of(gOld)
    data = np.asarray(data)
    stacked = not (data.shape == N or data.shape == N + (1,))
    a = data.reshape((-1,) + N)
    xs = node_states(gNew)
    maps, batched = map_table(D, A, b)
    vs, ins = [], []
    for m in (maps if maps is not None else [None]):
        y = xs if m is None else apply_map(xs, m[0], m[1])
        bad = ~np.isfinite(y).all(axis=1)                    # a state that is not finite is outside
        y = np.where(bad[:, None], np.asarray([np.asarray(v).ravel()[0] for v in gOld.vs])[None, :], y)
        outside = Q.locate(gOld, y)[2] | bad
        v = Q.eval_u_ref(gOld, a, y)
        v[:, outside] = np.nan
        vs.append(v)
        ins.append(~outside)
    return np.stack(vs), np.stack(ins), batched, stacked


def resample_ref(gOld, data, gNew=None, A=None, b=None, reduce=None, fill='max', dtype=np.float64, members=None):
    """(out, counts) of transformData: out [K,] [S,] + gNew.shape, counts [K,] [S] the nodes brought inside.  members: what
    members_ref gave for the same grids, data and maps (the tests that run many folds and fills of one case compute it once)."""
    gNew = gOld if gNew is None else gNew
    v, inside, batched, stacked = members_ref(gOld, data, gNew, A, b) if members is None else members
    K, S, M = v.shape
    if reduce is None:
        out, filled = v.copy(), np.broadcast_to(inside[:, None, :], v.shape)
    else:
        op = np.minimum if reduce == 'min' else np.maximum
        acc = np.full((S, M), np.nan)
        got = np.zeros(M, dtype=bool)
        with np.errstate(invalid='ignore'):
            for k in range(K):
                first, later = inside[k] & ~got, inside[k] & got
                acc[:, first] = v[k][:, first]
                acc[:, later] = op(acc[:, later], v[k][:, later])
                got |= inside[k]
        out, filled = acc[None], np.broadcast_to(got[None, None, :], (1, S, M))
    out = out.copy()
    counts = filled.sum(axis=2).astype(np.int64)
    for k in range(out.shape[0]):
        for s in range(S):
            f = filled[k, s]
            if fill == 'nan':
                val = np.nan
            elif fill == 'max':
                good = out[k, s][f]
                good = good[~np.isnan(good)]
                val = good.max() if good.size else np.nan
            else:
                val = float(fill)
            out[k, s][~f] = val
    lead = ((K,) if batched and reduce is None else ()) + ((S,) if stacked else ())
    return out.reshape(lead + shape_of(gNew)).astype(dtype), counts.reshape(lead)


# ------------------------------------------------------------------------------------------ shared test cases
# (source shape, destination shape, periodic axes): the smallest at which the decode, the corner loop and the chunking can go wrong
PAIRS = [((9, 8), (12, 7), ()),
         ((13, 11, 9), (9, 12, 10), (2,)),
         ((7, 6, 8, 5, 9), (6, 7, 5, 6, 8), (2,)),
         ((6, 5, 7, 5, 6, 8), (5, 6, 5, 4, 7, 6), (2, 5)),
         ((37,), (50,), ()),
         ((2, 2, 2, 2, 2), (2, 2, 2, 2, 2), ())]


def pair_bounds(src_shape, pd):
    """(source min, max; destination min, max): the destination is the source box scaled by 1.15 about its centre, moved by 0.05."""
    smin, smax = Q.grid_bounds(src_shape, pd)
    c, h = 0.5 * (smin + smax), 0.5 * (smax - smin)
    return smin, smax, c - 1.15 * h + 0.05, c + 1.15 * h + 0.05


def ref_pair(i):
    """(gOld, gNew) of PAIRS[i] as RefGrids; the last pair is one grid onto itself."""
    src, dst, pd = PAIRS[i]
    smin, smax, dmin, dmax = pair_bounds(src, pd)
    gOld = RefGrid(smin, smax, src, pd)
    return (gOld, gOld) if src == dst and i == len(PAIRS) - 1 else (gOld, RefGrid(dmin, dmax, dst, pd))


def rotation_map(D, theta, p0=0, p1=1, adim=None):
    """rotateData's A and b."""
    A, b = np.eye(D), np.zeros(D)
    c, s = np.cos(-theta), np.sin(-theta)
    A[p0, p0], A[p0, p1], A[p1, p0], A[p1, p1] = c, -s, s, c
    if adim is not None:
        b[adim] = -theta
    return A, b


def maps_for(D, gOld):
    """name -> (A, b) of the maps every pair is run with: the identity, a shift, a rotation by 0.4 in axes (0, 1) with axis 2 as
    the angle (where the grid has those axes)."""
    dx = np.asarray(gOld.dx, dtype=np.float64).ravel()
    out = {'identity': (None, None), 'shift': (np.eye(D), -(0.3 + 0.1 * np.arange(D)) * dx)}
    if D >= 2:
        out['rotation'] = rotation_map(D, 0.4, 0, 1, 2 if D >= 3 else None)
    return out


def field(grid, seed=0, stack=None):
    """A smooth array on the grid (or a time-first stack of `stack` of them) with an fp64 mantissa full of bits."""
    rng = np.random.default_rng(100 + seed)
    shape = shape_of(grid)
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in grid.vs], indexing='ij')
    out = []
    for s in range(stack or 1):
        w = rng.normal(size=grid.dim)
        a = sum(np.sin(w[d] * xs[d] + s) for d in range(grid.dim)) + 0.1 * rng.normal(size=shape)
        out.append(a)
    return np.stack(out) if stack else out[0]
