"""NumPy restatement of libhj_decomp.so (include/hj_decomp.h, levelsetpy_amd/decomp.py) -- TEST INFRASTRUCTURE, NOT PRODUCT
(the package never imports it).

back_project restates the conforming case with np.transpose / reshape / broadcasting: each subsystem array is moved into
the order of the full axes and given extent 1 on every axis it does not cover, then np.maximum / np.minimum fold the
subsystems left to right.  back_project_coords and points restate the interpolating variants through tests/query_ref.py's
eval_u_ref (the interpolant of eval_u, operation by operation).  All values are widened to fp64 first; an fp32 result is
the fp64 one rounded once.  active is the lowest subsystem whose widened value equals the fp64 result, -1 where it is NaN.
costate scatters query_ref's costate of the active subsystem to its full axes.
"""
import numpy as np

import query_ref as Q

OPS = {'intersection': np.maximum, 'union': np.minimum}


def _shape(g):
    return tuple(int(v) for v in np.asarray(g.N).ravel())


def _stack(g, data):
    """(array as (F,) + N in fp64, whether it carried a time axis)."""
    N = _shape(g)
    a = np.asarray(data)
    stacked = a.ndim == len(N) + 1 and a.shape[1:] == N
    return a.astype(np.float64).reshape((-1,) + N), stacked


def _fold(values, mode, dtype, return_active, stacked):
    """values: one broadcastable fp64 array (F_s, ...) per subsystem."""
    op = OPS[mode]
    shape = np.broadcast_shapes(*[v.shape for v in values])
    with np.errstate(invalid='ignore'):
        acc = np.broadcast_to(values[0], shape).copy()
        for v in values[1:]:
            acc = op(acc, v)
        active = np.full(shape, -1, dtype=np.int32)
        for s in reversed(range(len(values))):
            active[np.broadcast_to(values[s], shape) == acc] = s
    active[np.isnan(acc)] = -1
    out = acc.astype(dtype)
    if not stacked:
        out, active = out[0], active[0]
    return (out, active) if return_active else out


def back_project(shape, gs, datas, dims, mode='intersection', dtype=np.float64, return_active=False):
    """The conforming case on a full grid of `shape`: data_s[i[dims_s]] by transposition and broadcasting."""
    D = len(shape)
    values, stacked = [], False
    for g, d, axes in zip(gs, datas, dims):
        a, st = _stack(g, d)
        stacked |= st
        axes = [int(x) for x in axes]
        order = [int(k) for k in np.argsort(axes)]                 # the subsystem's axes in ascending full-axis order
        a = np.transpose(a, [0] + [1 + k for k in order])
        full = [1] * D
        for j, k in enumerate(order):
            full[axes[k]] = a.shape[1 + j]
        assert all(full[x] == shape[x] for x in axes), (full, shape)
        values.append(a.reshape([a.shape[0]] + full))
    return _fold([np.broadcast_to(v, (v.shape[0],) + tuple(shape)) for v in values], mode, dtype, return_active, stacked)


def points(gs, datas, dims, xs, mode='intersection', dtype=np.float64, return_active=False):
    """V at the states xs (M, D): op over eval_u_ref of every subsystem at its own columns."""
    xs = np.asarray(xs, dtype=np.float64)
    xs = xs.reshape(1, -1) if xs.ndim == 1 else xs
    values, stacked = [], False
    for g, d, axes in zip(gs, datas, dims):
        a, st = _stack(g, d)
        stacked |= st
        values.append(Q.eval_u_ref(g, a, xs[:, [int(x) for x in axes]]))
    return _fold(values, mode, dtype, return_active, stacked)


def node_states(coords):
    mesh = np.meshgrid(*coords, indexing='ij')
    return np.stack([m.ravel() for m in mesh], axis=1)


def back_project_coords(coords, gs, datas, dims, mode='intersection', dtype=np.float64, return_active=False):
    """The general case: the nodes of the target grid (one coordinate vector per full axis) as states."""
    coords = [np.asarray(c, dtype=np.float64).ravel() for c in coords]
    shape = tuple(c.size for c in coords)
    res = points(gs, datas, dims, node_states(coords), mode, dtype, return_active)
    res = res if return_active else (res,)
    res = tuple(r.reshape(r.shape[:-1] + shape) for r in res)
    return res if return_active else res[0]


def costate(gs, ogs, datas, dims, xs, scheme, mode='intersection'):
    """(M, D): query_ref's costate of the active subsystem on its own axes, 0 elsewhere, NaN where V is NaN.  ogs: the oracle
    grids of the subsystems; datas: single fp64 arrays."""
    xs = np.asarray(xs, dtype=np.float64)
    _, active = points(gs, datas, dims, xs, mode, return_active=True)
    out = np.zeros(xs.shape)
    out[active < 0] = np.nan
    for s in range(len(gs)):
        rows = np.nonzero(active == s)[0]
        if rows.size:
            axes = [int(x) for x in dims[s]]
            out[np.ix_(rows, axes)] = Q.costate_ref(ogs[s], datas[s], xs[np.ix_(rows, axes)], scheme)
    return out


def sep_grid(g, dims, data, xs='min'):
    """ds of sepGrid: query_ref's projection onto the axes of each dims entry (ascending)."""
    out = []
    for axes in dims:
        mask = np.ones(g.dim, dtype=bool)
        mask[[int(a) for a in axes]] = False
        out.append(Q.proj_ref(g, data, mask, xs) if mask.any() else np.asarray(data))
    return out
