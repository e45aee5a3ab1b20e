"""Decomposed value functions on the device: sepGrid, backProject, Decomposition (reference Grids/sep_grid.py:9).

Everything the solver runs is capped at four dimensions.  The standard way past that in Hamilton-Jacobi reachability is
decomposition into self-contained subsystems: each low-dimensional subsystem is solved on its own grid (three 2-D double
integrators are one HJIPDE_solve_batch call) and the full-dimensional value is

    V(x) = max_s V_s(x[dims[s]])     mode 'intersection' of the back-projections
    V(x) = min_s V_s(x[dims[s]])     mode 'union'

sepGrid cuts a grid and its data into subsystem grids; backProject writes V on the nodes of a full grid of up to 8
dimensions; Decomposition keeps the subsystems on the device and answers queries at states -- V, the active subsystem, the
costate, slices -- for spaces too large to hold (51^6 nodes are 140 GB).  All of it runs in libhj_decomp.so
(include/hj_decomp.h): `backproject_nodes_kernel` when the full grid's nodes are the subsystems' own (a pure index gather,
exact), `backproject_coords_kernel` when they are not (every subsystem interpolated at the node, eval_u's interpolant and
bits), `decomp_points_kernel` at states.  No intermediate array exists and nothing passes through the host.

What the operation means (Chen, Herbert, Vashishtha, Bansal, Tomlin: "Decomposition of reachable sets and tubes for a
class of nonlinear systems"): the UNION of back-projected reachable sets and tubes is exact.  The INTERSECTION is exact for
reachable sets and CONSERVATIVE for tubes: the intersection of the subsystems' tubes contains the full system's tube, it
need not equal it.

dims[s] lists the full axes that the axes of gs[s] stand for, in any order ([2, 0] is legal); subsystems may share axes
(a Dubins car as [0, 2], [1, 2]); an axis no subsystem covers is one along which V is constant.  datas[s] has the shape of
gs[s] or is a time-first stack (T_s,) + that shape with T_s 1 or T; fp64 or fp32 per subsystem, read as it is.

Arithmetic (the header has the definitions): values widened to fp64, np.maximum / np.minimum (a NaN on either side gives
NaN) folded left to right over the subsystems, an fp32 result rounded once at the store.  The active subsystem is the
lowest s whose value equals the result, -1 where the result is NaN.

NumPy in -> NumPy out; a device tensor or a HostView among the subsystems -> a tensor out.

Parity.  The reference's sepGrid cannot run: it calls proj, which raises for every kind of projection, and it has no
back-projection at all.  HELD to the NumPy restatement tests/decomp_ref.py: everything here.
"""
import ctypes as C

import numpy as np

from . import _dffi, _ffi, _qffi
from .context import is_tensor, require_gpu
from .utilities import Bundle, error
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data,
                       device_states as _device_states, stream as _stream, ptr as _ptr, fields as _fields,
                       descriptor as _descriptor, dtype_name as _dtype_name)

__all__ = ["sepGrid", "backProject", "Decomposition", "last_path"]

MAX_DIM, MAX_SUBS = _dffi.MAX_DIM, _dffi.MAX_SUBS
MODES = {'intersection': _dffi.OP_MAX, 'union': _dffi.OP_MIN}

_last_path = ""


def last_path():
    """The kernel the calling process's last back-projection or query ran (hjd_last_kernel)."""
    return _last_path


# ------------------------------------------------------------------------------------------ sepGrid
def sepGrid(g, dims, data=None, xs='min'):
    """sep_grid.py:9: (gs, ds), one grid and one projection per entry of dims.  gs[i], ds[i] = proj(g, data, mask_i, xs) with
    mask_i marking the axes NOT in dims[i]; xs as in proj ('min', 'max' or the point of the removed axes to slice at).  The
    axes of gs[i] are those of dims[i] in ASCENDING order, as proj keeps them: pass sorted(dims[i]) on to backProject.
    With data=None only the grids are built (as proj builds them) and ds is a list of None.

    The reference's own sepGrid cannot run: its proj raises for every kind of projection."""
    from .query import proj, _kept_grid
    Nall = [int(v) for v in np.asarray(g.N).ravel()]
    gs, ds = [], []
    for axes in dims:
        keep = sorted(set(int(a) for a in axes))
        if not keep or keep[0] < 0 or keep[-1] >= g.dim or len(keep) != len(list(axes)):
            error('dims entry %s: distinct axes of the %d of the grid' % (list(axes), g.dim))
        mask = np.ones(g.dim, dtype=bool)
        mask[keep] = False
        if data is None:
            gs.append(g if not mask.any() else _kept_grid(g, keep, [Nall[i] for i in keep], True))
            ds.append(None)
        else:
            gi, di = proj(g, data, mask, xs)
            gs.append(gi)
            ds.append(di)
    return gs, ds


# ------------------------------------------------------------------------------------------ marshalling
def _sub_tensor(data):
    """A subsystem array on the device as it is: fp32 stays fp32 (NumPy's too), anything but fp32 / fp64 becomes fp64."""
    data = _unlazy(data)
    if isinstance(data, np.ndarray) and data.dtype == np.float32:
        a = np.ascontiguousarray(data)
        return require_gpu().from_numpy(a if a.flags.writeable else a.copy()).to("cuda")
    return _device_data(data)


def _axes(g):
    return [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]


class Decomposition(object):
    """The subsystems of a decomposed value function, on the device once.

      gs, datas, dims   as in the module docstring
      mode              'intersection' (max) | 'union' (min)
      ndim              axes of the full space; default: one more than the largest axis any subsystem names

    .T is the number of stored time steps (None when no subsystem carries a time axis)."""

    def __init__(self, gs, datas, dims, mode='intersection', ndim=None):
        torch = require_gpu()
        if mode not in MODES:
            error('mode must be \'intersection\' or \'union\' (got %r)' % (mode,))
        if isinstance(gs, Bundle):
            gs, datas, dims = [gs], [datas], [dims]
        if not (len(gs) == len(datas) == len(dims)) or not 1 <= len(gs) <= MAX_SUBS:
            error('gs, datas and dims must list the same 1 .. %d subsystems' % MAX_SUBS)
        self.gs, self.mode = list(gs), mode
        self.dims = [[int(a) for a in np.asarray(d).ravel()] for d in dims]
        self.ndim = int(ndim) if ndim is not None else 1 + max(max(d) for d in self.dims)
        if not 1 <= self.ndim <= MAX_DIM:
            error('a full space of 1 .. %d axes has a device implementation (got %d)' % (MAX_DIM, self.ndim))
        self.wants_tensor = any(_wants_tensor(d) for d in datas)
        self.tensors, self.descs, subs, stacks = [], [], [], []
        for s, (g, d, axes) in enumerate(zip(self.gs, datas, self.dims)):
            if len(axes) != g.dim or len(set(axes)) != len(axes) or min(axes) < 0 or max(axes) >= self.ndim:
                error('dims[%d] = %s: %d distinct axes of the %d of the full space' % (s, axes, g.dim, self.ndim))
            t = _sub_tensor(d)
            if self.tensors and t.device != self.tensors[0].device:
                t = t.to(self.tensors[0].device)
            desc, N = _descriptor(g, _dtype_name(t))
            F, stride = _fields(t, N)
            stacks.append(t.dim() == len(N) + 1 and tuple(t.shape[1:]) == N)
            self.tensors.append(t)
            self.descs.append((desc, N, F, stride))
        counts = set(F for (_, _, F, _), st in zip(self.descs, stacks) if st)
        self.T = max(counts) if counts else None
        if len(counts - {1}) > 1:
            error('the subsystems\' time stacks disagree: %s steps' % sorted(counts))
        self.F = self.T or 1
        for t, (desc, N, F, stride), axes in zip(self.tensors, self.descs, self.dims):
            subs.append((desc, t.data_ptr(), F, stride, axes))
        self.device = self.tensors[0].device
        self.desc = _dffi.decomp(self.ndim, MODES[mode], subs)
        self.dtype = 'float32' if all(t.dtype == torch.float32 for t in self.tensors) else 'float64'

    # ---- the three entry points
    def _finish(self, out, active, lead, return_active):
        global _last_path
        _last_path = _dffi.last_kernel()
        shape = (() if self.T is None else (self.F,)) + tuple(lead)
        res = [out.reshape(shape)] + ([active.reshape(shape)] if return_active else [])
        if not self.wants_tensor:
            res = [r.cpu().numpy() for r in res]
        return tuple(res) if return_active else res[0]

    def _out(self, count, dtype, return_active):
        torch = require_gpu()
        dtype = self.dtype if dtype is None else dtype
        if dtype not in ('float64', 'float32'):
            error('dtype must be \'float64\' or \'float32\' (got %r)' % (dtype,))
        out = torch.empty((self.F, count), dtype=torch.float64 if dtype == 'float64' else torch.float32, device=self.device)
        active = torch.empty((self.F, count), dtype=torch.int32, device=self.device) if return_active else None
        return out, active, _ffi.F64 if dtype == 'float64' else _ffi.F32

    def _on_nodes(self, N, coords, dtype, return_active):
        """coords None: the nodes kernel; else one fp64 vector per full axis: the interpolating kernel."""
        torch = require_gpu()
        out, active, did = self._out(int(np.prod(N, dtype=np.int64)), dtype, return_active)
        with torch.cuda.device(self.device):
            if coords is None:
                rc = _dffi.lib().hjd_backproject_nodes(C.byref(self.desc), _dffi.extents(N), self.F, _ptr(out), did, _ptr(active),
                                                       _stream(torch, self.device))
            else:
                tabs = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64).copy()).to(self.device) for c in coords]
                rc = _dffi.lib().hjd_backproject_coords(C.byref(self.desc), _dffi.extents(N), _dffi.tables([t.data_ptr() for t in tabs]),
                                                        self.F, _ptr(out), did, _ptr(active), _stream(torch, self.device))
            _dffi.check(rc)
        return out, active

    def _at_states(self, xs, dtype, return_active):
        torch = require_gpu()
        xs = _unlazy(xs)
        if not is_tensor(xs):
            xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim == 1:
            xs = xs.reshape(1, -1)
        if xs.ndim != 2 or xs.shape[1] != self.ndim:
            error('states must be an (M, %d) array' % self.ndim)
        x = _device_states(xs, self.device)
        M = int(x.shape[0])
        out, active, did = self._out(M, dtype, return_active)
        with torch.cuda.device(self.device):
            _dffi.check(_dffi.lib().hjd_points(C.byref(self.desc), _ptr(x), M, self.F, _ptr(out), int(did == _ffi.F64), _ptr(active),
                                               _stream(torch, self.device)))
        return out, active, x

    # ---- queries
    def eval_u(self, xs, dtype=None):
        """V at the states xs (one per row, ndim columns): (M,), or (T, M) for time stacks.  A state outside an extrapolated
        axis of a subsystem that covers it gives NaN; periodic axes wrap."""
        out, active, _ = self._at_states(xs, dtype, False)
        return self._finish(out, active, (out.shape[1],), False)

    def eval_active(self, xs):
        """The active subsystem at the states: int32 of eval_u's shape, -1 where V is NaN."""
        out, active, _ = self._at_states(xs, None, True)
        return self._finish(out, active, (out.shape[1],), True)[1]

    def eval_costate(self, xs, derivFunc=None, t=None):
        """grad V at the states: (M, ndim) fp64.  Each row is eval_costate of the state's ACTIVE subsystem on that
        subsystem's own axes, 0.0 on every other axis (V is locally the active subsystem's value, which does not depend on
        them), and NaN on every axis where V is NaN.  With time stacks, t is the stored step to differentiate."""
        from .query import eval_costate
        torch = require_gpu()
        if self.T is not None and self.T > 1 and t is None:
            error('the decomposition holds %d stored steps: pass t, the step to differentiate' % self.T)
        t = 0 if t is None else int(t) % self.F
        _, active, x = self._at_states(xs, 'float64', True)
        act = active[t].long()
        res = torch.zeros((x.shape[0], self.ndim), dtype=torch.float64, device=self.device)
        for s in torch.unique(act).tolist():
            rows = (act == s).nonzero().reshape(-1)
            if s < 0:
                res[rows] = float('nan')
                continue
            desc, N, F, stride = self.descs[s]
            field = self.tensors[s].reshape((F,) + N)[t if F > 1 else 0]
            cs = eval_costate(self.gs[s], field, x[rows][:, self.dims[s]], derivFunc)
            res[rows[:, None], torch.as_tensor(self.dims[s], device=self.device)[None, :]] = cs.to(torch.float64).reshape(len(rows), -1)
        return res if self.wants_tensor else res.cpu().numpy()

    # ---- on grids
    def on_grid(self, g, method='auto', dtype=None, return_active=False):
        """V on the nodes of the full grid g: backProject(g, ...) of these subsystems."""
        if g.dim != self.ndim:
            error('the grid has %d dimensions, the decomposition %d' % (g.dim, self.ndim))
        if method not in ('auto', 'nodes', 'interp'):
            error('method must be \'auto\', \'nodes\' or \'interp\' (got %r)' % (method,))
        full = _axes(g)
        N = [v.size for v in full]
        conform = all(np.array_equal(full[a], v) for gs, axes in zip(self.gs, self.dims) for a, v in zip(axes, _axes(gs)))
        if method == 'nodes' and not conform:
            error('the grids do not conform: a covered axis of g has other nodes than the subsystem\'s (method=\'interp\' interpolates)')
        out, active = self._on_nodes(N, None if (conform and method != 'interp') else full, dtype, return_active)
        return self._finish(out, active, tuple(N) + ((1,) if g.dim == 1 else ()), return_active)

    def slice(self, g, keep, at, dtype=None, return_active=False):
        """V on the nodes of the axes `keep` of g with every other axis fixed at the coordinates `at` (one per fixed axis, in
        axis order): an array over the kept axes.  Runs the interpolating kernel with one-node axes."""
        if g.dim != self.ndim:
            error('the grid has %d dimensions, the decomposition %d' % (g.dim, self.ndim))
        keep = sorted(set(int(a) for a in keep))
        gone = [a for a in range(g.dim) if a not in keep]
        at = np.asarray(at, dtype=np.float64).ravel()
        if not keep or keep[0] < 0 or keep[-1] >= g.dim or at.size != len(gone):
            error('keep names axes of g and `at` has one coordinate per other axis')
        coords = _axes(g)
        for a, v in zip(gone, at):
            coords[a] = np.array([v])
        out, active = self._on_nodes([c.size for c in coords], coords, dtype, return_active)
        return self._finish(out, active, tuple(coords[a].size for a in keep), return_active)


def backProject(g, gs, datas, dims, mode='intersection', method='auto', dtype=None, return_active=False):
    """The decomposed value function on the nodes of the full grid g: an array of g.shape, or (T,) + g.shape for time stacks
    [, the int32 active subsystem of the same shape].

      g        any grid Bundle of up to 8 dimensions; only g.vs and g.N are read, so a low_mem grid works
      method   'auto': backproject_nodes_kernel when every covered axis of g has the subsystem's own nodes (array_equal),
               else the interpolating backproject_coords_kernel; 'nodes' raises when they do not; 'interp' forces the latter
      dtype    'float64' | 'float32'; default fp32 when every subsystem is fp32, else fp64"""
    return Decomposition(gs, datas, dims, mode, ndim=g.dim).on_grid(g, method, dtype, return_active)
