"""Value-function queries on the device: eval_u, eval_costate, proj, augmentPeriodicData (reference
ValueFuncs/evaluate_u.py:15, data_proj.py:18, augment_periodic.py:12) -- what a caller does with the result of
HJIPDE_solve: V(x) and grad V(x) at many states, projections and slices.

All of it runs in libhj_query.so (include/hj_query.h): `interp_points_kernel` (V at states),
`costate_points_kernel` (grad V at states from the solver's own upwind source, without full-grid derivative
arrays) and `project_minmax_kernel`.  On 5-D and 6-D grids the same calls run in libhj_hiquery.so
(include/hj_hiquery.h: `hi_interp_points_kernel`, `hi_costate_points_kernel`, `hi_project_minmax_kernel`), which compiles
the same device functions at six axes; grids of seven and more axes are refused.  NumPy in -> NumPy out (fp64); a device tensor or HostView in -> a tensor
on the same device, in the data's dtype.  Stored value functions with a time axis are time FIRST, as
everywhere in this package.

Parity.  The reference's eval_u returns `v.take(0)` -- ONE value whatever the number of states --, raises on
every grid with a periodic axis >= 1 (augmentPeriodicData indexes `data[i, ...]`), and raises "out of bounds"
for states beyond the last node of a periodic axis 0; its proj raises for 'min', 'max' and slices alike.
Pinned to the reference (tests/golden/query.npz): eval_u of single in-domain states on non-periodic grids and
on grids periodic in axis 0.  UNPINNED, checked against the NumPy restatement tests/query_ref.py: many states,
every other periodic case, eval_costate, proj, augmentPeriodicData (the intended helperOC semantics).
"""
import ctypes as C

import numpy as np

from . import _ffi, _qffi, _xffi
from .context import grid_bc, is_tensor, require_gpu, _raw_stream_getter
from .lazy import HostView, DeviceArray
from .utilities import Bundle, error, warn
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, from_numpy as _from_numpy,      # noqa: F401
                       device_data as _device_data, device_states as _device_states, stream as _stream, ptr as _ptr,
                       fields as _fields, descriptor as _descriptor, dtype_name as _dtype_name, descriptor_hi as _descriptor_hi,
                       is_hi as _is_hi)

__all__ = ["eval_u", "eval_costate", "proj", "augmentPeriodicData"]


# ------------------------------------------------------------------------------------------ marshalling
def _library(g, dtype_name):
    """(binding, function prefix, descriptor, shape) of the library that serves grid g: libhj_query.so up to 4-D, libhj_hiquery.so
    (the same entry points on hjh_grid) at 5-D and 6-D."""
    if _is_hi(g):
        desc, N = _descriptor_hi(g, dtype_name)
        return _xffi, "hjx_", desc, N
    desc, N = _descriptor(g, dtype_name)
    return _qffi, "hjq_", desc, N


def last_kernel(g):
    """The kernel the calling thread's last query on a grid of g's dimension launched."""
    return (_xffi if _is_hi(g) else _qffi).last_kernel()


def interp_states(g, data, xs, out_f64=False):
    """V at states for one array or a stack on grid g: device tensors in, a (F, M) tensor out (F = 1 for one array).
    `xs` is an (M, dim) fp64 device tensor.  out_f64: the unrounded fp64 sum whatever the data's dtype."""
    torch = require_gpu()
    ffi, pre, desc, N = _library(g, _dtype_name(data))
    F, stride = _fields(data, N)
    if xs.dim() != 2 or xs.shape[1] != g.dim or xs.shape[0] < 1:
        error('states must be an (M, %d) array' % g.dim)
    M = int(xs.shape[0])
    out = torch.empty((F, M), dtype=torch.float64 if out_f64 else data.dtype, device=data.device)
    with torch.cuda.device(data.device):
        ffi.check(getattr(ffi.lib(), pre + "interp_points")(C.byref(desc), _ptr(data), F, stride, _ptr(xs), M, _ptr(out),
                                                            int(bool(out_f64)), _stream(torch, data.device)))
    return out


def costate_states(g, data, xs, scheme, out_f64=False, want_lr=False, want_value=False):
    """grad V at states: (F, M, dim) costates [, derivL, derivR (same shape), V (F, M)] from hjq_costate_points
    (hjx_costate_points at 5-D / 6-D)."""
    torch = require_gpu()
    ffi, pre, desc, N = _library(g, _dtype_name(data))
    F, stride = _fields(data, N)
    if xs.dim() != 2 or xs.shape[1] != g.dim or xs.shape[0] < 1:
        error('states must be an (M, %d) array' % g.dim)
    M = int(xs.shape[0])
    odt = torch.float64 if out_f64 else data.dtype
    mk = lambda *s: torch.empty(s, dtype=odt, device=data.device)       # noqa: E731
    cs = mk(F, M, g.dim)
    dl, dr = (mk(F, M, g.dim), mk(F, M, g.dim)) if want_lr else (None, None)
    val = mk(F, M) if want_value else None
    with torch.cuda.device(data.device):
        ffi.check(getattr(ffi.lib(), pre + "costate_points")(C.byref(desc), int(scheme), _ptr(data), F, stride, _ptr(xs), M,
                                                             _ptr(cs), _ptr(dl), _ptr(dr), _ptr(val), int(bool(out_f64)),
                                                             _stream(torch, data.device)))
    return cs, dl, dr, val


def _give(t, proto, squeeze0=False):
    """The result in the array type of `proto`."""
    if squeeze0:
        t = t[0]
    if _wants_tensor(proto):
        p = _unlazy(proto)
        return t if (not is_tensor(p) or p.is_cuda) else t.to(p.device)
    return t.detach().cpu().numpy()


def states_2d(g, xs):
    """States as rows: a vector is one state; a matrix whose column count is not g.dim is transposed (evaluate_u.py:83).
    Works on a copy -- the caller's array is never modified (the reference wraps it in place)."""
    xs = _unlazy(xs)
    nd = xs.dim() if is_tensor(xs) else np.ndim(xs)
    if not is_tensor(xs):
        xs = np.asarray(xs, dtype=np.float64)
    if nd == 1:
        xs = xs.reshape(1, -1)
    elif nd != 2:
        error('states must be a vector or a matrix with one state per row')
    if xs.shape[1] != g.dim:
        xs = xs.T
    if xs.shape[1] != g.dim:
        error('states must have g.dim = %d columns' % g.dim)
    return xs


def _is_single_state(g, xs):
    xs = _unlazy(xs)
    shape = tuple(xs.shape) if hasattr(xs, "shape") else np.shape(np.asarray(xs, dtype=np.float64))
    return len(shape) == 1 or (len(shape) == 2 and 1 in shape and int(np.prod(shape)) == g.dim)


def _ndim(a):
    a = _unlazy(a)
    return a.dim() if is_tensor(a) else np.ndim(a)


# ------------------------------------------------------------------------------------------ eval_u
def _eval_single(g, data, xs):
    """One grid; one array (-> (M,)) or a time-first stack (-> (T, M))."""
    nd = _ndim(data)
    gd = len(np.asarray(g.N).ravel())
    if nd not in (gd, gd + 1):
        error('Dimensions of input data and grid don\'t match!')
    t = _device_data(data)
    x = _device_states(states_2d(g, xs), t.device)
    out = interp_states(g, t, x)
    if nd == gd + 1 and _is_single_state(g, xs):
        return _give(out[:, 0], data)                   # option 2: one value per array
    return _give(out, data, squeeze0=(nd == gd))


def eval_u(gs, datas, xs, interp_method='linear'):
    """evaluate_u.py:15: the multilinear interpolant of value function(s) at state(s).

      1. one grid, one array, many states (one per row)           -> ALL M values, shape (M,)
      2. one grid, a list or a time-first stack of arrays, one state -> one value per array, shape (T,)
      3. lists of grids, arrays and states of equal length        -> one result per triple

    A time-first stack with many states gives (T, M).  Periodic axes wrap the state into the period (any number of
    periods away); a state outside an extrapolated axis gives NaN.  `xs` is transposed when its column count is not
    g.dim, as the reference does.

    Deviations from the shipped reference: its option 1 returns `v.take(0)`, the value at the FIRST state only --
    a defect, all M values are returned here; it modifies the caller's `xs` and grid in place -- neither is touched
    here; it raises on periodic axes >= 1 and past the last node of a periodic axis 0 (module docstring)."""
    if interp_method != 'linear':
        error('interp_method %r is not implemented: only \'linear\'' % (interp_method,))
    if isinstance(gs, Bundle) and not isinstance(datas, (list, tuple)):
        if not (is_tensor(_unlazy(xs)) or isinstance(xs, (np.ndarray, list, tuple))):
            error('Unrecognized combination of input data types!')
        return _eval_single(gs, datas, xs)                                     # options 1 and 2 (stack)
    if isinstance(gs, Bundle) and isinstance(datas, (list, tuple)):
        if not _is_single_state(gs, xs):                                       # option 2 wants ONE state
            error('Unrecognized combination of input data types!')
        if len(datas) == 0:
            error('datas is empty')
        vals = [_eval_single(gs, d, xs) for d in datas]
        return _stack(vals, datas[0], flat=True)
    if isinstance(gs, (list, tuple)) and isinstance(datas, (list, tuple)) and isinstance(xs, (list, tuple)):
        if not (len(gs) == len(datas) == len(xs)) or len(gs) == 0:
            error('the numbers of grids, value functions and states must be equal')
        vals = [_eval_single(gi, di, xi) for gi, di, xi in zip(gs, datas, xs)]
        return _stack(vals, datas[0], flat=all(_is_single_state(gi, xi) for gi, xi in zip(gs, xs)))
    error('Unrecognized combination of input data types!')


def _stack(vals, proto, flat):
    if _wants_tensor(proto):
        torch = require_gpu()
        if flat:
            return torch.cat([v.reshape(-1) for v in vals])
        return torch.stack(vals) if len(set(tuple(v.shape) for v in vals)) == 1 else vals
    if flat:
        return np.concatenate([np.asarray(v).reshape(-1) for v in vals])
    return np.stack(vals) if len(set(np.shape(v) for v in vals)) == 1 else vals


# ------------------------------------------------------------------------------------------ eval_costate
def point_scheme(derivFunc):
    """Scheme id for hjq_costate_points, or None when the derivative function has no point kernel: a foreign
    function, or the intended WENO5 (its epsilon is a reduction over the whole grid)."""
    from .spatial import scheme_id_of
    sid = scheme_id_of(derivFunc)
    if sid is None:
        return None
    sid = {4: _ffi.ENO2, 5: _ffi.ENO3}.get(sid, sid)      # the 'fast' ENO modes: hj_upwind computes the base scheme for them too
    return sid if sid in _qffi.POINT_SCHEMES else None


def eval_costate(g, data, xs, derivFunc=None, dims=None):
    """grad V at states: an (M, g.dim) array, (T, M, g.dim) for a time-first stack.

    Equal, bit for bit, to eval_u applied to computeGradients' derivC arrays of the same data -- the corner nodes'
    upwind derivatives come from the same source (hj_device.h upwind<>), 0.5 (L + R) and the interpolation are the
    same operations -- but only the 2^dim corner stencils of each state are read, and no full-grid array is written.
    derivFunc defaults to upwindFirstWENO5, dims (a mask) to every dimension, as computeGradients; columns of
    dimensions left out hold NaN.  upwindFirstENO2 / ENO3 / WENO5 (as shipped) run in costate_points_kernel; the
    intended WENO5 and foreign derivative functions take computeGradients and then the interpolation kernel.
    Non-finite data as computeGradients: a NaN / inf node counts as 1e6 in its neighbours' stencils and contributes
    NaN / inf itself.  Parity UNPINNED (the reference has no such function)."""
    from .spatial import upwindFirstWENO5
    if dims is None or (not is_tensor(dims) and not np.any(dims)):
        dims = np.ones(g.dim, dtype=bool)
    dims = np.asarray(dims).astype(bool).ravel()
    if dims.size != g.dim:
        error('dims must have one entry per grid dimension')
    if derivFunc is None:
        derivFunc = upwindFirstWENO5
    nd = _ndim(data)
    if nd not in (g.dim, g.dim + 1):
        error('Dimensions of input data and grid don\'t match!')
    sid = point_scheme(derivFunc)
    if sid is not None:
        t = _device_data(data)
        x = _device_states(states_2d(g, xs), t.device)
        cs = costate_states(g, t, x, sid)[0]
    else:
        cs = _costate_fallback(g, data, xs, derivFunc, dims)
    if not dims.all():
        cs[..., np.nonzero(~dims)[0].tolist()] = float('nan')
    return _give(cs, data, squeeze0=(nd == g.dim))


def _costate_fallback(g, data, xs, derivFunc, dims, out_f64=False):
    """computeGradients, then the interpolation kernel on its arrays -> (F, M, dim) tensor."""
    from .gradients import computeGradients
    torch = require_gpu()
    derivC, _, _ = computeGradients(g, _unlazy(data), dims, derivFunc)
    cols, x = [], None
    for d in range(g.dim):
        if not dims[d]:
            cols.append(None)
            continue
        t = _device_data(derivC[d])
        if x is None:
            x = _device_states(states_2d(g, xs), t.device)
        cols.append(interp_states(g, t, x, out_f64))
    first = next(c for c in cols if c is not None)
    cols = [torch.full_like(first, float('nan')) if c is None else c for c in cols]
    return torch.stack(cols, dim=-1)


# ------------------------------------------------------------------------------------------ proj
def augmentPeriodicData(g, data):
    """augment_periodic.py:12 with the semantics it was ported from (helperOC augmentPeriodicData.m): every periodic
    axis gains one node, vs[-1] + dx, that holds the data of index 0 ALONG THAT AXIS (the shipped reference takes
    `data[i, ...]`, plane i of axis 0, and raises for i >= 1).  Returns (gOut, dataOut) on copies: the caller's grid
    and array are not modified.  A time-first stack is augmented along its grid axes.  Parity UNPINNED."""
    bc, _ = grid_bc(g)
    gOut = Bundle(dict((k, v) for k, v in g.__dict__.items() if not k.startswith("_hj")))
    gOut.vs = [np.array(v, dtype=np.float64) for v in g.vs]
    data = _unlazy(data)
    lead = _ndim(data) - g.dim
    if lead not in (0, 1):
        error('Dimensions of input data and grid don\'t match!')
    out = data.clone() if is_tensor(data) else np.array(data)
    dx = np.asarray(g.dx, dtype=np.float64).ravel()
    for i in range(g.dim):
        if bc[i] != _ffi.BC_PERIODIC:
            continue
        v = gOut.vs[i]
        gOut.vs[i] = np.concatenate((v, np.reshape(v.ravel()[-1] + dx[i], (1,) * v.ndim)), 0)
        if is_tensor(out):
            torch = require_gpu()
            out = torch.cat((out, out.narrow(lead + i, 0, 1)), lead + i)
        else:
            out = np.concatenate((out, np.take(out, [0], axis=lead + i)), lead + i)
    return gOut, out


def _kept_grid(g, keep, N, process):
    """gOut as data_proj.py:136-150 builds it: min / max / bdry of the kept axes, N, processGrid when asked."""
    from .grids import processGrid
    gmin, gmax = np.asarray(g.min, dtype=np.float64).reshape(-1, 1), np.asarray(g.max, dtype=np.float64).reshape(-1, 1)
    gOut = Bundle(dict(dim=len(keep), min=gmin[keep], max=gmax[keep]))
    gOut.bdry = [g.bdry[i] for i in keep]
    if hasattr(g, "bdryData") and g.bdryData is not None:
        gOut.bdryData = [g.bdryData[i] for i in keep]
    gOut.N = np.asarray(N, dtype=np.int64).reshape(-1, 1)
    return processGrid(gOut) if process else gOut


# A projection kernel runs one thread (last axis kept) or one wavefront (last axis removed) per OUTPUT node.  On a 5-D / 6-D grid
# the usual projections keep two axes of six -- 625 output nodes for 2.4e8 cells at 25^6 --, far too few to fill the device.  With
# fewer output nodes than this, the leading removed axes are removed first, in a launch that still has this many output nodes and
# reads the array once; the rest is removed from its result, which is smaller by those axes' extents.  min and max are exact and
# a NaN survives both launches, so the result has the bits of the single launch.
PROJ_STAGE_NODES = 1 << 16


def _axes_bundle(g, keep):
    """What the descriptors read of grid g (dim, N, dx, vs, bdry), for the axes `keep` alone."""
    b = Bundle(dict(dim=len(keep), N=np.asarray(g.N).ravel()[keep].reshape(-1, 1), dx=np.asarray(g.dx).ravel()[keep].reshape(-1, 1),
                    vs=[g.vs[i] for i in keep], bdry=[g.bdry[i] for i in keep]))
    if hasattr(g, "bdryData") and g.bdryData is not None:
        b.bdryData = [g.bdryData[i] for i in keep]
    return b


def _project_minmax(g, t, gone, op):
    """min / max (op: _qffi.OP_*) of the contiguous (F,) + g.shape tensor t over the axes `gone` -> (F,) + kept shape."""
    ffi, pre, desc, N = _library(g, _dtype_name(t))
    F = int(t.shape[0])
    keep = [i for i in range(g.dim) if i not in gone]
    first = []
    if _is_hi(g) and int(np.prod([N[i] for i in keep])) < PROJ_STAGE_NODES:
        nodes = int(np.prod(N))
        for i in gone[:-1]:                                   # ascending: the last removed axis stays for the second launch
            if nodes // N[i] < PROJ_STAGE_NODES:
                break
            nodes //= N[i]
            first.append(i)
    if first:
        rest = [i for i in range(g.dim) if i not in first]
        part = _project_launch(ffi, pre, desc, N, t, F, first, op)
        return _project_minmax(_axes_bundle(g, rest), part, [k for k, i in enumerate(rest) if i in gone], op)
    return _project_launch(ffi, pre, desc, N, t, F, gone, op)


def _project_launch(ffi, pre, desc, N, t, F, gone, op):
    torch = require_gpu()
    out = torch.empty((F,) + tuple(n for i, n in enumerate(N) if i not in gone), dtype=t.dtype, device=t.device)
    with torch.cuda.device(t.device):
        ffi.check(getattr(ffi.lib(), pre + "project_minmax")(C.byref(desc), _ptr(t), F, int(np.prod(N)), sum(1 << i for i in gone), op,
                                                             _ptr(out), _stream(torch, t.device)))
    return out


def proj(g, data, dimsToRemove, xs=None, NOut=None, process=True):
    """data_proj.py:18: (gOut, dataOut) = the data on the grid of the axes NOT marked in dimsToRemove.

      xs None / 'min' / 'max'   union / intersection over the removed axes (project_minmax_kernel)
      xs a vector               the slice at that point of the removed axes, multilinear, periodic removed axes wrapped
                                (interp_points_kernel at the kept axes' nodes x the fixed coordinates)
      NOut                      nodes of the output grid when they differ from the kept axes' N: the result is
                                resampled onto gOut's nodes through the interpolation kernel

    `data` may carry a time axis, time FIRST (the result is then (T,) + gOut.shape), or be a list of arrays.  gOut is
    built as the reference builds it.  Keeping every dimension returns the inputs with a warning.  On a 5-D / 6-D grid a
    min / max that leaves fewer than PROJ_STAGE_NODES output nodes takes two launches (above), with the bits of one.  The shipped
    reference raises for every kind of projection: parity UNPINNED, checked against tests/query_ref.py."""
    rem = np.asarray(_unlazy(dimsToRemove) if not is_tensor(dimsToRemove) else dimsToRemove.cpu().numpy()).astype(bool).ravel()
    if rem.size != g.dim:
        error('Dimensions are inconsistent!')
    if not rem.any():
        warn('Input and output dimensions are the same!')
        return g, data
    if rem.all():
        error('proj cannot remove every dimension')
    if xs is None:
        xs = 'min'
    if isinstance(xs, str):
        if xs not in ('min', 'max'):
            error('xs must be a vector, \'min\', or \'max\'!')
    else:
        xs = np.asarray(_unlazy(xs).cpu().numpy() if is_tensor(_unlazy(xs)) else xs, dtype=np.float64).ravel()
        if xs.size != int(rem.sum()):
            error('Dimension of xs and dims do not match!')
    if isinstance(data, (list, tuple)):
        if len(data) == 0:
            error('Inconsistent input data dimensions!')
        proto = data[0]
        if _wants_tensor(proto):
            data = require_gpu().stack([_device_data(d) for d in data])
        else:
            data = np.stack([np.asarray(d, dtype=np.float64) for d in data])
    else:
        proto = data
    nd = _ndim(data)
    if nd not in (g.dim, g.dim + 1):
        error('Inconsistent input data dimensions!')
    keep = [i for i in range(g.dim) if not rem[i]]
    gone = [i for i in range(g.dim) if rem[i]]
    Nall = [int(v) for v in np.asarray(g.N).ravel()]
    Nkeep = [Nall[i] for i in keep]
    if NOut is None:
        Nout = list(Nkeep)
    else:
        Nout = [int(v) for v in np.asarray(NOut).ravel()]
        if len(Nout) == 1:
            Nout = Nout * len(keep)
        if len(Nout) != len(keep) or min(Nout) < 1:
            error('NOut must be a scalar or have one entry per kept dimension')
    gOut = _kept_grid(g, keep, Nout, process)
    torch = require_gpu()
    t = _device_data(data)
    N = _library(g, _dtype_name(t))[3]                   # (a grid no library serves is refused here, before any launch)
    F = _fields(t, N)[0]
    resample = Nout != Nkeep
    if isinstance(xs, str):
        out = _project_minmax(g, t.reshape((F,) + tuple(N)), gone, _qffi.OP_MIN if xs == 'min' else _qffi.OP_MAX)
        if resample:
            gK = _kept_grid(g, keep, Nkeep, True)
            out = interp_states(gK, out, _device_states(_node_states(gK, gOut, range(len(keep)), [], []), t.device))
            out = out.reshape((F,) + tuple(Nout))
    else:
        pts = _node_states(g, gOut if resample else None, keep, gone, xs)
        out = interp_states(g, t, _device_states(pts, t.device)).reshape((F,) + tuple(Nout))
    return gOut, _give(out, proto, squeeze0=(nd == g.dim))


def _nodes(gOut, k):
    """Nodes of axis k of an output grid (processGrid's linspace, :204, also when the grid was not processed)."""
    if hasattr(gOut, "vs"):
        return np.asarray(gOut.vs[k], dtype=np.float64).ravel()
    return np.linspace(float(np.asarray(gOut.min).ravel()[k]), float(np.asarray(gOut.max).ravel()[k]),
                       num=int(np.asarray(gOut.N).ravel()[k]))


def _node_states(g, gOut, keep, gone, fixed):
    """(M, g.dim) states: the nodes of the kept axes (gOut's when resampling, else g's own) in C order x the fixed
    coordinates of the removed axes."""
    axes = [(_nodes(gOut, k) if gOut is not None else np.asarray(g.vs[i], dtype=np.float64).ravel())
            for k, i in enumerate(keep)]
    mesh = np.meshgrid(*axes, indexing='ij') if axes else []
    M = int(np.prod([a.size for a in axes])) if axes else 1
    pts = np.empty((M, g.dim), dtype=np.float64)
    for k, i in enumerate(keep):
        pts[:, i] = mesh[k].ravel()
    for k, i in enumerate(gone):
        pts[:, i] = fixed[k]
    return pts
