"""Value functions moved across grids and frames on the device: transformData, migrateGrid, shiftData, rotateData.

Every node of a destination grid takes the multilinear interpolant of a stored array at an affine image y = A x + b of its
own coordinates -- coarse-to-fine migration (the identity), a shift, a rotation, and the union / intersection of one function
placed at K poses, V(x) = min_k V_base(A_k x + b_k), folded in registers.  All of it is one launch of `resample_kernel` in
libhj_resample.so (include/hj_resample.h states the rule operation by operation), on grids of 1 to 6 dimensions, from the
destination's coordinate vectors alone: no dense coordinate array is built, so a `low_mem` destination works.  The interpolant
is eval_u's (csrc/hj_query_dev.h), bit for bit.

migrateGrid, shiftData and rotateData carry helperOC's names and argument order (migrateGrid.m, shiftData.m, rotateData.m);
helperOC is not part of the reference this package is pinned to, so their parity is UNPINNED: they are checked against the
NumPy restatement tests/resample_ref.py and, bit for bit, against eval_u at the same coordinates.

NumPy in -> NumPy out; a device tensor or HostView in -> a tensor on the same device.  Stored value functions with a time axis
are time FIRST, as everywhere in this package.
"""
import ctypes as C
import numbers

import numpy as np

from . import _ffi, _hffi, _mffi
from .context import is_tensor, require_gpu
from .utilities import error
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, stream as _stream, ptr as _ptr, fields as _fields,
                       _descriptor)

__all__ = ["transformData", "migrateGrid", "shiftData", "rotateData", "shiftMap", "rotateMap", "last_path", "last_info"]

_REDUCE = {None: _mffi.REDUCE_NONE, 'min': _mffi.REDUCE_MIN, 'max': _mffi.REDUCE_MAX}

_last_path = ""
_LAST = [None]


def last_path():
    """The kernels the calling process's last resampling launched: "resample_kernel<double, 3, 0>;resample_counts_kernel[;resample_fill_kernel<3, 0>]"."""
    return _last_path


def last_info():
    """Of the calling process's last resampling: dict(counts = filled nodes per output array (int64, shape [K,] [S,]), nodes = the
    destination's node count, K, fields, kernel)."""
    return _LAST[0]


# ------------------------------------------------------------------------------------------ checks without a device
def _shape_of(a):
    a = _unlazy(a)
    return tuple(int(v) for v in (a.shape if hasattr(a, "shape") else np.shape(a)))


def _grid_shape(g):
    return tuple(int(v) for v in np.asarray(g.N).ravel())


def _fill(fill):
    """(fill_mode, fill_value) of 'max' | 'nan' | a number (a NaN number is 'nan')."""
    if isinstance(fill, str):
        if fill == 'max':
            return _mffi.FILL_MAX, 0.0
        if fill == 'nan':
            return _mffi.FILL_NAN, 0.0
    elif isinstance(fill, numbers.Real) and not isinstance(fill, bool):
        return (_mffi.FILL_NAN, 0.0) if fill != fill else (_mffi.FILL_VALUE, float(fill))
    error('fill must be \'max\', \'nan\' or a number (got %r)' % (fill,))


def _maps(D, A, b):
    """(K x (D D + D) fp64 table or None for the identity, K, whether a map was batched)."""
    if A is None and b is None:
        return None, 1, False
    A = np.eye(D) if A is None else np.asarray(A, dtype=np.float64)
    b = np.zeros(D) if b is None else np.asarray(b, dtype=np.float64)
    if A.shape[-2:] != (D, D) or A.ndim not in (2, 3):
        error('A must be (%d, %d) or (K, %d, %d) (got %s)' % (D, D, D, D, A.shape))
    if b.shape[-1:] != (D,) or b.ndim not in (1, 2):
        error('b must be (%d,) or (K, %d) (got %s)' % (D, D, b.shape))
    batched = A.ndim == 3 or b.ndim == 2
    K = A.shape[0] if A.ndim == 3 else (b.shape[0] if b.ndim == 2 else 1)
    if A.ndim == 3 and b.ndim == 2 and A.shape[0] != b.shape[0]:
        error('batched maps disagree on K: A has %d members, b has %d' % (A.shape[0], b.shape[0]))
    if K < 1:
        error('a batch of maps has at least one member')
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        error('A and b must be finite')
    table = np.empty((K, D * D + D), dtype=np.float64)
    table[:, :D * D] = np.broadcast_to(A.reshape(-1, D * D), (K, D * D))
    table[:, D * D:] = np.broadcast_to(b.reshape(-1, D), (K, D))
    return table, K, batched


def _check(gOld, data, gNew, A, b, reduce, fill, dtype):
    D = int(gOld.dim)
    if int(gNew.dim) != D:
        error('gOld.dim = %d and gNew.dim = %d differ: source and destination grids have the same dimension' % (D, int(gNew.dim)))
    if not 1 <= D <= _mffi.MAX_DIM:
        error('grid.dim must be 1..%d (got %d): grids of more than %d dimensions have no device implementation'
              % (_mffi.MAX_DIM, D, _mffi.MAX_DIM))
    if reduce not in _REDUCE:
        error('reduce must be None, \'min\' or \'max\' (got %r)' % (reduce,))
    mode, value = _fill(fill)
    if dtype not in (None, 'float64', 'float32'):
        error('dtype must be \'float64\' or \'float32\' (got %r)' % (dtype,))
    shape, N = _shape_of(data), _grid_shape(gOld)
    single = shape == N or shape == N + (1,)                 # (a 1-D grid's shape is (N, 1))
    if not (single or (len(shape) == D + 1 and shape[1:] == N and shape[0] >= 1)):
        error('data parameter does not agree in array size with grid')
    table, K, batched = _maps(D, A, b)
    return D, table, K, batched, mode, value, not single


# ------------------------------------------------------------------------------------------ the launch
def transformData(gOld, data, gNew=None, A=None, b=None, reduce=None, fill='max', dtype=None, return_info=False):
    """`data` on gOld, resampled onto gNew (None: gOld) through y = A x + b: out(x) = interpolant of data at y.

      A, b      (D, D) and (D,), or batches (K, D, D) / (K, D) of K maps (one may be batched alone); None: the identity / zero
      reduce    None: one result per map, shape [K,] [S,] + gNew.shape (the K axis only when a map was batched);
                'min' / 'max': the fold over the K maps, shape [S,] + gNew.shape.  Maps that send a node outside gOld's
                extrapolated axes are skipped there; a NaN stored in the data propagates (np.minimum / np.maximum)
      fill      the value of a node no map brings inside: 'max' (the largest non-NaN value among the nodes of the same output
                array that were brought inside, helperOC's dataNew(isnan) = max(dataNew) made precise; NaN when there is
                none), 'nan', or a number
      data      gOld.shape or a time-first stack (S,) + gOld.shape; fp32 data stays fp32
      dtype     'float64' | 'float32' of the result (None: the data's); an fp32 result is the fp64 one rounded once
      return_info   also return last_info()'s dict (counts: the nodes brought inside, per output array)

    Everything is checked before a device is asked for."""
    gNew = gOld if gNew is None else gNew
    D, table, K, batched, mode, value, stacked = _check(gOld, data, gNew, A, b, reduce, fill, dtype)
    torch = require_gpu()
    from .shapes import _coord_tables, _leaf_tensor
    t = _leaf_tensor(data)
    name = "float32" if t.dtype == torch.float32 else "float64"
    src, N = _descriptor(_hffi, gOld, name)
    S, stride = _fields(t, N)
    Nn = _grid_shape(gNew)
    dst = _mffi.extents_descriptor(Nn)
    coords = _coord_tables(gNew, torch, t.device)
    red = _REDUCE[reduce]
    arrays = S if red else K * S
    odt = {None: t.dtype, 'float64': torch.float64, 'float32': torch.float32}[dtype]
    out = torch.empty((arrays,) + Nn, dtype=odt, device=t.device)
    counts = torch.empty(arrays, dtype=torch.int64, device=t.device)
    work = torch.empty(int(_mffi.lib().hjm_workspace_size(arrays)) // 8, dtype=torch.int64, device=t.device)
    maps = torch.from_numpy(table).to(t.device) if table is not None else None
    with torch.cuda.device(t.device):
        _mffi.check(_mffi.lib().hjm_resample(C.byref(src), C.byref(dst), C.byref(_mffi.coord_table([c.data_ptr() for c in coords])),
                                             _ptr(t), S, stride, _ptr(maps), K, red, mode, value, _ptr(out),
                                             _ffi.F64 if odt == torch.float64 else _ffi.F32, _ptr(counts), _ptr(work),
                                             _stream(torch, t.device)))
    global _last_path
    _last_path = _mffi.last_kernel()
    lead = ((K,) if batched and not red else ()) + ((S,) if stacked else ())
    out = out.reshape(lead + Nn)
    info = dict(counts=counts.cpu().numpy().reshape(lead), nodes=int(np.prod(Nn)), K=K, fields=S, kernel=_last_path)
    _LAST[0] = info
    if not _wants_tensor(data):
        out = out.cpu().numpy()
    else:
        p = _unlazy(data)
        if is_tensor(p) and not p.is_cuda:
            out = out.to(p.device)
    return (out, info) if return_info else out


def migrateGrid(gOld, dataOld, gNew, fill='max'):
    """helperOC migrateGrid.m: dataOld on gOld resampled onto gNew's nodes (multilinear, periodic axes wrapped); nodes of gNew
    outside gOld's extrapolated axes take `fill` ('max': the largest value that was transferred).  Parity UNPINNED."""
    return transformData(gOld, dataOld, gNew, fill=fill)


def _rows(v, width, what):
    """A (width,) vector or a (K, width) batch as fp64; (array, batched)."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0 and width == 1:
        v = v.reshape(1)
    if v.ndim not in (1, 2) or v.shape[-1] != width:
        error('%s must be (%d,) or (K, %d) (got %s)' % (what, width, width, v.shape))
    return v, v.ndim == 2


def _pdims(g, pdims, count, what):
    p = [int(v) for v in np.asarray(pdims).ravel()]
    if (count is not None and len(p) != count) or len(set(p)) != len(p) or not p or min(p) < 0 or max(p) >= int(g.dim):
        error('%s must name %s distinct axes of the grid\'s %d (got %r)' % (what, 'two' if count == 2 else 'its', int(g.dim), pdims))
    return p


def shiftMap(g, shift, pdims):
    """(A, b) of shiftData: A = I, b[pdims] = -shift; b is (D,) or, for a batch of shifts, (K, D).  Host arithmetic only."""
    D = int(g.dim)
    p = _pdims(g, pdims, None, 'pdims')
    s, batched = _rows(shift, len(p), 'shift')
    b = np.zeros(s.shape[:-1] + (D,))
    b[..., p] = -s
    return np.eye(D), b


def shiftData(g, dataIn, shift, pdims, fill='max', reduce=None):
    """helperOC shiftData.m: dataIn moved by `shift` along the axes pdims, out(x) = dataIn(y) with y[pdims] = x[pdims] - shift.
    shift is (len(pdims),) or a batch (K, len(pdims)): K results, or their fold with reduce = 'min' / 'max'.  The subtraction is
    one rounding, x + (-shift).  Parity UNPINNED."""
    A, b = shiftMap(g, shift, pdims)
    return transformData(g, dataIn, g, A=A, b=b, reduce=reduce, fill=fill)


def rotateMap(g, theta, pdims, adim=None):
    """(A, b) of rotateData; theta a scalar or (K,): (D, D) and (D,), or (K, D, D) and (K, D).  NumPy's cos / sin, on the host."""
    D = int(g.dim)
    p0, p1 = _pdims(g, pdims, 2, 'pdims')
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim not in (0, 1):
        error('theta must be a scalar or (K,) (got %s)' % (th.shape,))
    if adim is not None and (int(adim) in (p0, p1) or not 0 <= int(adim) < D):
        error('adim must be an axis of the grid beside pdims (got %r)' % (adim,))
    lead = th.shape
    A = np.broadcast_to(np.eye(D), lead + (D, D)).copy()
    b = np.zeros(lead + (D,))
    c, s = np.cos(-th), np.sin(-th)
    A[..., p0, p0], A[..., p0, p1] = c, -s
    A[..., p1, p0], A[..., p1, p1] = s, c
    if adim is not None:
        b[..., int(adim)] = -th
    return A, b


def rotateData(g, dataIn, theta, pdims, adim=None, fill='max', reduce=None):
    """helperOC rotateData.m: dataIn rotated by theta (counter-clockwise) in the plane of the two position axes pdims, and moved by
    theta along the heading axis adim when there is one:
        y_p0 = cos(-theta) x_p0 - sin(-theta) x_p1,  y_p1 = sin(-theta) x_p0 + cos(-theta) x_p1,  y_adim = x_adim - theta.
    theta is a scalar or (K,).  The trigonometry is NumPy's, on the host; the device sees A and b.  Parity UNPINNED."""
    A, b = rotateMap(g, theta, pdims, adim)
    return transformData(g, dataIn, g, A=A, b=b, reduce=reduce, fill=fill)
