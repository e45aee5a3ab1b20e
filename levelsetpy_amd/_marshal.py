"""Marshalling shared by the front ends of the stateless libraries (every module that imports it): what
array type a result takes, how NumPy arrays, HostViews and tensors become contiguous device tensors, raw pointers and streams
for ctypes, and how a grid becomes the hjq_grid descriptor."""
import ctypes as C

import numpy as np

from . import _hffi, _qffi
from .context import array_dtype_name as dtype_name, grid_bc, is_tensor, require_gpu, _raw_stream_getter   # noqa: F401
from .lazy import HostView, DeviceArray
from .utilities import error


def unlazy(a):
    if isinstance(a, HostView):
        return a.device_tensor() if a.device_tensor() is not None else a.__array__()
    if isinstance(a, DeviceArray) and a.device_tensor() is not None:
        return a.device_tensor()
    return a


def wants_tensor(a):
    """NumPy in -> NumPy out; a device tensor or a HostView in -> a tensor out."""
    return is_tensor(a) or isinstance(a, HostView)


def from_numpy(torch, a):
    arr = np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    return torch.from_numpy(arr if arr.flags.writeable else arr.copy())


def device_data(a):
    """-> contiguous fp64 / fp32 tensor on the GPU (NumPy and other dtypes: fp64, as the reference path)."""
    torch = require_gpu()
    a = unlazy(a)
    if is_tensor(a):
        t = a if a.is_cuda else a.to("cuda")
        if t.dtype not in (torch.float64, torch.float32):
            t = t.to(torch.float64)
        return t.contiguous()               # never read a view with the strides of its base
    return from_numpy(torch, a).to("cuda")


def device_states(xs, device):
    torch = require_gpu()
    xs = unlazy(xs)
    if is_tensor(xs):
        return xs.detach().to(device=device, dtype=torch.float64).contiguous()
    return from_numpy(torch, xs).to(device)


def stream(torch, device):
    return C.c_void_p(_raw_stream_getter(torch)(device.index))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def fields(t, N):
    """(nfields, field_stride) of a contiguous tensor holding one grid array or a stack of them (time first)."""
    total = int(np.prod(N))
    shape = tuple(int(v) for v in t.shape)
    if shape == tuple(N) or shape == tuple(N) + (1,):
        return 1, total
    if len(shape) == len(N) + 1 and shape[1:] == tuple(N) and shape[0] >= 1:
        return shape[0], total
    error('data parameter does not agree in array size with grid')


def _descriptor(ffi, g, dtype_name):
    N = [int(v) for v in np.asarray(g.N).ravel()]
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
    bc, tz = grid_bc(g)
    return ffi.grid_descriptor(g.dim, N, [float(v[0]) for v in vs], [float(v[-1]) for v in vs], dx, bc, tz, dtype_name), tuple(N)


def descriptor(g, dtype_name):
    """(hjq_grid of grid g for data of `dtype_name` ('float64' / 'float32', see dtype_name(t)), g's shape as a tuple)."""
    if g.dim > _qffi.MAX_DIM:
        error('grids of more than %d dimensions have no device implementation' % _qffi.MAX_DIM)
    return _descriptor(_qffi, g, dtype_name)


def descriptor_hi(g, dtype_name):
    """descriptor's sibling for the queries of libhj_hiquery.so: (hjh_grid of a 5-D or 6-D grid g, g's shape as a tuple)."""
    if not _hffi.MIN_DIM <= g.dim <= _hffi.MAX_DIM:
        error('grid.dim must be %d..%d for the 5-D / 6-D queries (got %d): grids of more than %d dimensions have no device implementation'
              % (_hffi.MIN_DIM, _hffi.MAX_DIM, g.dim, _hffi.MAX_DIM))
    return _descriptor(_hffi, g, dtype_name)


def is_hi(g):
    """Whether grid g's queries run in libhj_hiquery.so (more than _qffi.MAX_DIM axes) and not in libhj_query.so / libhj_rollout.so."""
    return g.dim > _qffi.MAX_DIM
