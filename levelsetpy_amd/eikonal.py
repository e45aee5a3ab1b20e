"""Signed distance and first-arrival time on the device: signedDistance, addCRadius.

signedDistance turns any level-set function -- a union / intersection of shapes, a value function after a solve, a +-1
occupancy mask -- into the signed distance to its `level` set: it solves |grad u| = 1 / speed outward from the interface
with Godunov's first-order upwind scheme and returns sign(data - level) * u.  With a speed field u is the first-arrival
time from the interface; NaN nodes (and nodes of speed <= 0) are walls, which gives geodesic distances.  The interface
does not move: the nodes next to it are given their distance to the linearly interpolated crossing and stay frozen.

All of it runs in libhj_eikonal.so (include/hj_eikonal.h has the discrete problem, rule by rule): a fast iterative method
on tiles.  `eikonal_init_kernel` freezes the near nodes, `eikonal_tile_kernel` relaxes one tile per workgroup in LDS until
the tile is still and wakes the tiles behind the faces that changed, `eikonal_finish_kernel` applies sign, band and walls.
The host launches passes over the tiles until one changes nothing; tiles that were not woken leave at once.

Parity.  The reference has no such function: nothing is pinned.  HELD to the NumPy restatement tests/eikonal_ref.py:
everything here.
"""
import ctypes as C

import numpy as np

from . import _effi, _qffi
from .context import is_tensor, require_gpu, grid_bc
from .utilities import Bundle, error, warn
from ._marshal import unlazy as _unlazy, wants_tensor as _wants_tensor, stream as _stream, ptr as _ptr

__all__ = ["signedDistance", "addCRadius", "last_info", "last_path"]

SINGLE_SIGN = 'Implicit surface not visible because function has single sign on grid'

_LAST = [None]
_last_path = ""


def last_info():
    """Of the calling process's last signedDistance: dict(flags = int32 per member (bits NEG 1, POS 2, ZERO 4 of data - level
    over the nodes that are no walls), messages = the single-sign warnings, passes, active_tile_launch_fraction, K)."""
    return _LAST[0]


def last_path():
    """The kernels the calling process's last signedDistance ran (hje_last_kernel)."""
    return _last_path


def _shape_of(g):
    N = tuple(int(v) for v in np.asarray(g.N).ravel())
    if not 1 <= len(N) <= _qffi.MAX_DIM:
        error('signedDistance: grids of 1 to %d dimensions (got %d)' % (_qffi.MAX_DIM, len(N)))
    return N


def _check_arguments(g, shape, dtype_in, level, band, speed, dtype, max_passes):
    """Everything that can be refused without a device -> (N, K, level, band, speed scalar or None, speed array or None,
    element type name, max_passes)."""
    N = _shape_of(g)
    shape = tuple(int(v) for v in shape)
    if len(N) == 1 and shape == N + (1,):                # g.shape of a 1-D grid is (N, 1)
        shape = N
    if shape == N:
        K = None
    elif len(shape) == len(N) + 1 and shape[1:] == N and shape[0] >= 1:
        K = shape[0]
    else:
        error('data parameter does not agree in array size with grid')
    level = float(level)
    if level != level:
        error('level must not be NaN')
    band = float(band)
    if not band > 0.0:
        error('band must be a positive width (got %r)' % (band,))
    sp_scalar, sp_array = 1.0, None
    if speed is not None:
        if np.ndim(_unlazy(speed)) == 0:
            sp_scalar = float(speed)
            if not sp_scalar > 0.0:
                error('a scalar speed must be positive (got %r)' % (sp_scalar,))
        else:
            sp_array = _unlazy(speed)
            if tuple(int(v) for v in sp_array.shape) != N:
                error('speed must be None, a positive scalar or an array of the grid\'s shape %r (got %r)' % (N, tuple(sp_array.shape)))
    if dtype is None:
        dtype = dtype_in
    if dtype not in ('float64', 'float32'):
        error('dtype must be \'float64\' or \'float32\' (got %r)' % (dtype,))
    if max_passes is None:
        max_passes = _effi.default_max_passes(N)
    if int(max_passes) != max_passes or max_passes < 1:
        error('max_passes must be a positive whole number (got %r)' % (max_passes,))
    return N, K, level, band, sp_scalar, sp_array, dtype, int(max_passes)


def _dtype_in(data):
    if is_tensor(data):
        return 'float32' if str(data.dtype) == 'torch.float32' else 'float64'
    return 'float32' if isinstance(data, np.ndarray) and data.dtype == np.float32 else 'float64'


def signedDistance(g, data, level=0.0, band=np.inf, speed=None, dtype=None, max_passes=None, return_info=False):
    """sign(data - level) * u, u the distance to {data == level} (the first-arrival time from it under `speed`).

    g            a grid of 1 to 4 dimensions; only g.N, g.dx and g.bdry are read (a low_mem grid works).
    data         g.shape, or (K,) + g.shape for K members solved together; fp64 or fp32 (anything else is read as fp64).
                 NaN nodes are walls: they stay NaN and no front passes through them.
    band         no value above it is accepted and nodes not reached get +-band; tiles the band does not reach never run.
    speed        None, a positive scalar, or an array of g.shape shared by the members; a node of speed <= 0 or NaN is a wall.
    dtype        'float64' | 'float32' of the result (default: the data's); the arithmetic is fp64 either way.
    max_passes   passes over the tiles after which the call raises (default 8 * sum_d ceil(N_d / tile_d) + 64; walls that
                 make a maze may need more).
    return_info  also return Bundle(passes, active_tile_launch_fraction, path): passes up to and including the first that
                 changed nothing, and the share of ALL tile launches made (passes go out in groups of 8) that did work.

    NumPy in -> NumPy out; a device tensor or a HostView in -> a tensor out.  A member whose data has a single sign is
    +-inf (+-band) everywhere; last_info() then carries the reference's "single sign on grid" wording."""
    global _last_path
    raw = _unlazy(data)
    if not is_tensor(raw):
        raw = np.asarray(raw)
        if raw.dtype != np.float32:
            raw = np.asarray(raw, dtype=np.float64)
    N, K, level, band, sp_scalar, sp_array, dtype, max_passes = _check_arguments(
        g, raw.shape, _dtype_in(raw), level, band, speed, dtype, max_passes)
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    bc, tz = grid_bc(g)
    torch = require_gpu()
    # one element type per call: fp32 only when data and result both are; otherwise fp64 (widening is exact) and the
    # fp64 result is rounded once below
    solve = 'float32' if (dtype == 'float32' and _dtype_in(raw) == 'float32') else 'float64'
    tdtype = torch.float64 if solve == 'float64' else torch.float32
    if is_tensor(raw):
        t = raw if raw.is_cuda else raw.to('cuda')
    else:
        a = np.ascontiguousarray(raw)
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).to('cuda')
    t = t.to(tdtype).contiguous()                    # the kernels read and write one element type; never a view's strides
    given = tuple(t.shape)
    t = t.reshape(((K,) if K is not None else ()) + N)
    device = t.device
    sp = None
    if sp_array is not None:
        sp = sp_array if is_tensor(sp_array) else torch.from_numpy(np.ascontiguousarray(np.asarray(sp_array, dtype=np.float64)).copy())
        sp = sp.to(device=device, dtype=torch.float64).contiguous()
    nd = len(N)
    desc = _qffi.grid_descriptor(nd, N, [0.0] * nd, [0.0] * nd, dx, bc, tz, solve)
    members = 1 if K is None else K
    total = int(np.prod(N, dtype=np.int64))
    out = torch.empty(t.shape, dtype=tdtype, device=device)
    need = C.c_int64(0)
    lib = _effi.lib()
    _effi.check(lib.hje_workspace_size(desc, members, C.byref(need)))
    ws = torch.empty(max(need.value, 8) // 8 + 1, dtype=torch.int64, device=device)
    passes = C.c_int64(0)
    with torch.cuda.device(device):
        _effi.check(lib.hje_signed_distance(desc, _ptr(t), members, total, level, band, _ptr(sp), sp_scalar, _ptr(out), _ptr(ws),
                                            ws.numel() * 8, max_passes, C.byref(passes), _stream(torch, device)))
    _last_path = _effi.last_kernel()
    head = ws[:8 + (members + 1) // 2].cpu().numpy()
    counters = head[:8].view(np.uint64)
    flags = head[8:].view(np.int32)[:members].copy()
    # every pass launched counts, the ones after the first that changed nothing too: the loop launches them in groups
    launches = max(_effi.launched_passes(passes.value, max_passes), 1) * members * max(_effi.tile_count(N), 1)
    messages = []
    for k in np.nonzero((flags == _effi.NEG) | (flags == _effi.POS))[0]:
        messages.append(SINGLE_SIGN + (' (member %d)' % k if K is not None else ''))
        warn(messages[-1])
    info = dict(flags=flags, messages=messages, passes=int(passes.value), K=members,
                active_tile_launch_fraction=float(counters[0]) / launches, changed_tile_launches=int(counters[1]))
    _LAST[0] = info
    if dtype != solve:
        out = out.to(torch.float32)
    out = out.reshape(given)
    if not _wants_tensor(data):
        out = out.cpu().numpy()
    elif is_tensor(raw) and not raw.is_cuda:
        out = out.to(raw.device)
    if return_info:
        return out, Bundle(dict(passes=info['passes'], active_tile_launch_fraction=info['active_tile_launch_fraction'], path=_last_path))
    return out


def addCRadius(g, data, radius):
    """helperOC's addCRadius: the set {data <= 0} grown by `radius` (shrunk by a negative one): signedDistance(g, data) - radius.
    NumPy in -> NumPy out; a device tensor or a HostView in -> a tensor out."""
    return signedDistance(g, data) - float(radius)
