"""Sets measured on the device: setVolume, setCompare, setBounds, and truncateGrid to crop a grid to what setBounds found.

The set { data <= level } is that of the piecewise-linear interpolant on the Kuhn subdivision -- the one extract_level_set meshes --
and its volume is second order in the grid step where counting nodes is first order.  One launch of `measure_kernel` in
libhj_measure.so (include/hj_measure.h states the rule operation by operation) classifies every cell, works the cut cells simplex by
simplex and leaves per field a record of INTEGERS: counts of cells, the 128-bit sum of per-simplex fractions, counts of nodes and
the per-axis index range of the inside nodes.  Integer sums do not depend on their order: a result is reproducible bit for bit and
tests/measure_ref.py restates it with ==.  Grids of 1 to 6 dimensions; only g.vs, g.N, g.dx and g.bdry are read, so `low_mem` grids
work.  Periodic axes measure a full period.

Results are a handful of numbers and come back as host NumPy values: one small copy and one synchronisation per call.  Stored value
functions with a time axis are time FIRST, as everywhere in this package.

truncateGrid carries the reference's name, argument order and grid construction (Grids/truncate.py), on 1 to 6 axes where the
reference stops at 4; with dataOld given it always returns (gNew, dataNew), where the reference returns the grid alone for data that
is all zeros.
"""
import ctypes as C
import math

import numpy as np

from . import _ffi, _vffi
from .boundary import addGhostExtrapolate, addGhostPeriodic
from .context import is_tensor, require_gpu
from .grids import processGrid
from .utilities import Bundle, error
from ._marshal import unlazy as _unlazy, stream as _stream, ptr as _ptr, fields as _fields

__all__ = ["setVolume", "setCompare", "setBounds", "truncateGrid", "last_path", "last_info"]

_last_path = ""
_LAST = [None]


def last_path():
    """The kernels the calling process's last measurement launched: "measure_kernel<double, double, 3, 0>;measure_fold_kernel"."""
    return _last_path


def last_info():
    """Of the calling process's last measurement: the list (one per field; of setCompare: a dict of four such lists) of dicts
    cells, full, cut, invalid, Q_cut, Q, inside, nan, lo, hi -- Python integers, as include/hj_measure.h's record."""
    return _LAST[0]


# ------------------------------------------------------------------------------------------ checks without a device
def _grid_shape(g):
    return tuple(int(v) for v in np.asarray(g.N).ravel())


def _periodic(g):
    return tuple(d for d in range(int(g.dim)) if g.bdry[d] is addGhostPeriodic)


def _shape_of(a):
    a = _unlazy(a)
    return tuple(int(v) for v in (a.shape if hasattr(a, "shape") else np.shape(a)))


def _cell_volume(g):
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    v = dx[0]
    for s in dx[1:]:
        v = v * s
    return v


def _check(g, arrays, level):
    """-> (D, N, [stacked?] per array).  Everything that can be refused is refused here, before a device is asked for."""
    D = int(g.dim)
    if not 1 <= D <= _vffi.MAX_DIM:
        error('grid.dim must be 1..%d (got %d): grids of more than %d dimensions have no device implementation'
              % (_vffi.MAX_DIM, D, _vffi.MAX_DIM))
    N = _grid_shape(g)
    if min(N) < 2:
        error('every grid axis needs at least two nodes to have a cell (N = %s)' % (N,))
    for d in range(D):
        if g.bdry[d] is not addGhostPeriodic and g.bdry[d] is not addGhostExtrapolate:
            error('grid.bdry[%d] must be addGhostPeriodic or addGhostExtrapolate' % d)
    try:
        level = float(level)
    except (TypeError, ValueError):
        error('level must be a finite number (got %r)' % (level,))
    if not math.isfinite(level):
        error('level must be a finite number (got %r)' % (level,))
    stacked = []
    for a in arrays:
        shape = _shape_of(a)
        single = shape == N or shape == N + (1,)                 # (a 1-D grid's shape is (N, 1))
        if not (single or (len(shape) == D + 1 and shape[1:] == N and shape[0] >= 1)):
            error('data parameter does not agree in array size with grid')
        stacked.append(None if single else shape[0])
    return D, N, level, stacked


def _tensor(data):
    """The data on the device as it is: fp32 stays fp32 (NumPy's too), anything but fp32 / fp64 becomes fp64."""
    torch = require_gpu()
    data = _unlazy(data)
    if is_tensor(data):
        t = data if data.is_cuda else data.to("cuda")
        if t.dtype not in (torch.float64, torch.float32):
            t = t.to(torch.float64)
        return t.contiguous()
    a = np.asarray(data)
    a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to("cuda")


def _record(words, D):
    w = [int(v) for v in words]
    u = [v & 0xffffffffffffffff for v in w]
    q_cut = u[_vffi.QLO] | (u[_vffi.QHI] << 64)
    return dict(cells=w[_vffi.CELLS], full=w[_vffi.FULL], cut=w[_vffi.CUT], invalid=w[_vffi.INVALID], Q_cut=q_cut,
                Q=w[_vffi.FULL] * math.factorial(D) * _vffi.Q_ONE + q_cut, inside=w[_vffi.INSIDE], nan=w[_vffi.NAN],
                lo=w[_vffi.LO:_vffi.LO + D], hi=w[_vffi.HI:_vffi.HI + D])


# ------------------------------------------------------------------------------------------ the launch
def _run(g, a, b, level):
    """-> (records: list over fields of [record] or of [record of A, B, union, intersection], D, whether a was stacked)."""
    D, N, level, stacked = _check(g, [a] if b is None else [a, b], level)
    if b is not None and stacked[1] is not None and stacked[1] != (stacked[0] or 1) and stacked[1] != 1:
        error('a and b hold %s and %d fields: equal counts, or one field of b for all of a' % (stacked[0] or 1, stacked[1]))
    torch = require_gpu()
    ta = _tensor(a)
    name_a = "float32" if ta.dtype == torch.float32 else "float64"
    desc = _vffi.extents_descriptor(N, _periodic(g), name_a)
    S, stride_a = _fields(ta, N)
    tb, Sb, stride_b, name_b = None, 0, 0, None
    if b is not None:
        tb = _tensor(b)
        if tb.device != ta.device:
            tb = tb.to(ta.device)
        name_b = "float32" if tb.dtype == torch.float32 else "float64"
        Sb, stride_b = _fields(tb, N)
    sets = 1 if b is None else 4
    records = torch.empty((S, sets, _vffi.RECORD_WORDS), dtype=torch.int64, device=ta.device)
    work = torch.empty(int(_vffi.lib().hjv_workspace_size(C.byref(desc), S, int(b is not None))) // 8, dtype=torch.int64, device=ta.device)
    with torch.cuda.device(ta.device):
        _vffi.check(_vffi.lib().hjv_measure(C.byref(desc), _ptr(ta), S, stride_a, _ptr(tb), _ffi.F32 if name_b == "float32" else _ffi.F64,
                                            Sb, stride_b, level, _ptr(records), _ptr(work), _stream(torch, ta.device)))
    global _last_path
    _last_path = _vffi.last_kernel()
    host = records.cpu().numpy()                                 # the one copy; it waits for the stream
    return [[_record(host[f, s], D) for s in range(sets)] for f in range(S)], D, stacked[0] is not None


def _volume(Q, D, cellvol):
    return (Q / (math.factorial(D) * _vffi.Q_ONE)) * cellvol


def setVolume(g, data, level=0.0, return_info=False):
    """The volume of { data <= level } on grid g: a float, or an array (T,) for a time-first stack (or a leading batch axis).

      data          g.shape or (T,) + g.shape; NumPy, HostView or tensor; fp32 is widened, not copied
      return_info   also return dict(cells, full, cut, invalid, inside, nan, Q, volume_cell, kernel): the counts of cells by class
                    (invalid: a NaN or infinite corner, contributing nothing), of nodes inside and of NaN nodes -- integers, or
                    int64 arrays (T,) -- and Q, the exact integer(s) the volume is (Q / (D! 2^52)) volume_cell of

    Everything is checked before a device is asked for."""
    recs, D, stacked = _run(g, data, None, level)
    cellvol = _cell_volume(g)
    recs = [r[0] for r in recs]
    _LAST[0] = recs
    vols = np.array([_volume(r["Q"], D, cellvol) for r in recs], dtype=np.float64)
    out = vols if stacked else float(vols[0])
    if not return_info:
        return out
    info = dict(volume_cell=cellvol, kernel=_last_path, Q=[r["Q"] for r in recs] if stacked else recs[0]["Q"])
    for k in ("cells", "full", "cut", "invalid", "inside", "nan"):
        info[k] = np.array([r[k] for r in recs], dtype=np.int64) if stacked else recs[0][k]
    return out, info


def setCompare(g, a, b, level=0.0):
    """{ a <= level } against { b <= level } in one pass over both: Bundle(volA, volB, union, intersection, symdiff, iou), floats or
    arrays (T,) when a is a stack (b: as many fields, or one for all).  union and intersection are the sets of np.minimum(a, b) and
    np.maximum(a, b); no such array is made.  symdiff comes from the integer max(0, Q_union - Q_intersection); iou is the integer
    ratio Q_intersection / Q_union, NaN when the union is empty.  Either input may be fp32 or fp64."""
    recs, D, stacked = _run(g, a, b, level)
    cellvol = _cell_volume(g)
    _LAST[0] = dict((name, [r[s] for r in recs]) for s, name in enumerate(("A", "B", "union", "intersection")))
    cols = {k: [] for k in ("volA", "volB", "union", "intersection", "symdiff", "iou")}
    for r in recs:
        QU, QI = r[_vffi.SET_UNION]["Q"], r[_vffi.SET_INTERSECTION]["Q"]
        for k, s in (("volA", _vffi.SET_A), ("volB", _vffi.SET_B), ("union", _vffi.SET_UNION), ("intersection", _vffi.SET_INTERSECTION)):
            cols[k].append(_volume(r[s]["Q"], D, cellvol))
        cols["symdiff"].append(_volume(max(0, QU - QI), D, cellvol))
        cols["iou"].append(QI / QU if QU else float("nan"))
    return Bundle(dict((k, np.array(v, dtype=np.float64) if stacked else float(v[0])) for k, v in cols.items()))


def setBounds(g, data, level=0.0, pad=1):
    """The box that holds { data <= level }: Bundle(lo, hi, xmin, xmax), or None for an empty set.

      lo, hi       per axis the inclusive node range of the inside nodes (of all fields of a stack together), widened by `pad`
                   nodes and clipped to the grid; a periodic axis is never cropped (the set may straddle the seam): 0 and N - 1
      xmin, xmax   (D, 1) columns vs[lo] - dx / 2 and vs[hi] + dx / 2: truncateGrid(g, data, xmin, xmax) keeps exactly lo .. hi"""
    pad = int(pad)
    if pad < 0:
        error('pad must be >= 0 (got %d)' % pad)
    recs, D, _ = _run(g, data, None, level)
    recs = [r[0] for r in recs]
    _LAST[0] = recs
    N, per = _grid_shape(g), _periodic(g)
    if all(r["inside"] == 0 for r in recs):
        return None
    lo = [min(r["lo"][d] for r in recs) for d in range(D)]
    hi = [max(r["hi"][d] for r in recs) for d in range(D)]
    lo = [0 if d in per else max(0, lo[d] - pad) for d in range(D)]
    hi = [N[d] - 1 if d in per else min(N[d] - 1, hi[d] + pad) for d in range(D)]
    dx = [float(v) for v in np.asarray(g.dx).ravel()]
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
    xmin = np.array([[vs[d][lo[d]] - dx[d] / 2] for d in range(D)])
    xmax = np.array([[vs[d][hi[d]] + dx[d] / 2] for d in range(D)])
    return Bundle(dict(lo=np.array(lo, dtype=np.int64), hi=np.array(hi, dtype=np.int64), xmin=xmin, xmax=xmax))


# ------------------------------------------------------------------------------------------ the crop, on the host
def truncateGrid(gOld, dataOld=None, xmin=None, xmax=None, process=True):
    """Grids/truncate.py: the grid of gOld's nodes strictly inside (xmin, xmax), and dataOld cut to them.

    As the reference: strict inequalities; max += 1e-3 on an axis left with one node; a cropped axis becomes extrapolated.  Unlike
    it: 1 to 6 axes (the reference stops at 4), data is sliced where it lives (NumPy, tensor or HostView; time-first stacks
    allowed), gOld.bdry is not modified, and with dataOld given the return is always (gNew, dataNew) -- the reference returns gNew
    alone when dataOld is all zeros.  Without dataOld: gNew."""
    D = int(gOld.dim)
    if not 1 <= D <= _vffi.MAX_DIM:
        error('truncateGrid is implemented for grids of 1..%d dimensions (got %d)' % (_vffi.MAX_DIM, D))
    if xmin is None or xmax is None:
        error('truncateGrid needs xmin and xmax')
    xmin, xmax = np.asarray(xmin, dtype=np.float64).ravel(), np.asarray(xmax, dtype=np.float64).ravel()
    if xmin.size != D or xmax.size != D:
        error('xmin and xmax must have one entry per grid dimension (%d)' % D)
    small = 1e-3
    gNew = Bundle(dict(dim=D, vs=[None] * D, N=np.zeros((D, 1), dtype=np.int64), min=np.zeros((D, 1), dtype=np.float64),
                       max=np.zeros((D, 1), dtype=np.float64), bdry=list(gOld.bdry)))
    keep = []
    for i in range(D):
        v = np.asarray(gOld.vs[i], dtype=np.float64).ravel()
        idx = np.logical_and(v > xmin[i], v < xmax[i])
        if not idx.any():
            error('no node of axis %d lies strictly inside (%g, %g)' % (i, xmin[i], xmax[i]))
        keep.append(np.flatnonzero(idx))
        gNew.vs[i] = v[idx].reshape(-1, 1)
        gNew.N[i] = len(gNew.vs[i])
        gNew.min[i] = np.min(gNew.vs[i])
        gNew.max[i] = np.max(gNew.vs[i]) + (small if gNew.N[i] == 1 else 0.0)
        if gNew.N[i] < int(np.asarray(gOld.N).ravel()[i]):
            gNew.bdry[i] = addGhostExtrapolate
    if process:
        sparse = hasattr(gOld, "xs") and D > 1 and int(np.size(gOld.xs[0])) != int(np.prod(_grid_shape(gOld)))
        with np.errstate(divide="ignore"):                         # an axis of one node: dx = (max - min) / 0, as the reference
            gNew = processGrid(gNew, sparse_flag=sparse)
    if dataOld is None:
        return gNew
    N = _grid_shape(gOld)
    shape = _shape_of(dataOld)
    lead = 0 if shape == N or shape == N + (1,) else 1
    if not (lead == 0 or (len(shape) == D + 1 and shape[1:] == N)):
        error('data parameter does not agree in array size with grid')
    data = _unlazy(dataOld)
    if is_tensor(data):
        import torch
        out = data
        for d, k in enumerate(keep):
            out = out.index_select(lead + d, torch.as_tensor(k, device=data.device))
    else:
        out = np.asarray(data)
        for d, k in enumerate(keep):
            out = np.take(out, k, axis=lead + d)
    return gNew, out
