"""ctypes binding of libhj_decomp.so (include/hj_decomp.h): decomposed value functions put back together.

Three stateless entry points, a decomposition descriptor built on the grid descriptor of include/hj_query.h and a HIP
stream per call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi, _qffi

MAX_DIM, MAX_SUBS = 8, 8                           # HJD_MAX_DIM, HJD_MAX_SUBS
OP_MIN, OP_MAX = _qffi.OP_MIN, _qffi.OP_MAX        # HJQ_MIN (union), HJQ_MAX (intersection)


class Sub(C.Structure):
    """hjd_sub."""
    _fields_ = [("grid", _qffi.Grid), ("data", C.c_void_p), ("nfields", C.c_int64), ("field_stride", C.c_int64),
                ("axis", C.c_int32 * _qffi.MAX_DIM)]


class Decomp(C.Structure):
    """hjd_decomp."""
    _fields_ = [("ndim", C.c_int32), ("nsubs", C.c_int32), ("op", C.c_int32), ("reserved", C.c_int32), ("sub", Sub * MAX_SUBS)]


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
_pd, _pi64 = C.POINTER(Decomp), C.POINTER(C.c_int64)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjd_backproject_nodes": (_i, [_pd, _pi64, _i64, _vp, _i, _vp, _vp]),
    "hjd_backproject_coords": (_i, [_pd, _pi64, C.POINTER(_vp), _i64, _vp, _i, _vp, _vp]),
    "hjd_points": (_i, [_pd, _vp, _i64, _i64, _vp, _i, _vp, _vp]),
    "hjd_last_error": (C.c_char_p, []),
    "hjd_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_DECOMP_LIB", "libhj_decomp.so", "hjd", "hj_decomp error", SIGNATURES)


def decomp(ndim, op, subs):
    """hjd_decomp from (hjq_grid, data address, nfields, field_stride, axes) tuples.  Nothing is checked here: the library
    validates the descriptor before it launches anything."""
    d = Decomp()
    d.ndim, d.nsubs, d.op = int(ndim), len(subs), int(op)
    for s, (grid, addr, nfields, field_stride, axes) in enumerate(subs[:MAX_SUBS]):
        u = d.sub[s]
        u.grid, u.data, u.nfields, u.field_stride = grid, addr, int(nfields), int(field_stride)
        for k, a in enumerate(list(axes)[:_qffi.MAX_DIM]):
            u.axis[k] = int(a)
    return d


def extents(N):
    """The `N` argument: int64 values on the host."""
    return (C.c_int64 * max(1, len(N)))(*[int(n) for n in N])


def tables(addresses):
    """The `coord` argument: host array of device addresses."""
    return (C.c_void_p * max(1, len(addresses)))(*addresses)


def kernel_name(kind, dtype_name):
    """What hjd_last_kernel() reads after a call: kind 'nodes' | 'coords' | 'points', into this output type."""
    stem = {"nodes": "backproject_nodes_kernel", "coords": "backproject_coords_kernel", "points": "decomp_points_kernel"}[kind]
    return "%s<%s>" % (stem, "double" if dtype_name == "float64" else "float")
