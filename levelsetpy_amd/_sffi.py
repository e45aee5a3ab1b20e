"""ctypes binding of libhj_surface.so (include/hj_surface.h): level sets as indexed meshes.

Stateless entry points, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by
_ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi
from ._qffi import Grid, grid_descriptor  # noqa: F401  (hjq_grid)

_vp, _i, _i64, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t
_pg = C.POINTER(Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjs_workspace_size": (_i, [_pg, _i64, C.POINTER(_sz)]),
    "hjs_count": (_i, [_pg, _vp, _i64, _i64, _d, _vp, _sz, _vp, _vp]),
    "hjs_emit": (_i, [_pg, _vp, _i64, _i64, _d, _vp, _sz, C.POINTER(_i64), _vp, _vp, _vp]),
    "hjs_last_error": (C.c_char_p, []),
    "hjs_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, _last_kernel = _ffi.bind("HJ_SURFACE_LIB", "libhj_surface.so", "hjs", "hj_surface error", SIGNATURES)


def last_kernels():
    """The kernels the calling thread's last successful call launched, in order."""
    s = _last_kernel()
    return s.split(";") if s else []
