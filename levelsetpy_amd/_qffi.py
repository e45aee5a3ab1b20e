"""ctypes binding of libhj_query.so (include/hj_query.h): value-function queries at states.

Stateless entry points, a plain grid descriptor (hjq_grid, which the other stateless libraries share) and a HIP
stream per call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi

MAX_DIM = 4
OP_MIN, OP_MAX = 0, 1
POINT_SCHEMES = (_ffi.ENO2, _ffi.ENO3, _ffi.WENO5_ASSHIPPED)      # the schemes hjq_costate_points instantiates


class Grid(C.Structure):
    """hjq_grid."""
    _fields_ = [("ndim", C.c_int32), ("dtype", C.c_int32),
                ("N", C.c_int64 * MAX_DIM), ("xmin", C.c_double * MAX_DIM), ("xlast", C.c_double * MAX_DIM),
                ("dx", C.c_double * MAX_DIM), ("bc", C.c_int32 * MAX_DIM), ("toward_zero", C.c_int32 * MAX_DIM)]


_vp, _i, _i64, _u = C.c_void_p, C.c_int, C.c_int64, C.c_uint
_pg = C.POINTER(Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjq_interp_points": (_i, [_pg, _vp, _i64, _i64, _vp, _i64, _vp, _i, _vp]),
    "hjq_costate_points": (_i, [_pg, _i, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp]),
    "hjq_project_minmax": (_i, [_pg, _vp, _i64, _i64, _u, _i, _vp, _vp]),
    "hjq_last_error": (C.c_char_p, []),
    "hjq_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_QUERY_LIB", "libhj_query.so", "hjq", "hj_query error", SIGNATURES)


def grid_descriptor(ndim, N, xmin, xlast, dx, bc, tz, dtype_name):
    return _ffi.grid_descriptor(Grid, MAX_DIM, ndim, N, xmin, xlast, dx, bc, tz, dtype_name)
