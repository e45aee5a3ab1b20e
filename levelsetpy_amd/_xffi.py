"""ctypes binding of libhj_hiquery.so (include/hj_hiquery.h): value-function queries and rollouts on 5-D and 6-D grids.

Stateless entry points, the grid descriptor of include/hj_hidim.h (_hffi.Grid, built by _hffi.grid_descriptor), the plant
descriptor of include/hj_rollout.h (_rffi.Plant) and a HIP stream per call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi, _hffi, _qffi, _rffi

MIN_DIM, MAX_DIM = _hffi.MIN_DIM, _hffi.MAX_DIM    # HJH_MIN_DIM, HJH_MAX_DIM
OP_MIN, OP_MAX = _qffi.OP_MIN, _qffi.OP_MAX        # HJQ_MIN, HJQ_MAX
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes hjx_costate_points and hjx_rollout instantiate
PLANT_DIMS = _hffi.HAM_DIMS                        # the plants of hjx_rollout and their dimensions
Grid = _hffi.Grid
Plant = _rffi.Plant

_vp, _i, _i64, _u, _d = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_double
_pg = C.POINTER(Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjx_interp_points": (_i, [_pg, _vp, _i64, _i64, _vp, _i64, _vp, _i, _vp]),
    "hjx_costate_points": (_i, [_pg, _i, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _vp]),
    "hjx_project_minmax": (_i, [_pg, _vp, _i64, _i64, _u, _i, _vp, _vp]),
    "hjx_rollout": (_i, [_pg, _i, _vp, _i64, _i64, _vp, _i64, _i, _d, C.POINTER(Plant), _vp, _vp, _vp, _vp, _vp]),
    "hjx_last_error": (C.c_char_p, []),
    "hjx_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_HIQUERY_LIB", "libhj_hiquery.so", "hjx", "hj_hiquery error", SIGNATURES)


def _t(dtype_name):
    return "double" if dtype_name == "float64" else "float"


def interp_kernel_name(dtype_name):
    return "hi_interp_points_kernel<%s>" % _t(dtype_name)


def costate_kernel_name(dtype_name, ndim, scheme):
    return "hi_costate_points_kernel<%s, %d, %d>" % (_t(dtype_name), ndim, scheme)


def project_kernel_name(dtype_name, last_axis_removed):
    return "hi_project_minmax_kernel<%s, %s>" % (_t(dtype_name), "true" if last_axis_removed else "false")


def rollout_kernel_name(dtype_name, scheme, plant_id):
    return "hi_rollout_kernel<%s, %d, %d>" % (_t(dtype_name), scheme, plant_id)
