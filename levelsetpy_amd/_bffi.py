"""ctypes binding of libhj_batch.so (include/hj_batch.h): many problems on one grid, one launch per RK stage.

Stateless entry points, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a
missing library is an error.
"""
import ctypes as C

import numpy as np

from . import _ffi, _qffi

PAR_SLOTS = 8                                      # HJB_PAR_SLOTS
ARR_NONE, ARR_MIN, ARR_MAX, ARR_MAX_NEG = 0, 1, 2, 3   # HJB_ARR_*
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes batch_substep_kernel is instantiated for
HAM_DIMS = _ffi.HAM_DIMS
HAM_NAMES = {_ffi.HAM_DUBINS_REL: "HamDubinsRel", _ffi.HAM_DOUBLE_INTEGRATOR: "HamDoubleIntegrator",
             _ffi.HAM_DOUBLE_PENDULUM: "HamDoublePendulum"}


class Tables(C.Structure):
    """hjb_tables."""
    _fields_ = [("coord", C.c_void_p * _qffi.MAX_DIM), ("aux", C.c_void_p * 4)]


class Problem(C.Structure):
    """hjb_problem."""
    _fields_ = [("y_in", C.c_void_p), ("buf_a", C.c_void_p), ("buf_b", C.c_void_p), ("work", C.c_void_p),
                ("post_a", C.c_void_p), ("post_b", C.c_void_p), ("op_a", C.c_int32), ("op_b", C.c_int32)]


# hjb_entry as a NumPy record: a table of entries is built on the host and copied to the device as bytes
ENTRY = np.dtype([("src", "<u8"), ("y0", "<u8"), ("dst", "<u8"), ("post_a", "<u8"), ("post_b", "<u8"), ("dt", "<f8"),
                  ("active", "<i4"), ("post_prev", "<i4"), ("op_a", "<i4"), ("op_b", "<i4")])
assert ENTRY.itemsize == 64

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pg, _pt = C.POINTER(_qffi.Grid), C.POINTER(Tables)
_pd, _pi64, _pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjb_step_bounds": (_i, [_pg, _pt, _i, _vp, _i64, _vp, _pd, _pd, _vp]),
    "hjb_substep": (_i, [_pg, _pt, _i, _i, _i, _i, _vp, _vp, _i64, _vp]),
    "hjb_plan": (_i, [_i, _pd, _i64, _d, _d, _d, _d, _d, _pd, _pi64]),
    "hjb_integrate": (_i, [_pg, _pt, _i, _i, _i, _i, _i, _vp, _pd, C.POINTER(Problem), _i64, _d, _d, _d, _d, _d, _vp, _i64,
                           _pd, _pi64, _pi32, _vp]),
    "hjb_nan_flags": (_i, [_i, _vp, _i64, _i64, _vp, _vp]),
    "hjb_last_error": (C.c_char_p, []),
    "hjb_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_BATCH_LIB", "libhj_batch.so", "hjb", "hj_batch error", SIGNATURES)


def kernel_name(dtype_name, ham, scheme):
    """What hjb_last_kernel() reads after a substep of this instantiation."""
    return "batch_substep_kernel<%s, %s, %d>" % ("double" if dtype_name == "float64" else "float", HAM_NAMES[ham], scheme)
