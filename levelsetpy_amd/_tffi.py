"""ctypes binding of libhj_ttr.so (include/hj_ttr.h): time-to-reach functions.

Stateless entry points, plain pointers and a HIP stream per call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi

FIRST, NO_INTERP = 1, 2              # mode bits (HJT_FIRST, HJT_NO_INTERP)

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjt_ttr_init": (_i, [_i, _vp, _i64, _d, _d, _vp, _vp, _vp]),
    "hjt_ttr_update": (_i, [_i, _vp, _i64, _d, _d, _d, _i, _vp, _vp, _vp]),
    "hjt_ttr_from_stack": (_i, [_i, _vp, _i64, _i64, _i64, _vp, _d, _i, _vp, _vp]),
    "hjt_last_error": (C.c_char_p, []),
    "hjt_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_TTR_LIB", "libhj_ttr.so", "hjt", "hj_ttr error", SIGNATURES)
