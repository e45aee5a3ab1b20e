"""ctypes binding of libhj_filter.so (include/hj_filter.h): the least-restrictive safety filter -- filtered rollouts in one
launch, and the filter's decision at states.

Stateless entry points, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a missing
library is an error.
"""
import ctypes as C

from . import _ffi, _qffi, _rffi

SAFE, VIOLATED, LEFT_GRID = 0, 1, 2                # HJF_* status of a filtered trajectory
NOMINAL_TABLE, NOMINAL_VALUE = 0, 1                # HJF_NOMINAL_*
SLICE_CLOCK, SLICE_STATIC = 0, 1                   # HJF_SLICE_*
DSTB_WORST, DSTB_ZERO = 0, 1                       # HJF_DSTB_*
POLICIES = {'clock': SLICE_CLOCK, 'static': SLICE_STATIC}
DISTURBANCES = {'worst': DSTB_WORST, 'zero': DSTB_ZERO}
SCHEMES = _rffi.SCHEMES
PLANT_DIMS = _rffi.PLANT_DIMS
# the number of controls among a plant's held values (include/hj_filter.h's table)
PLANT_NU = {_ffi.HAM_DUBINS_REL: 1, _ffi.HAM_DOUBLE_INTEGRATOR: 1, _ffi.HAM_DOUBLE_PENDULUM: 2}
Plant = _rffi.Plant

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjf_rollout": (_i, [C.POINTER(_qffi.Grid), _i, _vp, _i64, _i64, _vp, _i64, _i, _d, C.POINTER(Plant), _i, _i64, _i, _vp, _vp,
                         _i64, _i64, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hjf_decide": (_i, [C.POINTER(_qffi.Grid), _i, _vp, _i64, _i64, _i64, _vp, _i64, C.POINTER(Plant), _vp, _d, _d, _i, _vp, _vp,
                        _vp, _vp, _vp, _vp]),
    "hjf_last_error": (C.c_char_p, []),
    "hjf_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_FILTER_LIB", "libhj_filter.so", "hjf", "hj_filter error", SIGNATURES)
