"""ctypes binding of libhj_rollout.so (include/hj_rollout.h): many optimal trajectories in one launch.

One stateless entry point, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a
missing library is an error.
"""
import ctypes as C

from . import _ffi, _qffi

MODE_MIN, MODE_MAX = 0, 1                          # HJR_MODE_*
REACHED, EXHAUSTED, LEFT_GRID = 0, 1, 2            # HJR_* status of a trajectory
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes hjr_rollout instantiates
PLANT_DIMS = _ffi.HAM_DIMS


class Plant(C.Structure):
    """hjr_plant."""
    _fields_ = [("id", C.c_int32), ("u_mode", C.c_int32), ("d_mode", C.c_int32), ("reserved", C.c_int32),
                ("params", C.c_double * 4)]


_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjr_rollout": (_i, [C.POINTER(_qffi.Grid), _i, _vp, _i64, _i64, _vp, _i64, _i, _d, C.POINTER(Plant), _vp, _vp, _vp, _vp, _vp]),
    "hjr_last_error": (C.c_char_p, []),
    "hjr_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_ROLLOUT_LIB", "libhj_rollout.so", "hjr", "hj_rollout error", SIGNATURES)


def plant_descriptor(ham_id, u_mode, d_mode, params):
    p = Plant()
    p.id, p.u_mode, p.d_mode, p.reserved = int(ham_id), int(u_mode), int(d_mode), 0
    for k in range(4):
        p.params[k] = float(params[k]) if k < len(params) else 0.0
    return p
