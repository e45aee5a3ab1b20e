"""ctypes binding of libhj_plant.so (include/hj_plant.h): rollouts of a plant registered at run time.

The grid descriptors of include/hj_query.h (2-D .. 4-D) and include/hj_hidim.h (5-D, 6-D), a plant descriptor of its own (hjp_plant)
and a HIP stream per call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi, _hffi, _qffi

PAR_SLOTS = 16                                     # HJP_PAR_SLOTS
MAX_CONTROLS = 8                                   # HJP_MAX_CONTROLS
MIN_DIM, MAX_DIM = 2, 6                            # HJP_MIN_DIM, HJP_MAX_DIM
PLANT_BASE = 1000000                               # HJP_PLANT_BASE
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes user_rollout_kernel is instantiated for
KERNEL_ROLLOUT, KERNEL_NOISY, KERNEL_FILTERED, KERNEL_DECIDE = 0, 1, 2, 3      # HJP_KERNEL_*
KINDS = {"rollout": KERNEL_ROLLOUT, "noisy": KERNEL_NOISY, "filtered": KERNEL_FILTERED, "decide": KERNEL_DECIDE}
KERNELS = ("user_rollout_kernel", "user_noisy_rollout_kernel", "user_filtered_rollout_kernel", "user_decide_points_kernel")


class Plant(C.Structure):
    """hjp_plant."""
    _fields_ = [("id", C.c_int32), ("u_mode", C.c_int32), ("d_mode", C.c_int32), ("nparams", C.c_int32),
                ("params", C.c_double * PAR_SLOTS)]


_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pi = C.POINTER(C.c_int)
_u64 = C.c_uint64
_roll = [_i, _vp, _i64, _i64, _vp, _i64, _i, _d, C.POINTER(Plant), _vp, _vp, _vp, _vp, _vp]
# hjn_rollout's, hjf_rollout's and hjf_decide's lists after the grid, with the plant descriptor this library's
_noisy = [_i, _vp, _i64, _i64, _vp, _i64, _i64, _u64, _u64, _vp, _vp, _d, _i, _i, _d, C.POINTER(Plant)] + [_vp] * 8
_filtered = [_i, _vp, _i64, _i64, _vp, _i64, _i, _d, C.POINTER(Plant), _i, _i64, _i, _vp, _vp, _i64, _i64, _i, _d, _d, _i] + [_vp] * 11
_decide = [_i, _vp, _i64, _i64, _i64, _vp, _i64, C.POINTER(Plant), _vp, _d, _d, _i] + [_vp] * 6

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjp_plant_register": (_i, [C.c_char_p, _i, _i, _i, _i, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, _pi]),
    "hjp_plant_info": (_i, [_i, _pi, _pi, _pi, _pi, _pi]),
    "hjp_plant_source": (_i, [_i, C.c_char_p, _i64]),
    "hjp_plant_cache_stats": (_i, [_pi, _pi]),
    "hjp_plant_compile_check": (_i, [_i, _i, _i]),
    "hjp_rollout": (_i, [C.POINTER(_qffi.Grid)] + _roll),
    "hjp_rollout_hi": (_i, [C.POINTER(_hffi.Grid)] + _roll),
    "hjp_plant_compile_kind": (_i, [_i, _i, _i, _i]),
    "hjp_noisy_rollout": (_i, [C.POINTER(_qffi.Grid)] + _noisy),
    "hjp_noisy_rollout_hi": (_i, [C.POINTER(_hffi.Grid)] + _noisy),
    "hjp_filtered_rollout": (_i, [C.POINTER(_qffi.Grid)] + _filtered),
    "hjp_filtered_rollout_hi": (_i, [C.POINTER(_hffi.Grid)] + _filtered),
    "hjp_decide": (_i, [C.POINTER(_qffi.Grid)] + _decide),
    "hjp_decide_hi": (_i, [C.POINTER(_hffi.Grid)] + _decide),
    "hjp_last_error": (C.c_char_p, []),
    "hjp_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_PLANT_LIB", "libhj_plant.so", "hjp", "hj_plant error", SIGNATURES)


def plant_descriptor(plant_id, u_mode, d_mode, params):
    p = Plant()
    p.id, p.u_mode, p.d_mode, p.nparams = int(plant_id), int(u_mode), int(d_mode), len(params)
    for k in range(PAR_SLOTS):
        p.params[k] = float(params[k]) if k < len(params) else 0.0
    return p


def kernel_name(dtype_name, scheme, plant_name, kind="rollout"):
    """What hjp_last_kernel() reads after a launch of this instantiation."""
    return "%s<%s, %d, PlantUser:%s>" % (KERNELS[KINDS[kind]], "double" if dtype_name == "float64" else "float", scheme, plant_name)
