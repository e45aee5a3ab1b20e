"""ctypes binding of libhj_stoch.so (include/hj_stoch.h): the Lax-Friedrichs term and trace(sigma^T D^2phi sigma) of a
constant sigma, one launch per RK stage.

Stateless entry points, the grid descriptor of include/hj_query.h, the tables of include/hj_batch.h and a HIP stream per
call.  Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _bffi, _ffi, _qffi

FORM_AUTO, FORM_GENERAL, FORM_DIAGONAL = 0, 1, 2   # HJW_FORM_*
SCHEMES = _bffi.SCHEMES                            # the schemes stoch_substep_kernel is instantiated for
HAM_DIMS = _bffi.HAM_DIMS
HAM_NAMES = _bffi.HAM_NAMES


class Entry(C.Structure):
    """hjb_entry, read on the host by hjw_substep."""
    _fields_ = [("src", C.c_void_p), ("y0", C.c_void_p), ("dst", C.c_void_p), ("post_a", C.c_void_p), ("post_b", C.c_void_p),
                ("dt", C.c_double), ("active", C.c_int32), ("post_prev", C.c_int32), ("op_a", C.c_int32), ("op_b", C.c_int32)]


assert C.sizeof(Entry) == 64

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pg, _pt = C.POINTER(_qffi.Grid), C.POINTER(_bffi.Tables)
_pd, _pi64, _pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjw_step_bound": (_i, [_pg, _pt, _i, _pd, _pd, _vp, _pd, _vp]),
    "hjw_substep": (_i, [_pg, _pt, _i, _i, _i, _i, _pd, _pd, _i, C.POINTER(Entry), _vp]),
    "hjw_plan": (_i, [_i, _d, _d, _d, _d, _d, _d, _pd, _pi64]),
    "hjw_integrate": (_i, [_pg, _pt, _i, _i, _i, _i, _i, _pd, _pd, _i, _d, C.POINTER(_bffi.Problem), _d, _d, _d, _d, _d,
                           _pd, _pi64, _pi32, _vp]),
    "hjw_last_error": (C.c_char_p, []),
    "hjw_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_STOCH_LIB", "libhj_stoch.so", "hjw", "hj_stoch error", SIGNATURES)


def kernel_name(ham, scheme, diagonal):
    """What hjw_last_kernel() reads after a substep of this instantiation."""
    return "stoch_substep_kernel<double, %s, %d, %d>" % (HAM_NAMES[ham], scheme, 1 if diagonal else 0)
