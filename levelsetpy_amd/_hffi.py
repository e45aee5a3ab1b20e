"""ctypes binding of libhj_hidim.so (include/hj_hidim.h): Hamilton-Jacobi substeps on 5-D and 6-D grids.

Stateless entry points, a grid descriptor of its own (hjh_grid: hjq_grid with six axes) and a HIP stream per call.
Loaded by _ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi, _qffi

MIN_DIM, MAX_DIM = 5, 6                            # HJH_MIN_DIM, HJH_MAX_DIM
PAR_SLOTS = 8                                      # HJH_PAR_SLOTS
HAM_PLANE5D, HAM_DUBINS_PAIR6D = 50, 51            # HJH_HAM_*
ARR_NONE, ARR_MIN, ARR_MAX, ARR_MAX_NEG = 0, 1, 2, 3   # HJH_ARR_*
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes the kernels are instantiated for
HAM_DIMS = {HAM_PLANE5D: 5, HAM_DUBINS_PAIR6D: 6}
HAM_NAMES = {HAM_PLANE5D: "HamPlane5D", HAM_DUBINS_PAIR6D: "HamDubinsPair6D"}
HAM_USER_BASE = 1000                               # HJH_HAM_USER_BASE: ids of systems registered at run time (hidim_ham.py)


class Grid(C.Structure):
    """hjh_grid."""
    _fields_ = [("ndim", C.c_int32), ("dtype", C.c_int32),
                ("N", C.c_int64 * MAX_DIM), ("xmin", C.c_double * MAX_DIM), ("xlast", C.c_double * MAX_DIM),
                ("dx", C.c_double * MAX_DIM), ("bc", C.c_int32 * MAX_DIM), ("toward_zero", C.c_int32 * MAX_DIM)]


class Tables(C.Structure):
    """hjh_tables."""
    _fields_ = [("coord", C.c_void_p * MAX_DIM), ("aux", C.c_void_p * 4)]


_vp, _i, _i64, _d, _u = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_uint
_pg, _pt = C.POINTER(Grid), C.POINTER(Tables)
_pd, _pi64, _pi32, _pvp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjh_substep": (_i, [_pg, _pt, _i, _i, _i, _i, _pd, _vp, _vp, _vp, _d, _i, _i, _vp, _i, _vp, _vp]),
    "hjh_step_bound": (_i, [_pg, _pt, _i, _pd, _vp, _pd, _pd, _vp]),
    "hjh_integrate": (_i, [_pg, _pt, _i, _i, _i, _i, _i, _pd, _d, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _d, _d, _d, _d, _d,
                           _pd, _pi64, _pi32, _vp]),
    "hjh_upwind": (_i, [_pg, _i, _vp, _u, _pvp, _pvp, _vp, _vp]),
    "hjh_ham_register": (_i, [C.c_char_p, _i, _i, C.c_char_p, _i, _pi32, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]),
    "hjh_ham_info": (_i, [_i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _pi32, C.POINTER(C.c_int)]),
    "hjh_ham_compile_check": (_i, [_i, _i, _i]),
    "hjh_ham_source": (_i, [_i, C.c_char_p, _i64]),
    "hjh_ham_cache_stats": (_i, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hjh_last_error": (C.c_char_p, []),
    "hjh_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_HIDIM_LIB", "libhj_hidim.so", "hjh", "hj_hidim error", SIGNATURES)


def grid_descriptor(ndim, N, xmin, xlast, dx, bc, tz, dtype_name):
    return _ffi.grid_descriptor(Grid, MAX_DIM, ndim, N, xmin, xlast, dx, bc, tz, dtype_name)


def decode(bound, check, g, ndim, node):
    """<prefix>_decode of the 1-D to 6-D libraries (`bound`, with the library's `check`): the multi-index their kernels' decode
    gives flat node `node` of the grid of descriptor g."""
    idx = (C.c_int32 * MAX_DIM)()
    check(bound(C.byref(g), int(node), C.byref(idx)))
    return tuple(idx[:ndim])


def params(values):
    """HJH_PAR_SLOTS doubles on the host, unused slots 0."""
    v = [float(x) for x in values]
    return (C.c_double * PAR_SLOTS)(*(v + [0.0] * (PAR_SLOTS - len(v))))


def ham_dim(ham):
    """State dimension of a system id: a built-in's, or a registration's (hjh_ham_info); None for an id nothing answers to."""
    ham = int(ham)
    if ham < HAM_USER_BASE:
        return HAM_DIMS.get(ham)
    nd = C.c_int()
    if lib().hjh_ham_info(ham, C.byref(nd), None, None, None, None) != 0:
        return None
    return int(nd.value)


def kernel_name(dtype_name, ham, scheme):
    """What hjh_last_kernel() reads after a substep of this instantiation."""
    if int(ham) >= HAM_USER_BASE:
        from .hidim_ham import name_of
        system = "HamUser:%s" % name_of(ham)
    else:
        system = HAM_NAMES[ham]
    return "hidim_substep_kernel<%s, %s, %d>" % ("double" if dtype_name == "float64" else "float", system, scheme)
