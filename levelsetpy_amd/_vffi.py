"""ctypes binding of libhj_measure.so (include/hj_measure.h): volumes, overlaps and bounds of sublevel sets on the device, on
grids of 1 to 6 dimensions.

Stateless entry points, a grid descriptor of include/hj_hidim.h (hjh_grid) and a HIP stream per call.  Loaded by _ffi.bind: a
missing library is an error.
"""
import ctypes as C

from . import _ffi, _hffi

MAX_DIM = 6                                        # HJV_MAX_DIM
RECORD_WORDS = 20                                  # HJV_RECORD_WORDS
CELLS, FULL, CUT, INVALID, QLO, QHI, INSIDE, NAN, LO, HI = 0, 1, 2, 3, 4, 5, 6, 7, 8, 14      # HJV_CELLS .. HJV_HI
SET_A, SET_B, SET_UNION, SET_INTERSECTION = 0, 1, 2, 3                                       # HJV_SET_*
MAX_SLOTS = 32                                     # HJV_MAX_SLOTS
Q_ONE = 1 << 52                                    # the whole simplex


class LaunchPlan(C.Structure):
    """hjv_launch_plan."""
    _fields_ = [("first_tail", C.c_int32), ("field_launches", C.c_int32), ("nfields", C.c_int64), ("total", C.c_int64),
                ("tail", C.c_int64), ("head", C.c_int64), ("chunks", C.c_int64), ("heads_per_launch", C.c_int64),
                ("launches", C.c_int64), ("blocks_full", C.c_int64), ("blocks_last", C.c_int64), ("slots", C.c_int64)]


_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pg = C.POINTER(_hffi.Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjv_measure": (_i, [_pg, _vp, _i64, _i64, _vp, _i, _i64, _i64, _d, _vp, _vp, _vp]),
    "hjv_workspace_size": (_i64, [_pg, _i64, _i]),
    "hjv_plan": (_i, [_pg, _i64, C.POINTER(LaunchPlan)]),
    "hjv_decode": (_i, [_pg, _i64, C.POINTER(C.c_int32 * MAX_DIM)]),
    "hjv_simplex_q_host": (_i, [_i, C.POINTER(_d), C.POINTER(C.c_uint64)]),
    "hjv_last_error": (C.c_char_p, []),
    "hjv_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_MEASURE_LIB", "libhj_measure.so", "hjv", "hj_measure error", SIGNATURES)


def extents_descriptor(N, periodic=(), dtype_name="float64"):
    """hjh_grid of the extents N and the periodic axes: all the library reads of a grid (ndim, dtype, N, bc)."""
    nd = len(N)
    bc = [1 if d in periodic else 0 for d in range(nd)]
    return _hffi.grid_descriptor(nd, [int(v) for v in N], [0.0] * nd, [0.0] * nd, [1.0] * nd, bc, [0] * nd, dtype_name)


def kernel_names(dtype_a, dtype_b, ndim):
    """What hjv_last_kernel() reads after a call; dtype_b None: a measurement, not a comparison."""
    c = {"float64": "double", "float32": "float"}
    return "measure_kernel<%s, %s, %d, %d>;measure_fold_kernel" % (c[dtype_a], c[dtype_b or dtype_a], ndim, dtype_b is not None)


def plan(N, nfields=1, periodic=()):
    """hjv_plan on a grid of extents N -> LaunchPlan.  No device is touched."""
    p = LaunchPlan()
    g = extents_descriptor(N, periodic)
    check(lib().hjv_plan(C.byref(g), int(nfields), C.byref(p)))
    return p


def decode(N, node):
    """hjv_decode: the multi-index the kernel's decode gives flat node `node` of a grid of extents N."""
    return _hffi.decode(lib().hjv_decode, check, extents_descriptor(N), len(N), node)


def simplex_q(f):
    """hjv_simplex_q_host: q of the simplex with vertex values f[0 .. D] in path order, by the device's function run on the host."""
    D = len(f) - 1
    arr = (_d * (D + 1))(*[float(v) for v in f])
    q = C.c_uint64()
    check(lib().hjv_simplex_q_host(D, arr, C.byref(q)))
    return int(q.value)
