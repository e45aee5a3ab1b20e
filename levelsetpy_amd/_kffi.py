"""ctypes binding of libhj_hishapes.so (include/hj_hishapes.h): implicit surface functions on grids of 1 to 6 dimensions.

Stateless entry points, the grid descriptor of include/hj_hidim.h (hjh_grid) and a HIP stream per call.  The opcodes,
limits and flags are libhj_shapes.so's (_gffi.py) with one leaf more, SPHERE_OF.  Loaded by _ffi.bind: a missing library is
an error.
"""
import ctypes as C
import functools

from . import _ffi, _gffi, _hffi

MAX_DIM = 6                                        # HJK_MAX_DIM
MAX_OPS, MAX_DEPTH, MAX_ARRAYS = _gffi.MAX_OPS, _gffi.MAX_DEPTH, _gffi.MAX_ARRAYS
SPHERE_OF = 10                                     # HJG_SPHERE_OF
Op, Array = _gffi.Op, _gffi.Array


class Program(C.Structure):
    """hjk_program."""
    _fields_ = [("n_ops", C.c_int32), ("n_arrays", C.c_int32), ("ops", Op * MAX_OPS), ("arrays", Array * MAX_ARRAYS),
                ("coord", C.c_void_p * MAX_DIM)]


class LaunchPlan(C.Structure):
    """hjk_launch_plan."""
    _fields_ = [("first_tail", C.c_int32), ("member_launches", C.c_int32), ("total", C.c_int64), ("tail", C.c_int64),
                ("head", C.c_int64), ("chunks", C.c_int64), ("heads_per_launch", C.c_int64), ("launches", C.c_int64),
                ("blocks_full", C.c_int64), ("blocks_last", C.c_int64)]


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjk_evaluate": (_i, [C.POINTER(_hffi.Grid), C.POINTER(Program), _vp, _i64, _i64, _vp, _i, _vp, _vp]),
    "hjk_plan": (_i, [C.POINTER(_hffi.Grid), _i64, C.POINTER(LaunchPlan)]),
    "hjk_decode": (_i, [C.POINTER(_hffi.Grid), _i64, C.POINTER(C.c_int32 * MAX_DIM)]),
    "hjk_last_error": (C.c_char_p, []),
    "hjk_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_HISHAPES_LIB", "libhj_hishapes.so", "hjk", "hj_hishapes error", SIGNATURES)


program = functools.partial(_gffi.program, cls=Program)                        # hjk_program, filled as hjg_program is
kernel_name = functools.partial(_gffi.kernel_name, kernel="hi_scene_kernel")    # what hjk_last_kernel() reads after an evaluation


def grid_descriptor(N, dtype_name="float64"):
    """hjh_grid of the extents N alone: all the library reads of a descriptor (ndim, dtype, N)."""
    nd = len(N)
    return _hffi.grid_descriptor(nd, [int(v) for v in N], [0.0] * nd, [0.0] * nd, [1.0] * nd, [0] * nd, [0] * nd, dtype_name)


def plan(N, K=1):
    """hjk_plan of a grid of extents N and K members -> LaunchPlan.  No device is touched."""
    p = LaunchPlan()
    g = grid_descriptor(N)
    check(lib().hjk_plan(C.byref(g), int(K), C.byref(p)))
    return p


def decode(N, node):
    """hjk_decode: the multi-index the kernel's decode gives flat node `node` of a grid of extents N."""
    return _hffi.decode(lib().hjk_decode, check, grid_descriptor(N), len(N), node)
