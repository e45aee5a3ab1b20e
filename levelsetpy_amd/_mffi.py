"""ctypes binding of libhj_resample.so (include/hj_resample.h): value functions resampled across grids and frames on the
device, on grids of 1 to 6 dimensions.

Stateless entry points, two grid descriptors of include/hj_hidim.h (hjh_grid) and a HIP stream per call.  Loaded by
_ffi.bind: a missing library is an error.
"""
import ctypes as C

from . import _ffi, _hffi

MAX_DIM = 6                                        # HJM_MAX_DIM
REDUCE_NONE, REDUCE_MIN, REDUCE_MAX = 0, 1, 2      # HJM_REDUCE_*
FILL_NAN, FILL_VALUE, FILL_MAX = 0, 1, 2           # HJM_FILL_*
COUNT_SLOTS = 32                                   # HJM_COUNT_SLOTS


class LaunchPlan(C.Structure):
    """hjm_launch_plan."""
    _fields_ = [("first_tail", C.c_int32), ("array_launches", C.c_int32), ("arrays", C.c_int64), ("total", C.c_int64),
                ("tail", C.c_int64), ("head", C.c_int64), ("chunks", C.c_int64), ("heads_per_launch", C.c_int64),
                ("launches", C.c_int64), ("blocks_full", C.c_int64), ("blocks_last", C.c_int64)]


_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pg = C.POINTER(_hffi.Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjm_resample": (_i, [_pg, _pg, C.POINTER(_vp * MAX_DIM), _vp, _i64, _i64, _vp, _i64, _i, _i, _d, _vp, _i, _vp, _vp, _vp]),
    "hjm_workspace_size": (_i64, [_i64]),
    "hjm_plan": (_i, [_pg, _i64, _i64, _i, C.POINTER(LaunchPlan)]),
    "hjm_decode": (_i, [_pg, _i64, C.POINTER(C.c_int32 * MAX_DIM)]),
    "hjm_last_error": (C.c_char_p, []),
    "hjm_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_RESAMPLE_LIB", "libhj_resample.so", "hjm", "hj_resample error", SIGNATURES)


def extents_descriptor(N, dtype_name="float64"):
    """hjh_grid of the extents N alone: all the library reads of a destination (ndim, N)."""
    nd = len(N)
    return _hffi.grid_descriptor(nd, [int(v) for v in N], [0.0] * nd, [0.0] * nd, [1.0] * nd, [0] * nd, [0] * nd, dtype_name)


def coord_table(pointers):
    """The D device pointers of the destination's coordinate vectors as the host array hjm_resample takes."""
    return (_vp * MAX_DIM)(*([int(p) for p in pointers] + [0] * (MAX_DIM - len(pointers))))


def kernel_names(dtype_name, ndim, reduce, fill_max):
    """What hjm_last_kernel() reads after a call: the resampling kernel, the sum of the counts [and the fill kernel of FILL_MAX]."""
    main = "resample_kernel<%s, %d, %d>" % ("double" if dtype_name == "float64" else "float", ndim, reduce)
    return main + ";resample_counts_kernel" + (";resample_fill_kernel<%d, %d>" % (ndim, min(reduce, 1)) if fill_max else "")


def plan(N, nfields=1, K=1, reduce=REDUCE_NONE):
    """hjm_plan onto a grid of extents N -> LaunchPlan.  No device is touched."""
    p = LaunchPlan()
    g = extents_descriptor(N)
    check(lib().hjm_plan(C.byref(g), int(nfields), int(K), int(reduce), C.byref(p)))
    return p


def decode(N, node):
    """hjm_decode: the multi-index the kernel's decode gives flat node `node` of a grid of extents N."""
    return _hffi.decode(lib().hjm_decode, check, extents_descriptor(N), len(N), node)
