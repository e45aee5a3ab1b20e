"""ctypes binding of libhj_batch.so (include/hj_batch.h): many problems on one grid, one launch per RK stage.

A library of its own beside libhj_mi355x.so (_ffi.py), libhj_query.so (_qffi.py), libhj_surface.so (_sffi.py),
libhj_ttr.so (_tffi.py) and libhj_rollout.so (_rffi.py): stateless entry points, the grid descriptor of _qffi and a HIP
stream per call.  As there, a missing library is an error -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi, _qffi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HJ_BATCH_LIB") or os.path.join(HERE, "csrc", "libhj_batch.so")

PAR_SLOTS = 8                                      # HJB_PAR_SLOTS
ARR_NONE, ARR_MIN, ARR_MAX, ARR_MAX_NEG = 0, 1, 2, 3   # HJB_ARR_*
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes batch_substep_kernel is instantiated for
HAM_DIMS = {_ffi.HAM_DUBINS_REL: 3, _ffi.HAM_DOUBLE_INTEGRATOR: 2, _ffi.HAM_DOUBLE_PENDULUM: 4}
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

_lib = None


def lib():
    """The loaded library; raises RuntimeError (loudly) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "levelsetpy_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C levelsetpy_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        # torch first, as _ffi.lib(): the process must share the HIP runtime its wheel bundles
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    """Non-zero return code -> ValueError (Unsupported for HJ_EUNSUPPORTED), as _ffi.check."""
    if rc != 0:
        msg = lib().hjb_last_error()
        text = (msg or b"hj_batch error").decode("utf-8", "replace") + " (code %d)" % rc
        raise (_ffi.Unsupported if rc == -3 else ValueError)(text)


def last_kernel():
    return (lib().hjb_last_kernel() or b"").decode()


def kernel_name(dtype_name, ham, scheme):
    """What hjb_last_kernel() reads after a substep of this instantiation."""
    return "batch_substep_kernel<%s, %s, %d>" % ("double" if dtype_name == "float64" else "float", HAM_NAMES[ham], scheme)
