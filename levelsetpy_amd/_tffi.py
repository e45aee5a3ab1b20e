"""ctypes binding of libhj_ttr.so (include/hj_ttr.h): time-to-reach functions.

A library of its own beside libhj_mi355x.so (_ffi.py), libhj_query.so (_qffi.py) and libhj_surface.so (_sffi.py):
stateless entry points, plain pointers and a HIP stream per call.  As there, a missing library is an error -- there is
no CPU fallback.
"""
import ctypes as C
import os

from . import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HJ_TTR_LIB") or os.path.join(HERE, "csrc", "libhj_ttr.so")

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
        msg = lib().hjt_last_error()
        text = (msg or b"hj_ttr error").decode("utf-8", "replace") + " (code %d)" % rc
        raise (_ffi.Unsupported if rc == -3 else ValueError)(text)


def last_kernel():
    return (lib().hjt_last_kernel() or b"").decode()
