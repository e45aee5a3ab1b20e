"""ctypes binding of libhj_surface.so (include/hj_surface.h): level sets as indexed meshes.

A library of its own beside libhj_mi355x.so (_ffi.py) and libhj_query.so (_qffi.py, whose grid descriptor it
shares): stateless entry points, a HIP stream per call.  As there, a missing library is an error -- there is
no CPU fallback.
"""
import ctypes as C
import os

from . import _ffi
from ._qffi import Grid, grid_descriptor  # noqa: F401  (hjq_grid)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HJ_SURFACE_LIB") or os.path.join(HERE, "csrc", "libhj_surface.so")

_vp, _i, _i64, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t
_pg = C.POINTER(Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjs_workspace_size": (_i, [_pg, _i64, C.POINTER(_sz)]),
    "hjs_count": (_i, [_pg, _vp, _i64, _i64, _d, _vp, _sz, _vp, _vp]),
    "hjs_emit": (_i, [_pg, _vp, _i64, _i64, _d, _vp, _sz, C.POINTER(_i64), _vp, _vp, _vp]),
    "hjs_last_error": (C.c_char_p, []),
    "hjs_last_kernel": (C.c_char_p, []),
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
        msg = lib().hjs_last_error()
        text = (msg or b"hj_surface error").decode("utf-8", "replace") + " (code %d)" % rc
        raise (_ffi.Unsupported if rc == -3 else ValueError)(text)


def last_kernels():
    """The kernels the calling thread's last successful call launched, in order."""
    s = (lib().hjs_last_kernel() or b"").decode()
    return s.split(";") if s else []
