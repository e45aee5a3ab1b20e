"""ctypes binding of libhj_rollout.so (include/hj_rollout.h): many optimal trajectories in one launch.

A library of its own beside libhj_mi355x.so (_ffi.py), libhj_query.so (_qffi.py), libhj_surface.so (_sffi.py) and
libhj_ttr.so (_tffi.py): one stateless entry point, the grid descriptor of _qffi and a HIP stream per call.  As there, a
missing library is an error -- there is no CPU fallback.
"""
import ctypes as C
import os

from . import _ffi, _qffi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HJ_ROLLOUT_LIB") or os.path.join(HERE, "csrc", "libhj_rollout.so")

MODE_MIN, MODE_MAX = 0, 1                          # HJR_MODE_*
REACHED, EXHAUSTED, LEFT_GRID = 0, 1, 2            # HJR_* status of a trajectory
SCHEMES = _qffi.POINT_SCHEMES                      # the schemes hjr_rollout instantiates
PLANT_DIMS = {_ffi.HAM_DUBINS_REL: 3, _ffi.HAM_DOUBLE_INTEGRATOR: 2, _ffi.HAM_DOUBLE_PENDULUM: 4}


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
        msg = lib().hjr_last_error()
        text = (msg or b"hj_rollout error").decode("utf-8", "replace") + " (code %d)" % rc
        raise (_ffi.Unsupported if rc == -3 else ValueError)(text)


def last_kernel():
    return (lib().hjr_last_kernel() or b"").decode()


def plant_descriptor(ham_id, u_mode, d_mode, params):
    p = Plant()
    p.id, p.u_mode, p.d_mode, p.reserved = int(ham_id), int(u_mode), int(d_mode), 0
    for k in range(4):
        p.params[k] = float(params[k]) if k < len(params) else 0.0
    return p
