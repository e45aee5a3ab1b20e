"""ctypes binding of libhj_mc.so (include/hj_mc.h): Monte Carlo rollouts of dx = f dt + G dW in one launch, and their
counter-based generator on the device and on the host.

Stateless entry points, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a missing
library is an error.  hjn_normals_host needs no GPU.
"""
import ctypes as C

import numpy as np

from . import _ffi, _qffi, _rffi

POLICY_EARLIEST, POLICY_CLOCK = 0, 1               # HJN_POLICY_*
POLICIES = {'earliest': POLICY_EARLIEST, 'clock': POLICY_CLOCK}
SCHEMES = _rffi.SCHEMES
PLANT_DIMS = _rffi.PLANT_DIMS
Plant = _rffi.Plant
MAX_ND = _qffi.MAX_DIM

_vp, _i, _i64, _u64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjn_rollout": (_i, [C.POINTER(_qffi.Grid), _i, _vp, _i64, _i64, _vp, _i64, _i64, _u64, _u64, _vp, _vp, _d, _i, _i, _d,
                         C.POINTER(Plant), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hjn_normals": (_i, [_u64, _u64, _i64, _i64, _i64, _i, _vp, _vp, _vp]),
    "hjn_normals_host": (_i, [_u64, _u64, _i64, _i64, _i64, _i, _vp, _vp]),
    "hjn_last_error": (C.c_char_p, []),
    "hjn_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_MC_LIB", "libhj_mc.so", "hjn", "hj_mc error", SIGNATURES)


def normals_host(seed, first, count, step0, nsteps, nd, words=False):
    """The generator on the host: (count, nsteps, nd) float64 normals [, (count, nsteps, (nd+1)//2, 4) uint32 words]."""
    out = np.empty((count, nsteps, nd), dtype=np.float64)
    w = np.empty((count, nsteps, (nd + 1) // 2, 4), dtype=np.uint32) if words else None
    check(lib().hjn_normals_host(int(seed), int(first), int(count), int(step0), int(nsteps), int(nd),
                                 w.ctypes.data if words else None, out.ctypes.data))
    return (out, w) if words else out
