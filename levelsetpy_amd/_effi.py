"""ctypes binding of libhj_eikonal.so (include/hj_eikonal.h): signed distance and first-arrival time from a level set.

Stateless entry points, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a
missing library is an error.
"""
import ctypes as C

from . import _ffi, _qffi

NEG, POS, ZERO = 1, 2, 4                           # HJE_NEG, HJE_POS, HJE_ZERO
FLAGS_OFFSET = 64                                  # HJE_FLAGS_OFFSET
GROUP = 8                                          # passes between two reads of the counters (GROUP of csrc/hj_eikonal.hip)
TILES = {1: (256,), 2: (16, 32), 3: (4, 8, 16), 4: (4, 4, 4, 8)}      # tile_dim of csrc/hj_eikonal.hip

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_pg = C.POINTER(_qffi.Grid)

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hje_workspace_size": (_i, [_pg, _i64, C.POINTER(_i64)]),
    "hje_signed_distance": (_i, [_pg, _vp, _i64, _i64, _d, _d, _vp, _d, _vp, _vp, _i64, _i64, C.POINTER(_i64), _vp]),
    "hje_last_error": (C.c_char_p, []),
    "hje_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_EIKONAL_LIB", "libhj_eikonal.so", "hje", "hj_eikonal error", SIGNATURES)


def tile_count(N):
    """Tiles of a grid of shape N."""
    n = 1
    for size, t in zip(N, TILES[len(N)]):
        n *= -(-int(size) // t)
    return n


def default_max_passes(N):
    """8 * sum_d ceil(N_d / tile_d) + 64."""
    return 8 * sum(-(-int(size) // t) for size, t in zip(N, TILES[len(N)])) + 64


def launched_passes(passes, max_passes):
    """Passes the host loop launched when the first `passes` of them sufficed: whole groups of GROUP, at most max_passes."""
    return min(-(-int(passes) // GROUP) * GROUP, int(max_passes))
