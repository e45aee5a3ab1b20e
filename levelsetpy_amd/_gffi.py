"""ctypes binding of libhj_shapes.so (include/hj_shapes.h): implicit surface functions and their set algebra.

One stateless entry point, the grid descriptor of include/hj_query.h and a HIP stream per call.  Loaded by _ffi.bind: a
missing library is an error.
"""
import ctypes as C

from . import _ffi, _qffi

MAX_OPS, MAX_DEPTH, MAX_ARRAYS = 64, 8, 8          # HJG_MAX_OPS, HJG_MAX_DEPTH, HJG_MAX_ARRAYS
SPHERE, CYLINDER, RECT, HALFSPACE, ARRAY, UNION, INTERSECT, DIFFERENCE, COMPLEMENT = range(1, 10)     # HJG_SPHERE ..
NEG, POS, ZERO = 1, 2, 4                           # HJG_NEG, HJG_POS, HJG_ZERO


class Op(C.Structure):
    """hjg_op."""
    _fields_ = [("code", C.c_int16), ("arg", C.c_int16), ("off", C.c_int32)]


class Array(C.Structure):
    """hjg_array."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("per_member", C.c_int32)]


class Program(C.Structure):
    """hjg_program."""
    _fields_ = [("n_ops", C.c_int32), ("n_arrays", C.c_int32), ("ops", Op * MAX_OPS), ("arrays", Array * MAX_ARRAYS),
                ("coord", C.c_void_p * _qffi.MAX_DIM)]


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "hjg_evaluate": (_i, [C.POINTER(_qffi.Grid), C.POINTER(Program), _vp, _i64, _i64, _vp, _i, _vp, _vp]),
    "hjg_last_error": (C.c_char_p, []),
    "hjg_last_kernel": (C.c_char_p, []),
}

LIB_PATH, lib, check, last_kernel = _ffi.bind("HJ_SHAPES_LIB", "libhj_shapes.so", "hjg", "hj_shapes error", SIGNATURES)


def program(ops, arrays=(), coord=(), cls=Program):
    """hjg_program (or, with cls, _kffi's hjk_program) from (code, arg, off) triples, (address, dtype id, per_member) triples and
    coordinate-table addresses.  Nothing is checked here: the library validates the program before it launches anything."""
    p = cls()
    p.n_ops, p.n_arrays = len(ops), len(arrays)
    for i, (code, arg, off) in enumerate(ops[:MAX_OPS]):
        p.ops[i].code, p.ops[i].arg, p.ops[i].off = int(code), int(arg), int(off)
    for s, (addr, dtype, per_member) in enumerate(arrays[:MAX_ARRAYS]):
        p.arrays[s].data, p.arrays[s].dtype, p.arrays[s].per_member = addr, int(dtype), int(bool(per_member))
    for d, addr in enumerate(coord):
        p.coord[d] = addr
    return p


def kernel_name(dtype_name, kernel="scene_kernel"):
    """What hjg_last_kernel() (with _kffi's kernel, hjk_last_kernel()) reads after an evaluation into this output type."""
    return "%s<%s>" % (kernel, "double" if dtype_name == "float64" else "float")
