"""CPU-only: the argument checks of libhj_shapes.so (include/hj_shapes.h) through ctypes: the refusals of
tests/tool_lib_cases.py, and valid programs up to the null output.  Every output pointer is null and every check comes before
the first HIP call, so no device is touched: a bad program is a refusal with a message, never a launch.  Also: the binding, the
header and the export table name the same functions, and the binding's constants and structures are the header's.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tool_lib_cases as T  # noqa: E402
from levelsetpy_amd import _ffi, _gffi, _qffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
G = _gffi


def grid(ndim=2, n=8, N0=None):
    N = [n] * ndim
    if N0 is not None:
        N[0] = N0
    return _qffi.grid_descriptor(ndim, N, [0.0] * ndim, [0.7] * ndim, [0.1] * ndim, [0] * ndim, [0] * ndim, "float64")


def call(g, ops, arrays=(), K=1, P=8, out_dtype=0, ndim=2):
    lib = G.lib()
    prog = G.program(ops, arrays, [FAKE] * ndim)
    before = lib.hjg_last_kernel()
    rc = lib.hjg_evaluate(C.byref(g), C.byref(prog), None, K, P, None, out_dtype, None, None)
    assert lib.hjg_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjg_last_error().decode()


SPH, ARR = (G.SPHERE, 0, 0), (G.ARRAY, 0, 0)
U, I, D, NOT = (G.UNION, 0, 0), (G.INTERSECT, 0, 0), (G.DIFFERENCE, 0, 0), (G.COMPLEMENT, 0, 0)

# the refusals are rows of tests/tool_lib_cases.py, asserted for every library by tests/test_tool_libs_host.py; here one by one
REFUSALS = [c for c in T.CASES if c[0] == "shapes"]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[1].split("-", 1)[1] for c in REFUSALS])
def test_refusals(case):
    before = G.last_kernel()
    rc, err, kernel = T.run(case)
    assert rc == case[4] and case[5] in err and kernel == before, T.line(case, rc, err, kernel)      # nothing was launched: the record stays


def test_valid_programs_pass_the_checks_and_stop_at_the_null_output():
    """Everything the library validates is in order: the refusal is the null output, the last check before a launch."""
    deepest = [SPH] * 8 + [U, I, D, NOT, U, I, D, U]
    longest = [SPH] + [NOT] * 63
    every = [(G.SPHERE, 0, 0), (G.CYLINDER, 3, 3), (G.RECT, 0, 4), (G.HALFSPACE, 0, 4), (G.ARRAY, 7, 0), U, I, D, NOT, U]
    arrays = [(FAKE, i % 2, i % 2) for i in range(8)]
    for ops, kw in ((deepest, {}), (longest, {}), (every, dict(arrays=arrays)), ([ARR], dict(arrays=arrays[:1], P=0))):
        rc, err = call(grid(), ops, **kw)
        assert rc == EINVAL and err == "null argument", err
    rc, err = call(grid(4, n=3), [(G.RECT, 0, 0), (G.SPHERE, 0, 3), D], ndim=4)
    assert rc == EINVAL and err == "null argument", err


def test_an_empty_grid_launches_nothing():
    rc, _ = call(grid(2, N0=0), [SPH])
    assert rc == OK


def test_check_maps_the_codes():
    rc, err = call(grid(), [SPH, U])
    with pytest.raises(ValueError) as info:
        G.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    rc, err = call(grid(), [SPH], out_dtype=7)
    with pytest.raises(_ffi.Unsupported):
        G.check(rc)
    G.check(0)


def test_a_refusal_leaves_the_other_libraries_records_alone():
    from levelsetpy_amd import _tffi
    _tffi.lib().hjt_ttr_init(7, None, 1, 0.0, 0.0, None, None, None)
    before = _tffi.lib().hjt_last_error()
    assert b"dtype" in before
    rc, err = call(grid(), [SPH, SPH])
    assert rc == EINVAL and "leaves 2" in err and _tffi.lib().hjt_last_error() == before


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_shapes.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjg_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(G.SIGNATURES) == ["hjg_evaluate", "hjg_last_error", "hjg_last_kernel"]
    out = subprocess.check_output(["nm", "-D", G.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hjg_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-fh-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    lib = G.lib()
    for name, (_, args) in G.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJG_MAX_OPS", G.MAX_OPS), ("HJG_MAX_DEPTH", G.MAX_DEPTH), ("HJG_MAX_ARRAYS", G.MAX_ARRAYS),
                      ("HJG_SPHERE", G.SPHERE), ("HJG_CYLINDER", G.CYLINDER), ("HJG_RECT", G.RECT), ("HJG_HALFSPACE", G.HALFSPACE),
                      ("HJG_ARRAY", G.ARRAY), ("HJG_UNION", G.UNION), ("HJG_INTERSECT", G.INTERSECT), ("HJG_DIFFERENCE", G.DIFFERENCE),
                      ("HJG_COMPLEMENT", G.COMPLEMENT), ("HJG_NEG", G.NEG), ("HJG_POS", G.POS), ("HJG_ZERO", G.ZERO)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert (G.MAX_OPS, G.MAX_DEPTH, G.MAX_ARRAYS) == (64, 8, 8)
    assert C.sizeof(G.Op) == 8 and C.sizeof(G.Array) == 16
    assert C.sizeof(G.Program) == 8 + 64 * 8 + 8 * 16 + 4 * 8
    import shapes_ref as R
    assert [getattr(R, n) for n in ("SPHERE", "CYLINDER", "RECT", "HALFSPACE", "ARRAY", "UNION", "INTERSECT", "DIFFERENCE", "COMPLEMENT",
                                     "NEG", "POS", "ZERO")] == [G.SPHERE, G.CYLINDER, G.RECT, G.HALFSPACE, G.ARRAY, G.UNION, G.INTERSECT,
                                                                G.DIFFERENCE, G.COMPLEMENT, G.NEG, G.POS, G.ZERO]


def test_the_makefile_builds_and_cleans_the_library():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\blibhj_shapes\.so\b", mk, re.M) and re.search(r"^\trm -f .*\blibhj_shapes\.so\b", mk, re.M)
    assert re.search(r"^libhj_shapes\.so: hj_shapes\.hip hj_tool_host\.h", mk, re.M) and "hj_shapes.hip" in mk.split("HIPCC ?=")[0]
