"""CPU-only: libhj_hishapes.so (include/hj_hishapes.h) through ctypes, in the manner of tests/test_shapes_host.py.

  * the argument checks of hjk_evaluate, hjk_plan and hjk_decode (the refusals of tests/tool_lib_cases.py, and valid programs up
    to the null output): every output pointer is null and every check comes before the first HIP call, so no
    device is touched -- a bad program is a refusal with a message, never a launch;
  * hjk_plan of the named grids and of the members past gridDim.y = 65535; what hjk_plan and hjk_decode refuse (that the launches
    cover every node once and that the decode is np.unravel_index: tests/test_node_index_host.py, for the three libraries that
    share the walk);
  * the binding, the header and the export table name the same functions; the Makefile keeps its old lines.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tool_lib_cases as T  # noqa: E402
from levelsetpy_amd import _ffi, _gffi, _hffi, _kffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
G, K = _gffi, _kffi


def grid(ndim=5, n=4, dtype="float64", N0=None):
    N = [n] * ndim
    if N0 is not None:
        N[0] = N0
    return K.grid_descriptor(N, dtype)


def call(g, ops, arrays=(), coord=None, P=64, out_dtype=0):
    lib = K.lib()
    prog = K.program(ops, arrays, [FAKE] * 6 if coord is None else coord)
    before = lib.hjk_last_kernel()
    rc = lib.hjk_evaluate(C.byref(g), C.byref(prog), None, 1, P, None, out_dtype, None, None)
    assert lib.hjk_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjk_last_error().decode()


SPH, ARR = (G.SPHERE, 0, 0), (G.ARRAY, 0, 0)
U, I, D, NOT = (G.UNION, 0, 0), (G.INTERSECT, 0, 0), (G.DIFFERENCE, 0, 0), (G.COMPLEMENT, 0, 0)
OF = (K.SPHERE_OF, 2, 0)

# the refusals are rows of tests/tool_lib_cases.py, asserted for every library by tests/test_tool_libs_host.py; here one by one
def refused(case):
    before = K.last_kernel()
    rc, err, kernel = T.run(case)
    assert rc == case[4] and case[5] in err and kernel == before, T.line(case, rc, err, kernel)      # nothing was launched: the record stays


REFUSALS = [c for c in T.CASES if c[0] == "hishapes" and c[2] == "hjk_evaluate"]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[1].split("-", 1)[1] for c in REFUSALS])
def test_refusals(case):
    refused(case)


def test_valid_programs_pass_the_checks_and_stop_at_the_null_output():
    """Everything the library validates is in order: the refusal is the null output, the last check before a launch."""
    deepest = [OF] * 8 + [U, I, D, NOT, U, I, D, U]
    longest = [OF] + [NOT] * 63
    every = [(G.SPHERE, 0, 0), (G.CYLINDER, 31, 6), (G.RECT, 0, 12), (G.HALFSPACE, 0, 22), (K.SPHERE_OF, 6, 0), (G.ARRAY, 7, 0), U, I, D, NOT, U, U]
    arrays = [(FAKE, i % 2, i % 2) for i in range(8)]
    for ops, kw in ((deepest, {}), (longest, {}), (every, dict(arrays=arrays, P=37)), ([ARR], dict(arrays=arrays[:1], P=0))):
        rc, err = call(grid(), ops, **kw)
        assert rc == EINVAL and err == "null argument", err
    for nd in range(1, 7):                                 # every dimension, the sixth coordinate table unused below 6
        rc, err = call(grid(nd, n=3), [(G.RECT, 0, 0), (K.SPHERE_OF, nd, 0), D], P=nd * nd + nd + 1, coord=[FAKE] * nd + [None] * (6 - nd))
        assert rc == EINVAL and err == "null argument", (nd, err)


def test_an_empty_grid_launches_nothing():
    for g in (grid(5, N0=0), grid(1, N0=0), grid(6, N0=0)):
        rc, _ = call(g, [OF])
        assert rc == OK
    p = K.plan((4, 0, 3, 2, 2))
    assert (p.total, p.tail, p.head, p.chunks, p.launches, p.blocks_full, p.blocks_last) == (0,) * 7


def test_check_maps_the_codes():
    rc, err = call(grid(), [SPH, U])
    with pytest.raises(ValueError) as info:
        K.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    rc, err = call(grid(), [SPH], out_dtype=7)
    with pytest.raises(_ffi.Unsupported):
        K.check(rc)
    K.check(0)


def test_a_refusal_leaves_the_shape_librarys_record_alone():
    rc = G.lib().hjg_evaluate(None, None, None, 1, 0, None, 0, None, None)
    before = G.lib().hjg_last_error()
    assert rc == EINVAL and b"null grid" in before
    rc, err = call(grid(), [SPH, SPH])
    assert rc == EINVAL and "leaves 2" in err and G.lib().hjg_last_error() == before


# ------------------------------------------------------------------------------------------ the plan (its walk: tests/test_node_index_host.py)
def test_plan_of_the_named_grids():
    p = K.plan((25,) * 6)
    assert (p.first_tail, p.head, p.tail, p.launches) == (0, 1, 25 ** 6, 1)
    p = K.plan((41,) * 6)
    # a launch has fewer than 2^32 threads, 2^24 - 1 workgroups: a grid past 2^32 nodes takes more than one
    assert 41 ** 6 > 2 ** 32 and (p.first_tail, p.head, p.tail, p.heads_per_launch, p.launches) == (1, 41, 41 ** 5, 37, 2)
    p = K.plan((3, 2 ** 31 - 1))
    assert (p.first_tail, p.head, p.tail, p.chunks, p.heads_per_launch, p.launches) == (1, 3, 2 ** 31 - 1, 2 ** 23, 1, 3)
    p = K.plan((46341, 46341, 2 ** 31 - 1))
    assert p.head == 46341 ** 2 > 2 ** 31 and p.heads_per_launch == 1 and p.launches == 46341 ** 2
    # members: gridDim.y ends at 65535
    assert [K.plan((2, 1, 2, 1, 2), k).member_launches for k in (1, 65535, 65536, 65537, 131071)] == [1, 1, 2, 2, 3]


def test_plan_refuses_what_the_grid_check_refuses():
    """An axis of 2^31 nodes or more is outside the descriptor's contract (as in libhj_shapes.so): (2^31 + 5, 2) is refused, by name."""
    rows = [c for c in T.CASES if c[0] == "hishapes" and (c[2] == "hjk_plan" or c[5] in ("N[0] = 2147483653", "N[1]", "2^63"))]
    assert len(rows) == 8
    for case in rows:
        refused(case)


# ------------------------------------------------------------------------------------------ the decode (against unravel_index: tests/test_node_index_host.py)
def test_decode_refuses_a_node_outside_the_grid():
    rows = [c for c in T.CASES if c[1] in ("decode-node-1", "decode-node60", "decode-null")]
    assert len(rows) == 3
    for case in rows:
        refused(case)


def test_one_source_for_the_interpreter():
    """The interpreter loop, the sign-flag vote and the program's checks stand once, in hj_shapes_dev.h: the two libraries' kernels
    and entry points are frames around them."""
    src = lambda n: open(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)).read()      # noqa: E731
    dev, users = src("hj_shapes_dev.h"), [src("hj_shapes.hip"), src("hj_hishapes.hip")]
    for marker in ("below[sp - 1]", "atomicOr", "stack underflow", "unknown opcode", "outside a row"):
        assert marker in dev and not any(marker in u for u in users), marker
    for name in ("check_program", "OP_NAMES"):
        assert len(re.findall(r"^static [^;=(]*\b%s\b" % name, dev, re.M)) == 1, name
        assert not any(re.search(r"^static [^;=(]*\b%s\b" % name, u, re.M) for u in users), name
    assert all('#include "hj_shapes_dev.h"' in u for u in users)


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_hishapes.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjk_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(K.SIGNATURES) == ["hjk_decode", "hjk_evaluate", "hjk_last_error", "hjk_last_kernel", "hjk_plan"]
    out = subprocess.check_output(["nm", "-D", K.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hjk_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-jl-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    kernels = sorted(set(re.findall(r"\b(_ZN3hjk15hi_scene_kernelI[df]E\w*)", out)))
    stubs = sorted(set(n for n in kernels if not n.endswith(".kd")))
    assert len(stubs) == 2 and "hi_scene_kernelIdE" in stubs[0] and "hi_scene_kernelIfE" in stubs[1], out
    lib = K.lib()
    for name, (_, args) in K.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJK_MAX_DIM", K.MAX_DIM), ("HJG_SPHERE_OF", K.SPHERE_OF)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert K.SPHERE_OF == G.COMPLEMENT + 1 == 10 and (K.MAX_OPS, K.MAX_DEPTH, K.MAX_ARRAYS) == (G.MAX_OPS, G.MAX_DEPTH, G.MAX_ARRAYS)
    assert C.sizeof(K.Program) == 8 + 64 * 8 + 8 * 16 + 6 * 8 == C.sizeof(G.Program) + 16
    assert C.sizeof(K.LaunchPlan) == 8 + 8 * 8 and _hffi.MAX_DIM == K.MAX_DIM
    import hishapes_ref as H
    assert H.SPHERE_OF == K.SPHERE_OF


def test_the_makefile_builds_the_library_beside_the_old_lines():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    all_lines = re.findall(r"^all:(.*)$", mk, re.M)
    assert len(re.findall(r"\blibhj_\w+\.so\b", " ".join(all_lines))) == 10 and "hishapes" not in " ".join(all_lines)
    libs = re.findall(r"^libs:(.*)$", mk, re.M)
    assert libs[0].split() == ["all", "libhj_hiquery.so", "libhj_plant.so"] and libs[1:] == [" libhj_hishapes.so"]
    assert re.search(r"^libhj_hishapes\.so: hj_hishapes\.hip hj_tool_host\.h hj_shapes_dev\.h", mk, re.M)
    assert re.search(r"^libhj_shapes\.so: hj_shapes\.hip hj_tool_host\.h hj_shapes_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-hishapes:", mk, re.M) and re.search(r"^\trm -f .*\blibhj_hishapes\.so\b", mk, re.M)
    assert "hj_hishapes.hip" in mk.split("HIPCC ?=")[0] and "hj_shapes_dev.h" in mk.split("HIPCC ?=")[0]
    assert re.search(r"^\.DEFAULT_GOAL := libs$", mk, re.M)
