"""CPU-only: the argument checks of libhj_decomp.so (include/hj_decomp.h) through ctypes, in the manner of
tests/test_shapes_host.py.  Every output pointer is null and every check comes before the first HIP call, so no device is
touched: a bad descriptor is a refusal with a message, never a launch.  Also: the binding, the header and the export table
name the same functions, and the binding's constants and structures are the header's.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from levelsetpy_amd import _dffi, _ffi, _qffi  # noqa: E402
from levelsetpy_amd import decomp as _front  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
D = _dffi


def grid(N=(8, 6), dtype="float64"):
    nd = len(N)
    return _qffi.grid_descriptor(nd, list(N), [0.0] * nd, [0.1 * (n - 1) for n in N], [0.1] * nd, [0] * nd, [0] * nd, dtype)


def sub(N=(8, 6), axes=(0, 1), data=FAKE, nfields=1, stride=None, dtype="float64", ndim=None, dtype_=None):
    """One (grid, data, nfields, field_stride, axes) entry; ndim / dtype_ overwrite the descriptor's fields with values that
    grid_descriptor() itself would not produce."""
    g = grid(N, dtype)
    if ndim is not None:
        g.ndim = ndim
    if dtype_ is not None:
        g.dtype = dtype_
    total = 1
    for n in N:
        total *= n
    return (g, data, nfields, total if stride is None else stride, axes)


def call(entry="nodes", subs=None, ndim=2, op=D.OP_MAX, N=(8, 6), nfields=1, out=None, out_dtype=0, coord="fake", xs=FAKE,
         nstates=5, null=False, nsubs=None, null_N=False):
    lib = D.lib()
    desc = D.decomp(ndim, op, subs if subs is not None else [sub()])
    if nsubs is not None:
        desc.nsubs = nsubs
    ref = None if null else C.byref(desc)
    before = lib.hjd_last_kernel()
    ext = None if null_N else D.extents(N)
    if entry == "nodes":
        rc = lib.hjd_backproject_nodes(ref, ext, nfields, out, out_dtype, None, None)
    elif entry == "coords":
        tabs = None if coord is None else D.tables([FAKE] * max(1, ndim) if coord == "fake" else coord)
        rc = lib.hjd_backproject_coords(ref, ext, tabs, nfields, out, out_dtype, None, None)
    else:
        rc = lib.hjd_points(ref, xs, nstates, nfields, out, out_dtype, None, None)
    assert lib.hjd_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjd_last_error().decode()


REFUSALS = [
    ("null-descriptor", dict(null=True), EINVAL, "null decomposition"),
    ("ndim0", dict(ndim=0), EINVAL, "ndim 0"),
    ("ndim9", dict(ndim=9), EINVAL, "ndim 9"),
    ("nsubs0", dict(nsubs=0), EINVAL, "nsubs 0"),
    ("nsubs9", dict(nsubs=9), EINVAL, "nsubs 9"),
    ("op2", dict(op=2), EINVAL, "op 2"),
    ("op-negative", dict(op=-1), EINVAL, "op -1"),
    ("nfields0", dict(nfields=0), EINVAL, "nfields = 0"),
    ("sub-ndim0", dict(subs=[sub(ndim=0)]), EINVAL, "subsystem 0: ndim 0"),
    ("sub-ndim5", dict(subs=[sub(), sub(ndim=5)]), EINVAL, "subsystem 1: ndim 5"),
    ("sub-dtype7", dict(subs=[sub(dtype_=7)]), EINVAL, "subsystem 0: unknown dtype 7"),
    ("sub-N0", dict(subs=[sub(N=(0, 6))], N=(0, 6)), EINVAL, "subsystem 0: N[0] = 0"),
    ("axis-outside", dict(subs=[sub(axes=(0, 2))]), EINVAL, "axis[1] = 2 is outside the 2 axes"),
    ("axis-negative", dict(subs=[sub(axes=(-1, 1))]), EINVAL, "axis[0] = -1 is outside"),
    ("axis-repeated", dict(subs=[sub(), sub(axes=(1, 1))]), EINVAL, "subsystem 1: axis[1] = 1 repeats"),
    ("sub-nfields", dict(subs=[sub(nfields=2)], nfields=3), EINVAL, "nfields 2: 1 or the 3"),
    ("sub-field-stride", dict(subs=[sub(nfields=3, stride=47)], nfields=3), EINVAL, "field_stride 47"),
    ("null-data", dict(subs=[sub(), sub(data=None)]), EINVAL, "subsystem 1: null data"),
    ("out-dtype7", dict(out_dtype=7), EUNSUPPORTED, "out_dtype 7"),
    ("coords-out-dtype7", dict(entry="coords", out_dtype=7), EUNSUPPORTED, "out_dtype 7"),
    ("null-N", dict(null_N=True), EINVAL, "null N"),
    ("N-negative", dict(N=(8, -6)), EINVAL, "N[1] = -6"),
    ("coords-N-negative", dict(entry="coords", N=(-8, 6)), EINVAL, "N[0] = -8"),
    ("not-conforming", dict(N=(8, 7)), EINVAL, "subsystem 0: axis 1 has 6 nodes, full axis 1 has 7"),
    ("not-conforming-permuted", dict(subs=[sub(axes=(1, 0))], N=(8, 6)), EINVAL, "subsystem 0: axis 0 has 8 nodes, full axis 1 has 6"),
    ("null-coord-tables", dict(entry="coords", coord=None), EINVAL, "null coordinate tables"),
    ("null-coord-axis1", dict(entry="coords", coord=[FAKE, None]), EINVAL, "coordinate table of axis 1"),
    ("null-out-nodes", dict(), EINVAL, "null output"),
    ("null-out-coords", dict(entry="coords", N=(3, 1)), EINVAL, "null output"),
    ("null-out-points", dict(entry="points"), EINVAL, "null output"),
    ("points-nstates-negative", dict(entry="points", nstates=-1), EINVAL, "nstates = -1"),
    ("points-null-states", dict(entry="points", xs=None), EINVAL, "null states"),
    ("points-sub-ndim5", dict(entry="points", subs=[sub(ndim=5)]), EINVAL, "subsystem 0: ndim 5"),
    ("points-op", dict(entry="points", op=7), EINVAL, "op 7"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, kw, code, word = case
    rc, err = call(**kw)
    assert rc == code and word in err, (rc, err)


def test_valid_descriptors_pass_the_checks_and_stop_at_the_null_output():
    """Everything the library validates is in order: the refusal is the null output, the last check before a launch."""
    eight = [sub(N=(3,), axes=(a,), dtype="float32" if a % 2 else "float64") for a in range(8)]
    shared = [sub(N=(8, 5), axes=(0, 2)), sub(N=(6, 5), axes=(1, 2), nfields=3, stride=30)]
    permuted = [sub(N=(5, 8), axes=(2, 0)), sub(N=(6,), axes=(1,))]
    for entry in ("nodes", "coords", "points"):
        for kw in (dict(subs=eight, ndim=8, N=(3,) * 8), dict(subs=shared, ndim=3, N=(8, 6, 5), nfields=3, op=D.OP_MIN),
                   dict(subs=permuted, ndim=3, N=(8, 6, 5)), dict(subs=[sub(N=(6,), axes=(1,))], ndim=2, N=(9, 6))):
            rc, err = call(entry, **kw)
            assert rc == EINVAL and err == "null output", (entry, err)
    rc, err = call("coords", subs=shared, ndim=3, N=(7, 7, 1), nfields=3)          # no conformity is asked of the general case
    assert rc == EINVAL and err == "null output", err


def test_an_empty_output_launches_nothing():
    assert call("nodes", subs=[sub(N=(6,), axes=(1,))], N=(0, 6))[0] == OK
    assert call("coords", N=(8, 0))[0] == OK
    assert call("points", nstates=0, xs=None)[0] == OK


def test_check_maps_the_codes():
    rc, err = call(ndim=9)
    with pytest.raises(ValueError) as info:
        D.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    rc, err = call(out_dtype=7)
    with pytest.raises(_ffi.Unsupported):
        D.check(rc)
    D.check(0)


def test_a_refusal_leaves_the_other_libraries_records_alone():
    from levelsetpy_amd import _tffi
    _tffi.lib().hjt_ttr_init(7, None, 1, 0.0, 0.0, None, None, None)
    before = _tffi.lib().hjt_last_error()
    assert b"dtype" in before
    rc, err = call(nsubs=0)
    assert rc == EINVAL and "nsubs" in err and _tffi.lib().hjt_last_error() == before


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_decomp.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjd_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(D.SIGNATURES) == ["hjd_backproject_coords", "hjd_backproject_nodes", "hjd_last_error", "hjd_last_kernel", "hjd_points"]
    out = subprocess.check_output(["nm", "-D", D.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hjd_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-ce-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    lib = D.lib()
    for name, (_, args) in D.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJD_MAX_DIM", D.MAX_DIM), ("HJD_MAX_SUBS", D.MAX_SUBS)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert (D.MAX_DIM, D.MAX_SUBS) == (8, 8) and _qffi.MAX_DIM == 4            # HJ_MAX_DIM stays 4
    assert (D.OP_MIN, D.OP_MAX) == (_qffi.OP_MIN, _qffi.OP_MAX) == (0, 1)
    assert C.sizeof(_qffi.Grid) == 8 + 4 * (8 + 8 + 8 + 8 + 4 + 4)
    assert C.sizeof(D.Sub) == C.sizeof(_qffi.Grid) + 8 + 8 + 8 + 4 * 4 == 208
    assert C.sizeof(D.Decomp) == 16 + 8 * 208 and C.sizeof(D.Decomp) < 4096
    fields = re.search(r"typedef struct hjd_sub \{(.*?)\} hjd_sub;", code, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\w+\])?;", fields) == [n for n, _ in D.Sub._fields_]
    fields = re.search(r"typedef struct hjd_decomp \{(.*?)\} hjd_decomp;", code, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\w+\])?;", fields) == [n for n, _ in D.Decomp._fields_]


def test_the_makefile_builds_and_cleans_the_library():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\blibhj_decomp\.so\b", mk, re.M) and re.search(r"^\trm -f .*\blibhj_decomp\.so\b", mk, re.M)
    assert re.search(r"^libhj_decomp\.so: hj_decomp\.hip hj_tool_host\.h hj_query_dev\.h", mk, re.M) and "hj_decomp.hip" in mk.split("HIPCC ?=")[0]
    assert re.search(r"^resource-usage-decomp:", mk, re.M)
    assert len(re.search(r"^all:(.*)$", mk, re.M).group(1).split()) == 8
