"""CPU-only: libhj_resample.so (include/hj_resample.h) through ctypes, and the front end's refusals, in the manner of
tests/test_hishapes_host.py.

  * every refusal of hjm_resample by message: each comes before the first HIP call, so no device is touched and the last-kernel
    record stays as it was;
  * hjm_plan of the named grids and of the output arrays past gridDim.y = 65535; what hjm_plan and hjm_decode refuse (that the
    launches cover every node once and that the decode is np.unravel_index: tests/test_node_index_host.py);
  * the binding, the header and the export table name the same functions; the Makefile builds the library beside the old lines;
  * what levelsetpy_amd.resample refuses, it refuses before it asks for a device.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_ref as R
import levelsetpy_amd as L
from levelsetpy_amd import _ffi, _hffi, _mffi as M, resample as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
NAN = float("nan")


def src_grid(ndim=3, n=8, dtype="float64", N=None, bc=None):
    N = [n] * ndim if N is None else list(N)
    g = _hffi.grid_descriptor(ndim, N + [1] * (ndim - len(N)), [0.0] * ndim, [0.1 * (v - 1) for v in N] + [0.0] * (ndim - len(N)), [0.1] * ndim,
                              [0] * ndim if bc is None else bc, [0] * ndim, dtype)
    return g


def dst_grid(N=(5, 6, 7), dtype="float64"):
    return M.extents_descriptor(list(N), dtype)


def call(src="default", dst="default", coord="default", data=FAKE, nfields=1, stride=0, maps=None, K=1, reduce=0, fill_mode=0,
         fill_value=0.0, out=FAKE, out_dtype=0, counts=FAKE, work=FAKE):
    lib = M.lib()
    src = src_grid() if src == "default" else src
    dst = dst_grid() if dst == "default" else dst
    table = M.coord_table([FAKE] * 6) if coord == "default" else coord
    before = lib.hjm_last_kernel()
    rc = lib.hjm_resample(C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None,
                          C.byref(table) if table is not None else None, data, nfields, stride, maps, K, reduce, fill_mode, fill_value,
                          out, out_dtype, counts, work, None)
    assert lib.hjm_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjm_last_error().decode()


def bad_dtype(g):
    g.dtype = 7
    return g


def with_ndim(g, ndim):
    g.ndim = ndim
    return g


REFUSALS = [
    ("null-src", dict(src=None), EINVAL, "null grid descriptor"),
    ("null-dst", dict(dst=None), EINVAL, "null grid descriptor"),
    ("ndim0", dict(src=with_ndim(src_grid(), 0)), EINVAL, "ndim 0"),
    ("ndim7", dict(src=with_ndim(src_grid(6), 7)), EINVAL, "ndim 7"),
    ("dst-ndim7", dict(src=src_grid(6), dst=with_ndim(dst_grid([4] * 6), 7)), EINVAL, "ndim 7"),
    ("ndim-differs", dict(dst=dst_grid((5, 6))), EINVAL, "source grid has 3 dimensions, the destination 2"),
    ("src-dtype7", dict(src=bad_dtype(src_grid())), EINVAL, "dtype 7"),
    ("dst-dtype7", dict(dst=bad_dtype(dst_grid())), EINVAL, "dtype 7"),
    ("out-dtype7", dict(out_dtype=7), EUNSUPPORTED, "out_dtype 7"),
    ("K0", dict(K=0), EINVAL, "K = 0"),
    ("K-negative", dict(K=-2), EINVAL, "K = -2"),
    ("nfields0", dict(nfields=0), EINVAL, "nfields = 0"),
    ("nfields-2^31", dict(nfields=2 ** 31, stride=512), EINVAL, "nfields = 2147483648"),
    ("stride-small", dict(nfields=2, stride=511), EINVAL, "field_stride 511 is smaller than the source grid (512)"),
    ("null-maps-K2", dict(K=2), EINVAL, "null maps with K = 2"),
    ("reduce3", dict(reduce=3), EINVAL, "unknown reduce 3"),
    ("reduce-negative", dict(reduce=-1), EINVAL, "unknown reduce -1"),
    ("fill-mode3", dict(fill_mode=3), EINVAL, "unknown fill_mode 3"),
    ("fill-value-nan", dict(fill_mode=M.FILL_VALUE, fill_value=NAN), EINVAL, "fill_value is NaN"),
    ("dst-axis-2^31", dict(dst=dst_grid((2, 2 ** 31, 2))), EINVAL, "N[1] = 2147483648"),
    ("src-axis-2^31", dict(src=src_grid(3, N=[2, 2 ** 31, 2])), EINVAL, "N[1] = 2147483648"),
    ("dst-axis-0", dict(dst=dst_grid((5, 0, 7))), EINVAL, "N[1] = 0"),
    ("dst-2^63", dict(src=src_grid(3), dst=dst_grid((2 ** 31 - 1,) * 3)), EINVAL, "2^63"),
    ("src-axis-of-one-node", dict(src=src_grid(3, N=[8, 1, 8])), EINVAL, "too small along dim 1"),
    ("src-bc9", dict(src=src_grid(3, bc=[0, 9, 0])), EINVAL, "boundary kind 9"),
    ("arrays-overflow", dict(maps=FAKE, K=2 ** 62, dst=dst_grid((2 ** 20, 2 ** 20, 4))), EINVAL, "exceeds 2^63"),
    ("null-coord", dict(coord=None), EINVAL, "null argument"),
    ("null-coord-axis2", dict(coord=M.coord_table([FAKE, FAKE, 0])), EINVAL, "coordinate table of axis 2"),
    ("null-data", dict(data=None), EINVAL, "null argument"),
    ("null-out", dict(out=None), EINVAL, "null argument"),
    ("null-counts", dict(counts=None), EINVAL, "null argument"),
    ("null-workspace", dict(work=None), EINVAL, "null argument"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, kw, code, word = case
    rc, err = call(**kw)
    assert rc == code and word in err, (rc, err)


def test_every_dimension_passes_the_checks_and_stops_at_the_null_output():
    """Everything the library validates is in order, in 1-D to 6-D, with maps, fields and each reduce / fill: the refusal is the
    null output, the last check before a launch.  A periodic axis may have one node."""
    for nd in range(1, 7):
        for reduce, mode in ((0, 0), (1, 1), (2, 2)):
            rc, err = call(src=src_grid(nd, n=3, bc=[1] + [0] * (nd - 1), N=[1] + [3] * (nd - 1)), dst=dst_grid([4] * nd),
                           coord=M.coord_table([FAKE] * nd), nfields=3, stride=3 ** (nd - 1), maps=FAKE, K=70000, reduce=reduce,
                           fill_mode=mode, fill_value=1.5, out=None)
            assert rc == EINVAL and err == "null argument", (nd, err)


def test_check_maps_the_codes():
    rc, err = call(K=0)
    with pytest.raises(ValueError) as info:
        M.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    with pytest.raises(_ffi.Unsupported):
        M.check(call(out_dtype=7)[0])
    M.check(0)
    assert M.lib().hjm_workspace_size(5) == 5 * (1 + M.COUNT_SLOTS) * 8 and M.lib().hjm_workspace_size(0) == 0


def test_a_refusal_leaves_another_librarys_record_alone():
    from levelsetpy_amd import _kffi
    assert _kffi.lib().hjk_plan(None, 1, None) == EINVAL
    before = _kffi.lib().hjk_last_error()
    rc, err = call(reduce=9)
    assert rc == EINVAL and "reduce 9" in err and _kffi.lib().hjk_last_error() == before


# ------------------------------------------------------------------------------------------ the plan (its walk: tests/test_node_index_host.py)
def test_plan_of_the_named_grids_and_of_the_output_arrays():
    p = M.plan((25,) * 6)
    assert (p.first_tail, p.head, p.tail, p.launches) == (0, 1, 25 ** 6, 1)
    p = M.plan((41,) * 6)
    # a launch has fewer than 2^32 threads, 2^24 - 1 workgroups: a grid past 2^32 nodes takes more than one
    assert 41 ** 6 > 2 ** 32 and (p.first_tail, p.head, p.tail, p.heads_per_launch, p.launches) == (1, 41, 41 ** 5, 37, 2)
    p = M.plan((46341, 46341, 2 ** 31 - 1))
    assert p.head == 46341 ** 2 > 2 ** 31 and p.heads_per_launch == 1 and p.launches == 46341 ** 2
    # output arrays: K x nfields without a fold, nfields with one; gridDim.y ends at 65535
    for K, F, reduce, arrays, launches in ((1, 1, 0, 1, 1), (65535, 1, 0, 65535, 1), (65537, 1, 0, 65537, 2), (300, 3, 0, 900, 1),
                                           (65537, 3, 0, 196611, 4), (65537, 3, 1, 3, 1), (2, 70000, 2, 70000, 2)):
        p = M.plan((3, 3), F, K, reduce)
        assert (p.arrays, p.array_launches) == (arrays, launches), (K, F, reduce)


def test_plan_and_decode_refuse_what_the_grid_check_refuses():
    lib, plan, idx = M.lib(), M.LaunchPlan(), (C.c_int32 * 6)()
    for N, word in (((2 ** 31 + 5, 2), "N[0] = 2147483653"), ((2, 2 ** 31), "N[1]"), ((2 ** 31 - 1,) * 3, "2^63"), ((4, 0), "N[1] = 0")):
        g = dst_grid(N)
        assert lib.hjm_plan(C.byref(g), 1, 1, 0, C.byref(plan)) == EINVAL and word in lib.hjm_last_error().decode()
        assert lib.hjm_decode(C.byref(g), 0, C.byref(idx)) == EINVAL and word in lib.hjm_last_error().decode()
    g = dst_grid((3, 4, 5))
    assert lib.hjm_plan(C.byref(g), 1, 0, 0, C.byref(plan)) == EINVAL and "K = 0" in lib.hjm_last_error().decode()
    assert lib.hjm_plan(C.byref(g), 1, 1, 5, C.byref(plan)) == EINVAL and "reduce 5" in lib.hjm_last_error().decode()
    assert lib.hjm_plan(C.byref(g), 1, 1, 0, None) == EINVAL and "null argument" in lib.hjm_last_error().decode()
    assert lib.hjm_plan(None, 1, 1, 0, C.byref(plan)) == EINVAL and "null grid" in lib.hjm_last_error().decode()
    for node in (-1, 60):
        assert lib.hjm_decode(C.byref(g), node, C.byref(idx)) == EINVAL and "node" in lib.hjm_last_error().decode()
    assert lib.hjm_decode(C.byref(g), 0, None) == EINVAL and "null argument" in lib.hjm_last_error().decode()


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_resample.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjm_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(M.SIGNATURES) == ["hjm_decode", "hjm_last_error", "hjm_last_kernel", "hjm_plan", "hjm_resample", "hjm_workspace_size"]
    out = subprocess.check_output(["nm", "-D", M.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hjm_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-ln-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    stubs = sorted(set(n for n in re.findall(r"\b(_ZN3hjm\d+resample_\w*kernelI\w*)", out) if not n.endswith(".kd")))
    main = [n for n in stubs if "15resample_kernelI" in n]
    fill = [n for n in stubs if "20resample_fill_kernelI" in n]
    assert len(main) == 2 * 6 * 3 and len(fill) == 6 * 2 and len(stubs) == 48, stubs      # (fp64, fp32) x 1 .. 6 axes x reduce; axes x fold
    lib = M.lib()
    for name, (_, args) in M.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJM_MAX_DIM", M.MAX_DIM), ("HJM_REDUCE_NONE", M.REDUCE_NONE), ("HJM_REDUCE_MIN", M.REDUCE_MIN),
                      ("HJM_REDUCE_MAX", M.REDUCE_MAX), ("HJM_FILL_NAN", M.FILL_NAN), ("HJM_FILL_VALUE", M.FILL_VALUE), ("HJM_FILL_MAX", M.FILL_MAX),
                      ("HJM_COUNT_SLOTS", M.COUNT_SLOTS)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert C.sizeof(M.LaunchPlan) == 8 + 9 * 8 and _hffi.MAX_DIM == M.MAX_DIM
    assert M.kernel_names("float64", 3, 0, True) == "resample_kernel<double, 3, 0>;resample_counts_kernel;resample_fill_kernel<3, 0>"
    assert M.kernel_names("float32", 6, 2, True) == "resample_kernel<float, 6, 2>;resample_counts_kernel;resample_fill_kernel<6, 1>"
    assert M.kernel_names("float64", 2, 1, False) == "resample_kernel<double, 2, 1>;resample_counts_kernel"


def test_the_makefile_builds_the_library_beside_the_old_lines():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    all_lines = re.findall(r"^all:(.*)$", mk, re.M)
    assert len(re.findall(r"\blibhj_\w+\.so\b", " ".join(all_lines))) == 10 and "resample" not in " ".join(all_lines)
    libs = re.findall(r"^libs:(.*)$", mk, re.M)
    assert libs[0].split() == ["all", "libhj_hiquery.so", "libhj_plant.so"] and libs[1:] == [" libhj_hishapes.so"]
    assert re.findall(r"^libs\s*:(.*)$", mk, re.M)[2:] == [" libhj_resample.so"]            # a prerequisite of the default goal
    assert re.search(r"^libhj_resample\.so: hj_resample\.hip hj_tool_host\.h hj_query_dev\.h hj_shapes_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-resample:.*\n\t.*-Rpass-analysis=kernel-resource-usage .*hj_resample\.hip$", mk, re.M)
    assert re.search(r"^\trm -f .*\blibhj_resample\.so\b", mk, re.M)
    assert "hj_resample.hip" in mk.split("HIPCC ?=")[0] and "libhj_resample.so" in mk.split("\n")[0]
    assert re.search(r"^\.DEFAULT_GOAL := libs$", mk, re.M)
    out = subprocess.check_output(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "-n", "-B", "libs"]).decode()
    assert "-o libhj_resample.so hj_resample.hip" in out


def test_the_interpolant_and_the_fold_are_not_restated():
    """The kernels call hj_query_dev.h's locate / interp_value and hj_shapes_dev.h's nmin / nmax; no existing source names the library."""
    src = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_resample.hip")).read()
    assert '#include "hj_query_dev.h"' in src and '#include "hj_shapes_dev.h"' in src and "#define HJ_QUERY_MAXD 6" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "hjq::interp_value<T>(" in code and "hjq::locate(" in code and "fmod(" not in code and "floor(" not in code
    assert not re.search(r"double n(min|max)\(", src)


# ------------------------------------------------------------------------------------------ the front end, without a device
def grids():
    gO = L.createGrid(np.array([[-1.0, -1.0, -1.0]]).T, np.array([[1.0, 1.0, 1.0]]).T, np.array([[5, 6, 7]]).T)
    gN = L.createGrid(np.array([[-1.2, -1.2, -1.2]]).T, np.array([[1.2, 1.2, 1.2]]).T, np.array([[4, 4, 4]]).T, low_mem=True)
    return gO, gN, np.zeros((5, 6, 7))


def grid_of(dim):
    return L.Bundle(dict(dim=dim, N=np.full((dim, 1), 3), vs=[np.zeros(3)] * dim, dx=np.ones((dim, 1)), bdry=[L.addGhostExtrapolate] * dim))


FRONT = [
    ("data-shape", lambda gO, gN, d: L.transformData(gO, np.zeros((5, 6, 8)), gN), "does not agree in array size"),
    ("stack-shape", lambda gO, gN, d: L.transformData(gO, np.zeros((2, 5, 7, 6)), gN), "does not agree in array size"),
    ("dims-differ", lambda gO, gN, d: L.transformData(gO, d, grid_of(2)), "gOld.dim = 3 and gNew.dim = 2"),
    ("dim7", lambda gO, gN, d: L.transformData(grid_of(7), np.zeros((3,) * 7)), "grid.dim must be 1..6"),
    ("A-shape", lambda gO, gN, d: L.transformData(gO, d, gN, A=np.eye(2)), "A must be (3, 3) or (K, 3, 3)"),
    ("b-shape", lambda gO, gN, d: L.transformData(gO, d, gN, b=np.zeros(4)), "b must be (3,) or (K, 3)"),
    ("K-disagrees", lambda gO, gN, d: L.transformData(gO, d, gN, A=np.zeros((2, 3, 3)), b=np.zeros((3, 3))), "disagree on K"),
    ("A-nan", lambda gO, gN, d: L.transformData(gO, d, gN, A=np.full((3, 3), np.nan)), "A and b must be finite"),
    ("b-inf", lambda gO, gN, d: L.transformData(gO, d, gN, b=np.array([0.0, np.inf, 0.0])), "A and b must be finite"),
    ("fill-word", lambda gO, gN, d: L.transformData(gO, d, gN, fill='min'), "fill must be"),
    ("fill-none", lambda gO, gN, d: L.migrateGrid(gO, d, gN, fill=None), "fill must be"),
    ("reduce-word", lambda gO, gN, d: L.transformData(gO, d, gN, reduce='sum'), "reduce must be"),
    ("dtype-word", lambda gO, gN, d: L.transformData(gO, d, gN, dtype='float16'), "dtype must be"),
    ("pdims-same", lambda gO, gN, d: L.rotateData(gO, d, 0.3, (1, 1)), "pdims must name two distinct axes"),
    ("pdims-three", lambda gO, gN, d: L.rotateData(gO, d, 0.3, (0, 1, 2)), "pdims must name two distinct axes"),
    ("pdims-outside", lambda gO, gN, d: L.rotateData(gO, d, 0.3, (0, 3)), "pdims must name two distinct axes"),
    ("adim-in-pdims", lambda gO, gN, d: L.rotateData(gO, d, 0.3, (0, 1), adim=1), "adim must be an axis"),
    ("theta-matrix", lambda gO, gN, d: L.rotateData(gO, d, np.zeros((2, 2)), (0, 1)), "theta must be a scalar or (K,)"),
    ("shift-width", lambda gO, gN, d: L.shiftData(gO, d, [0.1, 0.2, 0.3], (0, 1)), "shift must be (2,) or (K, 2)"),
    ("shift-pdims", lambda gO, gN, d: L.shiftData(gO, d, [0.1, 0.2], (0, 0)), "pdims must name its distinct axes"),
]


@pytest.mark.parametrize("case", FRONT, ids=[c[0] for c in FRONT])
def test_the_front_end_refuses_before_it_asks_for_a_device(case, monkeypatch):
    def no_device():
        raise AssertionError("require_gpu() was reached")
    monkeypatch.setattr(RS, "require_gpu", no_device)
    with pytest.raises(ValueError) as info:
        case[1](*grids())
    assert case[2] in str(info.value), str(info.value)


def test_the_maps_of_the_front_end_are_the_restatements():
    gO, gN, d = grids()
    A, b = RS.rotateMap(gO, 0.4, (0, 1), 2)
    A2, b2 = R.rotation_map(3, 0.4, 0, 1, 2)
    assert np.array_equal(A, A2) and np.array_equal(b, b2)
    A, b = RS.rotateMap(gO, [0.4, -1.0], (2, 0))
    assert A.shape == (2, 3, 3) and b.shape == (2, 3) and A[1, 2, 0] == -np.sin(1.0) and A[1, 0, 2] == np.sin(1.0) and not b.any()
    A, b = RS.shiftMap(gO, [[0.1, 0.2], [0.3, 0.4]], (2, 0))
    assert np.array_equal(A, np.eye(3)) and np.array_equal(b, [[-0.2, 0.0, -0.1], [-0.4, 0.0, -0.3]])
    table, K, batched = RS._maps(3, None, b)
    assert (K, batched) == (2, True) and np.array_equal(table[:, :9], np.tile(np.eye(3).ravel(), (2, 1))) and np.array_equal(table[:, 9:], b)
    assert RS._maps(3, None, None) == (None, 1, False)
    assert RS._fill('max') == (M.FILL_MAX, 0.0) and RS._fill(2) == (M.FILL_VALUE, 2.0) and RS._fill(NAN)[0] == M.FILL_NAN == RS._fill('nan')[0]
    for name in ("transformData", "migrateGrid", "shiftData", "rotateData"):
        assert getattr(L, name) is getattr(RS, name)
