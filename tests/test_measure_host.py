"""CPU-only: libhj_measure.so (include/hj_measure.h) through ctypes, and the front end's host side, in the manner of
tests/test_resample_host.py.

  * hjv_simplex_q_host, the DEVICE per-simplex function run on the host, equals tests/measure_ref.py on 10^4 random simplices per
    dimension, with ties, exact zeros, denormal-scale and 1e300-scale values;
  * every refusal of hjv_measure by code and text: each comes before the first HIP call, so no device is touched and the last-kernel
    record stays as it was;
  * hjv_plan of the named grids and of the fields past gridDim.y = 65535; what hjv_plan and hjv_decode refuse (that the launches
    cover every node once, the slots and that the decode is np.unravel_index: tests/test_node_index_host.py);
  * the binding, the header and the export table name the same functions; the Makefile builds the library beside the old lines;
  * truncateGrid against the restatement, on 1 to 6 axes, and against tests/golden/truncate.npz (the reference's own, 2-D to 4-D);
    setBounds' host arithmetic on records made by the restatement; what the front end refuses, it refuses before it asks for a device.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import measure_ref as R
import levelsetpy_amd as L
from levelsetpy_amd import _ffi, _vffi as V, measure as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read


# ------------------------------------------------------------------------------------------ the per-simplex function
@pytest.mark.parametrize("D", range(1, 7))
def test_the_host_run_of_the_device_function_equals_the_restatement(D):
    rng = np.random.default_rng(40 + D)
    seen = {"cut": 0, "ties": 0, "zeros": 0, "tiny": 0, "huge": 0, "full": 0, "empty": 0}
    for it in range(10000):
        f = rng.standard_normal(D + 1)
        kind = it % 10
        if kind == 1:
            f[rng.integers(0, D + 1)] = 0.0
            seen["zeros"] += 1
        elif kind == 2:
            f[rng.integers(0, D + 1)] = f[rng.integers(0, D + 1)]
            f[rng.integers(0, D + 1)] = -f[0]
            seen["ties"] += 1
        elif kind == 3:
            f *= 4e-310                                           # denormal values and differences
            seen["tiny"] += 1
        elif kind == 4:
            f *= 1e300
            seen["huge"] += 1
        elif kind == 5:
            f[:] = np.abs(f) * (1.0 if it % 20 == 5 else -1.0)
            f[rng.integers(0, D + 1)] *= float(it % 3 > 0)         # one sign, sometimes with a zero
        elif kind == 6:
            f = np.round(f * 2) / 2                               # halves: ties, zeros and exact thetas together
        want = R.simplex_q(f)
        assert V.simplex_q(f) == want, (D, list(f), V.simplex_q(f), want)
        seen["cut"] += 0 < want < R.Q_ONE
        seen["full"] += want == R.Q_ONE
        seen["empty"] += want == 0
    assert seen["cut"] > 3000 and seen["full"] > 200 and seen["empty"] > 200, seen


def test_simplex_q_host_refusals():
    lib, q = V.lib(), C.c_uint64()
    f = (C.c_double * 7)(*[1.0] * 7)
    for D in (0, 7, -1):
        assert lib.hjv_simplex_q_host(D, f, C.byref(q)) == EINVAL and ("D = %d" % D) in lib.hjv_last_error().decode()
    assert lib.hjv_simplex_q_host(3, None, C.byref(q)) == EINVAL and lib.hjv_simplex_q_host(3, f, None) == EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        f[2] = bad
        assert lib.hjv_simplex_q_host(3, f, C.byref(q)) == EINVAL and "f[2] is not finite" in lib.hjv_last_error().decode()
        assert lib.hjv_simplex_q_host(1, f, C.byref(q)) == OK         # f[2] is not read


# ------------------------------------------------------------------------------------------ refusals
def grid(N=(5, 6, 7), periodic=(), dtype="float64"):
    return V.extents_descriptor(list(N), periodic, dtype)


def call(g="default", a=FAKE, nfields=1, stride_a=0, b=None, b_dtype=0, nfields_b=1, stride_b=0, level=0.0, records=FAKE, work=FAKE):
    lib = V.lib()
    g = grid() if g == "default" else g
    before = lib.hjv_last_kernel()
    rc = lib.hjv_measure(C.byref(g) if g is not None else None, a, nfields, stride_a, b, b_dtype, nfields_b, stride_b, level, records, work, None)
    assert lib.hjv_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjv_last_error().decode()


def changed(g, **kw):
    for k, v in kw.items():
        if k == "bc":
            g.bc[v[0]] = v[1]
        else:
            setattr(g, k, v)
    return g


REFUSALS = [
    ("null-grid", dict(g=None), EINVAL, "null grid descriptor"),
    ("ndim0", dict(g=changed(grid(), ndim=0)), EINVAL, "ndim 0"),
    ("ndim7", dict(g=changed(grid((3,) * 6), ndim=7)), EINVAL, "ndim 7"),
    ("dtype7", dict(g=changed(grid(), dtype=7)), EINVAL, "dtype 7"),
    ("axis-of-one-node", dict(g=grid((5, 1, 7))), EINVAL, "N[1] = 1: an axis has at least two nodes"),
    ("axis-of-no-node", dict(g=grid((5, 6, 0))), EINVAL, "N[2] = 0"),
    ("axis-2^31", dict(g=grid((2, 2 ** 31, 2))), EINVAL, "N[1] = 2147483648"),
    ("grid-2^63", dict(g=grid((2 ** 31 - 1,) * 3)), EINVAL, "2^63"),
    ("bc9", dict(g=changed(grid(), bc=(1, 9))), EINVAL, "unknown boundary kind 9 along dim 1"),
    ("nfields0", dict(nfields=0), EINVAL, "nfields = 0"),
    ("nfields-2^31", dict(nfields=2 ** 31, stride_a=210), EINVAL, "nfields = 2147483648"),
    ("level-nan", dict(level=float("nan")), EINVAL, "level is not finite"),
    ("level-inf", dict(level=float("inf")), EINVAL, "level is not finite"),
    ("stride-a-small", dict(nfields=2, stride_a=209), EINVAL, "stride_a 209 is smaller than the grid (210)"),
    ("b-dtype7", dict(b=FAKE, b_dtype=7), EUNSUPPORTED, "b_dtype 7"),
    ("nfields-b", dict(nfields=3, stride_a=210, b=FAKE, nfields_b=2, stride_b=210), EINVAL, "nfields_b = 2: one field, or as many as a (3)"),
    ("stride-b-small", dict(nfields=3, stride_a=210, b=FAKE, nfields_b=3, stride_b=100), EINVAL, "stride_b 100 is smaller than the grid (210)"),
    ("null-a", dict(a=None), EINVAL, "null argument"),
    ("null-records", dict(records=None), EINVAL, "null argument"),
    ("null-workspace", dict(work=None), EINVAL, "null argument"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    _, kw, code, word = case
    rc, err = call(**kw)
    assert rc == code and word in err, (rc, err)


def test_every_dimension_passes_the_checks_and_stops_at_the_null_records():
    for nd in range(1, 7):
        for b in (None, FAKE):
            rc, err = call(g=grid((2,) + (3,) * (nd - 1), periodic=(0,), dtype="float32"), nfields=70000, stride_a=2 * 3 ** (nd - 1), b=b,
                           b_dtype=1, nfields_b=1, level=-2.5, records=None)
            assert rc == EINVAL and err == "null argument", (nd, err)


def test_check_maps_the_codes_and_the_workspace_follows_the_plan():
    rc, err = call(nfields=0)
    with pytest.raises(ValueError) as info:
        V.check(rc)
    assert str(info.value) == "%s (code %d)" % (err, EINVAL) and not isinstance(info.value, _ffi.Unsupported)
    with pytest.raises(_ffi.Unsupported):
        V.check(call(b=FAKE, b_dtype=7)[0])
    lib = V.lib()
    for N, slots in (((3, 2), 1), ((2,) * 6, 1), ((19, 17), 2), ((37, 37), 8), ((25,) * 6, 32), ((41,) * 6, 32)):
        assert V.plan(N).slots == slots, N
        for nf, cmp_ in ((1, 0), (5, 1)):
            g = grid(N)
            assert lib.hjv_workspace_size(C.byref(g), nf, cmp_) == nf * (4 if cmp_ else 1) * slots * V.RECORD_WORDS * 8
    g = grid((5, 1))
    assert lib.hjv_workspace_size(C.byref(g), 1, 0) == 0 and lib.hjv_workspace_size(None, 1, 0) == 0
    g = grid((5, 4))
    assert lib.hjv_workspace_size(C.byref(g), 0, 0) == 0


def test_a_refusal_leaves_another_librarys_record_alone():
    from levelsetpy_amd import _mffi
    assert _mffi.lib().hjm_plan(None, 1, 1, 0, None) == EINVAL
    before = _mffi.lib().hjm_last_error()
    rc, err = call(level=float("nan"))
    assert rc == EINVAL and "level" in err and _mffi.lib().hjm_last_error() == before


# ------------------------------------------------------------------------------------------ the plan and the decode (their walk: tests/test_node_index_host.py)
def test_plan_of_the_named_grids_and_of_the_fields():
    p = V.plan((25,) * 6)
    assert (p.first_tail, p.head, p.tail, p.launches) == (0, 1, 25 ** 6, 1)
    p = V.plan((41,) * 6)
    # a launch has fewer than 2^32 threads, 2^24 - 1 workgroups: a grid past 2^32 nodes takes more than one
    assert 41 ** 6 > 2 ** 32 and (p.first_tail, p.head, p.tail, p.heads_per_launch, p.launches) == (1, 41, 41 ** 5, 37, 2)
    p = V.plan((46341, 46341, 2 ** 31 - 1))
    assert p.head == 46341 ** 2 > 2 ** 31 and p.heads_per_launch == 1 and p.launches == 46341 ** 2
    for F, launches in ((1, 1), (65535, 1), (65536, 2), (131071, 3)):
        p = V.plan((3, 2), F)
        assert (p.nfields, p.field_launches) == (F, launches)


def test_plan_and_decode_refuse_what_the_grid_check_refuses():
    lib, plan, idx = V.lib(), V.LaunchPlan(), (C.c_int32 * 6)()
    for N, word in (((2 ** 31 + 5, 2), "N[0] = 2147483653"), ((2, 2 ** 31), "N[1]"), ((2 ** 31 - 1,) * 3, "2^63"), ((4, 1), "N[1] = 1")):
        g = grid(N)
        assert lib.hjv_plan(C.byref(g), 1, C.byref(plan)) == EINVAL and word in lib.hjv_last_error().decode()
        assert lib.hjv_decode(C.byref(g), 0, C.byref(idx)) == EINVAL and word in lib.hjv_last_error().decode()
    g = grid((3, 4, 5))
    assert lib.hjv_plan(C.byref(g), 0, C.byref(plan)) == EINVAL and "nfields = 0" in lib.hjv_last_error().decode()
    assert lib.hjv_plan(C.byref(g), 1, None) == EINVAL and "null argument" in lib.hjv_last_error().decode()
    assert lib.hjv_plan(None, 1, C.byref(plan)) == EINVAL and "null grid" in lib.hjv_last_error().decode()
    for node in (-1, 60):
        assert lib.hjv_decode(C.byref(g), node, C.byref(idx)) == EINVAL and "node" in lib.hjv_last_error().decode()
    assert lib.hjv_decode(C.byref(g), 0, None) == EINVAL and "null argument" in lib.hjv_last_error().decode()


# ------------------------------------------------------------------------------------------ header, binding, export table
def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_measure.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjv_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(V.SIGNATURES) == ["hjv_decode", "hjv_last_error", "hjv_last_kernel", "hjv_measure", "hjv_plan",
                                                "hjv_simplex_q_host", "hjv_workspace_size"]
    out = subprocess.check_output(["nm", "-D", V.LIB_PATH]).decode()
    exported = sorted(set(re.findall(r" T (hjv_[a-z0-9_]+)", out)))
    assert exported == declared, (exported, declared)
    assert not re.findall(r" T (hj[a-uw-z]?_[a-z0-9_]+)", out)            # one translation unit: nothing of another library
    stubs = sorted(set(n for n in re.findall(r"\b(_ZN3hjv\d+measure_\w*kernel\w*)", out) if not n.endswith(".kd")))
    main = [n for n in stubs if "14measure_kernelI" in n]
    assert len(main) == 2 * 6 + 4 * 6 and len(stubs) == 37, stubs         # (fp64, fp32) x 1 .. 6 axes; four type pairs x axes; the fold
    lib = V.lib()
    for name, (_, args) in V.SIGNATURES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        count = 0 if decl in ("", "void") else decl.count(",") + 1
        assert count == len(args), (name, count, len(args))


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJV_MAX_DIM", V.MAX_DIM), ("HJV_RECORD_WORDS", V.RECORD_WORDS), ("HJV_CELLS", V.CELLS), ("HJV_FULL", V.FULL),
                      ("HJV_CUT", V.CUT), ("HJV_INVALID", V.INVALID), ("HJV_QLO", V.QLO), ("HJV_QHI", V.QHI), ("HJV_INSIDE", V.INSIDE),
                      ("HJV_NAN", V.NAN), ("HJV_LO", V.LO), ("HJV_HI", V.HI), ("HJV_SET_A", V.SET_A), ("HJV_SET_B", V.SET_B),
                      ("HJV_SET_UNION", V.SET_UNION), ("HJV_SET_INTERSECTION", V.SET_INTERSECTION), ("HJV_MAX_SLOTS", V.MAX_SLOTS)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert C.sizeof(V.LaunchPlan) == 8 + 10 * 8 and V.Q_ONE == R.Q_ONE == 2 ** 52 and V.HI + V.MAX_DIM == V.RECORD_WORDS
    assert V.kernel_names("float64", None, 3) == "measure_kernel<double, double, 3, 0>;measure_fold_kernel"
    assert V.kernel_names("float32", "float64", 6) == "measure_kernel<float, double, 6, 1>;measure_fold_kernel"


def test_the_makefile_builds_the_library_beside_the_old_lines():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert "measure" not in " ".join(re.findall(r"^all:(.*)$", mk, re.M))
    assert re.search(r"^\$\(\.DEFAULT_GOAL\): libhj_measure\.so$", mk, re.M) and re.search(r"^\.DEFAULT_GOAL := libs$", mk, re.M)
    assert re.search(r"^libhj_measure\.so: hj_measure\.hip hj_measure_dev\.h hj_tool_host\.h hj_shapes_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-measure:.*\n\t.*-Rpass-analysis=kernel-resource-usage .*hj_measure\.hip$", mk, re.M)
    assert re.search(r"^\trm -f .*\blibhj_measure\.so\b", mk, re.M)
    assert "hj_measure.hip" in mk.split("HIPCC ?=")[0] and "libhj_measure.so" in mk.split("\n")[0]
    for goal in ([], ["libs"]):
        out = subprocess.check_output(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "-n", "-B"] + goal).decode()
        assert "-o libhj_measure.so hj_measure.hip" in out and "-o libhj_resample.so hj_resample.hip" in out


def test_the_rule_is_written_once_and_nothing_is_restated():
    """The kernel and the host entry point call hj_measure_dev.h's simplex_q; the minimum and maximum are hj_shapes_dev.h's; no float
    atomic exists."""
    src = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_measure.hip")).read()
    dev = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "hj_measure_dev.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert '#include "hj_measure_dev.h"' in src and '#include "hj_shapes_dev.h"' in src
    assert code.count("simplex_q<") == 2 and "__host__ __device__ __forceinline__ unsigned long long simplex_q(" in dev
    assert not re.search(r"double n(min|max)\(", src) and "theta" not in code
    assert not re.search(r"atomic\w*\([^;]*(double|float)", code) and "contract(off)" in dev


# ------------------------------------------------------------------------------------------ the front end, without a device
def pkg_grid(N, periodic=(), low_mem=False):
    vs, dx, mins, maxs = R.grid_vectors(N, periodic)
    col = lambda v, t=np.float64: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(mins), col(maxs), col(N, np.int64), list(periodic) if periodic else None, low_mem=low_mem)


def no_device():
    raise AssertionError("require_gpu() was reached")


@pytest.mark.parametrize("i", range(len(R.GRIDS)), ids=["x".join(map(str, N)) for N, _ in R.GRIDS])
def test_truncate_grid_is_the_restatement_on_one_to_six_axes(i, monkeypatch):
    monkeypatch.setattr(MS, "require_gpu", no_device)
    N, per = R.GRIDS[i]
    D = len(N)
    g = pkg_grid(N, per, low_mem=D >= 5)
    vs, dx, _, _ = R.grid_vectors(N, per)
    data = R.field(N, per)
    xmin = np.array([vs[d][0] + (0.6 * dx[d] if d % 2 == 0 else -1.0) for d in range(D)])
    xmax = np.array([vs[d][-1] - (0.4 * dx[d] if d % 3 != 1 and N[d] >= 3 else -1.0) for d in range(D)])
    keep, ref = R.truncate_ref(vs, data, xmin, xmax)
    before = list(g.bdry)
    gN, dN = L.truncateGrid(g, data, xmin.reshape(-1, 1), xmax.reshape(-1, 1))
    assert isinstance(dN, np.ndarray) and np.array_equal(dN, ref) and dN.shape == tuple(len(k) for k in keep)
    assert list(g.bdry) == before                                 # the old grid keeps its boundary conditions
    for d in range(D):
        assert np.array_equal(np.asarray(gN.vs[d]).ravel(), vs[d][keep[d]]) and int(gN.N[d, 0]) == len(keep[d])
        assert float(gN.min[d, 0]) == vs[d][keep[d][0]]
        assert float(gN.max[d, 0]) == vs[d][keep[d][-1]] + (1e-3 if len(keep[d]) == 1 else 0.0)
        assert (gN.bdry[d] is L.addGhostPeriodic) == (d in per and len(keep[d]) == N[d])
        if len(keep[d]) > 1:
            assert float(gN.dx[d, 0]) == pytest.approx(dx[d], rel=1e-15)
    assert tuple(gN.shape) == (tuple(dN.shape) + (1,) if D == 1 else tuple(dN.shape))
    if D >= 5:
        assert np.size(gN.xs[0]) == gN.N[0, 0]                     # a low_mem grid stays low_mem
    # without data: the grid alone; a time-first stack; data of zeros still comes back
    assert np.array_equal(np.asarray(L.truncateGrid(g, None, xmin, xmax).vs[0]).ravel(), vs[0][keep[0]])
    stack = np.stack([data, 2 * data])
    assert np.array_equal(L.truncateGrid(g, stack, xmin, xmax)[1], R.truncate_ref(vs, stack, xmin, xmax, lead=1)[1])
    gZ, dZ = L.truncateGrid(g, np.zeros(N), xmin, xmax)
    assert dZ.shape == dN.shape and not dZ.any()
    assert L.truncateGrid(g, data, xmin, xmax, process=False)[0].vs[0].shape == (len(keep[0]), 1)


GOLDEN_CASES = ["g2_box", "g2_one_node", "g3_box", "g3_periodic_whole", "g4_box"]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_truncate_grid_is_the_references(name, golden, monkeypatch):
    """tests/golden/truncate.npz: Grids/truncate.py on 2-D, 3-D and 4-D grids (make_golden_truncate.py lists what it cannot run)."""
    monkeypatch.setattr(MS, "require_gpu", no_device)
    G = golden("truncate.npz")
    k = lambda s: G["%s_%s" % (name, s)]                          # noqa: E731
    pd = int(k("pd")[0])
    g = L.createGrid(k("min"), k("max"), k("N").reshape(-1, 1), None if pd < 0 else pd)
    for process in (False, True):
        with np.errstate(divide="ignore"):
            gN, dN = L.truncateGrid(g, k("data"), k("xmin"), k("xmax"), process=process)
        D = len(k("N"))
        assert np.array_equal(np.asarray(gN.N).reshape(-1), k("newN")) and np.array_equal(dN, k("newdata"))
        assert np.array_equal(np.asarray(gN.min).reshape(-1), k("newmin")) and np.array_equal(np.asarray(gN.max).reshape(-1), k("newmax"))
        assert [gN.bdry[d] is L.addGhostPeriodic for d in range(D)] == list(k("newperiodic"))
        for d in range(D):
            assert np.array_equal(np.asarray(gN.vs[d]).ravel(), k("newvs%d" % d)) and np.asarray(gN.vs[d]).shape == (k("newN")[d], 1)


def test_set_bounds_host_arithmetic_on_the_restatements_records(monkeypatch):
    """setBounds with the launch replaced by the restatement: padding, clipping, the periodic axis, the stack's union, the empty set."""
    N, per = R.GRIDS[2]
    g = pkg_grid(N, per)
    vs, dx, _, _ = R.grid_vectors(N, per)

    def fake_run(g_, a, b, level):
        a = np.asarray(a)
        fields = a if a.ndim == len(N) + 1 else a[None]
        return [[R.measure_ref(f, level, per)] for f in fields], len(N), a.ndim == len(N) + 1
    monkeypatch.setattr(MS, "_run", fake_run)
    X = np.meshgrid(*vs, indexing="ij")
    data = np.sqrt((X[0] - 0.1) ** 2 + X[1] ** 2) - 0.45
    rec = R.measure_ref(data, 0.0, per)
    assert 0 < rec["lo"][0] and rec["hi"][0] < N[0] - 1
    for pad in (0, 1, 2, 9):
        b = L.setBounds(g, data, pad=pad)
        lo, hi, xmin, xmax = R.bounds_ref(N, vs, dx, per, rec["lo"], rec["hi"], pad)
        assert list(b.lo) == lo and list(b.hi) == hi and np.array_equal(b.xmin.ravel(), xmin) and np.array_equal(b.xmax.ravel(), xmax)
        assert (lo[2], hi[2]) == (0, N[2] - 1)                      # the periodic axis is whole
        keep, _ = R.truncate_ref(vs, None, xmin, xmax)
        assert [list(k_) for k_ in keep] == [list(range(l, h + 1)) for l, h in zip(lo, hi)]
    assert list(L.setBounds(g, data, pad=9).lo) == [0, 0, 0]
    moved = np.sqrt((X[0] + 0.3) ** 2 + X[1] ** 2) - 0.3
    both = L.setBounds(g, np.stack([data, moved]), pad=0)
    r2 = R.measure_ref(moved, 0.0, per)
    assert list(both.lo) == [min(p, q) for p, q in zip(rec["lo"], r2["lo"])][:2] + [0]
    assert L.setBounds(g, np.ones(N)) is None
    with pytest.raises(ValueError):
        L.setBounds(g, data, pad=-1)


def grid_of(dim, n=3):
    return L.Bundle(dict(dim=dim, N=np.full((dim, 1), n), vs=[np.zeros(n)] * dim, dx=np.ones((dim, 1)), bdry=[L.addGhostExtrapolate] * dim))


FRONT = [
    ("data-shape", lambda g, d: L.setVolume(g, np.zeros((5, 6, 8))), "does not agree in array size"),
    ("stack-shape", lambda g, d: L.setVolume(g, np.zeros((2, 5, 7, 6))), "does not agree in array size"),
    ("dim7", lambda g, d: L.setVolume(grid_of(7), np.zeros((3,) * 7)), "grid.dim must be 1..6"),
    ("one-node-axis", lambda g, d: L.setVolume(grid_of(2, 1), np.zeros((1, 1))), "at least two nodes"),
    ("level-nan", lambda g, d: L.setVolume(g, d, float("nan")), "level must be a finite number"),
    ("level-word", lambda g, d: L.setVolume(g, d, "zero"), "level must be a finite number"),
    ("compare-b-shape", lambda g, d: L.setCompare(g, d, np.zeros((5, 6))), "does not agree in array size"),
    ("compare-counts", lambda g, d: L.setCompare(g, np.zeros((3, 5, 6, 7)), np.zeros((2, 5, 6, 7))), "equal counts, or one field"),
    ("bounds-level", lambda g, d: L.setBounds(g, d, float("inf")), "level must be a finite number"),
    ("bounds-pad", lambda g, d: L.setBounds(g, d, pad=-1), "pad must be >= 0"),
    ("truncate-no-bounds", lambda g, d: L.truncateGrid(g, d), "needs xmin and xmax"),
    ("truncate-bounds-length", lambda g, d: L.truncateGrid(g, d, [0.0, 0.0], [1.0, 1.0]), "one entry per grid dimension"),
    ("truncate-empty-axis", lambda g, d: L.truncateGrid(g, d, [-1, 0.01, -1], [1, 0.02, 1]), "no node of axis 1"),
    ("truncate-data-shape", lambda g, d: L.truncateGrid(g, np.zeros((5, 6)), [-2] * 3, [2] * 3), "does not agree in array size"),
]


@pytest.mark.parametrize("case", FRONT, ids=[c[0] for c in FRONT])
def test_the_front_end_refuses_before_it_asks_for_a_device(case, monkeypatch):
    monkeypatch.setattr(MS, "require_gpu", no_device)
    g = L.createGrid(np.array([[-1.0, -1.0, -1.0]]).T, np.array([[1.0, 1.0, 1.0]]).T, np.array([[5, 6, 7]]).T)
    with pytest.raises(ValueError) as info:
        case[1](g, np.zeros((5, 6, 7)))
    assert case[2] in str(info.value), str(info.value)


def test_the_exports():
    for name in ("setVolume", "setCompare", "setBounds", "truncateGrid"):
        assert getattr(L, name) is getattr(MS, name)
    assert MS.last_path() == "" or "measure_kernel" in MS.last_path()
