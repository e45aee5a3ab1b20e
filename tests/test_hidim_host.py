"""CPU-only: libhj_hidim.so (include/hj_hidim.h) through ctypes, in the manner of tests/test_decomp_host.py, and the two systems
of dynamics.py that run on it.  Every data pointer is a fake or null and every check comes before the first HIP call, so no
device is touched: a bad argument is a refusal with a message, never a launch.

  * the binding, the header and the export table name the same functions, argument counts included; constants and structs
  * every refusal: ndim 4 and 7, the intended WENO5, a system on the wrong ndim, null tables, ...
  * the census: 12 substep and 12 upwind instantiations, the bound kernel per (type, system), nothing else
  * the schedule is hjb_plan's: one statement of the time arithmetic in the sources, and the interval without a step
  * Plane5D / DubinsPair6D: the NumPy methods equal the restatements of tests/hidim_cases.py; native_of's identity rule
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _bffi, _ffi, _hffi, _qffi  # noqa: E402
from levelsetpy_amd.dynamics import native_of, native_plant  # noqa: E402
import hidim_cases as HC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
H = _hffi


def grid(N=(7, 6, 8, 5, 9), dtype="float64"):
    nd = len(N)
    return H.grid_descriptor(nd, list(N), [0.0] * nd, [0.1 * (n - 1) for n in N], [0.1] * nd, [0] * nd, [0] * nd, dtype)


def tables(ncoord=6, naux=4):
    t = H.Tables()
    for d in range(ncoord):
        t.coord[d] = FAKE
    for s in range(naux):
        t.aux[s] = FAKE
    return t


def substep(g=None, tab="fake", scheme=_ffi.ENO2, ham=H.HAM_PLANE5D, stage=_ffi.STAGE_EULER, rs=0, par="fake", src=FAKE, y0=None,
            dst=FAKE + 8, post_prev=0, op_a=0, post_a=None, op_b=0, post_b=None):
    lib = H.lib()
    g = grid() if g is None else g
    before = lib.hjh_last_kernel()
    rc = lib.hjh_substep(C.byref(g) if g != "null" else None, C.byref(tables()) if tab == "fake" else (None if tab is None else C.byref(tab)),
                         scheme, ham, stage, rs, H.params([1, 1, -1]) if par == "fake" else par, src, y0, dst, 0.01, post_prev,
                         op_a, post_a, op_b, post_b, None)
    assert lib.hjh_last_kernel() == before                  # nothing was launched: the record stays
    return rc, lib.hjh_last_error().decode()


def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_hidim.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


# ------------------------------------------------------------------------------------------ ABI
def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjh_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(H.SIGNATURES)
    for need in ("hjh_substep", "hjh_step_bound", "hjh_integrate", "hjh_upwind", "hjh_last_error", "hjh_last_kernel"):
        assert need in declared
    out = subprocess.check_output(["nm", "-D", H.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (hjh_[a-z0-9_]+)", out))) == declared
    lib = H.lib()
    for name, (_, args) in H.SIGNATURES.items():
        assert hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        assert (0 if decl in ("", "void") else decl.count(",") + 1) == len(args), name


def test_constants_and_structures_are_the_headers():
    code = header_code()
    for name, val in (("HJH_MIN_DIM", H.MIN_DIM), ("HJH_MAX_DIM", H.MAX_DIM), ("HJH_HAM_PLANE5D", H.HAM_PLANE5D),
                      ("HJH_HAM_DUBINS_PAIR6D", H.HAM_DUBINS_PAIR6D), ("HJH_ARR_MIN", H.ARR_MIN), ("HJH_ARR_MAX", H.ARR_MAX),
                      ("HJH_ARR_MAX_NEG", H.ARR_MAX_NEG)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == val, name
    assert (H.MIN_DIM, H.MAX_DIM) == (5, 6) and _qffi.MAX_DIM == 4                          # HJ_MAX_DIM stays 4
    mi = open(os.path.join(ROOT, "include", "hj_mi355x.h")).read()
    assert re.search(r"#define HJ_MAX_DIM 4\b", mi)
    assert int(re.search(r"#define HJH_PAR_SLOTS (\d+)", code).group(1)) == H.PAR_SLOTS == 8
    assert (H.ARR_MIN, H.ARR_MAX, H.ARR_MAX_NEG) == (_bffi.ARR_MIN, _bffi.ARR_MAX, _bffi.ARR_MAX_NEG)    # numbered as hjb_entry's
    assert C.sizeof(H.Grid) == 8 + 6 * (8 + 8 + 8 + 8 + 4 + 4) and C.sizeof(H.Tables) == 80
    for struct, cls in (("hjh_grid", H.Grid), ("hjh_tables", H.Tables)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        assert re.findall(r"(\w+)(?:\[\w+\])?;", fields) == [n for n, _ in cls._fields_]
    # the ids are neither a solver system's nor a run-time registration's
    assert not {H.HAM_PLANE5D, H.HAM_DUBINS_PAIR6D} & set(_ffi.HAM_DIMS) and max(H.HAM_DIMS) < _ffi.HAM_USER_BASE
    assert H.HAM_DIMS == {H.HAM_PLANE5D: 5, H.HAM_DUBINS_PAIR6D: 6} and H.SCHEMES == (_ffi.ENO2, _ffi.ENO3, _ffi.WENO5_ASSHIPPED)


def test_the_makefile_builds_and_cleans_the_library():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\blibhj_hidim\.so\b", mk, re.M) and re.search(r"^\trm -f .*\blibhj_hidim\.so\b", mk, re.M)
    assert re.search(r"^libhj_hidim\.so: hj_hidim\.hip hj_tool_host\.h hj_split\.h hj_device\.h", mk, re.M) and "hj_hidim.hip" in mk.split("HIPCC ?=")[0]
    assert re.search(r"^resource-usage-hidim:", mk, re.M)
    libs = set(sum((line.split() for line in re.findall(r"^all:(.*)$", mk, re.M)), []))
    assert len(libs) == 10 and all(os.path.exists(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)) for n in libs)
    # the library links nothing of the solver
    needed = subprocess.check_output(["readelf", "-d", H.LIB_PATH]).decode()
    assert "libhj_" not in needed.replace("libhj_hidim.so", "")


# ------------------------------------------------------------------------------------------ refusals
REFUSALS = [
    ("ndim4", dict(g=grid((7, 6, 8, 5))), EINVAL, "5..6"),
    ("ndim7", dict(g=grid((7, 6, 8, 5, 9, 4))), EINVAL, "5..6"),          # (patched to 7 below)
    ("null-grid", dict(g="null"), EINVAL, "null grid"),
    ("dtype7", dict(g=grid(dtype="float64")), EINVAL, "dtype"),           # (patched below)
    ("null-tables", dict(tab=None), EINVAL, "null tables"),
    ("null-coord", dict(tab=tables(ncoord=4)), EINVAL, "coordinate table of axis 4"),
    ("null-aux", dict(tab=tables(naux=1)), EINVAL, "aux table 1"),
    ("null-aux-6d", dict(g=grid((6, 5, 7, 5, 6, 8)), ham=H.HAM_DUBINS_PAIR6D, tab=tables(naux=3)), EINVAL, "aux table 3"),
    ("weno5-intended", dict(scheme=_ffi.WENO5), EUNSUPPORTED, "scheme 2"),
    ("eno-fast", dict(scheme=4), EUNSUPPORTED, "scheme 4"),
    ("plane-on-6d", dict(g=grid((6, 5, 7, 5, 6, 8))), EINVAL, "lives on 5-D"),
    ("pair-on-5d", dict(ham=H.HAM_DUBINS_PAIR6D), EINVAL, "lives on 6-D"),
    ("solver-system", dict(ham=_ffi.HAM_DUBINS_REL), EUNSUPPORTED, "Hamiltonian 0"),
    ("null-params", dict(par=None), EINVAL, "null parameters"),
    ("small-N", dict(g=grid((7, 6, 2, 5, 9))), EINVAL, "N[2]"),
    ("stage", dict(stage=5), EINVAL, "stage 5"),
    ("post-prev", dict(post_prev=3), EINVAL, "post-step operator 3"),
    ("array-op", dict(op_a=4, post_a=FAKE), EINVAL, "array operator"),
    ("op-without-array", dict(op_b=H.ARR_MAX_NEG), EINVAL, "without its array"),
    ("null-src", dict(src=None), EINVAL, "null argument"),
    ("alias", dict(dst=FAKE), EINVAL, "alias"),
    ("y0-missing", dict(stage=_ffi.STAGE_RK3_FULL), EINVAL, "reads y0"),
]
REFUSALS[1][1]["g"].ndim = 7
REFUSALS[3][1]["g"].dtype = 7


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_substep_refuses(case):
    _, kw, code, word = case
    rc, err = substep(**kw)
    assert rc == code and word in err, (rc, err)
    with pytest.raises(_ffi.Unsupported if code == EUNSUPPORTED else ValueError) as info:
        H.check(rc)
    assert word in str(info.value) and (code == EUNSUPPORTED or not isinstance(info.value, _ffi.Unsupported))


def test_the_other_entry_points_refuse_before_any_launch():
    lib = H.lib()
    g5, g4, t = grid(), grid((7, 6, 8, 5)), tables()
    par = H.params([1, 1, -1])
    before = lib.hjh_last_kernel()
    sb = C.c_double()
    vp = (C.c_void_p * 6)(*([FAKE] * 6))
    calls = [
        (lambda: lib.hjh_step_bound(C.byref(g4), C.byref(t), H.HAM_PLANE5D, par, FAKE, C.byref(sb), None, None), EINVAL, "5..6"),
        (lambda: lib.hjh_step_bound(C.byref(g5), C.byref(t), H.HAM_PLANE5D, par, None, C.byref(sb), None, None), EINVAL, "null argument"),
        (lambda: lib.hjh_step_bound(C.byref(g5), None, H.HAM_PLANE5D, par, FAKE, C.byref(sb), None, None), EINVAL, "null tables"),
        (lambda: lib.hjh_upwind(C.byref(g4), _ffi.ENO2, FAKE, 1, vp, vp, None, None), EINVAL, "5..6"),
        (lambda: lib.hjh_upwind(C.byref(g5), _ffi.WENO5, FAKE, 1, vp, vp, None, None), EUNSUPPORTED, "scheme 2"),
        (lambda: lib.hjh_upwind(C.byref(g5), _ffi.ENO2, FAKE, 0, vp, vp, None, None), EINVAL, "axis_mask"),
        (lambda: lib.hjh_upwind(C.byref(g5), _ffi.ENO2, FAKE, 1 << 5, vp, vp, None, None), EINVAL, "axis_mask"),
        (lambda: lib.hjh_upwind(C.byref(g5), _ffi.ENO2, None, 1, vp, vp, None, None), EINVAL, "null argument"),
        (lambda: lib.hjh_upwind(C.byref(g5), _ffi.ENO2, FAKE, 2, (C.c_void_p * 6)(FAKE, None), vp, None, None), EINVAL, "axis 1"),
    ]

    def integ(g=g5, scheme=_ffi.ENO3, order=3, sbv=0.1, y=FAKE, a=FAKE + 8, b=FAKE + 16, w=FAKE + 24, tf=1.0):
        return lib.hjh_integrate(C.byref(g), C.byref(t), scheme, H.HAM_PLANE5D, order, 0, 0, par, sbv, y, a, b, w, 0, None, 0, None,
                                 0.0, tf, 0.8, 1e300, 1e-4, None, None, None, None)
    calls += [
        (lambda: integ(g=g4), EINVAL, "5..6"),
        (lambda: integ(scheme=_ffi.WENO5), EUNSUPPORTED, "scheme 2"),
        (lambda: integ(order=4), EINVAL, "order"),
        (lambda: integ(w=None), EINVAL, "work buffer"),
        (lambda: integ(b=FAKE + 8), EINVAL, "distinct"),
        (lambda: integ(sbv=0.0), EINVAL, "step bound must be positive"),
    ]
    for fn, code, word in calls:
        rc = fn()
        assert rc == code and word in lib.hjh_last_error().decode(), (rc, lib.hjh_last_error())
        assert lib.hjh_last_kernel() == before


# ------------------------------------------------------------------------------------------ census
def test_census_of_the_library():
    """The kernels libhj_hidim.so ships: hidim_substep_kernel for 2 types x 2 systems x 3 schemes (each named by _hffi.kernel_name
    and launched by tests/test_gpu_hidim.py::test_every_substep_instantiation_and_stage), hidim_upwind_kernel for 2 types x 2
    dimensions x 3 schemes, hidim_bound_kernel per (type, system) -- and nothing else."""
    out = subprocess.check_output(["nm", "-D", "-C", H.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+<[^(]*>)\(", out))
    want = {"hidim_substep_kernel<%s, hjh::%s<%s>, %d>" % (t, h, t, k) for t in ("double", "float") for h in H.HAM_NAMES.values() for k in H.SCHEMES}
    want |= {"hidim_upwind_kernel<%s, %d, %d>" % (t, nd, k) for t in ("double", "float") for nd in (5, 6) for k in H.SCHEMES}
    assert len(want) == 24
    want |= {"hidim_bound_kernel<%s, hjh::%s<%s> >" % (t, h, t) for t in ("double", "float") for h in H.HAM_NAMES.values()}
    assert stubs == want, sorted(stubs ^ want)
    assert H.kernel_name("float64", H.HAM_DUBINS_PAIR6D, 3) == "hidim_substep_kernel<double, HamDubinsPair6D, 3>"
    assert H.kernel_name("float32", H.HAM_PLANE5D, 0) == "hidim_substep_kernel<float, HamPlane5D, 0>"


# ------------------------------------------------------------------------------------------ the schedule
def test_the_schedule_is_hjb_plans():
    """hjh_integrate plans with the function hjb_plan plans with: one definition in the shared host layer, called by both libraries and
    restated by neither.  (tests/test_gpu_hidim.py holds the step counts and times of real intervals to hjb_plan with ==.)"""
    src = lambda n: open(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)).read()      # noqa: E731
    host, batch, hidim = src("hj_tool_host.h"), src("hj_batch.hip"), src("hj_hidim.hip")
    assert len(re.findall(r"^static int plan_problem\(", host, re.M)) == 1 and len(re.findall(r"^static double step_time\(", host, re.M)) == 1
    for text in (batch, hidim):
        assert "plan_problem(" in text and not re.search(r"^static \w+ (plan_problem|step_time)\(", text, re.M) and "tThreeHalf" not in text
    # an interval that needs no step launches nothing, reports t0 and no step, and the result stays in y_in: as hjb_plan says
    lib = H.lib()
    g, t, par = grid(), tables(), H.params([1, 1, -1])
    for order in (1, 2, 3):
        tout, n, where = C.c_double(-1), C.c_int64(-1), C.c_int32(-1)
        rc = lib.hjh_integrate(C.byref(g), C.byref(t), _ffi.ENO3, H.HAM_PLANE5D, order, 0, 0, par, 0.05, FAKE, FAKE + 8, FAKE + 16, FAKE + 24,
                               0, None, 0, None, 0.5, 0.5 + 5e-5, 0.8, 1e300, 1e-4, C.byref(tout), C.byref(n), C.byref(where), None)
        assert rc == OK, lib.hjh_last_error()
        tb, nb = C.c_double(), C.c_int64()
        _bffi.check(_bffi.lib().hjb_plan(order, (C.c_double * 1)(0.05), 1, 0.5, 0.5 + 5e-5, 0.8, 1e300, 1e-4, C.byref(tb), C.byref(nb)))
        assert (tout.value, n.value, where.value) == (tb.value, nb.value, 0) == (0.5, 0, 0)


def test_what_the_three_stage_libraries_share_is_defined_once():
    """libhj_batch.so, libhj_stoch.so and libhj_hidim.so: the descriptor's fill_grid, key_to_double, array_op, struct Stage and the RK
    buffer rotation have one definition each -- in hj_stage_host.h, hj_stage_dev.h or (key_to_double, beside key_max) hj_device.h --
    and none in the libraries' own files.  (tests/test_stage_libs_host.py holds the three libraries' refusals to one table.)"""
    src = lambda n: open(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)).read()      # noqa: E731
    host, dev, device = src("hj_stage_host.h"), src("hj_stage_dev.h"), src("hj_device.h")
    own = {n: src(n) for n in ("hj_batch.hip", "hj_stoch.hip", "hj_hidim.hip", "hj_hidim_dev.h", "hj_api.hip")}
    definitions = {
        "fill_grid": r"^template <[^>]*>\s*(?:static |inline )*void fill_grid\(const \w+\* g,",
        "key_to_double": r"^(?:static |inline )*double key_to_double\(",
        "array_op": r"^(?:__device__ |__forceinline__ )+T array_op\(",
        "struct Stage": r"^struct Stage \{",
        "rotation": r"outs\[k & 1\]",
    }
    home = {"fill_grid": host, "key_to_double": device, "array_op": dev, "struct Stage": host, "rotation": host}
    # (hj_rk_integrate of hj_api.hip, the context's solver, steps with a bound it measures as it goes: its loop and its words stay its own)
    words = "the first stage buffer doubles as the output"
    assert host.count(words) == 1 and not any(words in text for n, text in own.items() if n != "hj_api.hip")
    for what, rx in definitions.items():
        assert len(re.findall(rx, home[what], re.M)) == 1, what
        for n, text in own.items():
            assert not re.search(rx, text, re.M), (what, n)
        for other in (host, dev, device):
            assert other is home[what] or not re.search(rx, other, re.M), what
    for n in ("hj_batch.hip", "hj_stoch.hip", "hj_hidim.hip"):
        assert '#include "hj_stage_host.h"' in own[n] and "rk_schedule(" in own[n] and "result_in(" in own[n], n
    # the device header is hipRTC's too (through hj_hidim_dev.h, and in the cache key's file list): nothing of the host layer in it
    assert '#include "hj_stage_dev.h"' in own["hj_hidim_dev.h"] and '"/hj_stage_dev.h"' in own["hj_hidim.hip"]
    assert "hj_tool::" not in dev and "#include \"hj_tool_host.h\"" not in dev and "#include \"hj_stage_host.h\"" not in dev


# ------------------------------------------------------------------------------------------ the systems
def lgrid(name, low_mem=False):
    gmin, gmax, N, pd = HC.limits(name)
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd, low_mem=low_mem)


@pytest.mark.parametrize("name", ["plane5d", "pair6d", "plane5d_long"])
def test_numpy_methods_equal_the_restatements(name):
    g, og = lgrid(name), HC.oracle_grid(name)
    for d in range(g.dim):
        assert np.array_equal(np.asarray(g.vs[d]), og.vs[d]) and float(np.asarray(g.dx).ravel()[d]) == float(og.dx.ravel()[d])
    sys_ = (L.Plane5D if g.dim == 5 else L.DubinsPair6D)(g, **HC.PARAMS[name])
    osys = HC.oracle_system(name, og, **HC.PARAMS[name])
    rng = np.random.default_rng(3)
    p = [rng.standard_normal(og.shape) for _ in range(g.dim)]
    data = HC.data(og)
    assert np.array_equal(sys_.hamiltonian(0.0, data, p, None), osys.hamiltonian(0.0, data, p, None))
    for d in range(g.dim):
        a, b = sys_.dissipation(0.0, data, None, None, None, d), osys.dissipation(0.0, data, None, None, None, d)
        assert np.array_equal(np.broadcast_to(a, og.shape), np.broadcast_to(b, og.shape)), d
    # a low_mem grid (sparse xs) gives the same values by broadcasting
    gs = lgrid(name, low_mem=True)
    ss = (L.Plane5D if g.dim == 5 else L.DubinsPair6D)(gs, **HC.PARAMS[name])
    assert np.array_equal(ss.hamiltonian(0.0, data, p, None), osys.hamiltonian(0.0, data, p, None))


def test_native_of_recognises_the_new_systems_by_identity():
    g5, g6 = lgrid("plane5d"), lgrid("pair6d")
    a, b = L.Plane5D(g5, 0.8, 1.3, 'max'), L.DubinsPair6D(g6, 1.5, 1.1, 0.9, 1.4)
    assert native_of(a.hamiltonian, a.dissipation) == (a, H.HAM_PLANE5D, [0.8, 1.3, 1.0, 0.0])
    assert native_of(b.hamiltonian, b.dissipation) == (b, H.HAM_DUBINS_PAIR6D, [1.5, 1.1, 0.9, 1.4])
    assert L.Plane5D(g5).native()[1][2] == -1.0                                 # u_mode 'min' is the default
    assert native_of(a.hamiltonian, b.dissipation) is None
    assert L.Plane5D(g6).native() is None and L.DubinsPair6D(g5).native() is None     # the wrong dimension

    class Mine(L.DubinsPair6D):
        def hamiltonian(self, t, data, p, sd=None):
            return L.DubinsPair6D.hamiltonian(self, t, data, p, sd) * 1.0

    class Mine5(L.Plane5D):
        def dissipation(self, t, data, lo, hi, sd, dim):
            return L.Plane5D.dissipation(self, t, data, lo, hi, sd, dim)

    class Renamed(L.Plane5D):
        pass

    m, m5, r = Mine(g6), Mine5(g5), Renamed(g5)
    assert native_of(m.hamiltonian, m.dissipation) is None and native_of(m5.hamiltonian, m5.dissipation) is None
    assert native_of(r.hamiltonian, r.dissipation)[1] == H.HAM_PLANE5D
    # the rollout kernel has no 5-D / 6-D plant
    assert native_plant(a) is None and native_plant(b) is None
    with pytest.raises(ValueError):
        L.Plane5D(g5, u_mode='sideways')


def test_the_dynsys_protocol():
    g5, g6 = lgrid("plane5d"), lgrid("pair6d")
    a, b = L.Plane5D(g5, 0.8, 1.3, 'min'), L.DubinsPair6D(g6, 1.5, 1.1, 0.9, 1.4)
    x5, p5 = np.array([0.1, -0.2, 0.7, 1.2, -0.4]), np.array([0.3, -0.5, 0.2, -0.7, 0.9])
    u = a.get_opt_u(0.0, p5, None, x5)
    assert u == (0.8, -1.3) and a.get_opt_u(0.0, p5, 'max', x5) == (-0.8, 1.3) and a.get_opt_v(0.0, p5, None, x5) is None
    f = a.dynamics(0.0, x5, u)
    assert np.array_equal(f, [1.2 * np.cos(0.7), 1.2 * np.sin(0.7), -0.4, 0.8, -1.3])
    # the Hamiltonian is the optimum of p.f over the controls: p.f at the optimal control is H's expression
    H5 = p5[0] * f[0] + p5[1] * f[1] + p5[2] * f[2] - 0.8 * abs(p5[3]) - 1.3 * abs(p5[4])
    assert abs(float(np.dot(p5, f)) - H5) < 1e-15
    x6, p6 = np.array([0.1, -0.2, 0.7, 1.2, -0.4, 2.0]), np.array([0.3, -0.5, 0.2, -0.7, 0.9, -0.6])
    ue, dp = b.get_opt_u(0.0, p6, None, x6), b.get_opt_v(0.0, p6, None, x6)
    assert (ue, dp) == (0.9, 1.4)
    f = b.dynamics(0.0, x6, ue, dp)
    assert np.array_equal(f, [1.5 * np.cos(0.7), 1.5 * np.sin(0.7), 0.9, 1.1 * np.cos(2.0), 1.1 * np.sin(2.0), 1.4])
    x1 = b.update_state(ue, 0.01, x6, dp)
    assert x1.shape == (6,) and np.allclose(x1, x6 + 0.01 * f, atol=1e-3) and b.x is x1
    assert a.update_state(u, 0.01, x5).shape == (5,)


def test_seven_dimensions_stay_refused():
    from levelsetpy_amd import hidim
    g7 = L.createGrid(np.zeros((7, 1)), np.ones((7, 1)), 3 * np.ones((7, 1), dtype=np.int64))
    with pytest.raises(ValueError, match=r"1\.\.6"):
        hidim.check_dim(g7)
    with pytest.raises(ValueError, match=r"1\.\.6"):
        L.upwindFirstENO2(g7, np.zeros(g7.shape), 0)
    sd = L.Bundle(dict(grid=g7, hamFunc=None, partialFunc=None))
    with pytest.raises(ValueError, match=r"1\.\.6"):
        L.HJIPDE_solve(np.zeros(g7.shape), [0.0, 0.1], sd, None, L.Bundle(dict(quiet=True)))


def test_explain_plan_names_the_library():
    g6 = lgrid("pair6d")
    b = L.DubinsPair6D(g6)
    sd = L.Bundle(dict(grid=g6, hamFunc=b.hamiltonian, partialFunc=b.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    assert L.explain_plan(sd) == dict(path='built-in', ham_id=H.HAM_DUBINS_PAIR6D, params=[5.0, 5.0, 5.0, 5.0], library='libhj_hidim.so')
    sd2 = L.Bundle(dict(grid=g6, hamFunc=lambda *a: 0, partialFunc=lambda *a: 0, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
    e = L.explain_plan(sd2)
    assert e['path'] == 'split' and 'Plane5D / DubinsPair6D' in e['reason'] and e['library'] == 'libhj_hidim.so'
