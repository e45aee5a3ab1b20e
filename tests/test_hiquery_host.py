"""CPU-only: libhj_hiquery.so (include/hj_hiquery.h) through ctypes, in the manner of tests/test_hidim_host.py.  Every data
pointer is a fake or null and every check comes before the first HIP call, so no device is touched: a bad argument is a refusal
with a message, never a launch.

  * the binding, the header and the export table name the same functions, argument counts included; constants; the descriptor
  * the Makefile builds the library under plain `make`, cleans it, and its `all:` lines still name ten libraries
  * every refusal of the four entry points
  * the census: 2 interp + 12 costate + 4 projection + 12 rollout kernels, each mapped to the GPU test that launches it
  * what stays: _marshal.descriptor refuses a 5-D grid, _rffi.PLANT_DIMS is _ffi.HAM_DIMS, native_plant knows no 5-D / 6-D plant
  * the plants restated in tests/hiquery_cases.py are dynamics.py's dynSys methods
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
from levelsetpy_amd import _ffi, _hffi, _marshal, _qffi, _rffi  # noqa: E402
from levelsetpy_amd import _xffi as X  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd.dynamics import native_plant, native_plant_hi  # noqa: E402
import hiquery_cases as XC  # noqa: E402
import rollout_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
FAKE = 0x1000                       # a non-null address where a check wants one: only compared with null, never read
N5, N6 = (7, 6, 8, 5, 9), (6, 5, 7, 5, 6, 8)


def grid(N=N5, dtype="float64"):
    nd = len(N)
    return _hffi.grid_descriptor(nd, list(N), [0.0] * nd, [0.1 * (n - 1) for n in N], [0.1] * nd, [0] * nd, [0] * nd, dtype)


def patched(g, **kw):
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def header_code():
    txt = open(os.path.join(ROOT, "include", "hj_hiquery.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


# ------------------------------------------------------------------------------------------ ABI
def test_binding_header_and_exports_name_the_same_functions():
    code = header_code()
    declared = sorted(set(re.findall(r"\b(hjx_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(X.SIGNATURES)
    assert declared == ["hjx_costate_points", "hjx_interp_points", "hjx_last_error", "hjx_last_kernel", "hjx_project_minmax", "hjx_rollout"]
    out = subprocess.check_output(["nm", "-D", X.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (hjx_[a-z0-9_]+)", out))) == declared
    lib = X.lib()
    for name, (_, args) in X.SIGNATURES.items():
        assert hasattr(lib, name)
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        assert (0 if decl in ("", "void") else decl.count(",") + 1) == len(args), name
    # the same argument lists as the <= 4-D entry points, on the other descriptor
    for name, other in (("interp_points", _qffi), ("costate_points", _qffi), ("project_minmax", _qffi), ("rollout", _rffi)):
        pre = "hjq_" if other is _qffi else "hjr_"
        assert X.SIGNATURES["hjx_" + name][1][1:] == other.SIGNATURES[pre + name][1][1:], name


def test_constants_and_the_descriptor_are_the_headers():
    hid = open(os.path.join(ROOT, "include", "hj_hidim.h")).read()
    for name, val in (("HJH_MIN_DIM", X.MIN_DIM), ("HJH_MAX_DIM", X.MAX_DIM)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, hid).group(1)) == val
    qh = open(os.path.join(ROOT, "include", "hj_query.h")).read()
    assert int(re.search(r"HJQ_MIN = (\d+)", qh).group(1)) == X.OP_MIN and int(re.search(r"HJQ_MAX = (\d+)", qh).group(1)) == X.OP_MAX
    # no third descriptor type: hjh_grid for the grid, hjr_plant for the plant
    code = header_code()
    assert "typedef struct" not in code and '#include "hj_hidim.h"' in code and '#include "hj_rollout.h"' in code
    assert X.Grid is _hffi.Grid and X.Plant is _rffi.Plant and X.SIGNATURES["hjx_rollout"][1][0]._type_ is _hffi.Grid
    assert X.PLANT_DIMS is _hffi.HAM_DIMS and X.SCHEMES == (_ffi.ENO2, _ffi.ENO3, _ffi.WENO5_ASSHIPPED)
    assert (X.MIN_DIM, X.MAX_DIM) == (5, 6) and _qffi.MAX_DIM == 4                          # HJ_MAX_DIM stays 4
    assert re.search(r"#define HJ_MAX_DIM 4\b", open(os.path.join(ROOT, "include", "hj_mi355x.h")).read())


def test_the_makefile_builds_and_cleans_the_library():
    mk = open(os.path.join(ROOT, "levelsetpy_amd", "csrc", "Makefile")).read()
    # not on an `all:` line (tests count those), yet what a plain `make` builds
    libs = set(sum((line.split() for line in re.findall(r"^all:(.*)$", mk, re.M)), []))
    assert len(libs) == 10 and "libhj_hiquery.so" not in libs
    goal = re.search(r"^\.DEFAULT_GOAL := (\w+)$", mk, re.M).group(1)
    deps = re.search(r"^%s:(.*)$" % goal, mk, re.M).group(1).split()
    assert "all" in deps and "libhj_hiquery.so" in deps
    assert re.search(r"^\trm -f .*\blibhj_hiquery\.so\b", mk, re.M) and "hj_hiquery.hip" in mk.split("HIPCC ?=")[0]
    assert re.search(r"^libhj_hiquery\.so: hj_hiquery\.hip hj_tool_host\.h hj_query_dev\.h hj_rollout_dev\.h hj_device\.h", mk, re.M)
    assert re.search(r"^libhj_rollout\.so: hj_rollout\.hip hj_tool_host\.h hj_query_dev\.h hj_rollout_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-hiquery:", mk, re.M)
    dry = subprocess.check_output(["make", "-C", os.path.join(ROOT, "levelsetpy_amd", "csrc"), "-n", "-B"]).decode()
    assert "-o libhj_hiquery.so hj_hiquery.hip" in dry and "-o libhj_hidim.so hj_hidim.hip" in dry
    assert os.path.exists(X.LIB_PATH)
    # the library links nothing of the other libraries
    needed = subprocess.check_output(["readelf", "-d", X.LIB_PATH]).decode()
    assert "libhj_" not in needed.replace("libhj_hiquery.so", "")


def test_one_source_for_the_arithmetic():
    """locate, corner, interp_value, gather_axis, group_sum, a corner's derivatives, the bodies of the costate and projection
    kernels, the RK4 step, sgn and the trajectory are defined once, in the two shared headers, and restated by none of the
    translation units that use them; so are the host side's make_grid, fill_stencil and the rollout checks."""
    src = lambda n: open(os.path.join(ROOT, "levelsetpy_amd", "csrc", n)).read()      # noqa: E731
    qdev, rdev = src("hj_query_dev.h"), src("hj_rollout_dev.h")
    users = [src(n) for n in ("hj_query.hip", "hj_rollout.hip", "hj_decomp.hip", "hj_hiquery.hip", "hj_plant.hip")]
    for fn in ("locate", "corner", "interp_value", "gather_axis", "group_sum", "proj_base", "corner_derivs", "costate_body", "proj_loops",
               "project_body"):
        pat = r"^__device__ __forceinline__ \w[\w ]* %s\(" % fn
        assert len(re.findall(pat, qdev, re.M)) == 1, fn
        assert not any(re.search(pat, u, re.M) for u in users), fn
    for fn in ("sgn", "rk4", "rollout_body"):
        pat = r"^__device__ __forceinline__ \w+ %s\(" % fn
        assert len(re.findall(pat, rdev, re.M)) == 1, fn
        assert not any(re.search(pat, u, re.M) for u in users), fn
    for fn, home in (("make_grid", qdev), ("fill_stencil", qdev), ("check_rollout", rdev)):
        pat = r"^static \w+ %s\(" % fn
        assert len(re.findall(pat, home, re.M)) == 1 and len(re.findall(pat, qdev + rdev, re.M)) == 1, fn
        assert not any(re.search(pat, u, re.M) for u in users), fn
    # the checks' texts, too: each stands once, and in none of the five files
    for text in ("out of range", "grid too large", "a rollout needs at least two stored sets", "u_mode / d_mode must be", "unknown projection"):
        assert (qdev + rdev).count(text) == 1 and not any(text in u for u in users), text
    # no costate or projection loop outside hj_query_dev.h: the kernels of the two libraries are frames around the bodies
    for u in users:
        assert "gather_axis<" not in u and "acc.take(" not in u and "static_assert(MAXD ==" not in u
    hi = src("hj_hiquery.hip")
    assert "#define HJ_QUERY_MAXD 6" in hi and '#include "hj_query_dev.h"' in hi and '#include "hj_rollout_dev.h"' in hi
    assert "HJ_QUERY_MAXD HJ_MAX_DIM" in qdev                                       # every other library compiles it at 4


# ------------------------------------------------------------------------------------------ refusals
def interp(g=None, data=FAKE, xs=FAKE, out=FAKE, nfields=1, nstates=1):
    return lambda lib: lib.hjx_interp_points(None if g == "null" else C.byref(g or grid()), data, nfields, 15120, xs, nstates, out, 0, None)


def costate(g=None, scheme=_ffi.ENO2, data=FAKE, xs=FAKE, out=FAKE):
    return lambda lib: lib.hjx_costate_points(None if g == "null" else C.byref(g or grid()), scheme, data, 1, 15120, xs, 1, out, None, None,
                                              None, 0, None)


def project(g=None, mask=1, op=0, data=FAKE, out=FAKE):
    return lambda lib: lib.hjx_project_minmax(None if g == "null" else C.byref(g or grid()), data, 1, 15120, mask, op, out, None)


def rollout(g=None, scheme=_ffi.ENO2, plant=_hffi.HAM_PLANE5D, data=FAKE, x0=FAKE, nstates=1, sub=4, ntimes=2, stride=None, u_mode=0):
    def call(lib):
        gg = grid() if g in (None, "null") else g
        n = 1
        for d in range(6):
            n *= gg.N[d]
        p = None if plant is None else _rffi.plant_descriptor(plant, u_mode, 0, [1.0] * 4)
        return lib.hjx_rollout(None if g == "null" else C.byref(gg), scheme, data, ntimes, n if stride is None else stride, x0, nstates, sub,
                               0.01, None if p is None else C.byref(p), FAKE, FAKE, None, FAKE, None)
    return call


G4, G7, GD = grid((7, 6, 8, 5)), patched(grid(N6), ndim=7), patched(grid(), dtype=7)
REFUSALS = [(fn.__name__ + "-" + cid, fn(**kw), code, word) for fn in (interp, costate, project, rollout) for cid, kw, code, word in (
    ("ndim4", dict(g=G4), EINVAL, "5..6"), ("ndim7", dict(g=G7), EINVAL, "5..6"), ("null-grid", dict(g="null"), EINVAL, "null grid"),
    ("dtype7", dict(g=GD), EINVAL, "dtype"), ("null-data", dict(data=None), EINVAL, "null argument"),
    ("bc9", dict(g=patched(grid(), bc=(C.c_int32 * 6)(0, 9, 0, 0, 0, 0))), EINVAL, "boundary"))]
REFUSALS += [
    ("interp-null-states", interp(xs=None), EINVAL, "null argument"),
    ("interp-null-out", interp(out=None), EINVAL, "null argument"),
    ("interp-no-states", interp(nstates=0), EINVAL, "positive"),
    ("interp-N1", interp(g=grid((7, 6, 8, 1, 9))), EINVAL, "too small"),
    ("costate-null-states", costate(xs=None), EINVAL, "null argument"),
    ("costate-null-out", costate(out=None), EINVAL, "null argument"),
    ("costate-weno5-intended", costate(scheme=_ffi.WENO5), EUNSUPPORTED, "scheme 2"),
    ("costate-eno2-fast", costate(scheme=4), EUNSUPPORTED, "scheme 4"),
    ("costate-eno3-fast", costate(scheme=5), EUNSUPPORTED, "scheme 5"),
    ("costate-N2", costate(g=grid((7, 6, 2, 5, 9))), EINVAL, "too small"),
    ("project-empty-mask", project(mask=0), EINVAL, "remove_mask"),
    ("project-full-mask-5d", project(mask=0b11111), EINVAL, "remove_mask"),
    ("project-full-mask-6d", project(g=grid(N6), mask=0b111111), EINVAL, "remove_mask"),
    ("project-axis-5-on-5d", project(mask=0b100000), EINVAL, "remove_mask"),
    ("project-op", project(op=2), EINVAL, "projection 2"),
    ("project-null-out", project(out=None), EINVAL, "null argument"),
    ("rollout-weno5-intended", rollout(scheme=_ffi.WENO5), EUNSUPPORTED, "scheme 2"),
    ("rollout-eno-fast", rollout(scheme=4), EUNSUPPORTED, "scheme 4"),
    ("rollout-plane-on-6d", rollout(g=grid(N6), plant=_hffi.HAM_PLANE5D), EINVAL, "5 states"),
    ("rollout-pair-on-5d", rollout(plant=_hffi.HAM_DUBINS_PAIR6D), EINVAL, "6 states"),
    ("rollout-solver-plant", rollout(plant=_ffi.HAM_DUBINS_REL), EUNSUPPORTED, "plant 0"),
    ("rollout-user-plant", rollout(plant=_ffi.HAM_USER_BASE), EUNSUPPORTED, "plant %d" % _ffi.HAM_USER_BASE),
    ("rollout-null-plant", rollout(plant=None), EINVAL, "null plant"),
    ("rollout-sub0", rollout(sub=0), EINVAL, "sub_samples"),
    ("rollout-one-set", rollout(ntimes=1), EINVAL, "two stored sets"),
    ("rollout-stride", rollout(stride=100), EINVAL, "field_stride"),
    ("rollout-mode", rollout(u_mode=2), EINVAL, "u_mode"),
    ("rollout-negative", rollout(nstates=-1), EINVAL, "negative"),
    ("rollout-null-x0", rollout(x0=None), EINVAL, "null argument"),
    ("rollout-N2", rollout(g=grid((7, 6, 2, 5, 9))), EINVAL, "too small"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_entry_points_refuse_before_any_launch(case):
    _, call, code, word = case
    lib = X.lib()
    before = lib.hjx_last_kernel()
    rc = call(lib)
    err = lib.hjx_last_error().decode()
    assert rc == code and word in err, (rc, err)
    assert lib.hjx_last_kernel() == before                  # nothing was launched: the record stays
    with pytest.raises(_ffi.Unsupported if code == EUNSUPPORTED else ValueError) as info:
        X.check(rc)
    assert word in str(info.value) and (code == EUNSUPPORTED or not isinstance(info.value, _ffi.Unsupported))


def test_no_states_is_nothing_to_do():
    lib = X.lib()
    before = lib.hjx_last_kernel()
    for g, plant in ((grid(), 50), (grid(N6), 51)):
        assert rollout(g=g, plant=plant, nstates=0, data=None, x0=None)(lib) == OK
    assert lib.hjx_last_kernel() == before


# ------------------------------------------------------------------------------------------ census
GPU_TEST = {"hi_interp_points_kernel": "test_eval_u_bitwise", "hi_costate_points_kernel": "test_eval_costate_is_gradients_then_eval_u",
            "hi_project_minmax_kernel": "test_proj_minmax_bitwise", "hi_rollout_kernel": "test_one_control_step_on_every_plant_and_scheme"}


def census():
    want = {X.interp_kernel_name(t) for t in ("float64", "float32")}
    want |= {X.costate_kernel_name(t, nd, k) for t in ("float64", "float32") for nd in (5, 6) for k in X.SCHEMES}
    want |= {X.project_kernel_name(t, w) for t in ("float64", "float32") for w in (False, True)}
    want |= {X.rollout_kernel_name(t, k, p) for t in ("float64", "float32") for k in X.SCHEMES for p in X.PLANT_DIMS}
    return want


def test_census_of_the_library():
    """Exactly 30 kernels, and each is launched -- its name asserted through hjx_last_kernel -- by a test of
    tests/test_gpu_hiquery.py."""
    out = subprocess.check_output(["nm", "-D", "-C", X.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+<[^(]*>)\(", out))
    want = census()
    assert len(want) == 2 + 12 + 4 + 12 == 30
    assert stubs == want, sorted(stubs ^ want)
    assert X.costate_kernel_name("float64", 6, 1) == "hi_costate_points_kernel<double, 6, 1>"
    assert X.rollout_kernel_name("float32", 0, 51) == "hi_rollout_kernel<float, 0, 51>"
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_hiquery.py")).read()
    for kernel in want:
        test = GPU_TEST[kernel.split("<")[0]]
        body = gpu[gpu.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert "launched(" in body, test


# ------------------------------------------------------------------------------------------ what stays, and the front end's rules
def test_the_four_axis_descriptor_and_the_plant_table_stay():
    g5, _ = XC.grids("plane5d")
    with pytest.raises(ValueError, match="more than 4 dimensions"):
        _marshal.descriptor(g5, "float64")
    desc, N = _marshal.descriptor_hi(g5, "float32")
    assert isinstance(desc, _hffi.Grid) and N == N5 and (desc.ndim, desc.dtype) == (5, _ffi.F32)
    assert [desc.N[d] for d in range(6)] == list(N5) + [1] and [desc.bc[d] for d in range(5)] == [0, 0, 1, 0, 0]
    assert _rffi.PLANT_DIMS is _ffi.HAM_DIMS and not set(_hffi.HAM_DIMS) & set(_ffi.HAM_DIMS)
    g4 = L.createGrid(np.zeros((4, 1)), np.ones((4, 1)), 5 * np.ones((4, 1), dtype=np.int64))
    g7 = L.createGrid(np.zeros((7, 1)), np.ones((7, 1)), 3 * np.ones((7, 1), dtype=np.int64))
    for g in (g4, g7):
        with pytest.raises(ValueError, match=r"5\.\.6"):
            _marshal.descriptor_hi(g, "float64")
    assert _marshal.is_hi(g5) and _marshal.is_hi(g7) and not _marshal.is_hi(g4)


def test_native_plant_hi_is_the_identity_rule():
    g5, g6 = XC.grids("plane5d")[0], XC.grids("pair6d")[0]
    a, b = L.Plane5D(g5, 0.8, 1.3, 'max'), L.DubinsPair6D(g6, 1.5, 1.1, 0.9, 1.4)
    assert native_plant_hi(a) == (_hffi.HAM_PLANE5D, [0.8, 1.3, 0.0, 0.0]) and native_plant_hi(b) == (_hffi.HAM_DUBINS_PAIR6D, [1.5, 1.1, 0.9, 1.4])
    assert native_plant(a) is None and native_plant(b) is None and native_plant_hi(L.DoubleIntegrator(g5, 1)) is None
    assert native_plant_hi(L.Plane5D(g6)) is None and native_plant_hi(L.DubinsPair6D(g5)) is None     # the wrong dimension

    class Lazy(L.DubinsPair6D):
        def get_opt_u(self, t, deriv, uMode, x):
            return 0.5 * L.DubinsPair6D.get_opt_u(self, t, deriv, uMode, x)

    class Renamed(L.Plane5D):
        pass

    assert native_plant_hi(Lazy(g6)) is None and native_plant_hi(Renamed(g5))[0] == _hffi.HAM_PLANE5D
    c = L.Plane5D(g5)
    c.update_state = lambda *args: None                      # an instance attribute shadows the method
    assert native_plant_hi(c) is None
    assert native_plant_hi(L.Plane5D(g5, a_max=np.ones(3))) is None


@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_the_restated_plants_are_the_dynsys_methods(name):
    """tests/hiquery_cases.py's controls and f against get_opt_u / get_opt_v / dynamics / update_state of dynamics.py, state by
    state: the controls exactly, an RK4 step within 4 ulp (NumPy's array sin / cos against its scalar ones)."""
    g, og = XC.grids(name)
    sys_, par = XC.system(name, g), XC.PLANT_PAR[name]
    controls, f, nd = R.PLANTS[name]
    rng = np.random.default_rng(2)
    Xs, P = rng.standard_normal((40, nd)), rng.standard_normal((40, nd))
    P[0, :] = 0.0                                            # sgn(0) = +1
    P[1, :] = np.nan
    for uMode, dMode in (('max', 'min'), ('min', 'max')):
        c0, c1, sw = controls(par, P, Xs, uMode, dMode)
        step = R.rk4(lambda Z: f(par, Z, c0, c1), Xs, 0.05)
        for m in range(40):
            u = sys_.get_opt_u(0.0, P[m], uMode, Xs[m])
            d = sys_.get_opt_v(0.0, P[m], dMode, Xs[m])
            mine = (c0[m], c1[m]) if name == "plane5d" else c0[m]
            assert np.array_equal(np.asarray(u, dtype=np.float64), np.asarray(mine), equal_nan=True), (m, u, mine)
            assert d is None if name == "plane5d" else np.array_equal(d, c1[m], equal_nan=True)
            if m != 1:
                x1 = sys_.update_state(u, 0.05, Xs[m], d)
                assert np.max(np.abs(x1 - step[m])) <= 4 * np.spacing(np.max(np.abs(step[m]))), m
