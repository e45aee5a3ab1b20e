"""CPU-only: libhj_filter.so without a device (levelsetpy_amd/_fffi.py, include/hj_filter.h).

  * the header, the binding and the export table name the same functions and enums; the kernel stubs are the two families;
  * the Makefile builds the library under both goals;
  * every refusal row of tests/filter_cases.py returns its code with its text and leaves the sentinel-filled outputs untouched:
    every check comes before the first HIP call, so host arrays stand in for the device's;
  * the front end refuses before it asks for a device;
  * the trajectory, the plants and the decision have one source each.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_cases as FC  # noqa: E402
import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import computeSafeTrajs, safeControls  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _ffi, _fffi, safety  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "levelsetpy_amd", "csrc")


def test_binding_header_and_exports_name_the_same_functions():
    txt = open(os.path.join(ROOT, "include", "hj_filter.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    declared = sorted(set(re.findall(r"\b(hjf_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_fffi.SIGNATURES) == ["hjf_decide", "hjf_last_error", "hjf_last_kernel", "hjf_rollout"]
    out = subprocess.check_output(["nm", "-D", _fffi.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (hjf_[a-z0-9_]+)", out))) == declared
    for name, (_, args) in _fffi.SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).strip()
        assert (0 if decl in ("", "void") else decl.count(",") + 1) == len(args), name
    enums = dict(HJF_SAFE=_fffi.SAFE, HJF_VIOLATED=_fffi.VIOLATED, HJF_LEFT_GRID=_fffi.LEFT_GRID, HJF_NOMINAL_TABLE=_fffi.NOMINAL_TABLE,
                 HJF_NOMINAL_VALUE=_fffi.NOMINAL_VALUE, HJF_SLICE_CLOCK=_fffi.SLICE_CLOCK, HJF_SLICE_STATIC=_fffi.SLICE_STATIC,
                 HJF_DSTB_WORST=_fffi.DSTB_WORST, HJF_DSTB_ZERO=_fffi.DSTB_ZERO)
    assert sorted(set(re.findall(r"\b(HJF_[A-Z_]+)\s*=", code))) == sorted(enums)
    for name, val in enums.items():
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == val, name
    assert (safety.SAFE, safety.VIOLATED, safety.LEFT_GRID) == (0, 1, 2)
    # the table of controls: the header's, the device traits' and the binding's
    dev = open(os.path.join(CSRC, "hj_filter_dev.h")).read()
    for ham, nu in (("HJ_HAM_DUBINS_REL", 1), ("HJ_HAM_DOUBLE_INTEGRATOR", 1), ("HJ_HAM_DOUBLE_PENDULUM", 2)):
        assert int(re.search(r"struct Held<%s> \{[^}]*NU = (\d)" % ham, dev).group(1)) == nu == _fffi.PLANT_NU[getattr(_ffi, ham[3:])]


def test_the_kernel_stubs_are_the_two_families():
    out = subprocess.check_output(["nm", "-D", "-C", _fffi.LIB_PATH]).decode()
    assert set(re.findall(r"__device_stub__(\w+)", out)) == {"filtered_rollout_kernel", "decide_points_kernel"}
    full = set(re.findall(r"__device_stub__(\w+<[^>]*>)\(", out))
    want = set("%s<%s, %d, %d>" % (k, t, s, p) for k in ("filtered_rollout_kernel", "decide_points_kernel") for t in ("double", "float")
               for s in (0, 1, 3) for p in (0, 1, 2))
    assert full == want and len(full) == 36


def test_the_makefile_builds_the_library_and_the_trajectory_has_one_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^libhj_filter\.so: hj_filter\.hip hj_filter_dev\.h hj_tool_host\.h hj_query_dev\.h hj_rollout_dev\.h hj_plants_dev\.h", mk, re.M)
    assert re.search(r"^resource-usage-filter:.*\n\t.*-Rpass-analysis=kernel-resource-usage .*hj_filter\.hip$", mk, re.M)
    assert re.search(r"^\trm -f .*\blibhj_filter\.so\b", mk, re.M) and "libhj_filter.so" in mk.split("\n")[0]
    assert "hj_filter.hip" in mk.split("HIPCC ?=")[0]
    for goal in ([], ["libs"]):
        out = subprocess.check_output(["make", "-C", CSRC, "-n", "-B"] + goal).decode()
        assert "-o libhj_filter.so hj_filter.hip" in out and "-o libhj_mc.so hj_mc.hip" in out
    needed = subprocess.check_output(["readelf", "-d", _fffi.LIB_PATH]).decode()
    assert "libhj_" not in needed.replace("libhj_filter.so", "")
    src = lambda n: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, n)).read())      # noqa: E731
    hip, dev, body = src("hj_filter.hip"), src("hj_filter_dev.h"), open(os.path.join(CSRC, "hj_rollout_dev.h")).read()
    # one trajectory: both kernels are rollout_body around FilterHooks, which NoHooks and NoisyHooks do not know of
    assert hip.count("hjr::rollout_body<") == 2 and hip.count("FilterHooks<T, PLANT,") == 2
    assert "struct NoHooks { static constexpr bool plain = true; };" in body and "Filter" not in src("hj_mc_dev.h")
    assert "struct filter_of" in body and body.count("filter_of<HK>::") == 3
    # one set of plants, one decision, one set of point queries
    assert "struct Plant<" not in hip + dev and open(os.path.join(CSRC, "hj_plants_dev.h")).read().count("template <> struct Plant<") == 3
    assert len(re.findall(r"__device__ __forceinline__ bool decide\(", dev)) == 1 and dev.count("hjf::decide<PLANT>(") == 2
    for fn in ("locate(", "corner(", "gather_axis", "group_sum", "UP::template lr"):
        assert fn not in hip + dev, fn
    assert "nmin(" in dev and "double nmin" not in dev                      # hj_mc_dev.h's
    for word in ("atomic", "__shared__", "__shfl", "__syncthreads"):
        assert word not in hip + dev, word
    # each refusal's text stands once
    for text in ("split over states", "must not be NaN", "no filter kernel", "level must be finite", "is neither HJF_DSTB_WORST"):
        assert hip.count(text) == 1, text


def _check_rows(call, rows, last_error):
    lib = _fffi.lib()
    f64, i32, u8, ins = FC.arrays()
    before = {k: v.copy() for k, v in ins.items()}
    for kw, code, word in rows:
        rc = call(lib, f64, i32, u8, ins, **kw)
        assert rc == code, (kw, rc, last_error())
        assert word in last_error(), (kw, last_error())
        assert FC.untouched(f64, i32, u8), kw
    assert all(np.array_equal(before[k], ins[k]) for k in ins)
    return lib, f64, i32, u8, ins


def test_rollout_refusals_touch_nothing():
    lib, f64, i32, u8, ins = _check_rows(FC.rollout_call, FC.ROLLOUT_ROWS, lambda: _fffi.lib().hjf_last_error())
    with pytest.raises(_ffi.Unsupported):
        _fffi.check(FC.rollout_call(lib, f64, i32, u8, ins, scheme=_ffi.WENO5))
    with pytest.raises(ValueError):
        _fffi.check(FC.rollout_call(lib, f64, i32, u8, ins, margin=FC.NAN))
    # nothing to do: fine whatever the optional arrays, and launches nothing
    assert FC.rollout_call(lib, f64, i32, u8, ins, M=0) == 0 and _fffi.last_kernel() == ""
    assert FC.rollout_call(lib, f64, i32, u8, ins, M=0, margin=FC.INF, traj=None, active=None, applied=None) == 0
    assert FC.rollout_call(lib, f64, i32, u8, ins, M=0, policy=_fffi.SLICE_STATIC, stride=0) == 0
    assert FC.untouched(f64, i32, u8)


def test_decide_refusals_touch_nothing():
    lib, f64, i32, u8, ins = _check_rows(FC.decide_call, FC.DECIDE_ROWS, lambda: _fffi.lib().hjf_last_error())
    assert FC.decide_call(lib, f64, i32, u8, ins, M=0) == 0 and _fffi.last_kernel() == ""
    assert FC.decide_call(lib, f64, i32, u8, ins, M=0, costate=None, margin=-FC.INF) == 0
    assert FC.untouched(f64, i32, u8)


def test_the_front_end_refuses_before_it_asks_for_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    for name in ("require_gpu", "_device_data", "_device_states"):
        monkeypatch.setattr(safety, name, no_device)
    g = L.createGrid(np.array([[-1.], [-1.]]), np.array([[1.], [1.]]), np.array([[9], [9]]), None)
    g3 = L.createGrid(-np.ones((3, 1)), np.ones((3, 1)), 9 * np.ones((3, 1), dtype=np.int64), None)
    tau = np.linspace(0, 0.3, 4)
    data, xs, table = np.zeros((4, 9, 9)), np.zeros((5, 2)), np.zeros((5, 3, 1))
    di = L.DoubleIntegrator(g, 1)
    B = lambda **kw: L.Bundle(kw)                                           # noqa: E731
    bad = [
        (data, tau[:-1], xs, table, None),                                  # one time stamp short
        (data, tau[::-1], xs, table, None),                                 # descending
        (data, tau, np.zeros((5, 3)), table, None),                         # states of another dimension
        (data, tau, xs, np.zeros((5, 2, 1)), None),                         # a table of another horizon
        (data, tau, xs, np.zeros((4, 3, 1)), None),                         # ... of other states
        (data, tau, xs, np.zeros((5, 3, 2)), None),                         # ... of two controls for a plant with one
        (data, tau, xs, table, B(uMode='up')),
        (data, tau, xs, table, B(dMode='down')),
        (data, tau, xs, table, B(subSamples=0)),
        (data, tau, xs, table, B(margin=float("nan"))),
        (data, tau, xs, table, B(margin='wide')),
        (data, tau, xs, table, B(level=float("inf"))),
        (data, tau, xs, table, B(policy='earliest')),
        (data, tau, xs, table, B(disturbance='none')),
        (data, tau, xs, table, B(policy='static', slice=4)),
        (data, tau, xs, table, B(policy='static', slice=-1)),
        (data[0], tau, xs, table, None),                                    # one field under the clock
        (data[0], tau, xs, table, B(policy='clock')),
        (data[0], tau, xs, table, B(policy='static', slice=1)),
        (data, tau, xs, B(data=np.zeros((4, 9, 8))), None),                 # a nominal stack on another grid
        (data, tau, xs, B(data=np.zeros((3, 9, 9))), None),
        (data, tau, xs, B(data=data, uMode='up'), None),
        (data, tau, xs, B(uMode='min'), None),
    ]
    for d, t, x, nominal, args in bad:
        with pytest.raises(ValueError):
            computeSafeTrajs(g, d, t, di, x, nominal, args)
    with pytest.raises(ValueError):
        computeSafeTrajs(g3, np.zeros((4, 9, 9, 8)), tau, di, np.zeros((5, 3)), np.zeros((5, 3, 1)), None)   # a stack on another grid
    for d, x, u, args in ((data, xs, np.zeros((5, 1)), B(slice=4)), (data[0], xs, np.zeros((5, 1)), B(slice=1)),
                          (data[0], xs, np.zeros((4, 1)), None), (data[0], xs, np.zeros((5, 2)), None),
                          (data[0], np.zeros((5, 3)), np.zeros((5, 1)), None), (data[0], xs, np.zeros((5, 1)), B(margin=float("nan"))),
                          (np.zeros((9, 8)), xs, np.zeros((5, 1)), None)):
        with pytest.raises(ValueError):
            safeControls(g, d, di, x, u, args)
    assert safety.LAUNCH_THREADS == 2 ** 32 - 256 and callable(safety.last_path)
