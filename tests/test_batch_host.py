"""CPU-only: the host side of HJIPDE_solve_batch (levelsetpy_amd/batch.py, include/hj_batch.h) -- no device is touched.

  * the schedule planner against the oracle's odeCFL3 driven by HJIPDE_solve's time loop, times compared with ==, and
    hjb_plan (the same loop in C) against the planner;
  * the structs and enums of _bffi against the header, the census of the built library (the binding itself against the header
    and the export table: tests/test_tool_libs_host.py);
  * the eligibility rule: every disqualifier selects the host loop, with its reason.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import levelsetpy_amd as L
from levelsetpy_amd import _bffi, _ffi, batch
from oracle import hj_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 1e-4            # HJIPDE_solve's (hji_solver.py:185)

# a bound that needs several steps per interval, one whose first step overshoots the short interval (one clipped step),
# and one in between whose last step of an interval is a short remainder
BOUNDS = [0.0137, 0.31, 0.0521]
TAU = [0.0, 0.05, 0.11, 0.3]


def oracle_times(sb, tau, factor=0.8):
    """Per interval, the times HJIPDE_solve's loop passes through with the oracle's odeCFL3 and a term of step bound sb."""
    term = lambda t, y: (np.zeros_like(y), sb)          # noqa: E731
    y = np.zeros((4, 1))
    out = []
    for i in range(1, len(tau)):
        tNow, row = tau[i - 1], []
        while tNow < tau[i] - SMALL:                    # hji_solver.py:536
            tNow, y = O.ode_cfl_3(term, [tNow, tau[i]], y, factor, single_step=True)
            row.append(float(tNow))
        out.append(row)
    return out


def test_planner_equals_the_oracle_time_loop():
    times, steps = batch.plan_schedule(BOUNDS, TAU)
    assert steps.shape == (3, 3)
    for b, sb in enumerate(BOUNDS):
        ref = oracle_times(sb, TAU)
        assert [len(r) for r in ref] == list(steps[b])
        for i in range(3):
            assert times[b][i] == ref[i], (b, i, times[b][i], ref[i])        # ==, not close
    # the three bounds really differ in their step counts, and one interval is a single clipped step
    assert len({tuple(r) for r in steps}) == 3 and steps[1, 0] == 1 and steps.max() >= 4
    # the last stamp of every interval is the interval's end up to the stop tolerance
    for b in range(3):
        for i in range(3):
            assert TAU[i + 1] - SMALL <= times[b][i][-1] <= TAU[i + 1]


def test_planner_orders_and_integrator_loop():
    """Orders 1 and 2 use odeCFL1 / odeCFL2's time expressions; stop_tol < 0 is the integrators' own loop."""
    for order, ode in ((1, O.ode_cfl_1), (2, O.ode_cfl_2), (3, O.ode_cfl_3)):
        sb = 0.0137
        term = lambda t, y: (np.zeros_like(y), sb)      # noqa: E731
        t, ref = 0.1, []
        while 0.2 - t >= 100 * np.finfo(float).eps * 0.2:
            t, _ = ode(term, [t, 0.2], np.zeros((2, 1)), 0.7, single_step=True)
            ref.append(float(t))
        dts, ts = batch.plan_interval(sb, 0.1, 0.2, 0.7, stop_tol=-1.0, order=order)
        assert ts == ref and len(dts) == len(ts)
        assert all(dt == min(0.7 * sb, 0.2 - t0) for dt, t0 in zip(dts, [0.1] + ts[:-1]))
    assert batch.plan_interval(0.01, 0.3, 0.3)[0] == []                        # nothing to do: no step, not a step of dt = 0
    assert batch.plan_interval(0.01, 0.3, 0.3 + 0.5 * SMALL)[0] == []
    assert batch.plan_interval(1.0, 0.0, 1.0, maxStep=0.25)[0] == [0.25] * 4
    with pytest.raises(ValueError):
        batch.plan_interval(0.0, 0.0, 1.0)


def test_c_planner_equals_the_python_planner():
    lib = _bffi.lib()
    sb = np.array(BOUNDS)
    for order in (1, 2, 3):
        for i in range(len(TAU) - 1):
            for tol in (SMALL, -1.0):
                t, n = np.zeros(3), np.zeros(3, dtype=np.int64)
                rc = lib.hjb_plan(order, sb.ctypes.data_as(_bffi._pd), 3, TAU[i], TAU[i + 1], 0.8, 1e300, tol,
                                  t.ctypes.data_as(_bffi._pd), n.ctypes.data_as(_bffi._pi64))
                assert rc == 0, lib.hjb_last_error()
                for b in range(3):
                    dts, ts = batch.plan_interval(sb[b], TAU[i], TAU[i + 1], 0.8, 1e300, tol, order)
                    assert n[b] == len(ts) and t[b] == (ts[-1] if ts else TAU[i])
    assert lib.hjb_plan(4, sb.ctypes.data_as(_bffi._pd), 3, 0.0, 1.0, 0.8, 1e300, SMALL, None, None) == -1
    bad = np.array([0.0])
    assert lib.hjb_plan(3, bad.ctypes.data_as(_bffi._pd), 1, 0.0, 1.0, 0.8, 1e300, SMALL, None, None) == -1
    assert b"step bound" in lib.hjb_last_error()


# ------------------------------------------------------------------------------------------ header agreement
def header_text():
    txt = open(os.path.join(ROOT, "include", "hj_batch.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_census_of_the_batch_library():
    """The kernels libhj_batch.so ships: the 18 instantiations of batch_substep_kernel (2 types x 3 systems x 3 schemes, each named
    by _bffi.kernel_name and launched by tests/test_gpu_batch.py::test_every_instantiation_equals_hj_rk_substep), the bound kernel
    per (type, system), the NaN kernel per type -- and nothing else."""
    out = subprocess.check_output(["nm", "-D", "-C", _bffi.LIB_PATH]).decode()
    stubs = sorted(set(re.findall(r"__device_stub__(\w+<[^(]*>)\(", out)))
    sub = [s for s in stubs if s.startswith("batch_substep_kernel<")]
    want = {"batch_substep_kernel<%s, hj::%s<%s>, %d>" % (t, h, t, k) for t in ("double", "float") for h in _bffi.HAM_NAMES.values()
            for k in _bffi.SCHEMES}
    assert set(sub) == want and len(want) == 18, sorted(set(sub) ^ want)
    for ham, name in _bffi.HAM_NAMES.items():
        for dt, t in (("float64", "double"), ("float32", "float")):
            for k in _bffi.SCHEMES:
                assert _bffi.kernel_name(dt, ham, k) == "batch_substep_kernel<%s, %s, %d>" % (t, name, k)
    rest = [s for s in stubs if not s.startswith("batch_substep_kernel<")]
    assert len([s for s in rest if s.startswith("batch_bound_kernel<")]) == 6 and len([s for s in rest if s.startswith("batch_nan_kernel<")]) == 2
    assert len(rest) == 8, rest


def test_structs_and_enums_match_the_header():
    txt = header_text()
    assert int(re.search(r"#define HJB_PAR_SLOTS (\d+)", txt).group(1)) == _bffi.PAR_SLOTS
    for name, val in (("HJB_ARR_NONE", _bffi.ARR_NONE), ("HJB_ARR_MIN", _bffi.ARR_MIN), ("HJB_ARR_MAX", _bffi.ARR_MAX),
                      ("HJB_ARR_MAX_NEG", _bffi.ARR_MAX_NEG)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, txt).group(1)) == val
    # field order of the three structs
    for struct, fields in (("hjb_entry", list(_bffi.ENTRY.names)), ("hjb_problem", [f[0] for f in _bffi.Problem._fields_]),
                           ("hjb_tables", [f[0] for f in _bffi.Tables._fields_])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first = re.sub(r"^(const\s+)?(void\*|double|int32_t)\s*", "", decl)
                names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in first.split(",")]
        assert names == fields, (struct, names, fields)
    assert _bffi.ENTRY.itemsize == 64 and C.sizeof(_bffi.Problem) == 56 and C.sizeof(_bffi.Tables) == 64


# ------------------------------------------------------------------------------------------ eligibility
def grid3(n=(13, 11, 9)):
    return L.createGrid(np.array([[-.75, -1.25, -np.pi]]).T, np.array([[3.25, 1.25, np.pi * (1 - 2 / n[2])]]).T,
                        np.array(n, dtype=np.int64).reshape(-1, 1), 2)


def sd_of(g, s, fn=None):
    d = dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation)
    if fn is not None:
        d["derivFunc"] = fn
    return L.Bundle(d)


def setup(B=3, fn=L.upwindFirstENO2):
    g = grid3()
    sds = [sd_of(g, L.DubinsVehicleRel(g, 1 + .25 * b, 1), fn) for b in range(B)]
    return g, sds, np.zeros((B,) + tuple(g.shape))


def test_eligible_batch_is_classified_for_the_device():
    g, sds, d0 = setup()
    st, why = batch.classify(d0, sds)
    assert why is None and st.grid is g and st.ham == _ffi.HAM_DUBINS_REL and st.scheme == _ffi.ENO2
    assert [p[:4] for p in st.params] == [[1 + .25 * b, 1 + .25 * b, 1.0, 2.0] for b in range(3)] and all(len(p) == 8 for p in st.params)
    # the default derivative function is the as-shipped WENO5, as in HJIPDE_solve
    g, sds, d0 = setup(fn=None)
    st, why = batch.classify(d0, sds)
    assert why is None and st.scheme == _ffi.WENO5_ASSHIPPED
    # an equal grid built twice is one grid; every accepted compMethod
    g2 = grid3()
    sds[1] = sd_of(g2, L.DubinsVehicleRel(g2, 2, 1))
    for comp in (None, 'none', 'set', 'minVOverTime', 'maxVOverTime', 'minVWithV0', 'maxVWithV0', 'minVWithL', 'maxVWithL',
                 'minVWithTarget', 'maxVWithTarget'):
        args = L.Bundle(dict(keepLast=True, quiet=True, targetFunction=d0, obstacleFunction=d0[0]))
        assert batch.classify(d0, sds, comp, args)[1] is None, comp


class _Sub(L.DubinsVehicleRel):
    def hamiltonian(self, t, data, value_derivs, finite_diff_bundle=None):
        return L.DubinsVehicleRel.hamiltonian(self, t, data, value_derivs, finite_diff_bundle)


def disqualifiers():
    def other_grid(g, sds, d0):
        g2 = grid3((13, 11, 10))
        sds[1] = sd_of(g2, L.DubinsVehicleRel(g2, 1, 1), L.upwindFirstENO2)

    def other_bc(g, sds, d0):
        g2 = L.createGrid(g.min, g.max, g.N, None)
        sds[2] = sd_of(g2, L.DubinsVehicleRel(g2, 1, 1), L.upwindFirstENO2)

    def foreign(g, sds, d0):
        s = L.DubinsVehicleRel(g, 1, 1)
        sds[0] = L.Bundle(dict(grid=g, hamFunc=lambda *a: s.hamiltonian(*a), partialFunc=s.dissipation, derivFunc=L.upwindFirstENO2))

    def subclass(g, sds, d0):
        sds[1] = sd_of(g, _Sub(g, 1, 1), L.upwindFirstENO2)

    def mixed_systems(g, sds, d0):
        a, b = L.DubinsVehicleRel(g, 1, 1), L.DubinsVehicleRel(g, 2, 1)
        sds[0] = L.Bundle(dict(grid=g, hamFunc=a.hamiltonian, partialFunc=b.dissipation, derivFunc=L.upwindFirstENO2))

    def deriv(fn):
        def f(g, sds, d0):
            sds[2].derivFunc = fn
        return f

    def llf(g, sds, d0):
        sds[1].dissFunc = L.artificialDissipationLLF

    return [
        ("another grid", other_grid, None, {}, "another grid"),
        ("another boundary", other_bc, None, {}, "another grid"),
        ("foreign callbacks", foreign, None, {}, "not the methods of a built-in system"),
        ("subclass", subclass, None, {}, "not the methods of a built-in system"),
        ("two objects", mixed_systems, None, {}, "not the methods of a built-in system"),
        ("intended WENO5", deriv(L.upwindFirstWENO5Intended), None, {}, "intended WENO5"),
        ("foreign derivative", deriv(lambda g, d, i: None), None, {}, "derivative function"),
        ("mixed schemes", deriv(L.upwindFirstENO3), None, {}, "another derivative function"),
        ("local dissipation", llf, None, {}, "artificialDissipationGLF"),
        ("compMethod", None, "minWithZero", {}, "compMethod"),
        ("unknown compMethod", None, "median", {}, "compMethod"),
        ("stopInit", None, None, dict(stopInit=np.zeros(3)), "stopping condition"),
        ("stopConverge", None, None, dict(stopConverge=True), "stopping condition"),
        ("stopSetInclude", None, None, dict(stopSetInclude=np.zeros((13, 11, 9))), "stopping condition"),
        ("discount", None, "minVWithL", dict(discountFactor=0.9, targetFunction=np.zeros((13, 11, 9))), "discounting"),
        ("SDModFunc", None, None, dict(SDModFunc=lambda *a: a[0]), "SDModFunc"),
        ("computeTTR", None, None, dict(computeTTR=True), "computeTTR"),
        ("timed target", None, "minVWithL", dict(targetFunction=np.zeros((3, 2, 13, 11, 9))), "varies in time"),
        ("timed obstacle", None, None, dict(obstacleFunction=np.zeros((3, 2, 13, 11, 9))), "varies in time"),
        ("history", None, None, dict(_history=True), "time history"),
    ]


@pytest.mark.parametrize("case", disqualifiers(), ids=lambda c: c[0])
def test_each_disqualifier_selects_the_host_loop(case):
    name, change, comp, args, word = case
    g, sds, d0 = setup()
    if change is not None:
        change(g, sds, d0)
    if args.pop("_history", False):
        d0 = np.zeros((3, 2) + tuple(g.shape))
    st, why = batch.classify(d0, sds, comp, L.Bundle(dict(args)))
    assert st is None and word in why, (name, why)


def test_weno5_mode_and_registered_hamiltonians_disqualify():
    g, sds, d0 = setup(fn=L.upwindFirstWENO5)
    assert batch.classify(d0, sds)[1] is None
    L.set_weno5_mode("weno5")
    try:
        assert "intended WENO5" in batch.classify(d0, sds)[1]
    finally:
        L.set_weno5_mode("asshipped")
    L.set_eno_mode("fast")
    try:
        g, sds, d0 = setup(fn=L.upwindFirstENO3)
        assert "no batched kernel" in batch.classify(d0, sds)[1]
    finally:
        L.set_eno_mode("exact")
    # a 2-D system on the 3-D grid has no kernel there
    g, sds, d0 = setup()
    s = L.DoubleIntegrator(g, 1)
    assert batch.classify(d0, [sd_of(g, s, L.upwindFirstENO2)] * 3)[1] is not None


def test_front_end_argument_errors_need_no_device():
    g, sds, d0 = setup()
    with pytest.raises(ValueError, match="tau"):
        L.HJIPDE_solve_batch(d0, [0.0], sds)
    with pytest.raises(ValueError, match="holds 3 problems"):
        L.HJIPDE_solve_batch(d0, [0.0, 0.1], sds[:2])
    with pytest.raises(ValueError, match="systems"):
        L.HJIPDE_solve_batch(d0, [0.0, 0.1], sds[0])
    with pytest.raises(ValueError, match="one array per problem"):
        L.HJIPDE_solve_batch(d0, [0.0, 0.1], sds, 'minVWithL', L.Bundle(dict(targetFunction=np.zeros((2,) + tuple(g.shape)))))
    with pytest.raises(ValueError, match="array size"):
        L.HJIPDE_solve_batch(d0[:, :-1], [0.0, 0.1], sds)
