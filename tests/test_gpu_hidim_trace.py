"""GPU tests of Python callbacks traced into hidim_substep_kernel on 5-D / 6-D grids (levelsetpy_amd/trace_ham.py behind set_hidim_trace; the
pairs are tests/hidim_trace_cases.py's, grids and data tests/hidim_cases.py's and tests/hidim_user_cases.py's).

  1. term parity: termLaxFriedrichs of each stored-table pair (and of the Dubins pair, whose tables the tracer hoists) with the switch on
     against the split path of the same callbacks and against the built-in / hand-registered kernel: ENO2 / ENO3 array_equal in fp64 and
     fp32, stepBound ==; the as-shipped WENO5 within 1e-11 of the oracle (fp32: _fp32_close of tests/test_gpu_fp32.py)
  2. hoisted trig: the quadrotor with np.sin / np.cos inside the callbacks against the NumPy oracle driven by the same callbacks
  3. HJIPDE_solve over two tau intervals, switch on against switch off: minVOverTime, a target with an obstacle, NumPy and tensor input, a
     low_mem grid
  4. a speed and a stored table changed in place between two solves (nothing compiled); two traced systems on one grid
  5. a pair whose hamFunc changes behind the tracer's back is dropped with a warning; a pair that reads data or t keeps the split path
  6. a fresh child process loads the traced kernels from the disk cache
  7. guarded buffers (tests/guarded_pool.py): the traced fused term and a traced hjh_integrate interval, 5-D and 6-D
  8. switch off: the same calls take the split path
"""
import ctypes as C
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _hffi, hidim, term  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402
import guarded_pool as GP  # noqa: E402
import hidim_cases as HC  # noqa: E402
import hidim_trace_cases as TC  # noqa: E402
import hidim_user_cases as UC  # noqa: E402
from test_gpu_fp32 import _fp32_close  # noqa: E402
from test_gpu_hidim import DERIV, SID, SMALL, Case, arr, case, close, dev, pool  # noqa: E402
from test_gpu_hidim_user import quad  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENO = ["ENO2", "ENO3"]
OFF_WHY = 'hamFunc / partialFunc are not the methods of Plane5D / DubinsPair6D or of a system registered with register_hidim_hamiltonian'


@pytest.fixture
def switch_on():
    prev = L.set_hidim_trace(True)
    yield
    L.set_hidim_trace(prev)


def bundle(g, s, scheme):
    return L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=DERIV[scheme]))


class Traced(object):
    """A case of tests/test_gpu_hidim.py / test_gpu_hidim_user.py (.c: grid, data, oracle, the built-in or hand-registered system) with the
    same system written as callbacks only (.s)."""

    def __init__(self, name):
        self.name, self._oracle = name, {}
        if name == "plane":
            self.c = case("plane5d")
            self.s = TC.PlanePair(self.c.g, **HC.PARAMS["plane5d"])
            self.ref_sd = self.c.sd
        elif name == "dubins":
            self.c = case("pair6d")
            self.s = TC.DubinsPair(self.c.g, **HC.PARAMS["pair6d"])
            self.ref_sd = self.c.sd
        else:
            self.c = quad()
            self.s = (TC.QuadTables if name == "quad_tables" else TC.QuadInline)(self.c.g, UC.QUAD_PAR)
            src, axes, par = TC.quad_hand_registration()
            reg = L.register_hidim_hamiltonian("planar_quad_as_the_callbacks", 6, src, nparams=8, aux_axes=axes)
            q = TC.QuadTables(self.c.g, UC.QUAD_PAR)
            self.hand = reg(self.c.g, par, tables=[t.ravel() for t in (q.cos4, q.sin4, q.u1, q.u3)])
            self.ref_sd = lambda scheme: bundle(self.c.g, self.hand, scheme)
        self.g, self.data, self.shape = self.c.g, self.c.data, self.c.shape

    def sd(self, scheme):
        return bundle(self.g, self.s, scheme)

    def oracle(self, scheme, dtype="float64"):
        """(ydot, stepBound) of the oracle on the data rounded to `dtype`, computed once."""
        if (scheme, dtype) not in self._oracle:
            d = self.data if dtype == "float64" else self.data.astype(np.float32).astype(np.float64)
            ydot, sb = O.term_lax_friedrichs(self.c.og, self.c.osys, scheme, 0.0, d.reshape(-1))
            self._oracle[(scheme, dtype)] = (ydot.reshape(self.shape), sb)
        return self._oracle[(scheme, dtype)]


_traced = {}


def traced(name):
    if name not in _traced:
        _traced[name] = Traced(name)
    return _traced[name]


def lf(sd, y):
    yd, sb, _ = L.termLaxFriedrichs(0.0, y, sd)
    return (yd.cpu().numpy() if torch.is_tensor(yd) else np.asarray(yd)).reshape(-1), sb, hidim.last_path()


def traced_path(dtype, scheme):
    return r"hidim_substep_kernel<%s, HamUser:traced_[0-9a-f]{12}, %d>" % ("double" if dtype == "float64" else "float", SID[scheme])


# ------------------------------------------------------------------------------------------ 1. term parity
@pytest.mark.parametrize("scheme", ENO)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["plane", "dubins", "quad_tables"])
def test_traced_term_equals_the_split_path_and_the_native_kernel(name, dtype, scheme):
    import re
    t = traced(name)
    y = dev(t.data, dtype).reshape(-1, 1)
    assert L.get_hidim_trace() is False
    split, sb_s, p_s = lf(t.sd(scheme), y)
    assert "HamUser" not in p_s and "substep" not in p_s
    native, sb_n, p_n = lf(t.ref_sd(scheme), y)
    assert p_n.startswith("hidim_substep_kernel<") and "traced_" not in p_n
    prev = L.set_hidim_trace(True)
    try:
        got, sb_t, p_t = lf(t.sd(scheme), y)
    finally:
        L.set_hidim_trace(prev)
    assert re.fullmatch(traced_path(dtype, scheme), p_t), p_t
    print("%s %s %s: %d cells differ from the split path, %d from the native kernel; stepBound %.17g / %.17g / %.17g"
          % (name, dtype, scheme, int(np.sum(got != split)), int(np.sum(got != native)), sb_t, sb_s, sb_n))
    assert not np.isnan(got).any() and np.array_equal(got, split) and np.array_equal(got, native)
    # stepBound: the traced system's is hidim_bound_kernel's, as the native system's: ==.  The split path reduces alpha over arrays of the
    # caller's type: == in fp64; in fp32 its bound differs from ANY fused kernel's in the last fp32 bits (the built-in's does by as much:
    # 0.0730125522 against 0.0730125515 on the 5-D case), so there the fp32 tests' rule for the bound applies (tests/test_gpu_hidim.py: 1e-5)
    assert sb_t == sb_n
    assert sb_t == sb_s if dtype == "float64" else abs(sb_t - sb_s) <= 1e-5 * sb_s
    if name == "quad_tables" and dtype == "float64":
        # the expression written by hand for tests/test_gpu_hidim_user.py divides Cv / m in the element type: the same number in fp64
        hand, sb_h, _ = lf(t.c.sd(scheme), y)
        assert np.array_equal(got, hand) and sb_t == sb_h


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["plane", "dubins", "quad_tables"])
def test_traced_weno5_is_within_the_suites_bound_of_the_oracle(name, dtype, switch_on):
    t = traced(name)
    ydot, sb = t.oracle("WENO5_ASSHIPPED", dtype)
    got, sb_t, p_t = lf(t.sd("WENO5_ASSHIPPED"), dev(t.data, dtype).reshape(-1, 1))
    assert "HamUser:traced_" in p_t
    if dtype == "float64":
        close(got, ydot, "WENO5_ASSHIPPED", name)
        assert abs(sb_t - sb) <= 1e-11 * max(1.0, sb)
    else:
        _fp32_close(got.reshape(t.shape), ydot, "WENO5_ASSHIPPED", name)
        assert abs(sb_t - sb) <= 1e-5 * sb


# ------------------------------------------------------------------------------------------ 2. hoisted trig
@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
def test_hoisted_trig_equals_the_numpy_oracle(scheme, switch_on):
    """np.sin(grid.xs[4]) / np.cos(grid.xs[4]) inside the callbacks: tables NumPy makes from grid.vs[4], so the kernel computes with the
    numbers the callbacks compute with under NumPy."""
    t = traced("quad_inline")
    osys = TC.QuadInline(t.c.og, UC.QUAD_PAR)                    # the same callbacks on the oracle's grid, on NumPy arrays
    ydot, sb = O.term_lax_friedrichs(t.c.og, osys, scheme, 0.0, t.data.reshape(-1))
    got, sb_t, p_t = lf(t.sd(scheme), t.data.reshape(-1, 1))                                          # NumPy in
    assert "HamUser:traced_" in p_t
    e = L.explain_plan(t.sd(scheme))
    assert e["path"] == "traced" and e["hoisted"] == [(4, "sin(x[4])"), (4, "cos(x[4])")] and "sin(" not in e["source"] and "cos(" not in e["source"]
    close(got, ydot, scheme, "quadrotor, trig inside the callbacks")
    if scheme.startswith("ENO"):
        assert sb_t == sb
    else:
        assert abs(sb_t - sb) <= 1e-11 * max(1.0, sb)


# ------------------------------------------------------------------------------------------ 3. solve parity
def solve(t, s, comp, tensors, g=None, **extra):
    """(data, tau, path) of HJIPDE_solve over two tau intervals (two steps, then one) with the callbacks of s."""
    g = t.g if g is None else g
    sb = t.oracle("ENO2")[1]
    tau = np.array([0.0, 1.2 * 0.8 * sb, 1.9 * 0.8 * sb])
    args = dict(quiet=True, **extra)
    if comp == "minVWithL":
        x = t.c.og.xs
        args.update(targetFunction=np.sqrt((x[0] - 0.5) ** 2 + x[2] ** 2 + 0.02) - 0.8 + 0 * t.data,
                    obstacleFunction=np.sqrt((x[0] + 1.0) ** 2 + (x[2] - 0.5) ** 2 + 0.02) - 0.4 + 0 * t.data)
    data, tout, outs = L.HJIPDE_solve(dev(t.data) if tensors else t.data, tau, bundle(g, s, "ENO2"), comp, L.Bundle(args))
    assert outs.path == hidim.last_path()
    assert torch.is_tensor(data) == tensors
    return (data.cpu().numpy() if tensors else np.asarray(data)), np.asarray(tout), outs.path


@pytest.mark.parametrize("name,comp,tensors", [("plane", "minVOverTime", False), ("quad_tables", "minVWithL", True), ("dubins", "minVOverTime", True)])
def test_solve_with_the_switch_on_equals_the_switch_off(name, comp, tensors):
    import re
    t = traced(name)
    off, tau_off, p_off = solve(t, t.s, comp, tensors)
    assert p_off == "split: " + OFF_WHY
    prev = L.set_hidim_trace(True)
    try:
        on, tau_on, p_on = solve(t, t.s, comp, tensors)
    finally:
        L.set_hidim_trace(prev)
    assert re.fullmatch(traced_path("float64", "ENO2"), p_on), p_on
    assert on.shape == (3,) + t.shape and np.array_equal(tau_on, tau_off) and not np.isnan(on).any()
    print("%s %s: %d cells differ" % (name, comp, int(np.sum(on != off))))
    assert np.array_equal(on, off)
    assert not np.array_equal(on[1], on[0]) and not np.array_equal(on[2], on[1])


def test_solve_on_a_low_mem_grid(switch_on):
    import re
    t = traced("plane")
    lm = Case("plane5d", low_mem=True)
    assert lm.g.xs[0].shape != lm.shape                         # sparse xs
    s = TC.PlanePair(lm.g, **HC.PARAMS["plane5d"])
    on, _, p_on = solve(t, s, "minVOverTime", False, g=lm.g, keepLast=True)
    assert re.fullmatch(traced_path("float64", "ENO2"), p_on), p_on
    L.set_hidim_trace(False)
    off, _, p_off = solve(t, t.s, "minVOverTime", False, keepLast=True)
    assert p_off.startswith("split: ") and np.array_equal(on, off)


# ------------------------------------------------------------------------------------------ 4. state changes
def test_a_speed_and_a_table_changed_in_place():
    t = traced("plane")
    s = TC.PlanePair(t.g, **HC.PARAMS["plane5d"])

    def both():
        L.set_hidim_trace(False)
        off, _, p_off = solve(t, s, "minVOverTime", True, keepLast=True)
        L.set_hidim_trace(True)
        try:
            on, _, p_on = solve(t, s, "minVOverTime", True, keepLast=True)
        finally:
            L.set_hidim_trace(False)
        assert p_off.startswith("split: ") and "HamUser:traced_" in p_on
        assert np.array_equal(on, off)
        return on, p_on
    first, path = both()
    stats = L.hidim_kernel_cache_stats()
    s.a_max = 0.45
    second, path2 = both()
    assert path2 == path and not np.array_equal(second, first)                 # the new result, by the same kernel
    s.cos2[...] = 0.6 * s.cos2
    third, path3 = both()
    assert path3 == path and not np.array_equal(third, second)
    assert L.hidim_kernel_cache_stats() == stats                               # nothing compiled, nothing loaded: parameters and tables are data


def test_two_traced_systems_on_one_grid_keep_their_own_tables(switch_on):
    t = traced("plane")
    a = TC.PlanePair(t.g, **HC.PARAMS["plane5d"])
    b = TC.PlanePair(t.g, **HC.PARAMS["plane5d"])
    b.cos2, b.sin2 = b.sin2.copy(), b.cos2.copy()
    y = dev(t.data).reshape(-1, 1)
    L.set_hidim_trace(False)
    want = [lf(bundle(t.g, s, "ENO3"), y) for s in (a, b)]
    L.set_hidim_trace(True)
    assert not np.array_equal(want[0][0], want[1][0])
    sda, sdb = bundle(t.g, a, "ENO3"), bundle(t.g, b, "ENO3")
    paths = set()
    for _ in range(2):
        for sd, (ydot, sb, _) in ((sda, want[0]), (sdb, want[1])):
            got, sb_t, p = lf(sd, y)
            paths.add(p)
            assert sb_t == sb and np.array_equal(got, ydot)
    assert len(paths) == 1 and "HamUser:traced_" in paths.pop()                # one registration, two systems
    # the built-in system of the same grid still reads the grid's own tables
    got, sb_t, _ = lf(t.c.sd("ENO3"), y)
    assert np.array_equal(got, want[0][0]) and sb_t == want[0][1]


# ------------------------------------------------------------------------------------------ 5. verification
def test_a_pair_that_changes_behind_the_tracers_back_is_dropped():
    t = traced("plane")
    ref = TC.Fickle(t.g, **HC.PARAMS["plane5d"])
    zeros = [np.zeros(t.shape)] * 5
    ref.hamiltonian(0.0, zeros[0], zeros, None)                                # its first call, spent: every later one is what the split path runs
    off, _, p_off = solve(t, ref, "minVOverTime", True, keepLast=True)
    plain, _, _ = solve(t, t.s, "minVOverTime", True, keepLast=True)
    assert p_off.startswith("split: ") and not np.array_equal(off, plain)
    s = TC.Fickle(t.g, **HC.PARAMS["plane5d"])
    prev = L.set_hidim_trace(True)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            on, _, p_on = solve(t, s, "minVOverTime", True, keepLast=True)
    finally:
        L.set_hidim_trace(prev)
    assert any("disagrees with the callbacks" in str(x.message) for x in w), [str(x.message) for x in w]
    assert p_on.startswith("split: ") and "were not traced" in p_on
    assert np.array_equal(on, off)


@pytest.mark.parametrize("cls,word", [(TC.DataReader, "data"), (TC.TimeReader, "time t"), (TC.RangeReader, "costate range")])
def test_untraceable_pairs_keep_the_split_path_with_the_reason(cls, word, switch_on):
    t = traced("plane")
    s = cls(t.g, **HC.PARAMS["plane5d"])
    on, _, p_on = solve(t, s, None, True, keepLast=True)
    assert p_on.startswith("split: " + OFF_WHY + ", and were not traced: the callbacks cannot be traced: ") and word in p_on, p_on
    L.set_hidim_trace(False)
    off, _, p_off = solve(t, s, None, True, keepLast=True)
    assert p_off == "split: " + OFF_WHY and np.array_equal(on, off)


# ------------------------------------------------------------------------------------------ 6. the disk cache
_CACHE_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["HJ_TEST_ROOT"], "tests"))
import levelsetpy_amd as L
import hidim_trace_cases as TC
import hidim_user_cases as UC
gmin, gmax, N, pd = UC.quad_limits()
col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)
g = L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)
s = TC.QuadInline(g, UC.QUAD_PAR)
sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
assert L.get_hidim_trace()
yd, sb, _ = L.termLaxFriedrichs(0.0, UC.quad_data(UC.quad_oracle_grid()).reshape(-1, 1), sd)
print(json.dumps(dict(stats=L.hidim_kernel_cache_stats(), sb=sb, sum=float(np.asarray(yd).sum()), path=L.hidim.last_path(),
                      files=sorted(os.listdir(os.environ["HJ_RTC_CACHE"])))))
"""


def test_a_second_process_finds_the_traced_kernels_in_the_disk_cache(tmp_path):
    """Each process is a fresh child of this one (nothing replaces the program of a process that has opened the GPU); HJ_TRACE_HIDIM=1 turns
    the switch on in it."""
    cache = tmp_path / "rtc"

    def run():
        env = dict(os.environ, HJ_RTC_CACHE=str(cache), HJ_TEST_ROOT=ROOT, HJ_TRACE_HIDIM="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run([sys.executable, "-c", _CACHE_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])
    first = run()
    assert "HamUser:traced_" in first["path"]
    assert first["stats"] == [2, 0] and len(first["files"]) == 2            # the substep and the bound kernel, both compiled
    second = run()
    assert second["stats"] == [0, 2] and second["files"] == first["files"]  # both loaded, nothing compiled
    assert (second["sb"], second["sum"], second["path"]) == (first["sb"], first["sum"], first["path"])


# ------------------------------------------------------------------------------------------ 7. guarded buffers
@pytest.mark.parametrize("name", ["plane", "quad_tables"])
def test_traced_kernels_stay_inside_their_arrays(name, switch_on):
    """The traced fused term (hjh_substep, HJ_STAGE_YDOT with restrict_sign) and a traced hjh_integrate interval (two RK3 steps, max with the
    previous state, an obstacle) on views of tests/guarded_pool.py's pool: guards intact, inputs unchanged, every cell of every output written,
    the same bits as on fresh arrays."""
    t = traced(name)
    dtype = "float64"
    plan = term.native_plan(t.sd("ENO2"), dev(t.data).reshape(-1, 1))         # traced and verified on this data
    assert plan is not None and plan.traced
    system, ham, par = plan.system, plan[2], list(plan[3])
    hg = hidim.hi_grid(t.g, dtype)
    tab = hg.tables_of(system)[0]
    sb = hg.step_bound(ham, par, system)
    other = t.c.other if hasattr(t.c, "other") else UC.quad_data(t.c.og, 8)

    def op_term(F):
        y = F.inp("y", arr(t.data, dtype))
        out = F.out("out", t.shape)
        F.arm()
        hidim._substep(hg, _ffi.ENO2, ham, par, _ffi.STAGE_YDOT, -1, y.view, None, out.view, tab=tab)
        return {"kernel": _hffi.last_kernel()}

    def op_integrate(F):
        y, pb = F.inp("y", arr(t.data, dtype)), F.inp("pb", arr(0.1 - other, dtype))
        a, b, w = F.out("a", t.shape), F.out("b", t.shape), F.out("w", t.shape)
        F.arm()
        tout, n, where = C.c_double(), C.c_int64(), C.c_int32()
        _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(tab), _ffi.ENO2, ham, 3, -1, _ffi.POST_MAX_PREV, _hffi.params(par), sb,
                                         hg.ptr(y.view), hg.ptr(a.view), hg.ptr(b.view), hg.ptr(w.view), 0, None, _hffi.ARR_MAX_NEG, hg.ptr(pb.view),
                                         0.0, 1.5 * 0.8 * sb, 0.8, 1e300, SMALL, C.byref(tout), C.byref(n), C.byref(where), hg.stream()))
        return {"t": tout.value, "n": n.value, "where": where.value}

    ref, _ = GP.run_case(op_term, pool(dtype), offsets=GP.OFFSETS, what=name + " traced term")
    assert ref["kernel"] == _hffi.kernel_name(dtype, ham, _ffi.ENO2) and "HamUser:traced_" in ref["kernel"]
    ref, _ = GP.run_case(op_integrate, pool(dtype), offsets=GP.OFFSETS, what=name + " traced integrate")
    assert (ref["n"], ref["where"]) == (2, 2)


# ------------------------------------------------------------------------------------------ 8. switch off
def test_with_the_switch_off_the_same_calls_take_the_split_path():
    t = traced("quad_tables")
    assert L.get_hidim_trace() is False
    sd = t.sd("ENO3")
    _, _, p = lf(sd, dev(t.data).reshape(-1, 1))
    assert "substep" not in p and term.native_plan(sd, dev(t.data).reshape(-1, 1)) is None
    assert L.explain_plan(sd) == dict(path='split', reason='on a grid of 6 dimensions only Plane5D / DubinsPair6D with artificialDissipationGLF run '
                                                          'fused; the tracer stops at 4-D', library='libhj_hidim.so')
    _, _, p = solve(t, t.s, "minVOverTime", False, keepLast=True)
    assert p == "split: " + OFF_WHY
