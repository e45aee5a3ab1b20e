"""CPU-only: Python callbacks traced into a body for register_hidim_hamiltonian on 5-D / 6-D grids (levelsetpy_amd/trace_ham.py behind
set_hidim_trace; the pairs are tests/hidim_trace_cases.py's).  hipRTC cross-compiles for gfx950 without a device.

  1. the switch: default off, exported, HJ_TRACE_HIDIM sets the initial value, flipping it bumps the attach epoch
  2. the four pairs trace: aux_axes, the tables' values, a body without col[] / hjtab / device trig, evaluate() == the callbacks
  3. a changed speed: the same key, new params; a changed stored table: the same key, new aux_tables
  4. refusals: five stored tables, a range-reading alpha, data, t -- each TraceError names its cause
  5. slot allocation: stored tables first, hoisted values heaviest first, left-overs stay device math, equal tables share a slot;
     HJ_TRACE_HOIST=off leaves the trig on the device
  6. the registration compiles for gfx950 (one ENO and one WENO scheme, fp64 and fp32); its id, name and tables reach the system object
  7. explain_plan: switch off, today's dictionary word for word; switch on, path='traced' with library='libhj_hidim.so'
  8. a dozen seeded random expression pairs at 5-D: evaluate() against the callbacks
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _hffi, term, trace_ham as T  # noqa: E402
from levelsetpy_amd.user_ham import ATTACH_EPOCH  # noqa: E402
import hidim_cases as HC  # noqa: E402
import hidim_trace_cases as TC  # noqa: E402
import hidim_user_cases as UC  # noqa: E402
from test_hidim_host import lgrid  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quad_grid():
    gmin, gmax, N, pd = UC.quad_limits()
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    return L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)


_made = {}


def pair(name):
    """(grid, system) of a case, made once."""
    if name not in _made:
        if name == "plane":
            g = lgrid("plane5d")
            s = TC.PlanePair(g, **HC.PARAMS["plane5d"])
        elif name == "dubins":
            g = lgrid("pair6d")
            s = TC.DubinsPair(g, **HC.PARAMS["pair6d"])
        else:
            g = quad_grid()
            s = (TC.QuadTables if name == "quad_tables" else TC.QuadInline)(g, UC.QUAD_PAR)
        _made[name] = (g, s)
    return _made[name]


PAIRS = ["plane", "dubins", "quad_tables", "quad_inline"]
SHAPES = {"plane": (7, 6, 8, 5, 9), "dubins": (6, 5, 7, 5, 6, 8), "quad_tables": (5, 6, 5, 7, 8, 6), "quad_inline": (5, 6, 5, 7, 8, 6)}


def trace(name):
    g, s = pair(name)
    return T.trace_callbacks(g, s.hamiltonian, s.dissipation)


def sd_of(g, s, deriv=None):
    return L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF,
                         derivFunc=deriv or L.upwindFirstENO2))


@pytest.fixture
def switch_on():
    prev = L.set_hidim_trace(True)
    yield
    L.set_hidim_trace(prev)


def vec(g, d):
    return np.asarray(g.vs[d], dtype=np.float64).ravel()


def callbacks_equal_evaluate(g, s, tr, seed):
    rng = np.random.default_rng(seed)
    shape = tuple(int(n) for n in np.asarray(g.N).ravel())
    p = [rng.standard_normal(shape) for _ in range(g.dim)]
    data = rng.standard_normal(shape)
    H, alpha = tr.evaluate(g.xs, p)
    want = s.hamiltonian(0.0, data, p, None)
    assert np.array_equal(np.broadcast_to(H, shape), np.broadcast_to(want, shape)), "H"
    for d in range(g.dim):
        a = s.dissipation(0.0, data, None, None, None, d)
        assert np.array_equal(np.broadcast_to(alpha[d], shape), np.broadcast_to(a, shape)), "alpha[%d]" % d


# ------------------------------------------------------------------------------------------ 1. the switch
def test_the_switch_is_off_by_default_and_bumps_the_epoch():
    assert L.get_hidim_trace() is False and T.hidim_enabled() is False
    assert "set_hidim_trace" in T.__all__ and "get_hidim_trace" in T.__all__
    e0 = ATTACH_EPOCH[0]
    assert L.set_hidim_trace(True) is False and L.get_hidim_trace() is True and ATTACH_EPOCH[0] == e0 + 1
    assert L.set_hidim_trace(False) is True and L.get_hidim_trace() is False and ATTACH_EPOCH[0] == e0 + 2
    assert "derivative arrays" in L.set_hidim_trace.__doc__          # the known cost of the first use is documented at the switch


def test_the_environment_sets_the_initial_value():
    """Fresh interpreters (no GPU is touched): HJ_TRACE_HIDIM=1 turns the switch on, HJ_TRACE=0 still disables all tracing."""
    code = "import levelsetpy_amd as L; from levelsetpy_amd import trace_ham as T; print(L.get_hidim_trace(), T.hidim_enabled())"
    outs = []
    for extra in (dict(HJ_TRACE_HIDIM="1"), dict(HJ_TRACE_HIDIM="1", HJ_TRACE="0"), dict()):
        env = dict((k, v) for k, v in os.environ.items() if k not in ("HJ_TRACE_HIDIM", "HJ_TRACE"))
        env.update(extra, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(p.stdout.strip().splitlines()[-1])
    assert outs == ["True True", "True False", "False False"]


# ------------------------------------------------------------------------------------------ 2. the four pairs
@pytest.mark.parametrize("name", PAIRS)
def test_the_pairs_trace(name):
    g, s = pair(name)
    assert tuple(int(n) for n in np.asarray(g.N).ravel()) == SHAPES[name]
    tr = trace(name)
    assert tr.dim == g.dim and tr.aux_axes == s.AXES and len(tr.aux_tables) == len(s.AXES)
    assert tr.column_source is None and tr.ncol == 0 and tr.uses_range is False
    assert all(t.dtype == np.float64 and t.shape == (SHAPES[name][ax],) for t, ax in zip(tr.aux_tables, tr.aux_axes))
    for word in ("col[", "hjtab", "cos(", "sin(", "dmin", "dmax"):
        assert word not in tr.source, (word, tr.source)
    assert "aux[%d]" % (len(s.AXES) - 1) in tr.source and "H = " in tr.source and "alpha[%d] = " % (g.dim - 1) in tr.source
    assert len(tr.params) <= 8 and T._Tracer.MAX_PAR == _hffi.PAR_SLOTS == 8
    callbacks_equal_evaluate(g, s, tr, 11)


def test_the_tables_are_numpys():
    """Stored tables arrive as they were stored; a hoisted table is np.cos / np.sin of grid.vs[d], bit for bit."""
    tr = trace("plane")
    g = pair("plane")[0]
    assert tr.hoisted == [] and np.array_equal(tr.aux_tables[0], np.cos(vec(g, 2))) and np.array_equal(tr.aux_tables[1], np.sin(vec(g, 2)))
    tr = trace("dubins")
    g = pair("dubins")[0]
    assert tr.hoisted == [(2, "cos(x[2])"), (2, "sin(x[2])"), (5, "cos(x[5])"), (5, "sin(x[5])")] and tr.hoisted_slots == [0, 1, 2, 3]
    for t, f, d in zip(tr.aux_tables, (np.cos, np.sin, np.cos, np.sin), (2, 2, 5, 5)):
        assert np.array_equal(t, f(vec(g, d)))
    tr = trace("quad_inline")
    g = pair("quad_inline")[0]
    assert tr.hoisted == [(4, "sin(x[4])"), (4, "cos(x[4])")]
    assert np.array_equal(tr.aux_tables[0], np.sin(vec(g, 4))) and np.array_equal(tr.aux_tables[1], np.cos(vec(g, 4)))
    tr = trace("quad_tables")
    s = pair("quad_tables")[1]
    assert tr.hoisted == []
    for t, want in zip(tr.aux_tables, (s.cos4, s.sin4, s.u1, s.u3)):
        assert np.array_equal(t, want.ravel())


# ------------------------------------------------------------------------------------------ 3. state changes
def test_a_changed_speed_keeps_the_key():
    g = lgrid("plane5d")
    s = TC.PlanePair(g, **HC.PARAMS["plane5d"])
    a = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    s.a_max = 0.55
    b = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert T._key_of(a) == T._key_of(b) and a.params == [0.8, -1.0, 1.3] and b.params == [0.55, -1.0, 1.3]
    assert all(np.array_equal(u, v) for u, v in zip(a.aux_tables, b.aux_tables))


def test_a_changed_table_keeps_the_key():
    g = lgrid("plane5d")
    s = TC.PlanePair(g, **HC.PARAMS["plane5d"])
    a = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert a.state.fresh()
    s.cos2[...] = 0.5 * s.cos2
    assert not a.state.fresh()                                        # what a cached plan re-traces on
    b = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert T._key_of(a) == T._key_of(b) and a.params == b.params
    assert np.array_equal(b.aux_tables[0], 0.5 * np.cos(vec(g, 2))) and np.array_equal(a.aux_tables[0], np.cos(vec(g, 2)))
    assert np.array_equal(a.aux_tables[1], b.aux_tables[1])
    assert T._key_of(a)[-1] == (2, 2) and len(T._key_of(a)) == 6       # the axes are part of the key, the values are not


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_name_their_cause():
    g = lgrid("plane5d")
    kw = HC.PARAMS["plane5d"]
    for cls, words in ((TC.FiveTables, ("5 stored tables", "four table slots")), (TC.RangeReader, ("costate range", "derivMin")),
                       (TC.DataReader, ("data",)), (TC.TimeReader, ("time t",))):
        s = cls(g, **kw)
        with pytest.raises(T.TraceError) as e:
            T.trace_callbacks(g, s.hamiltonian, s.dissipation)
        for w in words:
            assert w in str(e.value), (cls.__name__, str(e.value))
    # the same pairs on the split path: they are plain callbacks, and run
    s = TC.RangeReader(g, **kw)
    shape = tuple(int(n) for n in np.asarray(g.N).ravel())
    lo, hi = [-np.ones(shape)] * 5, [np.ones(shape)] * 5
    assert np.array_equal(s.dissipation(0.0, lo[0], lo, hi, None, 3), np.full(shape, kw["a_max"] + 0.01 * 2.0))


# ------------------------------------------------------------------------------------------ 5. slot allocation
class Greedy(TC.PlanePair):
    """Two stored tables and four candidates for hoisting: tanh(x0) / (2 + x0^2) (two expensive operations), exp(x1), cos(x4), sin(x4)."""

    def hamiltonian(self, t, data, p, sd=None):
        x = self.grid.xs
        heavy = np.tanh(x[0]) / (2 + x[0] ** 2)
        return TC.PlanePair.hamiltonian(self, t, data, p, sd) + p[0] * heavy + p[1] * np.exp(x[1]) + p[4] * np.cos(x[4]) + p[3] * np.sin(x[4])


def test_slots_stored_first_then_heaviest():
    g = lgrid("plane5d")
    s = Greedy(g, **HC.PARAMS["plane5d"])
    tr = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert tr.aux_axes == (2, 2, 0, 1) and tr.nstored == 2 and tr.hoisted_slots == [2, 3]
    assert [h[0] for h in tr.hoisted] == [0, 1] and "tanh" in tr.hoisted[0][1] and tr.hoisted[1][1] == "exp(x[1])"
    v0 = vec(g, 0)
    assert np.array_equal(tr.aux_tables[2], np.tanh(v0) / (2 + v0 ** 2)) and np.array_equal(tr.aux_tables[3], np.exp(vec(g, 1)))
    assert "cos(x[4])" in tr.source and "sin(x[4])" in tr.source and "tanh" not in tr.source and "exp(" not in tr.source
    callbacks_equal_evaluate(g, s, tr, 5)


class Shared(TC.PlanePair):
    """np.cos(x2) inside the callback is the stored table's bytes: one slot."""

    def hamiltonian(self, t, data, p, sd=None):
        return TC.PlanePair.hamiltonian(self, t, data, p, sd) + p[4] * np.cos(self.grid.xs[2])


def test_equal_tables_share_a_slot_and_hoisting_can_be_turned_off(monkeypatch):
    g = lgrid("plane5d")
    s = Shared(g, **HC.PARAMS["plane5d"])
    tr = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert tr.aux_axes == (2, 2) and tr.hoisted == [] and "cos(" not in tr.source
    g6, q = pair("quad_inline")
    monkeypatch.setenv("HJ_TRACE_HOIST", "off")
    off = T.trace_callbacks(g6, q.hamiltonian, q.dissipation)
    assert off.aux_axes == () and off.aux_tables == [] and "cos(x[4])" in off.source and "sin(x[4])" in off.source
    monkeypatch.delenv("HJ_TRACE_HOIST")
    assert T._key_of(off) != T._key_of(trace("quad_inline"))


# ------------------------------------------------------------------------------------------ 6. the registration
@pytest.mark.parametrize("name", PAIRS)
def test_the_registration_compiles_for_gfx950(name):
    g, s = pair(name)
    tr = trace(name)
    reg = T._registration(tr)
    assert isinstance(reg, L.HidimRegistration) and reg.name.startswith("traced_") and len(reg.name) == len("traced_") + 12
    assert reg.ham_id >= _hffi.HAM_USER_BASE and reg.dim == g.dim and reg.aux_axes == s.AXES and reg.nparams == len(tr.params)
    assert T._registration(trace(name)) is reg                        # the same expression: the same registration
    for scheme, dtype in (("ENO3", "float64"), ("WENO5_ASSHIPPED", "float64"), ("ENO3", "float32"), ("WENO5_ASSHIPPED", "float32")):
        reg.check(scheme, dtype)
    src = reg.source()
    assert tr.source in src and "#pragma clang fp contract(off)" in src and "struct HamUser" in src
    assert _hffi.kernel_name("float64", reg.ham_id, 1) == "hidim_substep_kernel<double, HamUser:%s, 1>" % reg.name


def test_the_system_object_carries_the_tables(switch_on):
    g = lgrid("plane5d")
    s = TC.PlanePair(g, **HC.PARAMS["plane5d"])
    sd = sd_of(g, s)
    system, ham, par = T.traced_native(sd)
    assert system._hj_native is system and ham == system.reg.ham_id and par == [0.8, -1.0, 1.3]
    assert len(system.tables) == 2 and np.array_equal(system.tables[0], np.cos(vec(g, 2)))
    s.cos2[...] = -s.cos2
    s.alpha_max = 2.0
    assert system.params() == [0.8, -1.0, 2.0] and system.reg.ham_id == ham                # re-traced: the same kernel,
    assert np.array_equal(system.tables[0], -np.cos(vec(g, 2)))                            # new parameters and new tables


# ------------------------------------------------------------------------------------------ 7. explain_plan
class OnlyHere(TC.QuadInline):
    """An expression no other test meets: its kernel cannot have been verified on data earlier in the process, whatever ran before."""

    def hamiltonian(self, t, data, p, sd=None):
        return TC.QuadInline.hamiltonian(self, t, data, p, sd) + 0.375 * p[0]


def test_explain_plan_with_the_switch_off_and_on():
    g = pair("quad_inline")[0]
    s = OnlyHere(g, UC.QUAD_PAR)
    sd = sd_of(g, s)
    off = dict(path='split', reason='on a grid of 6 dimensions only Plane5D / DubinsPair6D with artificialDissipationGLF run fused; the '
                                    'tracer stops at 4-D', library='libhj_hidim.so')
    assert L.get_hidim_trace() is False and L.explain_plan(sd) == off
    assert term.native_plan(sd) is None
    prev = L.set_hidim_trace(True)
    try:
        e = L.explain_plan(sd)
        plan = term._plan_of(sd)                                      # the plan exists; native_plan hands it out once it is verified on data
        assert term.native_plan(sd) is None and plan is not None and plan.traced and plan[2] >= _hffi.HAM_USER_BASE
        assert e["path"] == "traced" and e["library"] == "libhj_hidim.so" and e["ham_id"] == plan[2] and e["params"] == list(plan[3])
        assert sorted(e) == sorted(["path", "library", "ham_id", "params", "source", "aux_axes", "hoisted", "verified", "verified_dtypes", "unchecked"])
        assert e["aux_axes"] == (4, 4) and e["hoisted"] == [(4, "sin(x[4])"), (4, "cos(x[4])")] and e["verified"] is False and e["verified_dtypes"] == []
        assert e["source"] == T.trace_callbacks(g, s.hamiltonian, s.dissipation).source
        # untraceable pairs: the split path, with the tracer's reason
        g5 = lgrid("plane5d")
        r = L.explain_plan(sd_of(g5, TC.RangeReader(g5, **HC.PARAMS["plane5d"])))
        assert r["path"] == "split" and "costate range" in r["reason"] and r["library"] == "libhj_hidim.so"
        r = L.explain_plan(sd_of(g5, TC.DataReader(g5, **HC.PARAMS["plane5d"])))
        assert r["path"] == "split" and "data" in r["reason"]
        # the built-in and the registered answers do not change with the switch
        b = L.DubinsPair6D(g)
        assert L.explain_plan(sd_of(g, b)) == dict(path='built-in', ham_id=_hffi.HAM_DUBINS_PAIR6D, params=[5.0, 5.0, 5.0, 5.0], library='libhj_hidim.so')
    finally:
        L.set_hidim_trace(prev)
    # taken back: the cached traced plan is not used any more, and the answer is the old one
    assert term.native_plan(sd) is None and L.explain_plan(sd) == off


def test_hj_trace_0_disables_the_hidim_tracer_too(switch_on, monkeypatch):
    g, s = pair("plane")
    monkeypatch.setenv("HJ_TRACE", "0")
    sd = sd_of(g, s)
    assert term.native_plan(sd) is None
    assert L.explain_plan(sd)["reason"].endswith("the tracer stops at 4-D")


# ------------------------------------------------------------------------------------------ 8. random expressions
@pytest.mark.parametrize("seed", range(12))
def test_random_pairs_at_5d(seed):
    g = lgrid("plane5d")
    s = TC.random_pair(g, 1000 + seed)
    tr = T.trace_callbacks(g, s.hamiltonian, s.dissipation)
    assert tr.column_source is None and len(tr.aux_axes) <= 4 and "col[" not in tr.source
    callbacks_equal_evaluate(g, s, tr, seed)
