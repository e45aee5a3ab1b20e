"""GPU: state changes reach the fused kernels that were traced from Python callbacks, and the first-use check catches a wrong kernel.

A traced plan runs an expression whose parameters and tables were read from Python state at some earlier time; the split path and the
reference call the callbacks every time.  Everything here is compared against two references: the split path on the same schemeData
(HJ_TRACE=0) and the NumPy oracle driven by the same callbacks or system -- after state changes in place (every holder of
tests/test_trace_state.py), inside integrator spans whose hooks change the system, and on first use of a kernel that is wrong on one plane."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, integration as I, term as TM, trace_ham as TH  # noqa: E402
from levelsetpy_amd.context import device_grid  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

from test_gpu_parity import mk, sdata, close, close_eno  # noqa: E402
from test_gpu_trace_ham import DubinsAbs, _kernel  # noqa: E402
from test_trace_state import CASES, SAME_TEXT, N, _closure_case  # noqa: E402

SMALL = 100 * np.finfo(np.float64).eps


def grids():
    return mk([-2., -2., -np.pi], [2., 2., np.pi * (1 - 2 / N[2])], N, 2)


def data(og, seed=5):
    return O.shape_sphere(og, None, 1.0) + 0.03 * np.random.default_rng(seed).standard_normal(og.shape)


class Via(object):
    """The oracle's system protocol around a schemeData's own callbacks (the oracle hands them NumPy arrays and no schemeData)."""

    def __init__(self, sd):
        self.sd = sd

    def hamiltonian(self, t, data, p, _=None):
        return self.sd.hamFunc(t, data, p, self.sd)

    def dissipation(self, t, data, lo, hi, _, dim):
        return self.sd.partialFunc(t, data, lo, hi, self.sd, dim)


def split_term(sd, y, monkeypatch):
    monkeypatch.setenv("HJ_TRACE", "0")
    try:
        own = L.Bundle(dict(sd.__dict__))          # a Bundle of its own: no cached plan
        assert L.explain_plan(own)["path"] == "split"
        out = L.termLaxFriedrichs(0., y, own)
    finally:
        monkeypatch.delenv("HJ_TRACE")
    return out


def kernel_of(g, y):
    dg = device_grid(g, "float32" if torch.is_tensor(y) and y.dtype == torch.float32 else "float64")
    return dg.lib.hj_last_kernel(dg.ctx).decode()


def as_np(a):
    return a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_changes_reach_the_fused_term(name, monkeypatch):
    """Three termLaxFriedrichs calls with two changes in place between them: every result equals the split path's and the oracle's."""
    g, og = grids()
    case = CASES[name](g)
    d0 = data(og)
    if name == "attribute (control)":
        y, tol = d0.reshape(-1, 1), 1e-11                                   # a NumPy caller
    elif name == "dict attribute":
        y, tol = torch.as_tensor(d0.reshape(-1, 1), device="cuda", dtype=torch.float32), 2e-4
    else:
        y, tol = torch.as_tensor(d0.reshape(-1, 1), device="cuda"), 1e-11
    stats = None
    for k in (0, 1, 2):
        if k:
            case.change(k)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fused, sb_f, _ = L.termLaxFriedrichs(0., y, case.sd)
        assert "hipRTC" in kernel_of(g, y), kernel_of(g, y)
        if name in SAME_TEXT:
            if stats is None:
                stats = L.kernel_cache_stats()
            assert L.kernel_cache_stats() == stats, "a change of a parameter compiled a kernel"
        split, sb_s, _ = split_term(case.sd, y, monkeypatch)
        yo, sbo = O.term_lax_friedrichs(og, Via(case.sd), "WENO5_ASSHIPPED", 0., d0.reshape(-1, 1))
        close(as_np(fused), as_np(split), tol, what="%s, call %d: traced vs split" % (name, k))
        close(as_np(fused), yo, tol, what="%s, call %d: traced vs oracle" % (name, k))
        rel = 1e-13 if tol < 1e-6 else 1e-5
        assert abs(sb_f - sb_s) <= rel * sb_s and abs(sb_f - sbo) <= rel * sbo, (k, sb_f, sb_s, sbo)


@pytest.mark.parametrize("shape", [(20,), (20, 1)])
def test_per_axis_gain_broadcasts_in_the_fused_term(shape, monkeypatch):
    """On a cube grid a (n,) gain belongs to the LAST axis and a (n, 1) gain to the second to last, as NumPy broadcasts them."""
    n = (20, 20, 20)
    g, og = mk([-1., -1.5, -2.], [1.5, 1., 0.5], n, None)
    gain = (1.0 + 0.5 * np.sin(np.linspace(0., 3., 20))).reshape(shape)

    class Gain(object):
        def __init__(self, grid):
            self.grid = grid

        def _g(self, like):
            return torch.as_tensor(gain, device=like.device) if torch.is_tensor(like) else gain

        def hamiltonian(self, t, data, p, sd=None):
            return self._g(p[0]) * p[0] + 0.5 * p[1] - 0.25 * abs(p[2])

        def dissipation(self, t, data, lo, hi, sd, dim):
            return [abs(self._g(data)) + 0 * data, 0.5, 0.25][dim]
    d0 = O.shape_sphere(og, None, 0.6) + 0.02 * np.random.default_rng(3).standard_normal(og.shape)
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    sd = sdata(g, Gain(g), L.upwindFirstWENO5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # no "disagrees with the callbacks"
        fused, sb_f, _ = L.termLaxFriedrichs(0., y, sd)
    assert "hipRTC" in _kernel(g), _kernel(g)
    split, sb_s, _ = split_term(sd, y, monkeypatch)
    yo, sbo = O.term_lax_friedrichs(og, Gain(og), "WENO5_ASSHIPPED", 0., d0.reshape(-1, 1))
    close(as_np(fused), as_np(split), 1e-11, what="gain %s: traced vs split" % (shape,))
    close(as_np(fused), yo, 1e-11, what="gain %s: traced vs oracle" % (shape,))
    assert abs(sb_f - sb_s) <= 1e-13 * sb_s and abs(sb_f - sbo) <= 1e-13 * sbo


# ---------------------------------------------------------------------------------------------- hooks inside an integrator span
def _speeds(t):
    return 1.0 + 0.25 * np.sin(3.0 * t), 1.0 + 0.2 * np.cos(2.0 * t)


def _rel_hook(s, t):
    s.v_e, s.w_p = _speeds(t)


def _oracle_span(og, sd_of, schedule, d0, tf, factor):
    """Single oracle RK3 steps with the same schedule applied between them (ode_cfl_3.py: a hook's result is the next step's state)."""
    t, y, steps = 0., d0.reshape(-1, 1), 0
    while tf - t >= SMALL * abs(tf):
        sd = sd_of()
        t, y = O.ode_cfl_3(lambda tt, yy: O.term_lax_friedrichs(og, Via(sd), "WENO5_ASSHIPPED", tt, yy), [t, tf], y, factor, single_step=True)
        steps += 1
        schedule(t, steps)
    return t, y, steps


class Branchy(L.DubinsVehicleRel):
    """The same Hamiltonian behind Python control flow on array values: neither built in nor traceable -- the split path."""

    def hamiltonian(self, t, data, p, sd=None):
        if float(abs(p[0]).max()) >= 0:
            return L.DubinsVehicleRel.hamiltonian(self, t, data, p, sd)
        return 0 * p[0]


@pytest.mark.parametrize("form", ["built-in in place", "traced dict", "new schemeData", "terminalEvent", "becomes unfusable"])
def test_hooks_inside_a_span_reach_the_next_step(form, monkeypatch):
    g, og = grids()
    d0 = data(og, 7)
    factor = 0.8

    def setup():
        """(schemeData holder, schedule(t, steps) applied after each step) -- fresh state for each of the two runs."""
        box = {}
        if form == "traced dict":
            case = _closure_case(g)
            cfg = case.cfg
            box["sd"] = case.sd

            def schedule(t, steps):
                cfg["v"] = 1.3 + 0.4 * np.sin(5.0 * t)
        else:
            s = L.DubinsVehicleRel(g, 1, 1)
            box["sd"] = sdata(g, s, L.upwindFirstWENO5)
            if form in ("new schemeData", "becomes unfusable"):
                other = (L.DubinsVehicleRel if form == "new schemeData" else Branchy)(g, 1.5, 0.75)

                def schedule(t, steps):
                    if steps == 3:
                        box["sd"] = L.Bundle(dict(box["sd"].__dict__, hamFunc=other.hamiltonian, partialFunc=other.dissipation))
            else:
                def schedule(t, steps):
                    _rel_hook(s, t)
        return box, schedule
    box, schedule = setup()
    sb0 = O.term_lax_friedrichs(og, Via(box["sd"]), "WENO5_ASSHIPPED", 0., d0.reshape(-1, 1))[1]
    tf = 7.5 * factor * sb0
    count = [0]

    def post(t, y, sd):
        count[0] += 1
        schedule(t, count[0])
        return y, box["sd"] if form in ("new schemeData", "becomes unfusable") else sd

    def terminal(t, y, tOld, yOld, sd):
        count[0] += 1
        schedule(t, count[0])
        return 1.0, sd
    opts = dict(factorCFL=factor, singleStep='off')
    if form == "terminalEvent":
        opts["terminalEvent"] = terminal
    else:
        opts["postTimestep"] = post
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    generic, real = [], I._integrate_generic
    monkeypatch.setattr(I, "_integrate_generic", lambda *a, **k: generic.append(a[2]) or real(*a, **k))
    t, yn, _ = L.odeCFL3(L.termLaxFriedrichs, [0., tf], y, L.odeCFLset(L.Bundle(opts)), box["sd"])
    if form == "becomes unfusable":
        # fused for three steps, then the rest of the span on the generic loop from where the hook left it
        assert len(generic) == 1 and 0. < generic[0][0] < tf, generic
    else:
        assert not generic, "the span left the fused path"
    box, schedule = setup()
    to, yo, steps = _oracle_span(og, lambda: box["sd"], schedule, d0, tf, factor)
    assert count[0] == steps >= 6, (count[0], steps)
    assert abs(float(t) - to) <= 1e-13, (float(t), to)
    close(as_np(yn), yo, 1e-11, what="%s: span vs oracle steps" % form)


def test_a_hook_that_changes_nothing_keeps_the_device_path(monkeypatch):
    g, og = grids()
    d0 = data(og, 8)
    sd = sdata(g, L.DubinsVehicleRel(g, 1, 1), L.upwindFirstWENO5)
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    called = []
    monkeypatch.setattr(I, "_integrate_generic", lambda *a, **k: called.append(1))
    t, y_hook, _ = L.odeCFL3(L.termLaxFriedrichs, [0., 0.05], y, L.odeCFLset(L.Bundle(dict(factorCFL=.8, postTimestep=lambda t, y, s: (y, s)))), sd)
    # the same steps one singleStep call at a time: the same launches, the same bits
    op = L.odeCFLset(L.Bundle(dict(factorCFL=.8, singleStep='on')))
    ts, ys = 0., y
    while 0.05 - ts >= SMALL * 0.05:
        ts, ys, _ = L.odeCFL3(L.termLaxFriedrichs, [ts, 0.05], ys, op, sd)
    assert not called and float(t) == float(ts) and torch.equal(y_hook, ys)


# ---------------------------------------------------------------------------------------------- the first-use check
@pytest.fixture
def fresh_registry(monkeypatch):
    monkeypatch.setattr(TH, "_REG_BY_SOURCE", {})
    monkeypatch.setattr(TH, "_BAD_SOURCES", set())
    monkeypatch.setattr(TH, "_CHURN", {})


def test_a_kernel_wrong_on_one_plane_is_dropped(fresh_registry, monkeypatch):
    """520 x 10 x 10: one plane is 0.19 % of the nodes -- below the share of isolated ENO outliers the check allows, but not isolated."""
    n = (520, 10, 10)
    g, og = mk([0., -1., -1.], [519 / 512, 1., 1.], n, None)          # dx = 1/512: x0 = i / 512 exactly, 0.5 is plane 256

    class Switch(object):
        def __init__(self, grid):
            self.grid = grid

        def hamiltonian(self, t, data, p, sd=None):
            x0 = torch.as_tensor(np.asarray(self.grid.xs[0]), device=p[0].device) if torch.is_tensor(p[0]) else self.grid.xs[0]
            gate = x0 > 0.5
            gate = gate.double() if torch.is_tensor(gate) else gate
            return (1.31 - 0.01 * gate) * p[0] + 0.5 * p[1] - 0.25 * abs(p[2])

        def dissipation(self, t, data, lo, hi, sd, dim):
            return [1.31, 0.5, 0.25][dim]
    d0 = O.shape_sphere(og, [0.1, 0., 0.], 0.3) + 0.002 * np.random.default_rng(13).standard_normal(og.shape)
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    obj = Switch(g)
    split, sb_s, _ = split_term(sdata(g, obj, L.upwindFirstENO2), y, monkeypatch)
    monkeypatch.setitem(TH._CMP, "gt", ">=")
    # the kernel is wrong on exactly plane 256 (launched directly, before the check sees it)
    sd0 = sdata(g, obj, L.upwindFirstENO2)
    system, ham, par = TH.traced_native(sd0)
    assert ">=" in system.reg.device_src
    plan = TM._Plan((g, _ffi.SCHEME_IDS["ENO2"], ham, par), _ffi.DISS_GLF, system, False, True)
    wrong, _, _ = TM._fused_term(plan, 0., y, 0)
    diff = (wrong.reshape(-1, 1) - split).abs().reshape(n).cpu().numpy()
    scale = float(split.abs().max())
    planes = np.nonzero((diff > 1e-9 * scale).any(axis=(1, 2)))[0]
    # (the rule before: at most 0.2 % of the nodes off, by at most 5 % of the scale -- this kernel passed it)
    assert list(planes) == [256] and int((diff[256] > 1e-9 * scale).sum()) >= 90 and diff.max() <= 5e-2 * scale
    assert float(np.mean(diff > 1e-9 * scale)) <= 2e-3
    # first use through the public call: dropped with the warning, the split path's result bit for bit
    sd = sdata(g, obj, L.upwindFirstENO2)
    with pytest.warns(UserWarning, match="disagrees with the callbacks"):
        out, sb, _ = L.termLaxFriedrichs(0., y, sd)
    assert torch.equal(out, split) and sb == sb_s
    assert L.explain_plan(sd)["path"] == "split"


def test_isolated_eno_stencil_flips_are_still_accepted(fresh_registry, monkeypatch):
    n = (22, 20, 24)
    g, og = mk([-2., -2., -np.pi], [2., 2., np.pi * (1 - 2 / n[2])], n, 2)
    d0 = O.shape_sphere(og, None, 1.0) + 0.03 * np.random.default_rng(5).standard_normal(og.shape)
    y = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    veh = DubinsAbs(g, 1.3, 0.7)
    for scheme, fn in (("ENO2", L.upwindFirstENO2), ("ENO3", L.upwindFirstENO3)):
        sd = sdata(g, veh, fn)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fused, sb_f, _ = L.termLaxFriedrichs(0., y, sd)
        assert "hipRTC" in _kernel(g), _kernel(g)
        yo, sbo = O.term_lax_friedrichs(og, DubinsAbs(og, 1.3, 0.7), scheme, 0., d0.reshape(-1, 1))
        close_eno(as_np(fused), yo, 1e-11, what="%s first use" % scheme)
        assert abs(sb_f - sbo) <= 1e-13 * sbo


def test_each_floating_type_is_checked_on_its_own_first_use(fresh_registry, monkeypatch):
    g, og = grids()
    case = CASES["attribute (control)"](g)
    d0 = data(og)
    calls = []
    real = TM._split_term
    monkeypatch.setattr(TM, "_split_term", lambda *a: calls.append(1) or real(*a))
    y64 = torch.as_tensor(d0.reshape(-1, 1), device="cuda")
    L.termLaxFriedrichs(0., y64, case.sd)
    assert len(calls) == 1 and L.explain_plan(case.sd)["verified_dtypes"] == ["float64"]
    L.termLaxFriedrichs(0., y64, case.sd)
    assert len(calls) == 1
    y32 = y64.float()
    f32, sb32, _ = L.termLaxFriedrichs(0., y32, case.sd)
    assert len(calls) == 2 and L.explain_plan(case.sd)["verified_dtypes"] == ["float32", "float64"]
    assert "hipRTC" in kernel_of(g, y32)
    L.termLaxFriedrichs(0., y32, case.sd)
    assert len(calls) == 2
    yo, sbo = O.term_lax_friedrichs(og, Via(case.sd), "WENO5_ASSHIPPED", 0., d0.reshape(-1, 1))
    close(as_np(f32), yo, 2e-4, what="fp32 first use")


def test_an_error_of_the_unverified_fused_leg_falls_back_to_the_split_path(fresh_registry, monkeypatch):
    g, og = grids()
    case = CASES["attribute (control)"](g)
    y = torch.as_tensor(data(og).reshape(-1, 1), device="cuda")
    split, sb_s, _ = split_term(case.sd, y, monkeypatch)

    def fail(*a, **k):
        raise ValueError("hj_lf_term: simulated failure")
    monkeypatch.setattr(TM, "_fused_term", fail)
    with pytest.warns(UserWarning, match="failed on first use"):
        out, sb, _ = L.termLaxFriedrichs(0., y, case.sd)
    assert torch.equal(out, split) and sb == sb_s
    key = TH._key_of(TH.trace_callbacks(g, case.sd.hamFunc, case.sd.partialFunc, case.sd))
    assert key in TH._BAD_SOURCES and key not in TH._REG_BY_SOURCE
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out2, _, _ = L.termLaxFriedrichs(0., y, case.sd)          # remembered: no second attempt
    assert torch.equal(out2, split)
