"""GPU tests of libhj_hidim.so (include/hj_hidim.h) and of the package's surface on grids of 5 and 6 dimensions, against the
NumPy oracle (which is dimension-generic) and the restated systems of tests/hidim_cases.py.  The suite's rule:
ENO2 / ENO3 in fp64 array_equal and the step bound ==; the as-shipped WENO5 in fp64 within 1e-11 max(1, |ref|_inf); fp32 by
_fp32_close of tests/test_gpu_fp32.py against the oracle on the fp32-rounded data.

  1. routing: HJIPDE_solve on a 5-D grid (on a tree without the library: "grid.dim must be 1..4")
  2. hjh_substep: every instantiation, every stage; hjh_step_bound
  3. hjh_integrate (three RK3 steps, one RK2, one RK1; the schedule against hjb_plan), odeCFL3, HJIPDE_solve
  4. hjh_upwind through upwindFirst* and computeGradients
  5. the split path: the same systems as plain callbacks; 3-D Dubins padded into 5-D
  6. every supported compMethod with a target and an obstacle, static and time-varying, against a loop over the oracle
  7. refusals name the option
  8. guarded buffers (tests/guarded_pool.py) for all entry points in 5-D and 6-D
(The census of the library's __device_stub__s is in tests/test_hidim_host.py: it needs no device.)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _bffi, _ffi, _hffi, hidim  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402
import guarded_pool as GP  # noqa: E402
import hidim_cases as HC  # noqa: E402
from test_gpu_fp32 import _fp32_close  # noqa: E402

SMALL = 1e-4
TD = {"float64": torch.float64, "float32": torch.float32}
DERIV = {"ENO2": L.upwindFirstENO2, "ENO3": L.upwindFirstENO3, "WENO5_ASSHIPPED": L.upwindFirstWENO5}
SID = {"ENO2": _ffi.ENO2, "ENO3": _ffi.ENO3, "WENO5_ASSHIPPED": _ffi.WENO5_ASSHIPPED}
SCHEMES = ["ENO2", "ENO3", "WENO5_ASSHIPPED"]
STAGES = {"YDOT": _ffi.STAGE_YDOT, "EULER": _ffi.STAGE_EULER, "RK3_HALF": _ffi.STAGE_RK3_HALF, "RK3_FULL": _ffi.STAGE_RK3_FULL,
          "RK2_FULL": _ffi.STAGE_RK2_FULL}


# ------------------------------------------------------------------------------------------ cases, made once
class Case(object):
    def __init__(self, name, low_mem=False):
        gmin, gmax, N, pd = HC.limits(name)
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        self.name = name
        self.g = L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd, low_mem=low_mem)
        self.og = HC.oracle_grid(name)
        self.shape = self.og.shape
        self.n = int(np.prod(self.shape))
        self.sys = (L.Plane5D if self.g.dim == 5 else L.DubinsPair6D)(self.g, **HC.PARAMS[name])
        self.osys = HC.oracle_system(name, self.og, **HC.PARAMS[name])
        self.ham, self.par = self.sys.native()
        self.data = HC.data(self.og, 7)
        self.other = HC.data(self.og, 8)
        self._terms = {}

    def sd(self, scheme, plain=False):
        s = self.sys
        ham, part = (s.hamiltonian, s.dissipation)
        if plain:               # the same expressions as callbacks nobody has a kernel for
            ham, part = (lambda t, d, p, sd_=None: s.hamiltonian(t, d, p, sd_)), (lambda t, d, lo, hi, sd_, i: s.dissipation(t, d, lo, hi, sd_, i))
        return L.Bundle(dict(grid=self.g, hamFunc=ham, partialFunc=part, dissFunc=L.artificialDissipationGLF, derivFunc=DERIV[scheme]))

    def term(self, scheme, dtype="float64"):
        """(data, ydot, stepBound) of the oracle on the data rounded to `dtype`, computed once."""
        key = (scheme, dtype)
        if key not in self._terms:
            d = self.data if dtype == "float64" else self.data.astype(np.float32).astype(np.float64)
            ydot, sb = O.term_lax_friedrichs(self.og, self.osys, scheme, 0.0, d.reshape(-1))
            self._terms[key] = (d, ydot.reshape(self.shape), sb)
        return self._terms[key]

    def oterm(self, scheme):
        return lambda t, y: O.term_lax_friedrichs(self.og, self.osys, scheme, t, y)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def dev(a, dtype="float64"):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=TD[dtype]).to("cuda")


def close(got, ref, scheme, what=""):
    """The suite's fp64 rule."""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    if scheme.startswith("WENO"):
        tol = 1e-11 * max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got - ref).max())
        print("%s %s: max |diff| %.3g (bound %.3g)" % (what, scheme, err, tol))
        assert err <= tol, (what, err, tol)
    else:
        bad = int(np.sum(got != ref))
        print("%s %s: %d cells differ" % (what, scheme, bad))
        assert np.array_equal(got, ref), (what, bad)


# ------------------------------------------------------------------------------------------ 1. routing
def test_hjipde_solve_runs_on_a_5d_grid():
    """NumPy in -> NumPy out, a device tensor in -> a device tensor out, the same bits; last_path() names the kernel."""
    c = case("plane5d")
    tf = 1.5 * 0.8 * c.term("ENO2")[2]
    data, tau, outs = L.HJIPDE_solve(c.data, [0.0, tf], c.sd("ENO2"), None, L.Bundle(dict(quiet=True, keepLast=True)))
    assert isinstance(data, np.ndarray) and data.shape == c.shape and np.array_equal(tau, [0.0, tf])
    assert hidim.last_path() == outs.path == "hidim_substep_kernel<double, HamPlane5D, 0>"
    dt_, _, _ = L.HJIPDE_solve(dev(c.data), [0.0, tf], c.sd("ENO2"), None, L.Bundle(dict(quiet=True, keepLast=True)))
    assert torch.is_tensor(dt_) and dt_.is_cuda and np.array_equal(dt_.cpu().numpy(), data)
    tr, yr = O.ode_cfl_3(c.oterm("ENO2"), [0.0, tf], c.data.reshape(-1), 0.8)
    assert tr == tf
    close(data, yr, "ENO2", "HJIPDE_solve 5-D")


def test_a_6d_pair_value_function_from_numpy_and_from_a_tensor():
    c = case("pair6d")
    tf = 0.8 * c.term("WENO5_ASSHIPPED")[2]
    data, tau, outs = L.HJIPDE_solve(c.data, [0.0, tf], c.sd("WENO5_ASSHIPPED"), "minVOverTime", L.Bundle(dict(quiet=True)))
    assert isinstance(data, np.ndarray) and data.shape == (2,) + c.shape and np.array_equal(data[0], c.data)
    assert outs.path == "hidim_substep_kernel<double, HamDubinsPair6D, 3>"
    dt_, _, _ = L.HJIPDE_solve(dev(c.data), [0.0, tf], c.sd("WENO5_ASSHIPPED"), "minVOverTime", L.Bundle(dict(quiet=True)))
    assert torch.is_tensor(dt_) and dt_.is_cuda and np.array_equal(dt_.cpu().numpy(), data)
    _, yr = O.ode_cfl_3(c.oterm("WENO5_ASSHIPPED"), [0.0, tf], c.data.reshape(-1), 0.8)
    close(data[1], np.minimum(yr, c.data.reshape(-1)), "WENO5_ASSHIPPED", "HJIPDE_solve 6-D")


# ------------------------------------------------------------------------------------------ 2. substeps
def stage_ref(stage, y, y0, dt, ydot):
    e = y + dt * ydot
    if stage == "YDOT":
        return ydot
    if stage == "EULER":
        return e
    if stage == "RK3_HALF":
        return 0.25 * (3 * y0 + e)
    if stage == "RK3_FULL":
        return (1 / 3) * (y0 + 2 * e)
    return 0.5 * (y0 + e)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["plane5d", "pair6d", "plane5d_long"])
def test_every_substep_instantiation_and_stage(name, dtype, scheme):
    c = case(name)
    d, ydot, sb = c.term(scheme, dtype)
    y0 = c.other if dtype == "float64" else c.other.astype(np.float32).astype(np.float64)
    hg = hidim.hi_grid(c.g, dtype)
    got_sb = hg.step_bound(c.ham, c.par)
    if dtype == "float64":
        assert got_sb == sb, (got_sb, sb)
    else:
        assert abs(got_sb - sb) <= 1e-5 * sb, (got_sb, sb)
    dt = 0.8 * sb
    src, y0d, out = dev(d, dtype), dev(y0, dtype), torch.empty(c.shape, dtype=TD[dtype], device="cuda")
    for stage, sid in STAGES.items():
        out.fill_(float("nan"))
        hidim._substep(hg, SID[scheme], c.ham, c.par, sid, 0, src, y0d if sid >= _ffi.STAGE_RK3_HALF else None, out, dt)
        assert _hffi.last_kernel() == _hffi.kernel_name(dtype, c.ham, SID[scheme])
        ref = stage_ref(stage, d, y0, dt, ydot)
        if dtype == "float64":
            close(out.cpu().numpy(), ref, scheme, "%s %s" % (name, stage))
        else:
            _fp32_close(out.cpu().numpy(), ref, scheme, "%s %s" % (name, stage))


@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_restrict_and_post_operators_of_a_stage(name):
    """restrict_sign, post_prev and the two array operators of the last stage, against NumPy on the oracle's ydot (ENO3, fp64)."""
    c = case(name)
    d, ydot, sb = c.term("ENO3")
    hg = hidim.hi_grid(c.g, "float64")
    dt = 0.8 * sb
    src, y0d, pa, pb = dev(d), dev(c.other), dev(c.other + 0.1), dev(0.3 - c.data)
    out = torch.empty(c.shape, dtype=torch.float64, device="cuda")
    for rs, clamp in ((+1, lambda v: np.maximum(v, 0)), (-1, lambda v: np.minimum(v, 0))):
        hidim._substep(hg, _ffi.ENO3, c.ham, c.par, _ffi.STAGE_YDOT, rs, src, None, out)
        assert np.array_equal(out.cpu().numpy(), clamp(ydot))
    hidim._substep(hg, _ffi.ENO3, c.ham, c.par, _ffi.STAGE_RK3_FULL, 0, src, y0d, out, dt, _ffi.POST_MIN_PREV, _hffi.ARR_MAX, pa, _hffi.ARR_MAX_NEG, pb)
    ref = np.maximum(np.maximum(np.minimum(stage_ref("RK3_FULL", d, c.other, dt, ydot), c.other), c.other + 0.1), -(0.3 - c.data))
    assert np.array_equal(out.cpu().numpy(), ref)
    hidim._substep(hg, _ffi.ENO3, c.ham, c.par, _ffi.STAGE_EULER, 0, src, None, out, dt, _ffi.POST_MAX_PREV, _hffi.ARR_MIN, pa)
    assert np.array_equal(out.cpu().numpy(), np.minimum(np.maximum(stage_ref("EULER", d, None, dt, ydot), d), c.other + 0.1))
    # termLaxFriedrichs / termRestrictUpdate are this kernel: NumPy in, a column / a vector out
    sd = c.sd("ENO3")
    yd, sbt, _ = L.termLaxFriedrichs(0.0, d.reshape(-1, 1), sd)
    assert np.asarray(yd).shape == (c.n, 1) and np.array_equal(np.asarray(yd).reshape(c.shape), ydot) and sbt == sb
    yr, sbr, _ = L.termRestrictUpdate(0.0, dev(d).reshape(-1), L.Bundle(dict(innerFunc=L.termLaxFriedrichs, innerData=sd, positive=0)))
    assert tuple(yr.shape) == (c.n,) and np.array_equal(yr.cpu().numpy().reshape(c.shape), np.minimum(ydot, 0)) and sbr == sb


# ------------------------------------------------------------------------------------------ 3. integration
_refs = {}


def span_ref(name, scheme):
    """Three RK3 steps of the oracle (the third cut short by tf), one RK2 and one RK1 step; computed once."""
    key = (name, scheme)
    if key not in _refs:
        c = case(name)
        sb = c.term(scheme)[2]
        tf = 2.5 * 0.8 * sb
        y = c.data.reshape(-1)
        r = {"tf": tf, 3: O.ode_cfl_3(c.oterm(scheme), [0.0, tf], y, 0.8)}
        t1 = 0.7 * 0.8 * sb            # one step, cut short by the end of the span
        r["t1"] = t1
        r[2] = O.ode_cfl_2(c.oterm(scheme), [0.0, t1], y, 0.8)
        r[1] = O.ode_cfl_1(c.oterm(scheme), [0.0, t1], y, 0.8)
        _refs[key] = r
    return _refs[key]


SPANS = [("plane5d", "ENO3"), ("plane5d", "WENO5_ASSHIPPED"), ("pair6d", "ENO2")]


def integrate(c, scheme, order, t0, tf, stop_tol=-1.0, post_prev=0):
    hg = hidim.hi_grid(c.g, "float64")
    y = dev(c.data)
    a, b, w = (torch.full(c.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    sb = hg.step_bound(c.ham, c.par)
    tout, n, where = C.c_double(), C.c_int64(), C.c_int32()
    _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(hg.tab), SID[scheme], c.ham, order, 0, post_prev, _hffi.params(c.par), sb,
                                     hg.ptr(y), hg.ptr(a), hg.ptr(b), hg.ptr(w), 0, None, 0, None, t0, tf, 0.8, 1e300, stop_tol,
                                     C.byref(tout), C.byref(n), C.byref(where), hg.stream()))
    assert np.array_equal(y.cpu().numpy(), c.data)                    # y_in is never written
    tb, nb = C.c_double(), C.c_int64()
    _bffi.check(_bffi.lib().hjb_plan(order, (C.c_double * 1)(sb), 1, t0, tf, 0.8, 1e300, stop_tol, C.byref(tb), C.byref(nb)))
    assert (tout.value, n.value) == (tb.value, nb.value)              # the schedule is hjb_plan's
    return tout.value, n.value, (y, a, b)[where.value].cpu().numpy()


@pytest.mark.parametrize("name,scheme", SPANS)
def test_hjh_integrate_against_the_oracle(name, scheme):
    c, r = case(name), span_ref(name, scheme)
    t, n, y = integrate(c, scheme, 3, 0.0, r["tf"])
    assert n == 3 and t == r[3][0], (n, t, r[3][0])
    close(y, r[3][1], scheme, "RK3 x 3")
    for order in (2, 1):
        t, n, y = integrate(c, scheme, order, 0.0, r["t1"])
        assert n == 1 and t == r[order][0], (order, n, t, r[order][0])
        close(y, r[order][1], scheme, "RK%d" % order)


@pytest.mark.parametrize("name,scheme", SPANS)
def test_odecfl_and_hjipde_solve_against_the_oracle(name, scheme):
    c, r = case(name), span_ref(name, scheme)
    sd = c.sd(scheme)
    op = L.odeCFLset(L.Bundle(dict(factorCFL=0.8)))
    t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [0.0, r["tf"]], dev(c.data).reshape(-1, 1), op, sd)
    assert float(t) == r[3][0]
    close(y.cpu().numpy(), r[3][1], scheme, "odeCFL3")
    for order, ode in ((2, L.odeCFL2), (1, L.odeCFL1)):
        t, y, _ = ode(L.termLaxFriedrichs, [0.0, r["t1"]], c.data.reshape(-1, 1), op, sd)           # NumPy in
        assert float(t) == r[order][0] and not torch.is_tensor(y)
        close(np.asarray(y), r[order][1], scheme, "odeCFL%d" % order)
    data, tau, _ = L.HJIPDE_solve(c.data, [0.0, r["tf"]], sd, None, L.Bundle(dict(quiet=True, keepLast=True)))
    close(data, r[3][1], scheme, "HJIPDE_solve")


# ------------------------------------------------------------------------------------------ 4. derivatives
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("name", ["plane5d", "pair6d"])
def test_upwind_and_gradients_against_the_oracle(name, scheme):
    c = case(name)
    ofn = {"ENO2": O.upwind_first_eno2, "ENO3": O.upwind_first_eno3, "WENO5_ASSHIPPED": lambda g, d, i: O.upwind_first_weno5(g, d, i, 'asshipped')}[scheme]
    refs = [ofn(c.og, c.data, i) for i in range(c.g.dim)]
    derivC, derivL, derivR = L.computeGradients(c.g, dev(c.data), derivFunc=DERIV[scheme])          # one launch for every axis
    assert hidim.last_path() == "hidim_upwind_kernel<double, %d, %d>" % (c.g.dim, SID[scheme])
    for i in range(c.g.dim):
        close(derivL[i].cpu().numpy(), refs[i][0], scheme, "derivL[%d]" % i)
        close(derivR[i].cpu().numpy(), refs[i][1], scheme, "derivR[%d]" % i)
        close(derivC[i].cpu().numpy(), 0.5 * (refs[i][0] + refs[i][1]), scheme, "derivC[%d]" % i)
        # the reductions the kernel leaves as keys are the arrays' own
        from levelsetpy_amd.spatial import cached_minmax
        lo, hi = cached_minmax(derivL[i], derivR[i])
        assert lo == min(float(derivL[i].min()), float(derivR[i].min())) and hi == max(float(derivL[i].max()), float(derivR[i].max()))
    # one axis at a time, NumPy in -> NumPy out (the first, a periodic and the last axis)
    for i in (0, 2, c.g.dim - 1):
        dl, dr = DERIV[scheme](c.g, c.data, i)
        assert isinstance(dl, np.ndarray) and np.array_equal(dl, derivL[i].cpu().numpy()) and np.array_equal(dr, derivR[i].cpu().numpy())
    # fp32 data in, fp32 out
    d32 = c.data.astype(np.float32)
    dl, dr = DERIV[scheme](c.g, dev(d32, "float32"), 1)
    assert dl.dtype == torch.float32
    r32 = ofn(c.og, d32.astype(np.float64), 1)
    _fp32_close(dl.cpu().numpy(), r32[0], scheme, "fp32 derivL")
    _fp32_close(dr.cpu().numpy(), r32[1], scheme, "fp32 derivR")


# ------------------------------------------------------------------------------------------ 5. the split path
@pytest.mark.parametrize("name,scheme", [("plane5d", "ENO3"), ("pair6d", "ENO2"), ("plane5d", "WENO5_ASSHIPPED")])
def test_plain_callbacks_equal_the_fused_path(name, scheme):
    c = case(name)
    tf = 1.5 * 0.8 * c.term(scheme)[2]
    args = L.Bundle(dict(quiet=True, keepLast=True))
    fused, _, o1 = L.HJIPDE_solve(dev(c.data), [0.0, tf], c.sd(scheme), "maxVOverTime", args)
    assert o1.path.startswith("hidim_substep_kernel<")
    split, _, o2 = L.HJIPDE_solve(dev(c.data), [0.0, tf], c.sd(scheme, plain=True), "maxVOverTime", args)
    assert o2.path.startswith("split: ") and hidim.last_path() == o2.path and L.explain_plan(c.sd(scheme, plain=True))["path"] == "split"
    close(split.cpu().numpy(), fused.cpu().numpy(), scheme, "split vs fused")


def test_low_mem_grids_work_on_both_paths():
    c, s = case("plane5d"), Case("plane5d", low_mem=True)
    assert s.g.xs[0].shape != s.shape                         # sparse xs
    tf = 0.8 * c.term("ENO2")[2]
    args = L.Bundle(dict(quiet=True, keepLast=True))
    ref, _, _ = L.HJIPDE_solve(c.data, [0.0, tf], c.sd("ENO2"), None, args)
    for plain in (False, True):
        got, _, _ = L.HJIPDE_solve(c.data, [0.0, tf], s.sd("ENO2", plain=plain), None, args)
        assert np.array_equal(got, ref), plain


def test_dubins_3d_padded_into_5d_equals_the_3d_solve():
    """Data constant and alpha = 0 along axes 3 and 4: the 5-D split path computes the 3-D solve's bits in every (axis 3, axis 4) column
    (the identity holds in the oracle bit for bit).  The coefficients are made with NumPy on the host, as the 3-D system's tables are."""
    N3, tail = (9, 8, 10), (4, 5)
    col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
    lo3, hi3 = [-1.0, -1.1, 0.0], [1.2, 1.0, 2 * np.pi * (1 - 1 / N3[2])]
    g3 = L.createGrid(col(lo3, np.float64), col(hi3, np.float64), col(N3, np.int64), 2)
    g5 = L.createGrid(col(lo3 + [0.0, -1.0], np.float64), col(hi3 + [1.0, 1.0], np.float64), col(N3 + tail, np.int64), [2])
    x = [np.asarray(v) for v in g3.xs]
    rng = np.random.default_rng(11)
    d3 = np.sqrt(x[0] ** 2 + x[1] ** 2 + 0.01) - 0.5 + 0.05 * np.sin(3 * x[0]) * np.cos(2 * x[2]) + 0.02 * rng.standard_normal(N3)
    d5 = np.ascontiguousarray(np.broadcast_to(d3[..., None, None], N3 + tail))
    ve, vp, w = 1.0, 0.7, 1.3
    pad = lambda a: dev(np.ascontiguousarray(np.broadcast_to(a[..., None, None], N3 + tail)))      # noqa: E731
    A, B, X1, X2 = pad(ve - vp * np.cos(x[2])), pad(vp * np.sin(x[2])), pad(x[0] + 0 * x[2]), pad(x[1] + 0 * x[2])
    a0, a1 = pad(np.abs(ve - vp * np.cos(x[2])) + np.abs(w * x[1])), pad(np.abs(vp * np.sin(x[2])) + np.abs(w * x[0]))

    def ham(t, data, p, sd=None):
        return p[0] * A - p[1] * B - w * (p[0] * X2 - p[1] * X1 - p[2]).abs() + w * p[2].abs()

    def part(t, data, lo, hi, sd, i):
        return [a0, a1, w + w, 0.0, 0.0][i]

    s3 = L.DubinsVehicleRel(g3, u_bound=1.0, w_bound=w)
    s3.v_e, s3.v_p = ve, vp
    assert s3.native()[1] == [ve, vp, w, w + w]
    sd3 = L.Bundle(dict(grid=g3, hamFunc=s3.hamiltonian, partialFunc=s3.dissipation, derivFunc=L.upwindFirstENO2))
    sd5 = L.Bundle(dict(grid=g5, hamFunc=ham, partialFunc=part, derivFunc=L.upwindFirstENO2))
    tau = [0.0, 0.05]
    args = L.Bundle(dict(quiet=True, keepLast=True))
    r3, _, _ = L.HJIPDE_solve(d3, tau, sd3, "minVOverTime", args)
    r5, _, o = L.HJIPDE_solve(d5, tau, sd5, "minVOverTime", args)
    assert o.path.startswith("split: ")
    assert np.array_equal(r5, np.broadcast_to(np.asarray(r3)[..., None, None], N3 + tail))


# ------------------------------------------------------------------------------------------ 6. comp methods
def oracle_solve(c, scheme, tau, comp, targets, obstacles):
    """HJIPDE_solve's loop (hji_solver.py:509-656) over the oracle: -> the states at tau[1:]."""
    restrict = comp == "minWithZero"
    term = O.term_restrict_update(lambda t, y: O.term_lax_friedrichs(c.og, c.osys, scheme, t, y.reshape(-1, 1)), positive=False) if restrict else c.oterm(scheme)
    y = c.data.reshape(-1)
    y_init = y
    out = []
    for i in range(1, len(tau)):
        tg = None if targets is None else (targets[i] if targets.ndim == c.g.dim + 1 else targets).reshape(-1)
        ob = None if obstacles is None else (obstacles[i] if obstacles.ndim == c.g.dim + 1 else obstacles).reshape(-1)
        tNow = tau[i - 1]
        while tNow < tau[i] - SMALL:
            yLast = y
            tNow, y = O.ode_cfl_3(term, [tNow, tau[i]], y, 0.8, single_step=True)
            if comp == "minVOverTime":
                y = np.minimum(y, yLast)
            elif comp == "maxVOverTime":
                y = np.maximum(y, yLast)
            elif comp == "minVWithV0":
                y = np.minimum(y, y_init)
            elif comp == "maxVWithV0":
                y = np.maximum(y, y_init)
            elif comp in ("minVWithL", "minVWithTarget"):
                y = np.minimum(y, tg)
            elif comp in ("maxVWithL", "maxVWithTarget"):
                y = np.maximum(y, tg)
            if ob is not None:
                y = np.maximum(y, -ob)
        out.append(y.reshape(c.shape))
    return out


COMPS = [None, "set", "minWithZero", "minVOverTime", "maxVOverTime", "minVWithV0", "maxVWithV0", "minVWithL", "maxVWithL", "minVWithTarget", "maxVWithTarget"]


@pytest.mark.parametrize("varying", [False, True], ids=["static", "time-varying"])
@pytest.mark.parametrize("comp", COMPS)
def test_comp_methods_with_target_and_obstacle(comp, varying):
    c = case("plane5d")
    scheme = "ENO2"
    sb = c.term(scheme)[2]
    tau = np.array([0.0, 1.2 * 0.8 * sb, 1.9 * 0.8 * sb])          # two steps, then one
    x = c.og.xs
    target = np.sqrt((x[0] - 0.5) ** 2 + x[1] ** 2 + 0.02) - 0.8 + 0 * c.data
    obstacle = np.sqrt((x[0] + 1.0) ** 2 + (x[1] - 0.5) ** 2 + 0.02) - 0.4 + 0 * c.data
    if varying:
        target = np.stack([target + 0.1 * k for k in range(3)])
        obstacle = np.stack([obstacle - 0.05 * k for k in range(3)])
    ref = oracle_solve(c, scheme, tau, comp, target, obstacle)
    args = dict(quiet=True, targetFunction=target, obstacleFunction=obstacle)
    data, tout, _ = L.HJIPDE_solve(c.data, tau, c.sd(scheme), comp, L.Bundle(dict(args)))             # store-all
    assert data.shape == (3,) + c.shape and np.array_equal(tout, tau) and np.array_equal(data[0], c.data)
    for i in (1, 2):
        close(data[i], ref[i - 1], scheme, "%s tau[%d]" % (comp, i))
    last, _, _ = L.HJIPDE_solve(dev(c.data), tau, c.sd(scheme), comp, L.Bundle(dict(args, lowMemory=True)))
    assert torch.is_tensor(last) and np.array_equal(last.cpu().numpy(), data[2])
    if comp in (None, "minWithZero", "minVWithL", "maxVOverTime"):
        split, _, o = L.HJIPDE_solve(c.data, tau, c.sd(scheme, plain=True), comp, L.Bundle(dict(args, keepLast=True)))
        assert o.path.startswith("split: ") and np.array_equal(split, data[2])


def test_stop_converge():
    c = case("plane5d")
    sb = c.term("ENO2")[2]
    tau = 0.8 * sb * np.arange(4)
    sd = c.sd("ENO2")
    ref = oracle_solve(c, "ENO2", tau, None, None, None)
    states = [c.data] + ref
    change = [float(np.abs(states[i + 1] - states[i]).max()) for i in range(3)]
    k = int(np.argmin(change))
    thr = change[k] * (1 + 1e-9)                       # the first interval whose change is below it is interval k
    assert all(v >= thr for i, v in enumerate(change) if i < k)
    data, tout, outs = L.HJIPDE_solve(c.data, tau, sd, None, L.Bundle(dict(quiet=True, stopConverge=True, convergeThreshold=thr)))
    assert np.array_equal(tout, tau[:k + 2]) and outs.stoptau == tau[k + 1] and data.shape == (k + 2,) + c.shape
    assert np.array_equal(data[k + 1], ref[k])


# ------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("name,value", [("stopInit", [0.0] * 5), ("stopSetInclude", np.zeros(3)), ("stopSetIntersect", np.zeros(3)),
                                        ("discountFactor", 0.9), ("discountMode", "Kene"), ("SDModFunc", lambda *a: a[0]),
                                        ("computeTTR", True), ("ignoreBoundary", True)])
def test_refused_options_name_themselves(name, value):
    c = case("plane5d")
    with pytest.raises(ValueError, match=name):
        L.HJIPDE_solve(c.data, [0.0, 0.01], c.sd("ENO2"), None, L.Bundle({"quiet": True, name: value}))


def test_refused_schemes_and_dissipations_name_themselves():
    c = case("plane5d")
    sd = c.sd("ENO2")
    sd.derivFunc = L.upwindFirstWENO5Intended
    with pytest.raises(ValueError, match="upwindFirstWENO5Intended"):
        L.HJIPDE_solve(c.data, [0.0, 0.01], sd, None, L.Bundle(dict(quiet=True)))
    with pytest.raises(ValueError, match="upwindFirstWENO5Intended"):
        L.upwindFirstWENO5Intended(c.g, c.data, 0)
    for fn in (L.artificialDissipationLLF, L.artificialDissipationLLLF):
        sd = c.sd("ENO2")
        sd.dissFunc = fn
        with pytest.raises(ValueError, match=fn.__name__):
            L.HJIPDE_solve(c.data, [0.0, 0.01], sd, None, L.Bundle(dict(quiet=True)))
    with pytest.raises(ValueError, match="compMethod"):
        L.HJIPDE_solve(c.data, [0.0, 0.01], c.sd("ENO2"), "sideways", L.Bundle(dict(quiet=True)))


# ------------------------------------------------------------------------------------------ 8. guarded buffers
_pools = {}


def pool(dtype):
    if dtype not in _pools:
        _pools[dtype] = GP.GuardedPool(TD[dtype], "cuda", 1 << 21)
    return _pools[dtype]


def arr(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=TD[dtype])


@pytest.mark.parametrize("name,dtype", [("plane5d", "float64"), ("pair6d", "float32"), ("plane5d_long", "float32"), ("pair6d", "float64")])
def test_kernels_stay_inside_their_arrays(name, dtype):
    """hjh_substep (RK3_FULL with min-with-previous and both array operators), hjh_upwind (every axis, with keys), hjh_step_bound and
    hjh_integrate (two RK3 steps) on views of tests/guarded_pool.py's pool, at element offsets 0-3, guards of NaN and +-1e30: guards intact,
    inputs unchanged, every cell of every output written, the same bits as on fresh arrays.  The cell counts are no multiples of 256."""
    c = case(name)
    hg = hidim.hi_grid(c.g, dtype)
    sb = hg.step_bound(c.ham, c.par)
    nd = c.g.dim
    offsets = GP.OFFSETS if dtype == "float64" else (0, 1)
    # the 64-bit keys are no grid array: they need 8-byte alignment, which an fp32 view at an odd element offset does not have
    keys = torch.zeros((4 * _hffi.MAX_DIM,), dtype=torch.int64, device="cuda")

    def op_substep(F):
        y, y0, pa, pb = (F.inp(k, arr(v, dtype)) for k, v in (("y", c.data), ("y0", c.other), ("pa", c.other + 0.2), ("pb", 0.1 - c.data)))
        out = F.out("out", c.shape)
        F.arm()
        hidim._substep(hg, _ffi.ENO3, c.ham, c.par, _ffi.STAGE_RK3_FULL, 0, y.view, y0.view, out.view, 0.5 * sb, _ffi.POST_MIN_PREV,
                       _hffi.ARR_MAX, pa.view, _hffi.ARR_MAX_NEG, pb.view)
        return {"kernel": _hffi.last_kernel()}

    def op_upwind(F):
        y = F.inp("y", arr(c.data, dtype))
        dl = [F.out("dL%d" % d, c.shape) for d in range(nd)]
        dr = [F.out("dR%d" % d, c.shape) for d in range(nd)]
        F.arm()
        vp = C.c_void_p * _hffi.MAX_DIM
        _hffi.check(hg.lib.hjh_upwind(C.byref(hg.desc), _ffi.WENO5_ASSHIPPED, hg.ptr(y.view), (1 << nd) - 1, vp(*[a.view.data_ptr() for a in dl]),
                                      vp(*[a.view.data_ptr() for a in dr]), hg.ptr(keys), hg.stream()))
        return {"kernel": _hffi.last_kernel()}

    def op_bound(F):
        F.arm()
        v, amax = C.c_double(), (C.c_double * _hffi.MAX_DIM)()
        _hffi.check(hg.lib.hjh_step_bound(C.byref(hg.desc), C.byref(hg.tab), c.ham, _hffi.params(c.par), hg.ptr(keys), C.byref(v), amax, hg.stream()))
        return {"sb": v.value, "amax": tuple(amax)}

    def op_integrate(F):
        y, pb = F.inp("y", arr(c.data, dtype)), F.inp("pb", arr(0.1 - c.data, dtype))
        a, b, w = F.out("a", c.shape), F.out("b", c.shape), F.out("w", c.shape)
        F.arm()
        tout, n, where = C.c_double(), C.c_int64(), C.c_int32()
        _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(hg.tab), _ffi.ENO2, c.ham, 3, -1, _ffi.POST_MAX_PREV, _hffi.params(c.par), sb,
                                         hg.ptr(y.view), hg.ptr(a.view), hg.ptr(b.view), hg.ptr(w.view), 0, None, _hffi.ARR_MAX_NEG, hg.ptr(pb.view),
                                         0.0, 1.5 * 0.8 * sb, 0.8, 1e300, SMALL, C.byref(tout), C.byref(n), C.byref(where), hg.stream()))
        return {"t": tout.value, "n": n.value, "where": where.value}

    ref, _ = GP.run_case(op_substep, pool(dtype), offsets=offsets, what=name + " substep")
    assert ref["kernel"] == _hffi.kernel_name(dtype, c.ham, _ffi.ENO3)
    ref, _ = GP.run_case(op_upwind, pool(dtype), offsets=offsets, what=name + " upwind")
    assert ref["kernel"] == "hidim_upwind_kernel<%s, %d, 3>" % ("double" if dtype == "float64" else "float", nd)
    ref, _ = GP.run_case(op_bound, pool(dtype), offsets=(0,), what=name + " bound")
    assert ref["sb"] == sb and ref["amax"][nd:] == (0.0,) * (_hffi.MAX_DIM - nd)
    ref, _ = GP.run_case(op_integrate, pool(dtype), offsets=offsets, what=name + " integrate")
    assert (ref["n"], ref["where"]) == (2, 2)
