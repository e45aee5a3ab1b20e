"""GPU tests of HJIPDE_solve_batch and libhj_batch.so (include/hj_batch.h): B problems on one grid, one launch per RK stage.

The project's standing claim is that the tiled kernels and direct_substep_kernel agree bit for bit; tests/conftest.py
sets HJ_DIRECT_BELOW=0, so every per-problem comparison here runs the TILED kernels and extends the claim to
batch_substep_kernel: everything below is compared with == / array_equal unless it is held to the NumPy oracle.

  1. HJIPDE_solve_batch against a Python loop of HJIPDE_solve: data, tau, step counts, final times (step counts and
     times also against the oracle's odeCFL3 driven by HJIPDE_solve's loop with the single solve's own step bound)
  2. against the NumPy oracle, one case per scheme
  3. every one of the 18 instantiations through hjb_substep against hj_rk_substep; hjb_last_kernel names it
  4. hjb_integrate at orders 1, 2, 3 against hj_rk_integrate
  5. a finished problem's buffers are byte-identical afterwards; B above the grid-dimension limit
  6. guarded buffers (tests/guarded_pool.py), one run per dimension
  7. the host loop: the intended WENO5; errors name the problems
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
from levelsetpy_amd import _bffi, _ffi, _marshal, batch  # noqa: E402
from levelsetpy_amd.context import DeviceGrid  # noqa: E402
from levelsetpy_amd.term import native_plan  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402
import guarded_pool as GP  # noqa: E402

SMALL = 1e-4
TD = {"float64": torch.float64, "float32": torch.float32}
DERIV = {"ENO2": L.upwindFirstENO2, "ENO3": L.upwindFirstENO3, "WENO5_ASSHIPPED": L.upwindFirstWENO5}
SID = {"ENO2": _ffi.ENO2, "ENO3": _ffi.ENO3, "WENO5_ASSHIPPED": _ffi.WENO5_ASSHIPPED}


# ------------------------------------------------------------------------------------------ cases
def mk(gmin, gmax, N, pd):
    g = L.createGrid(np.asarray(gmin, dtype=np.float64).reshape(-1, 1), np.asarray(gmax, dtype=np.float64).reshape(-1, 1),
                     np.asarray(N, dtype=np.int64).reshape(-1, 1), pd)
    og = O.Grid(gmin, gmax, [int(n) for n in N], list(pd) if isinstance(pd, (list, tuple)) else ([pd] if pd else []))
    return g, og


def smooth(g, seed):
    """A smooth field without symmetry: a bump per problem plus a small wave, no exact ENO ties."""
    rng = np.random.default_rng(seed)
    xs = [np.asarray(x, dtype=np.float64) for x in g.xs]
    c = [float(np.asarray(v).ravel()[len(v) // 2]) + 0.3 * rng.standard_normal() * float(np.asarray(g.dx).ravel()[d]) for d, v in enumerate(g.vs)]
    r2 = sum((x - cd) ** 2 for x, cd in zip(xs, c))
    wave = sum(np.sin((1.3 + 0.4 * d) * x + rng.uniform(0, 3)) for d, x in enumerate(xs))
    return np.sqrt(r2 + 0.05) - (0.4 + 0.1 * rng.uniform()) + 0.03 * wave


class Case(object):
    """One grid, B systems with spread parameters (their step bounds differ), B initial fields and targets."""

    def __init__(self, name, B, tau):
        self.name, self.B, self.tau = name, B, np.asarray(tau, dtype=np.float64)
        if name == "dubins":
            n = (13, 11, 9)
            self.g, self.og = mk([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / n[2])], n, 2)
            self.par = [(1.0 + 0.45 * b, 1.0 + 0.3 * (b % 3)) for b in range(B)]
            self.systems = [L.DubinsVehicleRel(self.g, u, w) for u, w in self.par]
            self.osystems = [O.DubinsRel(self.og, u, w) for u, w in self.par]
        elif name in ("integrator", "tiny"):
            n = (17, 12) if name == "integrator" else (9, 8)
            self.g, self.og = mk([-1.0, -1.5], [1.0, 1.5], n, None)
            self.par = [(0.6 + 0.9 * b,) for b in range(B)]
            self.systems = [L.DoubleIntegrator(self.g, u) for (u,) in self.par]
            self.osystems = [O.DoubleIntegrator(self.og, u) for (u,) in self.par]
        else:
            n = (8, 7, 8, 7)
            self.g, self.og = mk([-np.pi, -2.0, -np.pi, -2.0], [np.pi * (1 - 2 / n[0]), 2.0, np.pi * (1 - 2 / n[2]), 2.0], n, [0, 2])
            self.par = [(0.5 + 2.5 * b,) for b in range(B)]
            self.systems = [L.DoublePendulum4D(self.g, u) for (u,) in self.par]
            self.osystems = [O.DoublePendulum4D(self.og, u) for (u,) in self.par]
        self.shape = tuple(int(v) for v in np.asarray(self.g.N).ravel())
        assert all(e >= 7 for e in self.shape) and int(np.prod(self.shape)) % 256 != 0
        self.data0 = np.stack([smooth(self.g, 10 + b) for b in range(B)])
        self.targets = np.stack([smooth(self.g, 50 + b) + 0.1 for b in range(B)])

    def sds(self, fn=None):
        out = []
        for s in self.systems:
            d = dict(grid=self.g, hamFunc=s.hamiltonian, partialFunc=s.dissipation)
            if fn is not None:
                d["derivFunc"] = fn
            out.append(L.Bundle(d))
        return out


# tau: two intervals whose lengths are a few steps of the tightest problem and about one of the loosest
CASES = {"dubins": (5, [0.0, 0.05, 0.12]), "integrator": (3, [0.0, 0.11, 0.2]), "pendulum": (2, [0.0, 0.03, 0.05]),
         "tiny": (2, [0.0, 0.2, 0.35]), "single": (1, [0.0, 0.05, 0.12])}
_cases = {}


def case(name):
    if name not in _cases:
        B, tau = CASES[name]
        _cases[name] = Case("dubins" if name == "single" else name, B, tau)
    return _cases[name]


def arr(a, where):
    """The array as the caller's type: NumPy fp64, or a device tensor of the named type."""
    return a if where == "numpy" else torch.as_tensor(a, dtype=TD[where], device="cuda")


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def single_loop(c, where, keepLast, comp, fn=None, obstacles=None):
    """The reference: one HJIPDE_solve per problem, from fresh schemeData Bundles."""
    outs = []
    for b, sd in enumerate(c.sds(fn)):
        args = dict(quiet=True, keepLast=keepLast)
        if comp == "minVWithL":
            args["targetFunction"] = arr(c.targets[b], where)
        if obstacles is not None:
            args["obstacleFunction"] = arr(obstacles[b], where)
        d, tau, _ = L.HJIPDE_solve(arr(c.data0[b], where), c.tau, sd, comp, L.Bundle(args))
        outs.append((d, tau))
    return outs


def reference_times(c, fn=None):
    """Step counts per interval and final times from the SINGLE solve's own step bound (hj_static_step_bound) and the oracle's
    odeCFL3 driven by HJIPDE_solve's loop."""
    steps = np.zeros((c.B, len(c.tau) - 1), dtype=np.int64)
    tnow = np.zeros(c.B)
    dg = L.context.device_grid(c.g, "float64")
    for b, sd in enumerate(c.sds(fn or L.upwindFirstWENO5)):
        sd.dissFunc = L.artificialDissipationGLF
        sb = native_plan(sd).static_step_bound(dg)
        term = lambda t, y: (np.zeros_like(y), sb)          # noqa: E731
        for i in range(1, len(c.tau)):
            t = c.tau[i - 1]
            while t < c.tau[i] - SMALL:
                t, _ = O.ode_cfl_3(term, [t, c.tau[i]], np.zeros((2, 1)), 0.8, single_step=True)
                steps[b, i - 1] += 1
            tnow[b] = t
    return steps, tnow


# ------------------------------------------------------------------------------------------ 1. the single solve
FULL = [(w, k, cm) for w in ("numpy", "float32") for k in (True, False) for cm in (None, "minVOverTime", "minVWithL")]
SOME = [("numpy", True, None), ("float32", False, "minVOverTime"), ("float64", True, "minVWithL")]
EQUALITY = ([("dubins",) + p for p in FULL] + [("integrator",) + p for p in SOME] + [("pendulum",) + p for p in SOME]
            + [("tiny",) + p for p in SOME] + [("single", "numpy", False, "minVOverTime"), ("single", "float32", True, None)])


@pytest.mark.parametrize("name,where,keepLast,comp", EQUALITY, ids=lambda v: str(v))
def test_batch_equals_the_loop_of_single_solves(name, where, keepLast, comp):
    """fp64 (NumPy in) and fp32 / fp64 device tensors in; keepLast and store-all; none, minVOverTime and minVWithL with one
    target per problem.  As HJIPDE_solve, the batch computes in fp64 whatever the input's type."""
    c = case(name)
    args = dict(quiet=True, keepLast=keepLast)
    if comp == "minVWithL":
        args["targetFunction"] = arr(c.targets, where)
    data, tau, outs = L.HJIPDE_solve_batch(arr(c.data0, where), c.tau, c.sds(), comp, L.Bundle(args))
    assert batch.last_path() == _bffi.kernel_name("float64", c.systems[0].native()[0], _ffi.WENO5_ASSHIPPED) == outs.path
    assert torch.is_tensor(data) == (where != "numpy") and (not torch.is_tensor(data) or (data.is_cuda and data.dtype == torch.float64))
    assert tuple(data.shape) == ((c.B,) if keepLast else (c.B, len(c.tau))) + c.shape
    ref = single_loop(c, where, keepLast, comp)
    got = host(data)
    for b, (d, t) in enumerate(ref):
        assert torch.is_tensor(d) == torch.is_tensor(data)
        diff = int(np.sum(got[b] != host(d)))
        print("%s problem %d: %d differing cells, steps %s" % (name, b, diff, outs.steps[b]))
        assert np.array_equal(got[b], host(d)), (name, b, diff)
        assert np.array_equal(tau, t)
    steps, tnow = reference_times(c)
    assert np.array_equal(outs.steps, steps), (outs.steps, steps)
    assert np.array_equal(outs.tNow, tnow), (outs.tNow, tnow)
    # a condition of the test: in some interval two problems took different numbers of steps (the idle path ran)
    if c.B > 1:
        assert any(len(set(outs.steps[:, i])) > 1 for i in range(outs.steps.shape[1])), outs.steps


def test_batch_v0_obstacles_and_the_systems_form():
    """maxVWithV0 with a shared obstacle, minVWithL with a shared target and per-problem obstacles, and one Bundle +
    extraArgs.systems -- each against the loop."""
    c = case("dubins")
    obst = np.stack([smooth(c.g, 90 + b) + 0.3 for b in range(c.B)])
    one = L.Bundle(dict(grid=c.g, hamFunc=c.systems[0].hamiltonian, partialFunc=c.systems[0].dissipation))
    for comp, targ, ob in (("maxVWithV0", None, obst[0]), ("minVWithL", c.targets[1], obst), ("maxVOverTime", None, None)):
        args = dict(quiet=True, keepLast=True, systems=c.systems)
        if targ is not None:
            args["targetFunction"] = targ
        if ob is not None:
            args["obstacleFunction"] = ob
        data, _, outs = L.HJIPDE_solve_batch(c.data0, c.tau, one, comp, L.Bundle(args))
        assert outs.path.startswith("batch_substep_kernel")
        for b, sd in enumerate(c.sds()):
            a = dict(quiet=True, keepLast=True)
            if targ is not None:
                a["targetFunction"] = targ
            if ob is not None:
                a["obstacleFunction"] = ob if ob.ndim == c.g.dim else ob[b]
            d, _, _ = L.HJIPDE_solve(c.data0[b], c.tau, sd, comp, L.Bundle(a))
            assert np.array_equal(data[b], np.asarray(d)), (comp, b)


# ------------------------------------------------------------------------------------------ 2. the NumPy oracle
@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
def test_batch_against_the_numpy_oracle(scheme):
    """Two tau intervals on the Dubins shape.  The rules of tests/test_gpu_parity.py for the scheme: ENO2 / ENO3 run in NumPy's
    operation order and equal the oracle bit for bit; the as-shipped WENO5 is held to its close(..., 1e-11)."""
    c = case("dubins")
    B = 2
    data, tau, outs = L.HJIPDE_solve_batch(c.data0[:B], c.tau, c.sds(DERIV[scheme])[:B], None, L.Bundle(dict(quiet=True)))
    for b in range(B):
        term = lambda t, y: O.term_lax_friedrichs(c.og, c.osystems[b], scheme, t, y)      # noqa: E731
        y = c.data0[b].reshape(-1, 1)
        for i in range(1, len(c.tau)):
            t = c.tau[i - 1]
            while t < c.tau[i] - SMALL:
                t, y = O.ode_cfl_3(term, [t, c.tau[i]], y, 0.8, single_step=True)
            ref = y.reshape(c.shape)
            err = float(np.max(np.abs(data[b, i] - ref))) / max(1.0, float(np.max(np.abs(ref))))
            print("%s problem %d tau[%d]: %d differing cells, err %.3e" % (scheme, b, i, int(np.sum(data[b, i] != ref)), err))
            if scheme.startswith("ENO"):
                assert np.array_equal(data[b, i], ref), (scheme, b, i, err)
            else:
                assert err <= 1e-11, (scheme, b, i, err)
        assert outs.tNow[b] == t


# ------------------------------------------------------------------------------------------ 3. the 18 instantiations
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def entries(B, **cols):
    ent = np.zeros(B, dtype=_bffi.ENTRY)
    ent["active"] = 1
    for k, v in cols.items():
        ent[k] = [x.data_ptr() if torch.is_tensor(x) else x for x in v] if isinstance(v, (list, tuple)) else v
    return ent


def params_dev(c):
    rows = [list(s.native()[1]) + [0.0] * (_bffi.PAR_SLOTS - len(s.native()[1])) for s in c.systems]
    return torch.as_tensor(np.asarray(rows, dtype=np.float64), device="cuda")


def substep(c, dtype, scheme, stage, ent, B=None, restrict=0, par=None):
    desc, _ = _marshal.descriptor(c.g, dtype)
    tab = batch.tables(c.g, torch, torch.device("cuda", torch.cuda.current_device()), dtype)
    e = batch.upload_entries(ent, torch, "cuda")
    par = params_dev(c) if par is None else par
    _bffi.check(_bffi.lib().hjb_substep(C.byref(desc), C.byref(tab), SID[scheme], c.systems[0].native()[0], stage, restrict,
                                        p(par), p(e), len(ent) if B is None else B, stream()))
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("scheme", ["ENO2", "ENO3", "WENO5_ASSHIPPED"])
@pytest.mark.parametrize("name", ["dubins", "integrator", "pendulum"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_instantiation_equals_hj_rk_substep(dtype, name, scheme):
    """Stages EULER and RK3_FULL of every (type, system, scheme), per problem against hj_rk_substep on the same data; one
    problem also with the termRestrictUpdate clamp."""
    c = case(name)
    ham = c.systems[0].native()[0]
    dg = DeviceGrid(c.g, dtype)
    dg.bind_stream()
    y = arr(c.data0, dtype)
    y0 = arr(c.targets, dtype)
    dts = [0.011 + 0.004 * b for b in range(c.B)]
    for stage, restrict in ((_ffi.STAGE_EULER, 0), (_ffi.STAGE_RK3_FULL, 0), (_ffi.STAGE_RK3_FULL, -1)):
        out = torch.full_like(y, float("nan"))
        substep(c, dtype, scheme, stage, entries(c.B, src=list(y), y0=list(y0), dst=list(out), dt=dts), restrict=restrict)
        assert _bffi.last_kernel() == _bffi.kernel_name(dtype, ham, SID[scheme])
        for b, s in enumerate(c.systems):
            ref = torch.full_like(y[b], float("nan"))
            _ffi.check(dg.lib.hj_rk_substep(dg.ctx, SID[scheme], ham, _ffi.darr(s.native()[1]), 0., stage, dts[b], restrict,
                                            dg.ptr(y[b]), dg.ptr(y0[b]), dg.ptr(ref), 3, 0, dg.shape[0]))
            torch.cuda.synchronize()
            assert torch.equal(out[b], ref) and not bool(torch.isnan(ref).any()), (stage, b, int((out[b] != ref).sum()))


# ------------------------------------------------------------------------------------------ 4. RK orders
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_integrate_orders_equal_hj_rk_integrate(order, dtype):
    """hjb_integrate over one interval against hj_rk_integrate per problem: state, time, step count, and where the result is;
    with the integrators' own stopping test and with HJIPDE_solve's; min-with-previous fused into the last stage."""
    c = case("integrator")
    dev = torch.device("cuda", torch.cuda.current_device())
    ham = c.systems[0].native()[0]
    desc, _ = _marshal.descriptor(c.g, dtype)
    tab = batch.tables(c.g, torch, dev, dtype)
    par = params_dev(c)
    sbs = batch.step_bounds(c.g, tab, desc, ham, par, c.B, torch, dev)
    dg = DeviceGrid(c.g, dtype)
    dg.bind_stream()
    y = arr(c.data0, dtype)
    for tol, post in ((-1.0, _ffi.POST_NONE), (SMALL, _ffi.POST_MIN_PREV)):
        bufs = [torch.full((3,) + tuple(y.shape), float("nan"), dtype=y.dtype, device="cuda") for _ in range(2)]
        probs = []
        for b in range(c.B):
            q = _bffi.Problem()
            q.y_in, q.buf_a, q.buf_b, q.work = y[b].data_ptr(), bufs[0][0, b].data_ptr(), bufs[0][1, b].data_ptr(), bufs[0][2, b].data_ptr()
            probs.append(q)
        t, n, where = batch.integrate_batch(c.g, tab, desc, _ffi.ENO3, ham, par, sbs, probs, 0.02, 0.2, order, post,
                                            factorCFL=0.75, stop_tol=tol, torch=torch, device=dev)
        torch.cuda.synchronize()
        assert len(set(n)) > 1, n
        for b, s in enumerate(c.systems):
            parv = _ffi.darr(s.native()[1])
            sb1 = C.c_double()
            _ffi.check(dg.lib.hj_static_step_bound(dg.ctx, ham, parv, C.byref(sb1), None))
            assert sb1.value == sbs[b]
            _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, post))
            tout, ns, wh = C.c_double(), C.c_int64(), C.c_int()
            a, bb, w = bufs[1][0, b], bufs[1][1, b], bufs[1][2, b]
            try:
                _ffi.check(dg.lib.hj_rk_integrate(dg.ctx, order, _ffi.ENO3, ham, parv, 0.02, 0.2, 0.75, 1e300, 0, dg.ptr(y[b]), dg.ptr(a),
                                                  dg.ptr(bb), dg.ptr(w), 0, tol, C.byref(tout), C.byref(ns), C.byref(wh)))
            finally:
                _ffi.check(dg.lib.hj_ctx_set_post_step(dg.ctx, 0))
            torch.cuda.synchronize()
            assert (tout.value, ns.value, wh.value) == (t[b], n[b], where[b]) and wh.value in (1, 2)
            got, ref = bufs[0][where[b] - 1, b], (a, bb)[wh.value - 1]
            assert torch.equal(got, ref) and not bool(torch.isnan(ref).any()), (order, b, int((got != ref).sum()))
    assert torch.equal(y, arr(c.data0, dtype))


# ------------------------------------------------------------------------------------------ 5. idle problems, many problems
def test_finished_problems_are_left_alone():
    """Problem 0 needs one step, problem 1 five: in the launches of steps 2..5 problem 0 is inactive.  Its four buffers, each
    inside a sentinel-filled arena, end byte-identical to a run in which it is alone; an inactive entry of hjb_substep whose
    pointers are live arrays leaves them alone as well."""
    c = case("dubins")
    dev = torch.device("cuda", torch.cuda.current_device())
    ham = c.systems[0].native()[0]
    desc, N = _marshal.descriptor(c.g, "float64")
    n = int(np.prod(N))
    tab = batch.tables(c.g, torch, dev)
    par = params_dev(c)[:2].contiguous()
    pad = 300
    sent = torch.tensor(GP.SENTINEL_BITS[torch.float64], dtype=torch.int64, device="cuda")

    def arena():
        a = torch.empty((2, 4, n + 2 * pad), dtype=torch.float64, device="cuda")
        a.view(torch.int64).fill_(sent)
        a[:, 0, pad:pad + n] = arr(c.data0[:2], "float64").reshape(2, n)
        return a

    def problems(a, which):
        out = []
        for b in which:
            q = _bffi.Problem()
            q.y_in, q.buf_a, q.buf_b, q.work = (a[b, k, pad:].data_ptr() for k in range(4))
            out.append(q)
        return out

    both, alone = arena(), arena()
    sbs = np.array([1.0, 0.0125])
    t, ns, where = batch.integrate_batch(c.g, tab, desc, _ffi.WENO5_ASSHIPPED, ham, par, sbs, problems(both, (0, 1)), 0.0, 0.05,
                                         torch=torch, device=dev)
    assert list(ns) == [1, 5] and list(where) == [1, 1] and t[0] == 0.05
    batch.integrate_batch(c.g, tab, desc, _ffi.WENO5_ASSHIPPED, ham, par[:1], sbs[:1], problems(alone, (0,)), 0.0, 0.05,
                          torch=torch, device=dev)
    torch.cuda.synchronize()
    assert torch.equal(both[0].view(torch.int64), alone[0].view(torch.int64))
    live = both[0, :, pad:pad + n].view(torch.int64)
    assert bool((live[2] == sent).all()) and not bool((live[1] == sent).any()) and not bool((live[3] == sent).any())
    edge = torch.cat([both[0, :, :pad], both[0, :, pad + n:]], 1).view(torch.int64)
    assert bool((edge == sent).all())
    # hjb_substep: an inactive entry with live pointers, beside an active one
    before = both.clone()
    ent = entries(2, src=[both[0, 1, pad:], both[1, 1, pad:]], dst=[both[0, 2, pad:], both[1, 2, pad:]], dt=0.01)
    ent["active"] = [0, 1]
    substep(c, "float64", "ENO2", _ffi.STAGE_EULER, ent, par=par)
    assert torch.equal(both[0].view(torch.int64), before[0].view(torch.int64))
    assert not torch.equal(both[1, 2].view(torch.int64), before[1, 2].view(torch.int64))


def test_more_problems_than_one_launch_holds():
    """B = 65537 > gridDim.y's limit on the (9, 8) grid (fewer cells than a workgroup): three distinct problems repeated; every
    copy equals the three-problem launch."""
    c = case("tiny")
    B, n = 65537, 72
    y3 = arr(np.stack([c.data0[0], c.data0[1], c.targets[0]]), "float32").reshape(3, n)
    par3 = torch.as_tensor(np.asarray([[0.7] + [0] * 7, [1.9] + [0] * 7, [3.1] + [0] * 7], dtype=np.float64), device="cuda")
    idx = torch.arange(B, device="cuda") % 3
    y, par = y3[idx].contiguous(), par3[idx].contiguous()
    out = torch.full_like(y, float("nan"))
    ent = np.zeros(B, dtype=_bffi.ENTRY)
    ent["active"] = 1
    ent["src"] = y.data_ptr() + 4 * n * np.arange(B, dtype=np.uint64)
    ent["dst"] = out.data_ptr() + 4 * n * np.arange(B, dtype=np.uint64)
    ent["dt"] = 0.01 + 0.01 * (np.arange(B) % 3)
    substep(c, "float32", "ENO2", _ffi.STAGE_EULER, ent, par=par)
    ref = torch.full_like(y3, float("nan"))
    substep(c, "float32", "ENO2", _ffi.STAGE_EULER, entries(3, src=list(y3), dst=list(ref), dt=[0.01, 0.02, 0.03]), par=par3)
    assert not bool(torch.isnan(ref).any()) and torch.equal(out, ref[idx])


# ------------------------------------------------------------------------------------------ 6. guarded buffers
_pools = {}


def pool(dtype):
    if dtype not in _pools:
        _pools[dtype] = GP.GuardedPool(TD[dtype], "cuda", 1 << 18)
    return _pools[dtype]


@pytest.mark.parametrize("name", ["integrator", "dubins", "pendulum"])
def test_kernel_stays_inside_its_arrays(name):
    """hjb_substep (RK3_FULL with min-with-previous and both array operators) on B = 3 problems whose every array is a view of
    tests/guarded_pool.py's pool, at element offsets 0-3, guards of NaN and +-1e30: guards intact, inputs unchanged, every
    cell of every output written, the same bits as on fresh arrays.  The cell counts are no multiples of 256, so every
    problem's last workgroup -- the last problem's too -- is partial.  fp64 in 2-D and 4-D, fp32 in 3-D."""
    dtype = "float32" if name == "dubins" else "float64"
    c = Case(name, 3, [0.0, 0.1])
    fields = {"y": c.data0, "y0": c.targets, "pa": c.targets[::-1] + 0.2, "pb": c.data0[::-1] - 0.1}

    def op(F):
        a = dict((k, [F.inp("%s%d" % (k, b), arr(v[b], dtype)) for b in range(3)]) for k, v in fields.items())
        outs = [F.out("out%d" % b, c.shape) for b in range(3)]
        F.arm()
        ent = entries(3, dt=[0.01, 0.02, 0.015], post_prev=_ffi.POST_MIN_PREV, op_a=_bffi.ARR_MAX, op_b=_bffi.ARR_MAX_NEG)
        for k, col in (("y", "src"), ("y0", "y0"), ("pa", "post_a"), ("pb", "post_b")):
            ent[col] = [x.view.data_ptr() for x in a[k]]
        ent["dst"] = [x.view.data_ptr() for x in outs]
        substep(c, dtype, "ENO3", _ffi.STAGE_RK3_FULL, ent)
        return {"kernel": _bffi.last_kernel()}

    ref, _ = GP.run_case(op, pool(dtype), what=name)
    assert ref["kernel"] == _bffi.kernel_name(dtype, c.systems[0].native()[0], _ffi.ENO3)


# ------------------------------------------------------------------------------------------ 7. host loop, errors
def test_intended_weno5_takes_the_host_loop():
    c = case("integrator")
    L.set_weno5_mode("weno5")
    try:
        data, tau, outs = L.HJIPDE_solve_batch(c.data0, c.tau, c.sds(), "minVOverTime", L.Bundle(dict(quiet=True, keepLast=True)))
        assert batch.last_path().startswith("host loop: ") and "intended WENO5" in batch.last_path() and outs.steps is None
        ref = single_loop(c, "numpy", True, "minVOverTime")
    finally:
        L.set_weno5_mode("asshipped")
    for b, (d, t) in enumerate(ref):
        assert np.array_equal(data[b], np.asarray(d)) and np.array_equal(tau, t)
    # ... and a device tensor in gives a device tensor out on this path too
    L.set_weno5_mode("weno5")
    try:
        dt_, _, _ = L.HJIPDE_solve_batch(arr(c.data0, "float64"), c.tau, c.sds(), None, L.Bundle(dict(quiet=True, keepLast=True)))
    finally:
        L.set_weno5_mode("asshipped")
    assert torch.is_tensor(dt_) and dt_.is_cuda and tuple(dt_.shape) == (c.B,) + c.shape


def test_errors_name_the_problems():
    c = case("integrator")
    bad = c.data0.copy()
    bad[1, 3, 4] = np.nan
    bad[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match="Nans encountered"):
        L.HJIPDE_solve(bad[1], c.tau, c.sds()[1], None, L.Bundle(dict(quiet=True, keepLast=True)))
    with pytest.raises(ValueError, match=r"Nans encountered.*problems \[1, 2\]"):
        L.HJIPDE_solve_batch(bad, c.tau, c.sds(), None, L.Bundle(dict(quiet=True, keepLast=True)))
    with pytest.raises(ValueError, match=r"Nans encountered.*problems \[1, 2\]"):
        L.HJIPDE_solve_batch(bad, c.tau, c.sds(), None, L.Bundle(dict(quiet=True, keepLast=True, stopLevel=0.0)))   # the host loop
    assert batch.last_path().startswith("host loop: ")
    with pytest.raises(ValueError, match="target function"):
        L.HJIPDE_solve_batch(c.data0, c.tau, c.sds(), "minVWithL", L.Bundle(dict(quiet=True)))
    # the entry points refuse what they cannot run, and say so
    desc, _ = _marshal.descriptor(c.g, "float64")
    tab = batch.tables(c.g, torch, torch.device("cuda", torch.cuda.current_device()))
    lib = _bffi.lib()
    ent = batch.upload_entries(entries(1), torch, "cuda")
    par = params_dev(c)
    assert lib.hjb_substep(C.byref(desc), C.byref(tab), _ffi.WENO5, 1, 1, 0, p(par), p(ent), 1, stream()) == -3
    assert b"ENO2, ENO3" in lib.hjb_last_error()
    assert lib.hjb_substep(C.byref(desc), C.byref(tab), _ffi.ENO2, 0, 1, 0, p(par), p(ent), 1, stream()) == -1     # a 3-D system
    assert lib.hjb_substep(C.byref(desc), C.byref(tab), _ffi.ENO2, 1, 9, 0, p(par), p(ent), 1, stream()) == -1
    assert lib.hjb_substep(C.byref(desc), C.byref(tab), _ffi.ENO2, 1, 1, 0, p(par), p(ent), 0, stream()) == 0       # nothing to do
