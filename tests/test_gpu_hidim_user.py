"""GPU tests of systems registered at run time on 5-D / 6-D grids (levelsetpy_amd/hidim_ham.py, hjh_ham_* of include/hj_hidim.h).

  1. Plane5D and DubinsPair6D re-registered as expressions over tables (tests/hidim_user_cases.py) against their built-in kernels: ENO2 / ENO3
     in fp64 and fp32 array_equal for every stage, restrict_sign and post-step operator, the step bound ==, hjh_integrate at orders 1 to 3 == in
     data, time and step count; the as-shipped WENO5 against the oracle within the suite's 1e-11 (the built-in kernel writes H as one contracted
     expression, so the two kernels are not compared bit for bit there), fp32 by _fp32_close of tests/test_gpu_fp32.py
  2. the planar quadrotor -- the case no built-in kernel serves -- against the NumPy oracle driven by the restated callbacks: ENO2 / ENO3
     array_equal, the step bound ==, HJIPDE_solve over two tau intervals; the same callbacks unregistered take the split path, same bits
  3. the quadrotor with device sin / cos instead of tables: within 1e-11 of the oracle (the measured maximum is printed)
  4. two systems with different tables on one grid, used alternately
  5. guarded buffers (tests/guarded_pool.py) with a user id on the 5-D and the 6-D shape
  6. a second process finds the kernels in the disk cache
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _hffi, hidim  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402
import guarded_pool as GP  # noqa: E402
import hidim_cases as HC  # noqa: E402
import hidim_user_cases as UC  # noqa: E402
from test_gpu_fp32 import _fp32_close  # noqa: E402
from test_gpu_hidim import DERIV, SID, SMALL, STAGES, TD, arr, case, close, dev, oracle_solve, pool, stage_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENO = ["ENO2", "ENO3"]


def registration(dim):
    if dim == 5:
        return L.register_hidim_hamiltonian("plane5d_tables", 5, UC.PLANE_SRC, nparams=3, aux_axes=UC.PLANE_AXES)
    return L.register_hidim_hamiltonian("pair6d_tables", 6, UC.PAIR_SRC, nparams=4, aux_axes=UC.PAIR_AXES)


_users = {}


def user(name):
    """(the built-in case of tests/test_gpu_hidim.py, the same system registered: a system object around the built-in's own NumPy methods)."""
    if name not in _users:
        c = case(name)
        reg = registration(c.g.dim)
        par = c.par[:reg.nparams]
        vs = [np.asarray(v, dtype=np.float64).ravel() for v in c.g.vs]
        s = reg(c.g, par, tables=UC.builtin_tables(vs), hamiltonian=lambda self, t, d, p, sd=None: c.sys.hamiltonian(t, d, p, sd),
                dissipation=lambda self, t, d, lo, hi, sd, i: c.sys.dissipation(t, d, lo, hi, sd, i))
        _users[name] = (c, s, reg.ham_id, par)
    return _users[name]


def substep(hg, s, sid, ham, par, *a, **kw):
    hidim._substep(hg, sid, ham, par, *a, tab=hg.tables_of(s)[0], **kw)


# ------------------------------------------------------------------------------------------ 1. the re-registered built-ins
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", ["plane5d", "pair6d", "plane5d_long"])
def test_reregistered_systems_equal_the_builtin_kernels(name, dtype):
    c, s, ham, par = user(name)
    hg = hidim.hi_grid(c.g, dtype)
    sb = hg.step_bound(c.ham, c.par)
    assert hg.step_bound(ham, par, s) == sb                                       # hjh_step_bound: ==
    dt = 0.8 * sb
    src, y0d, pa, pb = dev(c.data, dtype), dev(c.other, dtype), dev(c.other + 0.1, dtype), dev(0.3 - c.data, dtype)
    ref, out = (torch.empty(c.shape, dtype=TD[dtype], device="cuda") for _ in range(2))

    def both(scheme, *a):
        ref.fill_(float("nan"))
        out.fill_(float("nan"))
        hidim._substep(hg, SID[scheme], c.ham, c.par, *a[:4], ref, *a[4:])
        assert _hffi.last_kernel() == _hffi.kernel_name(dtype, c.ham, SID[scheme])
        substep(hg, s, SID[scheme], ham, par, *a[:4], out, *a[4:])
        assert _hffi.last_kernel() == _hffi.kernel_name(dtype, ham, SID[scheme]) and "HamUser:" in _hffi.last_kernel()
        return ref.cpu().numpy(), out.cpu().numpy()

    for scheme in ENO:
        for stage, sid in STAGES.items():
            r, o = both(scheme, sid, 0, src, y0d if sid >= _ffi.STAGE_RK3_HALF else None, dt)
            assert not np.isnan(o).any() and np.array_equal(o, r), (scheme, stage, int(np.sum(o != r)))
        for rs in (+1, -1):
            r, o = both(scheme, _ffi.STAGE_YDOT, rs, src, None, 0.0)
            assert np.array_equal(o, r) and (o * rs >= 0).all(), (scheme, rs)
        r, o = both(scheme, _ffi.STAGE_RK3_FULL, -1, src, y0d, dt, _ffi.POST_MIN_PREV, _hffi.ARR_MAX, pa, _hffi.ARR_MAX_NEG, pb)
        assert np.array_equal(o, r), scheme
        r, o = both(scheme, _ffi.STAGE_EULER, 0, src, None, dt, _ffi.POST_MAX_PREV, _hffi.ARR_MIN, pa)
        assert np.array_equal(o, r), scheme
    # the as-shipped WENO5: against the oracle, by the suite's rules
    d, ydot, osb = c.term("WENO5_ASSHIPPED", dtype)
    y0 = c.other if dtype == "float64" else c.other.astype(np.float32).astype(np.float64)
    src = dev(d, dtype)
    for stage, sid in STAGES.items():
        out.fill_(float("nan"))
        substep(hg, s, _ffi.WENO5_ASSHIPPED, ham, par, sid, 0, src, y0d if sid >= _ffi.STAGE_RK3_HALF else None, out, dt)
        want = stage_ref(stage, d, y0, dt, ydot)
        if dtype == "float64":
            close(out.cpu().numpy(), want, "WENO5_ASSHIPPED", "%s %s" % (name, stage))
        else:
            _fp32_close(out.cpu().numpy(), want, "WENO5_ASSHIPPED", "%s %s" % (name, stage))


@pytest.mark.parametrize("name,scheme", [("plane5d", "ENO3"), ("pair6d", "ENO2")])
def test_hjh_integrate_of_a_reregistered_system(name, scheme):
    c, s, ham, par = user(name)
    hg = hidim.hi_grid(c.g, "float64")
    sb = hg.step_bound(c.ham, c.par)
    pb = dev(0.1 - c.data)

    def integrate(order, tf, hm, pr, tab):
        y = dev(c.data)
        a, b, w = (torch.full(c.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
        tout, n, where = C.c_double(), C.c_int64(), C.c_int32()
        _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(tab), SID[scheme], hm, order, -1, _ffi.POST_MAX_PREV, _hffi.params(pr), sb,
                                         hg.ptr(y), hg.ptr(a), hg.ptr(b), hg.ptr(w), 0, None, _hffi.ARR_MAX_NEG, hg.ptr(pb), 0.0, tf, 0.8, 1e300,
                                         SMALL, C.byref(tout), C.byref(n), C.byref(where), hg.stream()))
        assert np.array_equal(y.cpu().numpy(), c.data)
        return tout.value, n.value, where.value, (y, a, b)[where.value].cpu().numpy()

    for order, tf, steps in ((3, 2.5 * 0.8 * sb, 3), (2, 1.5 * 0.8 * sb, 2), (1, 0.7 * 0.8 * sb, 1)):
        t0, n0, w0, y0 = integrate(order, tf, c.ham, c.par, hg.tab)
        t1, n1, w1, y1 = integrate(order, tf, ham, par, hg.tables_of(s)[0])
        assert (t1, n1, w1) == (t0, n0, w0) and n0 == steps
        assert not np.isnan(y1).any() and np.array_equal(y1, y0), order
        assert "HamUser:" in _hffi.last_kernel()


# ------------------------------------------------------------------------------------------ 2. the quadrotor
class QuadCase(object):
    """The attributes oracle_solve of tests/test_gpu_hidim.py reads, for the quadrotor."""

    def __init__(self):
        gmin, gmax, N, pd = UC.quad_limits()
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        self.g = L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)
        self.og = UC.quad_oracle_grid()
        self.shape = self.og.shape
        self.n = int(np.prod(self.shape))
        self.osys = UC.QuadOracle(self.og)
        self.data = UC.quad_data(self.og, 7)
        self.reg = L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)
        self.sys = self.reg(self.g, UC.QUAD_PAR, tables=UC.quad_tables(self.g.vs), hamiltonian=UC.quad_ham, dissipation=UC.quad_diss)
        self._terms = {}

    def sd(self, scheme, plain=False, system=None):
        s = self.sys if system is None else system
        ham, part = s.hamiltonian, s.dissipation
        if plain:               # the same callbacks handed over unregistered
            ham, part = (lambda t, d, p, sd_=None: s.hamiltonian(t, d, p, sd_)), (lambda t, d, lo, hi, sd_, i: s.dissipation(t, d, lo, hi, sd_, i))
        return L.Bundle(dict(grid=self.g, hamFunc=ham, partialFunc=part, dissFunc=L.artificialDissipationGLF, derivFunc=DERIV[scheme]))

    def term(self, scheme):
        if scheme not in self._terms:
            ydot, sb = O.term_lax_friedrichs(self.og, self.osys, scheme, 0.0, self.data.reshape(-1))
            self._terms[scheme] = (ydot.reshape(self.shape), sb)
        return self._terms[scheme]

    def oterm(self, scheme):
        return lambda t, y: O.term_lax_friedrichs(self.og, self.osys, scheme, t, y)


_quad = []


def quad():
    if not _quad:
        _quad.append(QuadCase())
    return _quad[0]


def test_the_grids_agree():
    c = quad()
    for d in range(6):
        assert np.array_equal(np.asarray(c.g.vs[d]).ravel(), np.asarray(c.og.vs[d]).ravel())
    assert c.n % 256 != 0 and c.n > 256


@pytest.mark.parametrize("scheme", ENO)
def test_quadrotor_term_equals_the_oracle(scheme):
    c = quad()
    ydot, sb = c.term(scheme)
    yd, sbt, _ = L.termLaxFriedrichs(0.0, c.data.reshape(-1, 1), c.sd(scheme))
    assert hidim.last_path() == "hidim_substep_kernel<double, HamUser:planar_quad, %d>" % SID[scheme]
    assert sbt == sb, (sbt, sb)
    bad = int(np.sum(np.asarray(yd).reshape(c.shape) != ydot))
    print("quadrotor %s: %d cells differ from the oracle" % (scheme, bad))
    assert np.array_equal(np.asarray(yd).reshape(c.shape), ydot)
    yr, sbr, _ = L.termRestrictUpdate(0.0, dev(c.data).reshape(-1), L.Bundle(dict(innerFunc=L.termLaxFriedrichs, innerData=c.sd(scheme), positive=0)))
    assert np.array_equal(yr.cpu().numpy().reshape(c.shape), np.minimum(ydot, 0)) and sbr == sb
    # odeCFL3 runs it stage by stage
    tf = 1.5 * 0.8 * sb
    t, y, _ = L.odeCFL3(L.termLaxFriedrichs, [0.0, tf], dev(c.data).reshape(-1, 1), L.odeCFLset(L.Bundle(dict(factorCFL=0.8))), c.sd(scheme))
    tr, yr = O.ode_cfl_3(c.oterm(scheme), [0.0, tf], c.data.reshape(-1), 0.8)
    assert float(t) == tr and np.array_equal(y.cpu().numpy().reshape(-1), yr)


@pytest.mark.parametrize("comp", ["minVOverTime", "minVWithL"])
def test_quadrotor_solve_over_two_intervals(comp):
    c = quad()
    scheme = "ENO2"
    sb = c.term(scheme)[1]
    tau = np.array([0.0, 1.2 * 0.8 * sb, 1.9 * 0.8 * sb])          # two steps, then one
    x = c.og.xs
    target = obstacle = None
    if comp == "minVWithL":
        target = np.sqrt((x[0] - 0.5) ** 2 + x[2] ** 2 + 0.02) - 0.8 + 0 * c.data
        obstacle = np.sqrt((x[0] + 1.0) ** 2 + (x[2] - 0.5) ** 2 + 0.02) - 0.4 + 0 * c.data
    ref = oracle_solve(c, scheme, tau, comp, target, obstacle)
    args = dict(quiet=True)
    if target is not None:
        args.update(targetFunction=target, obstacleFunction=obstacle)
    data, tout, outs = L.HJIPDE_solve(c.data, tau, c.sd(scheme), comp, L.Bundle(dict(args)))
    fused_path = hidim.last_path()
    assert outs.path == fused_path == "hidim_substep_kernel<double, HamUser:planar_quad, 0>"
    assert data.shape == (3,) + c.shape and np.array_equal(tout, tau) and np.array_equal(data[0], c.data)
    for i in (1, 2):
        assert np.array_equal(data[i], ref[i - 1]), (comp, i, int(np.sum(data[i] != ref[i - 1])))
    # the same callbacks unregistered: the split path, the same bits
    split, tsplit, o2 = L.HJIPDE_solve(c.data, tau, c.sd(scheme, plain=True), comp, L.Bundle(dict(args)))
    assert o2.path.startswith("split: ") and hidim.last_path() == o2.path != fused_path
    assert np.array_equal(tsplit, tout) and np.array_equal(split, data)


# ------------------------------------------------------------------------------------------ 3. device sin / cos
def test_quadrotor_with_device_trigonometry():
    c = quad()
    reg = L.register_hidim_hamiltonian("planar_quad_trig", 6, UC.QUAD_TRIG_SRC, nparams=8)
    s = reg(c.g, UC.QUAD_PAR, hamiltonian=UC.quad_ham, dissipation=UC.quad_diss)
    worst = 0.0
    for scheme in ("ENO2", "ENO3", "WENO5_ASSHIPPED"):
        if scheme == "WENO5_ASSHIPPED":
            ydot, sb = O.term_lax_friedrichs(c.og, c.osys, scheme, 0.0, c.data.reshape(-1))
            ydot = ydot.reshape(c.shape)
        else:
            ydot, sb = c.term(scheme)
        yd, sbt, _ = L.termLaxFriedrichs(0.0, dev(c.data).reshape(-1, 1), c.sd(scheme, system=s))
        assert hidim.last_path() == "hidim_substep_kernel<double, HamUser:planar_quad_trig, %d>" % SID[scheme]
        err = float(np.abs(yd.cpu().numpy().reshape(c.shape) - ydot).max())
        tol = 1e-11 * max(1.0, float(np.abs(ydot).max()))
        print("quadrotor, device sin / cos, %s: max |ydot - oracle| %.3g (bound %.3g), stepBound rel. diff %.3g" % (scheme, err, tol, abs(sbt - sb) / sb))
        worst = max(worst, err)
        assert err <= tol and abs(sbt - sb) <= 1e-11 * max(1.0, sb)
    print("quadrotor, device sin / cos: measured maximum %.3g" % worst)


# ------------------------------------------------------------------------------------------ 4. per-system tables
class SwappedPlane(HC.Plane5D):
    """Plane5D with the cos and the sin table exchanged."""

    def hamiltonian(self, t, data, p, sd=None):
        x = self.grid.xs
        return (p[0] * (x[3] * np.sin(x[2])) + p[1] * (x[3] * np.cos(x[2])) + p[2] * x[4] + self.s * (self.a_max * np.abs(p[3]))
                + self.s * (self.alpha_max * np.abs(p[4])))

    def dissipation(self, t, data, derivMin, derivMax, sd, dim):
        x = self.grid.xs
        if dim == 0:
            return np.abs(x[3] * np.sin(x[2]))
        if dim == 1:
            return np.abs(x[3] * np.cos(x[2]))
        return HC.Plane5D.dissipation(self, t, data, derivMin, derivMax, sd, dim)


def test_two_systems_with_different_tables_on_one_grid():
    c, a, ham, par = user("plane5d")
    reg = registration(5)
    vs = [np.asarray(v, dtype=np.float64).ravel() for v in c.g.vs]
    b = reg(c.g, par, tables=UC.builtin_tables(vs)[::-1])
    assert b._hj_native.reg.ham_id == ham                              # one registration, two systems
    d, ydot_a, sb_a = c.term("ENO3")
    ydot_b, sb_b = O.term_lax_friedrichs(c.og, SwappedPlane(c.og, **HC.PARAMS["plane5d"]), "ENO3", 0.0, d.reshape(-1))
    assert not np.array_equal(ydot_a.reshape(-1), ydot_b)

    def sd(s):
        return L.Bundle(dict(grid=c.g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=DERIV["ENO3"]))
    sda, sdb = sd(a), sd(b)
    for _ in range(2):
        for sd_, ydot, sb in ((sda, ydot_a.reshape(-1), sb_a), (sdb, ydot_b.reshape(-1), sb_b)):
            yd, sbt, _ = L.termLaxFriedrichs(0.0, d.reshape(-1, 1), sd_)
            assert sbt == sb and np.array_equal(np.asarray(yd).reshape(-1), ydot)
    # the built-in system of the same grid still reads the grid's own tables
    yd, sbt, _ = L.termLaxFriedrichs(0.0, d.reshape(-1, 1), c.sd("ENO3"))
    assert sbt == sb_a and np.array_equal(np.asarray(yd).reshape(-1), ydot_a.reshape(-1))
    # a system whose tables change is uploaded again
    b.tables[0][:], b.tables[1][:] = a.tables[0], a.tables[1]
    yd, sbt, _ = L.termLaxFriedrichs(0.0, d.reshape(-1, 1), sdb)
    assert sbt == sb_a and np.array_equal(np.asarray(yd).reshape(-1), ydot_a.reshape(-1))


# ------------------------------------------------------------------------------------------ 5. guarded buffers
@pytest.mark.parametrize("name,dtype", [("plane5d", "float64"), ("pair6d", "float32"), ("pair6d", "float64")])
def test_registered_kernels_stay_inside_their_arrays(name, dtype):
    """hjh_substep (RK3_FULL with min-with-previous and both array operators), hjh_step_bound and hjh_integrate (two RK3 steps) with a user id
    on views of tests/guarded_pool.py's pool: guards intact, inputs unchanged, every cell of every output written, the same bits as on fresh
    arrays.  The cell counts are no multiples of 256."""
    c, s, ham, par = user(name)
    hg = hidim.hi_grid(c.g, dtype)
    tab = hg.tables_of(s)[0]
    sb = hg.step_bound(ham, par, s)
    nd = c.g.dim
    offsets = GP.OFFSETS if dtype == "float64" else (0, 1)
    keys = torch.zeros((4 * _hffi.MAX_DIM,), dtype=torch.int64, device="cuda")

    def op_substep(F):
        y, y0, pa, pb = (F.inp(k, arr(v, dtype)) for k, v in (("y", c.data), ("y0", c.other), ("pa", c.other + 0.2), ("pb", 0.1 - c.data)))
        out = F.out("out", c.shape)
        F.arm()
        hidim._substep(hg, _ffi.ENO3, ham, par, _ffi.STAGE_RK3_FULL, 0, y.view, y0.view, out.view, 0.5 * sb, _ffi.POST_MIN_PREV,
                       _hffi.ARR_MAX, pa.view, _hffi.ARR_MAX_NEG, pb.view, tab=tab)
        return {"kernel": _hffi.last_kernel()}

    def op_bound(F):
        F.arm()
        v, amax = C.c_double(), (C.c_double * _hffi.MAX_DIM)()
        _hffi.check(hg.lib.hjh_step_bound(C.byref(hg.desc), C.byref(tab), ham, _hffi.params(par), hg.ptr(keys), C.byref(v), amax, hg.stream()))
        return {"sb": v.value, "amax": tuple(amax)}

    def op_integrate(F):
        y, pb = F.inp("y", arr(c.data, dtype)), F.inp("pb", arr(0.1 - c.data, dtype))
        a, b, w = F.out("a", c.shape), F.out("b", c.shape), F.out("w", c.shape)
        F.arm()
        tout, n, where = C.c_double(), C.c_int64(), C.c_int32()
        _hffi.check(hg.lib.hjh_integrate(C.byref(hg.desc), C.byref(tab), _ffi.ENO2, ham, 3, -1, _ffi.POST_MAX_PREV, _hffi.params(par), sb,
                                         hg.ptr(y.view), hg.ptr(a.view), hg.ptr(b.view), hg.ptr(w.view), 0, None, _hffi.ARR_MAX_NEG, hg.ptr(pb.view),
                                         0.0, 1.5 * 0.8 * sb, 0.8, 1e300, SMALL, C.byref(tout), C.byref(n), C.byref(where), hg.stream()))
        return {"t": tout.value, "n": n.value, "where": where.value}

    ref, _ = GP.run_case(op_substep, pool(dtype), offsets=offsets, what=name + " user substep")
    assert ref["kernel"] == _hffi.kernel_name(dtype, ham, _ffi.ENO3)
    ref, _ = GP.run_case(op_bound, pool(dtype), offsets=(0,), what=name + " user bound")
    assert ref["sb"] == sb and ref["amax"][nd:] == (0.0,) * (_hffi.MAX_DIM - nd)
    ref, _ = GP.run_case(op_integrate, pool(dtype), offsets=offsets, what=name + " user integrate")
    assert (ref["n"], ref["where"]) == (2, 2)


# ------------------------------------------------------------------------------------------ 6. the disk cache
_CACHE_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["HJ_TEST_ROOT"], "tests"))
import levelsetpy_amd as L
import hidim_user_cases as UC
gmin, gmax, N, pd = UC.quad_limits()
col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)
g = L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd)
reg = L.register_hidim_hamiltonian("planar_quad", 6, UC.QUAD_SRC, nparams=8, aux_axes=UC.QUAD_AXES)
s = reg(g, UC.QUAD_PAR, tables=UC.quad_tables(g.vs))
sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
yd, sb, _ = L.termLaxFriedrichs(0.0, UC.quad_data(UC.quad_oracle_grid()).reshape(-1, 1), sd)
print(json.dumps(dict(stats=L.hidim_kernel_cache_stats(), sb=sb, sum=float(np.asarray(yd).sum()), files=sorted(os.listdir(os.environ["HJ_RTC_CACHE"])))))
"""


def test_a_second_process_finds_the_kernels_in_the_disk_cache(tmp_path):
    """Each process is a fresh child of this one (nothing replaces the program of a process that has opened the GPU)."""
    cache = tmp_path / "rtc"

    def run():
        env = dict(os.environ, HJ_RTC_CACHE=str(cache), HJ_TEST_ROOT=ROOT, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run([sys.executable, "-c", _CACHE_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])
    first = run()
    assert first["stats"] == [2, 0] and len(first["files"]) == 2            # the substep and the bound kernel, both compiled
    second = run()
    assert second["stats"] == [0, 2] and second["files"] == first["files"]  # both loaded, nothing compiled
    assert (second["sb"], second["sum"]) == (first["sb"], first["sum"])
