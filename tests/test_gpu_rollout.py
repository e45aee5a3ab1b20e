"""Many optimal trajectories in one launch (levelsetpy_amd/rollout.py, libhj_rollout.so) against the NumPy restatement
tests/rollout_ref.py, against computeOptTraj with the built-in systems' own dynSys methods, the host-loop fallback,
guarded-buffer runs, bad arguments and a census of the library's kernels.

UNPINNED throughout: the reference's computeOptTraj cannot run (levelsetpy_amd/opt_traj.py) and has no batched form.  The
value functions of the whole-horizon tests are solved on the CPU by oracle/hj_oracle.py (rollout_ref.solve_min_over_time),
so their inputs do not depend on the device.

Tolerances.  The double integrator has no trigonometry: every operation of the kernel is one the restatement states, and the
costates enter only through their signs -- exact equality.  Dubins and pendulum states pass through the device's sin / cos:
1e-12 absolute, where +-2 ulp in every sin / cos moves a state by about 2e-16 and a wrong control sign by about 1e-2.

Kernel -> test that launches it (each test asserts the name through hjr_last_kernel; test_census_of_the_rollout_library
checks the table against `nm -D libhj_rollout.so`):
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import computeOptTrajs  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _ffi, _marshal, _rffi, rollout  # noqa: E402

import query_ref as Q  # noqa: E402
import rollout_ref as R  # noqa: E402
from guarded_pool import GuardedPool, PlainAlloc, run_case  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {"float64": torch.float64, "float32": torch.float32}
ND = {"float64": np.float64, "float32": np.float32}
CT = {"float64": "double", "float32": "float"}
SCHEMES = {"ENO2": (L.upwindFirstENO2, 0), "ENO3": (L.upwindFirstENO3, 1), "WENO5_ASSHIPPED": (L.upwindFirstWENO5, 3)}
PLANT_ID = {"dubins": 0, "integrator": 1, "pendulum": 2}
PLANT_ND = {"dubins": 3, "integrator": 2, "pendulum": 4}
TOL = 1e-12

# kernel (as hjr_last_kernel names it: element type, scheme, plant) -> the test that launches it and asserts that name
CENSUS = dict(("rollout_kernel<%s, %d, %d>" % (ct, sid, pid), "test_one_control_step_on_every_plant_and_scheme")
              for ct in ("double", "float") for sid in (0, 1, 3) for pid in (0, 1, 2))
__doc__ += "\n".join("  %-34s %s" % kv for kv in sorted(CENSUS.items())) + "\n"


def launched(kernel, test):
    """The calling thread's last launch ran `kernel`, and the census credits it to `test`."""
    assert _rffi.last_kernel() == kernel, (_rffi.last_kernel(), kernel)
    assert CENSUS[kernel] == test


def dev(a, dtype="float64"):
    return torch.as_tensor(np.array(a), device="cuda").to(TD[dtype])        # (a copy: the shared cases are read-only)


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same(a, b):
    """Bit for bit, NaN equal to NaN (whatever its payload)."""
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------ shared cases and references
_CASES, _REFS = {}, {}


def integrator_case():
    """Grid 41^2 on [-1,1]^2, sphere target of radius 0.15, ENO3 + GLF, RK3 single steps at factorCFL 0.8 with minVOverTime,
    tau = linspace(0, 1, 21), flipped; the 8x8 lattice plus a state off the grid, one that leaves it and one in the target."""
    if "di" not in _CASES:
        from oracle import hj_oracle as O
        og = O.Grid([-1, -1], [1, 1], [41, 41], [])
        g = L.createGrid(np.array([[-1.], [-1.]]), np.array([[1.], [1.]]), np.array([[41], [41]]), None)
        tau = np.linspace(0, 1.0, 21)
        stack = R.solve_min_over_time(og, O.DoubleIntegrator(og, 1), O.shape_sphere(og, np.zeros((2, 1)), .15), tau, "ENO3")
        data = np.ascontiguousarray(stack[::-1])
        lat = np.linspace(-0.7, 0.7, 8)
        xs = np.array([[a, b] for a in lat for b in lat] + [[2.0, 0.0], [0.95, 0.9], [0.0, 0.0]])
        for a in (data, tau, xs):
            a.setflags(write=False)
        _CASES["di"] = (g, og, data, tau, xs)
    return _CASES["di"]


def integrator_ref(dtype):
    if ("di", dtype) not in _REFS:
        g, og, data, tau, xs = integrator_case()
        _REFS["di", dtype] = R.rollout_ref(og, data.astype(ND[dtype]), tau, "integrator", (1.0,), xs, 'min', 'min', 4, "ENO3")
    return _REFS["di", dtype]


def dubins_case():
    """The air3D box of examples/closed_loop_rollout.py on 21^3 nodes, periodic in axis 2, speed and turn 1, radius 0.5, ENO2,
    tau = linspace(0, 1, 11), flipped; of 256 drawn states the first 64 with V[0](x) < 0.15."""
    if "dub" not in _CASES:
        from oracle import hj_oracle as O
        n = 21
        gmin = np.array([[-.75, -1.25, -np.pi]]).T
        gmax = np.array([[3.25, 1.25, np.pi * (1 - 2 / n)]]).T
        og = O.Grid(gmin, gmax, [n] * 3, [2])
        g = L.createGrid(gmin, gmax, n * np.ones((3, 1), dtype=np.int64), 2)
        tau = np.linspace(0, 1.0, 11)
        stack = R.solve_min_over_time(og, O.DubinsRel(og, 1, 1), O.shape_cylinder(og, 2, np.zeros((3, 1)), .5), tau, "ENO2")
        data = np.ascontiguousarray(stack[::-1])
        lo, hi = np.array([0.0, -0.7, -np.pi]), np.array([1.6, 0.7, np.pi])
        draw = lo + np.random.default_rng(0).random((256, 3)) * (hi - lo)
        xs = draw[Q.eval_u_ref(og, data[0], draw) < 0.15][:64].copy()
        assert xs.shape == (64, 3)
        for a in (data, tau, xs):
            a.setflags(write=False)
        _CASES["dub"] = (g, og, data, tau, xs)
    return _CASES["dub"]


def smooth(g, seed=0):
    """A bent, asymmetric distance-like function, analytic and above -0.9: data[1] = data[0] + 1 then holds no state."""
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in g.vs], indexing='ij')
    r = np.sqrt(sum((x - 0.1 * (d + 1)) ** 2 for d, x in enumerate(xs)))
    return r + 0.2 * np.sin(2 * xs[0] + 0.3 * seed) * np.cos(xs[-1]) + 0.05 * np.sin(3.1 * xs[1] + 0.3) - 0.5


def plant_of(name, g):
    """(the package's system, the restatement's parameters)."""
    if name == "dubins":
        return L.DubinsVehicleRel(g, 0.75, 1.5), (0.75, 0.75, 1.5)
    if name == "integrator":
        return L.DoubleIntegrator(g, 0.8), (0.8,)
    return L.DoublePendulum4D(g, 1.25), (1.25,)


def padded(traj, T):
    out = np.full((traj.shape[0], T), np.nan)
    out[:, :traj.shape[1]] = traj
    return out


# ------------------------------------------------------------------------------------------ 1. whole horizon, bit for bit
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_double_integrator_whole_horizon_bitwise(where, dtype):
    """trajs, lengths, tEarliest and status equal the restatement EXACTLY, and every trajectory equals computeOptTraj's with
    DoubleIntegrator's own methods.  (A NumPy fp32 stack is widened to fp64 on its way to the device, as everywhere in the
    package: the fp64 kernel on fp32-rounded values.)"""
    g, og, data, tau, xs = integrator_case()
    rtraj, rlen, rte, rstat, _ = integrator_ref(dtype)
    lattice = rlen[:64]
    print("restatement: lengths %s, status counts %s" % (sorted(set(lattice.tolist())), np.bincount(rstat, minlength=3).tolist()))
    assert len(set(lattice.tolist())) >= 6                       # the inputs did not degenerate
    assert not np.isnan(rtraj[:64][np.arange(21)[None, None, :] < lattice[:, None, None] + np.zeros((1, 2, 1), dtype=int)]).any()
    assert rstat[64:].tolist() == [R.LEFT_GRID, R.LEFT_GRID, R.REACHED] and rlen[64:].tolist() == [21, 21, 1]
    d_in = data.astype(ND[dtype]) if where == "numpy" else dev(data, dtype)
    x_in = xs if where == "numpy" else dev(xs)
    plant = L.DoubleIntegrator(g, 1)
    plant.x = np.array([9.0, 9.0])
    args = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO3, tEarliest=True))
    trajs, lengths, ttau, outs = computeOptTrajs(g, d_in, tau, plant, x_in, args)
    assert _rffi.last_kernel() == "rollout_kernel<%s, 1, 1>" % ("double" if where == "numpy" else CT[dtype])
    assert outs.path == _rffi.last_kernel() and np.array_equal(plant.x, [9.0, 9.0]) and np.array_equal(ttau, tau)
    for a, dt in ((trajs, "float64"), (lengths, "int32"), (outs.tEarliest, "int32"), (outs.status, "int32")):
        assert (torch.is_tensor(a) and a.is_cuda) if where == "tensor" else isinstance(a, np.ndarray)
        assert str(a.dtype).endswith(dt)
    assert tuple(trajs.shape) == (67, 2, 21)
    err = np.nanmax(np.abs(np.nan_to_num(host(trajs)) - np.nan_to_num(rtraj)))
    flips = int((host(lengths) != rlen).sum())
    print("%s %s: max|traj - restatement| %.3e, %d lengths differ" % (where, dtype, err, flips))
    assert same(lengths, rlen), (host(lengths), rlen)
    assert same(outs.status, rstat) and same(outs.tEarliest, rte)
    assert same(trajs, rtraj), err
    # the default return has no extraOuts
    assert len(computeOptTrajs(g, d_in, tau, plant, x_in, L.Bundle(dict(uMode='min', derivFunc=L.upwindFirstENO3)))) == 3
    # each state through computeOptTraj with the system's own dynSys methods
    one = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO3))
    for m in range(67):
        sys_m = L.DoubleIntegrator(g, 1)
        sys_m.x = xs[m].copy()
        traj, t1 = L.computeOptTraj(g, d_in, tau, sys_m, one)
        assert traj.shape[1] == rlen[m] and np.array_equal(t1, tau[:rlen[m]]), (m, traj.shape, rlen[m])
        assert same(padded(traj, 21), host(trajs)[m]), m


# ------------------------------------------------------------------------------------------ 2. one control step, every kernel
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("plant", sorted(PLANT_ID))
def test_one_control_step_on_every_plant_and_scheme(plant, scheme, dtype):
    """T = 2 with data[1] = data[0] + 1, so tE = 0 is forced and the step is two sub-samples of {costate, controls, RK4} on
    smooth analytic data, for every periodic set and 200 states of query_ref.state_set (nodes, first / last cells, outside,
    periods away, the wrap cell).  Dubins and pendulum: within 1e-12 of the restatement; the double integrator: exactly."""
    fn, sid = SCHEMES[scheme]
    nd = PLANT_ND[plant]
    kernel = "rollout_kernel<%s, %d, %d>" % (CT[dtype], sid, PLANT_ID[plant])
    tau = np.array([0.0, 0.1])
    for k, pd in enumerate(Q.periodic_sets(nd)):
        g, og = Q.make_grids(Q.SHAPES[nd], pd)
        base = smooth(g, k).astype(ND[dtype])
        data = np.stack([base, base + ND[dtype](1)])
        xs = Q.state_set(g, 200)
        system, par = plant_of(plant, g)
        for uMode, dMode in (('max', 'min'), ('min', 'max')):
            rtraj, rlen, rte, rstat, fragile = R.rollout_ref(og, data, tau, plant, par, xs, uMode, dMode, 2, scheme)
            args = L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=2, derivFunc=fn, tEarliest=True))
            trajs, lengths, _, outs = computeOptTrajs(g, dev(data, dtype), tau, system, dev(xs), args)
            launched(kernel, "test_one_control_step_on_every_plant_and_scheme")
            got = host(trajs)
            assert (rlen == 2).all() and same(lengths, rlen) and same(outs.tEarliest, rte) and same(outs.status, rstat)
            assert np.array_equal(got[:, :, 0], xs)
            assert np.array_equal(np.isnan(got), np.isnan(rtraj)), (pd, uMode)
            ok = ~np.isnan(rtraj)
            err = float(np.max(np.abs(got[ok] - rtraj[ok])))
            print("%s %s %s pd=%s %s/%s: max|state - restatement| %.3e, %d fragile, %d NaN trajectories" % (
                plant, scheme, dtype, pd, uMode, dMode, err, int(fragile.sum()), int(np.isnan(rtraj[:, 0, 1]).sum())))
            if plant == "integrator":
                assert np.array_equal(got[ok], rtraj[ok]), (pd, uMode, err)
            else:
                assert err <= TOL, (pd, uMode, err)
        if not all(Q.periodic_axes(g)):
            assert np.isnan(rtraj[:, :, 1]).any() and (rstat == R.LEFT_GRID).any()


# ------------------------------------------------------------------------------------------ 3. whole horizon with trig
@gpu
@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_dubins_whole_horizon(where):
    """Within 1e-12 of the restatement, lengths and NaN patterns equal.  A trajectory is left out only if the restatement met a
    switching function with 0 < |s| < 1e-6 or a bisection value within 1e-6 of 1e-4; at most 4 of 64."""
    g, og, data, tau, xs = dubins_case()
    if "dub" not in _REFS:
        _REFS["dub"] = R.rollout_ref(og, data, tau, "dubins", (1.0, 1.0, 1.0), xs, 'max', 'min', 4, "ENO2")
    rtraj, rlen, rte, rstat, fragile = _REFS["dub"]
    keep = ~fragile
    print("restatement: %d of 64 fragile, lengths %s, %d leave the grid" % (
        int(fragile.sum()), sorted(set(rlen.tolist())), int((rstat == R.LEFT_GRID).sum())))
    assert fragile.sum() <= 4 and (rstat == R.LEFT_GRID).any() and len(set(rlen.tolist())) >= 3
    system = L.DubinsVehicleRel(g, 1, 1)
    args = L.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2, tEarliest=True))
    d_in, x_in = (data, xs) if where == "numpy" else (dev(data), dev(xs))
    trajs, lengths, _, outs = computeOptTrajs(g, d_in, tau, system, x_in, args)
    assert _rffi.last_kernel() == "rollout_kernel<double, 0, 0>"
    got = host(trajs)
    ok = ~np.isnan(rtraj[keep])
    err = float(np.max(np.abs(got[keep][ok] - rtraj[keep][ok])))
    print("%s: max|state - restatement| %.3e over %d trajectories" % (where, err, int(keep.sum())))
    assert np.array_equal(host(lengths)[keep], rlen[keep])
    assert np.array_equal(np.isnan(got[keep]), np.isnan(rtraj[keep]))
    assert np.array_equal(host(outs.status)[keep], rstat[keep]) and np.array_equal(host(outs.tEarliest)[keep], rte[keep])
    assert err <= TOL, err
    # one trajectory through computeOptTraj with the system's own methods: the same states up to the host's sin / cos
    m = int(np.nonzero(keep & (rlen >= 4) & (rstat != R.LEFT_GRID))[0][0])
    system.x = xs[m].copy()
    traj, _ = L.computeOptTraj(g, d_in, tau, system, L.Bundle(dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2)))
    assert traj.shape[1] == rlen[m] and float(np.max(np.abs(traj - got[m][:, :rlen[m]]))) <= TOL


# ------------------------------------------------------------------------------------------ 4. fallback
class _Plant(object):
    """xddot = u, |u| <= 1: a foreign class with the dynSys protocol of computeOptTraj."""

    def __init__(self, x=None):
        self.x = None if x is None else np.asarray(x, dtype=np.float64)

    def get_opt_u(self, t, deriv, uMode, x):
        s = np.sign(deriv[1]) if deriv[1] != 0 else 1.0
        return -s if uMode == 'min' else s

    def update_state(self, u, dt, x, d=None):
        k = lambda z: np.array([z[1], u])                                   # noqa: E731
        k1 = k(x); k2 = k(x + .5 * dt * k1); k3 = k(x + .5 * dt * k2); k4 = k(x + dt * k3)
        self.x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        return self.x


class _Lazy(L.DoubleIntegrator):
    """A subclass that overrides a protocol method: not the kernel's plant any more."""

    def get_opt_u(self, t, deriv, uMode, x):
        return 0.5 * L.DoubleIntegrator.get_opt_u(self, t, deriv, uMode, x)


@gpu
@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_foreign_plants_take_the_host_loop(where):
    g, og, data, tau, xs = integrator_case()
    pick = xs[[3, 12, 27, 36, 50, 64, 65, 66]]
    d_in, x_in = (data, pick) if where == "numpy" else (dev(data), dev(pick))
    args = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO3, tEarliest=True))
    computeOptTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in, args)
    before = _rffi.last_kernel()
    assert before == "rollout_kernel<double, 1, 1>" and rollout.last_path() == before
    for make in (lambda: _Plant(), lambda: _Lazy(g, 1)):
        plant = make()
        plant.x = np.array([7.0, 7.0])
        trajs, lengths, ttau, outs = computeOptTrajs(g, d_in, tau, plant, x_in, args)
        assert outs.path.startswith("host loop: ") and type(plant).__name__ in outs.path and rollout.last_path() == outs.path
        assert np.array_equal(plant.x, [7.0, 7.0])
        assert (torch.is_tensor(trajs) and trajs.is_cuda) if where == "tensor" else isinstance(trajs, np.ndarray)
        assert tuple(trajs.shape) == (8, 2, 21) and str(trajs.dtype).endswith("float64") and str(lengths.dtype).endswith("int32")
        for m in range(8):
            one = make()
            one.x = pick[m].copy()
            traj, t1 = L.computeOptTraj(g, d_in, tau, one, args)
            n = traj.shape[1]
            assert int(host(lengths)[m]) == n and same(host(trajs)[m], padded(traj, 21)), m
            want = R.LEFT_GRID if R.outside(og, traj.T).any() else (R.REACHED if n < 21 else R.EXHAUSTED)
            assert (want == R.LEFT_GRID) == (m in (5, 6)) and (want == R.REACHED or m != 7)
            assert int(host(outs.status)[m]) == want
            te = host(outs.tEarliest)[m]
            assert (te[min(n, 20):] == -1).all() and (te[:min(n, 20)] >= 0).all() and (np.diff(te[:min(n, 20)]) >= 0).all()
    # the built-in system on the kernel gives what its own methods give in the host loop (a derivFunc without a point kernel)
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    a = computeOptTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in, args)
    args_f = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=foreign, tEarliest=True))
    b = computeOptTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in[:3], args_f)
    assert b[3].path.startswith("host loop: derivFunc")
    assert same(host(a[0])[:3], b[0]) and same(host(a[1])[:3], b[1]) and same(host(a[3].status)[:3], b[3].status)
    assert same(host(a[3].tEarliest)[:3], b[3].tEarliest)


# ------------------------------------------------------------------------------------------ 5. bounds
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", 400 * 1000)
    return _POOLS[dtype]


def run_guarded(op, what):
    """run_case for an operation with arrays of three element types: op(F, S, arm) carves the fp64 arrays (states, traj, an
    fp64 stack) from F and the four-byte ones (an fp32 stack; the int32 outputs, as views of the fp32 pool, which compares
    bits) from S.  The fp64 pool drives run_case; the second pool is begun with the same fill and offset, checked after the
    call, and its results join the returned dict."""
    P32 = pool("float32")

    def both(a):
        b = P32.begin(a.fill, a.offset_elems) if isinstance(a, GuardedPool) else PlainAlloc(torch.float32, "cuda")
        res = dict(op(a, b, lambda: (a.arm(), b.arm())))
        if isinstance(a, GuardedPool):
            b.check()
        else:
            torch.cuda.synchronize()
        res.update(("s " + k, v) for k, v in b.results().items())
        return res
    return run_case(both, pool("float64"), what=what)[0]


def strided(data, stride, dtype, pad=-1e30):
    """The stack on the device, slices `stride` elements apart; the gaps hold a value that would change the result if read."""
    T = data.shape[0]
    n = data[0].size
    buf = torch.full(((T - 1) * stride + n,), pad, dtype=TD[dtype], device="cuda")
    d = dev(data.reshape(T, -1), dtype)
    for k in range(T):
        buf[k * stride:k * stride + n] = d[k]
    return buf


@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernel_stays_inside_its_arrays(dtype):
    """hjr_rollout on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 and with guards of NaN and
    +-1e30, an odd M and a field_stride larger than the field: guards intact, inputs unchanged, every element of every output
    written, the same bits as on fresh arrays.  The whole horizon in 2-D (4 lanes per trajectory) and one step in 4-D (16)."""
    lib = _rffi.lib()
    g2, _, data2, tau2, xs2 = integrator_case()
    g4, _ = Q.make_grids(Q.SHAPES[4], (3,))
    base4 = smooth(g4, 2)
    cases = [
        ("2-D", g2, data2, xs2, 1, _rffi.plant_descriptor(1, 0, 0, [1.0]), 4, float((tau2[1] - tau2[0]) / 4), "rollout_kernel<%s, 1, 1>"),
        ("4-D", g4, np.stack([base4, base4 + 1]), Q.state_set(g4, 131), 3, _rffi.plant_descriptor(2, 1, 0, [1.25]), 2, 0.05,
         "rollout_kernel<%s, 3, 2>"),
    ]
    for what, g, data, xs, sid, plant, sub, dt, kernel in cases:
        desc, N = _marshal.descriptor(g, dtype)
        T, n, M, nd = data.shape[0], data[0].size, xs.shape[0], g.dim
        assert M % 2 == 1
        stride = n + 3
        buf = strided(data, stride, dtype)
        x_t = dev(xs)

        def op(F, S, arm):
            a = (F if dtype == "float64" else S).inp("data", buf)
            x = F.inp("x0", x_t)
            traj = F.out("traj", (M, nd, T))
            length, te, status = S.out("length", (M,)), S.out("t_earliest", (M, T)), S.out("status", (M,))
            arm()
            _rffi.check(lib.hjr_rollout(C.byref(desc), sid, a.ptr, T, stride, x.ptr, M, sub, dt, C.byref(plant), traj.ptr,
                                        length.ptr, te.ptr, status.ptr, _stream()))
            return {"kernel": _rffi.last_kernel()}
        assert run_guarded(op, what)["kernel"] == kernel % CT[dtype]
        # the strided stack gives what the contiguous one gives, through the front end
        dense = rollout.rollout_states(g, dev(data, dtype), x_t, sid, sub, dt, plant, True)
        traj = torch.empty((M, nd, T), dtype=torch.float64, device="cuda")
        length, status = (torch.empty((M,), dtype=torch.int32, device="cuda") for _ in range(2))
        _rffi.check(lib.hjr_rollout(C.byref(desc), sid, p(buf), T, stride, p(x_t), M, sub, dt, C.byref(plant), p(traj), p(length),
                                    None, p(status), _stream()))                     # t_earliest is optional
        assert same(traj, dense[0]) and same(length, dense[1]) and same(status, dense[3])


# ------------------------------------------------------------------------------------------ 6. bad arguments, census
@gpu
def test_entry_point_refuses_bad_arguments():
    lib = _rffi.lib()
    g, og, data, tau, xs = integrator_case()
    desc, N = _marshal.descriptor(g, "float64")
    g3, _ = Q.make_grids(Q.SHAPES[3], ())
    desc3, _ = _marshal.descriptor(g3, "float64")
    d_t, x_t = dev(data), dev(xs[:5])
    T, n, M = 21, 41 * 41, 5
    traj = torch.full((M, 2, T), 5.0, dtype=torch.float64, device="cuda")
    ints = [torch.full(s, -77, dtype=torch.int32, device="cuda") for s in ((M,), (M, T), (M,))]
    di = _rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 0, 0, [1.0])
    dub = _rffi.plant_descriptor(_ffi.HAM_DUBINS_REL, 1, 0, [1.0, 1.0, 1.0, 2.0])

    def call(desc=desc, scheme=_ffi.ENO3, data=p(d_t), T=T, stride=n, x0=p(x_t), M=M, sub=4, dt=0.0125, plant=di,
             traj=p(traj), length=p(ints[0]), te=p(ints[1]), status=p(ints[2])):
        return lib.hjr_rollout(C.byref(desc) if desc is not None else None, scheme, data, T, stride, x0, M, sub, dt,
                               C.byref(plant) if plant is not None else None, traj, length, te, status, None)
    einval = [dict(data=None), dict(x0=None), dict(traj=None), dict(length=None), dict(status=None), dict(desc=None),
              dict(plant=None), dict(T=1), dict(T=0), dict(sub=0), dict(sub=-2), dict(plant=dub), dict(desc=desc3),
              dict(stride=n - 1), dict(M=-1), dict(dt=float("nan")),
              dict(plant=_rffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 2, 0, [1.0]))]
    for k, kw in enumerate(einval):
        assert call(**kw) == -1, kw
        assert lib.hjr_last_error(), kw
    for kw, word in ((dict(scheme=_ffi.WENO5), b"scheme"), (dict(scheme=9), b"scheme"),
                     (dict(plant=_rffi.plant_descriptor(_ffi.HAM_USER_BASE, 0, 0, [1.0])), b"plant")):
        assert call(**kw) == -3, kw
        assert word in lib.hjr_last_error()
    with pytest.raises(_ffi.Unsupported):
        _rffi.check(call(scheme=_ffi.WENO5))
    with pytest.raises(ValueError):
        _rffi.check(call(sub=0))
    assert call(M=0) == 0                                             # nothing to do: fine, and launches nothing
    torch.cuda.synchronize()
    assert bool((traj == 5.0).all()) and all(bool((a == -77).all()) for a in ints)          # no output was touched
    # the front end
    plant = L.DoubleIntegrator(g, 1)
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, tau[:-1], plant, x_t)                 # one time stamp short
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, tau[::-1], plant, x_t)                # descending
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, tau, plant, dev(np.zeros((4, 3))))    # states of another dimension
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, tau, plant, x_t, L.Bundle(dict(uMode='up')))
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, tau, plant, x_t, L.Bundle(dict(subSamples=0)))
    assert call() == 0 and _rffi.last_kernel() == "rollout_kernel<double, 1, 1>"
    torch.cuda.synchronize()
    assert not bool((traj == 5.0).any()) and not any(bool((a == -77).any()) for a in ints)   # a good call writes everything


@gpu
def test_census_of_the_rollout_library():
    """Every __device_stub__ of `nm -D libhj_rollout.so` is in CENSUS, and every entry names a test of this file that asserts
    the launch through hjr_last_kernel (the `launched(kernel, test)` calls)."""
    out = subprocess.check_output(["nm", "-D", "-C", _rffi.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+<[^>]*>)\(", out))
    assert stubs, "no kernels found in %s" % _rffi.LIB_PATH
    assert len(stubs) == 18 and stubs == set(CENSUS), (sorted(stubs - set(CENSUS)), sorted(set(CENSUS) - stubs))
    src = open(os.path.abspath(__file__)).read()
    for kernel, test in CENSUS.items():
        fn = globals().get(test)
        assert callable(fn), test
        body = src[src.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert 'launched(' in body and '"%s"' % test in body, test


def test_builtin_systems_speak_the_dynsys_protocol():
    """CPU: the new methods of the built-in systems against the restatement's formulas at random states and costates, every
    mode; sgn(0) = +1 and a NaN costate gives a NaN control; native_plant's identity rule."""
    from levelsetpy_amd.dynamics import native_plant
    rng = np.random.default_rng(3)
    for name in sorted(PLANT_ID):
        nd = PLANT_ND[name]
        g, _ = Q.make_grids(Q.SHAPES[nd], ())
        system, par = plant_of(name, g)
        assert system.x is None and native_plant(system) == system.native()
        controls, f, _ = R.PLANTS[name]
        X, P = rng.standard_normal((40, nd)), rng.standard_normal((40, nd))
        P[0] = 0.0
        P[1] = np.nan
        for uMode, dMode in (('max', 'min'), ('min', 'max')):
            c0, c1, _ = controls(par, P, X, uMode, dMode)
            for m in range(40):
                u = system.get_opt_u(0.0, P[m].tolist(), uMode, X[m])
                d = system.get_opt_v(0.0, P[m].tolist(), dMode, X[m])
                want_u = (c0[m], c1[m]) if name == "pendulum" else c0[m]
                assert same(np.array(u, dtype=np.float64), np.array(want_u, dtype=np.float64)), (name, m)
                assert (d is None) if name != "dubins" else same(np.float64(d), np.float64(c1[m]))
                if m >= 2:
                    xdot = system.dynamics(0.0, X[m], u, d)
                    assert np.max(np.abs(xdot - f(par, X[m:m + 1], c0[m:m + 1], c1[m:m + 1])[0])) <= 1e-13 * max(1.0, np.max(np.abs(xdot)))
                    new = system.update_state(u, 0.01, X[m], d)
                    want = R.rk4(lambda Z: f(par, Z, c0[m:m + 1], c1[m:m + 1]), X[m:m + 1], 0.01)[0]
                    assert new is system.x and np.max(np.abs(new - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))
                    if name == "integrator":
                        assert np.array_equal(new, want)
        with pytest.raises(ValueError):
            system.get_opt_u(0.0, P[2], 'up', X[2])
    g, _ = Q.make_grids(Q.SHAPES[2], ())
    assert native_plant(_Plant()) is None and native_plant(_Lazy(g, 1)) is None
    assert native_plant(L.DoubleIntegrator(g, np.array([1.0, 2.0]))) is None
    g3, _ = Q.make_grids(Q.SHAPES[3], ())
    vector = L.DubinsVehicleRel(g3, [1.0, 2.0], 1.0)
    assert native_plant(vector) is None
    with pytest.raises(ValueError):
        vector.get_opt_u(0.0, [0.1, 0.2, 0.3], 'max', np.zeros(3))
