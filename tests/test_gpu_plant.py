"""Rollouts of registered plants (levelsetpy_amd/plant.py, libhj_plant.so: user_rollout_kernel, compiled at run time) on the GPU.

  a. the five built-in plants registered again as text (tests/plant_cases.py) against their built-in kernels: one control step of every
     (scheme, dtype, uMode / dMode) and whole horizons on the stacks and the 64 states of tests/test_gpu_rollout.py and
     tests/test_gpu_hiquery.py -- traj, length, tEarliest and status bit for bit (the costate source, sin / cos and the statement order
     are the same), through computeOptTrajs and through the C ABI
  b. the planar quadrotor, which no built-in kernel serves: one control step and a whole horizon within 1e-12 of tests/rollout_ref.py,
     lengths, statuses and NaN patterns equal, and within 1e-12 of computeOptTraj with the object's own methods
  c. a plant with three controls and two disturbances, no trigonometry: equal to the restatement
  d. launch shapes and lifecycle: M = 0, 1, 5, 67, both element types, tEarliest null and given, two registrations used alternately, one
     object that solves fused and rolls out fused, the disk cache in a fresh child process
  e. guarded-buffer runs of hjp_rollout and hjp_rollout_hi
  f. every native refusal returns its code and leaves sentinel-filled outputs as they were

UNPINNED throughout: the reference's computeOptTraj cannot run (levelsetpy_amd/opt_traj.py) and has no batched form.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import computeOptTraj, computeOptTrajs, register_plant  # noqa: E402  (register_plant: the feature, missing before it)
from levelsetpy_amd import _ffi, _marshal, _pffi, _rffi, _xffi, hidim, rollout  # noqa: E402

import hiquery_cases as XC  # noqa: E402
import plant_cases as PC  # noqa: E402
import query_ref as Q  # noqa: E402
import rollout_ref as R  # noqa: E402
from guarded_pool import GuardedPool, PlainAlloc, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {"float64": torch.float64, "float32": torch.float32}
ND = {"float64": np.float64, "float32": np.float32}
SCHEMES = {"ENO2": (L.upwindFirstENO2, 0), "ENO3": (L.upwindFirstENO3, 1), "WENO5_ASSHIPPED": (L.upwindFirstWENO5, 3)}
MODES = (('max', 'min'), ('min', 'max'))
MODE_ID = {'min': 0, 'max': 1}
TOL = 1e-12


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
    return C.c_void_p(t.data_ptr()) if t is not None else None


def step_cases(name):
    """[(grid, oracle grid, two-slice analytic data (fp64), states)] for one control step of a plant: every periodic set of
    tests/test_gpu_rollout.py on the small shapes up to 4-D, the case of tests/test_gpu_hiquery.py at 5-D / 6-D."""
    nd = PC.BUILTIN[name][0] if name in PC.BUILTIN else {"lin": 4, "quad": 6}[name]
    out = []
    if name == "quad":
        g, og = PC.quad_grids()
        out.append((g, og, XC.smooth(g, 1), Q.state_set(g, 203)))
    elif nd >= 5:
        g, og = XC.grids(name)
        xs = Q.state_set(g, 203)
        xs[100, 0] = np.nan
        out.append((g, og, XC.smooth(g, 1), xs))
    else:
        for k, pd in enumerate(Q.periodic_sets(nd)):
            g, og = Q.make_grids(Q.SHAPES[nd], pd)
            out.append((g, og, XC.smooth(g, k), Q.state_set(g, 200)))
    return out


def both_ways(g, data_t, tau, xs_t, fn, sid, sub, system, desc, uMode, dMode):
    """(computeOptTrajs' (traj, length, tEarliest, status, path), the C ABI's (traj, length, tEarliest, status)) of one call."""
    args = L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=sub, derivFunc=fn, tEarliest=True))
    trajs, lengths, _, outs = computeOptTrajs(g, data_t, tau, system, xs_t, args)
    dt = (tau[1] - tau[0]) / sub
    return (trajs, lengths, outs.tEarliest, outs.status, outs.path), rollout.rollout_states(g, data_t, xs_t, sid, sub, dt, desc, True)


# ------------------------------------------------------------------------------------------ a. built-in plants, registered again
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("name", sorted(PC.BUILTIN))
def test_a_builtin_plant_registered_again_gives_the_builtin_kernels_bits(name, scheme, dtype):
    """One control step (T = 2 with data[1] = data[0] + 1, so tE = 0 is forced: two sub-samples of {costate, controls, RK4}) from 200 /
    203 states -- nodes, first / last cells, outside, periods away, the wrap cell, a NaN state.  Everything equal, NaN patterns included."""
    fn, sid = SCHEMES[scheme]
    reg = PC.register_builtin(name)
    par = PC.BUILTIN_PAR[name]
    tau = np.array([0.0, 0.1])
    hi = PC.BUILTIN[name][0] >= 5
    for g, og, base, xs in step_cases(name):
        base = base.astype(ND[dtype])
        data_t, xs_t = dev(np.stack([base, base + ND[dtype](1)]), dtype), dev(xs)
        builtin = PC.builtin_system(name, g)
        mine = PC.wrapped(reg, builtin, par)
        for uMode, dMode in MODES:
            bd = _rffi.plant_descriptor(PC.BUILTIN_ID[name], MODE_ID[uMode], MODE_ID[dMode], list(par))
            ud = _pffi.plant_descriptor(reg.plant_id, MODE_ID[uMode], MODE_ID[dMode], list(par))
            b_front, b_abi = both_ways(g, data_t, tau, xs_t, fn, sid, 2, builtin, bd, uMode, dMode)
            assert b_front[4] == (_xffi.rollout_kernel_name(dtype, sid, PC.BUILTIN_ID[name]) if hi else
                                  "rollout_kernel<%s, %d, %d>" % ("double" if dtype == "float64" else "float", sid, PC.BUILTIN_ID[name]))
            u_front, u_abi = both_ways(g, data_t, tau, xs_t, fn, sid, 2, mine, ud, uMode, dMode)
            assert u_front[4] == _pffi.kernel_name(dtype, sid, reg.name) == rollout.last_path() == _pffi.last_kernel()
            nan = int(np.isnan(host(b_front[0])[:, 0, 1]).sum())
            diff = int(((host(u_front[0]) != host(b_front[0])) & ~(np.isnan(host(u_front[0])) & np.isnan(host(b_front[0])))).sum())
            print("%s %s %s %s/%s: %d NaN trajectories, %d elements differ from the built-in kernel's" % (name, scheme, dtype, uMode, dMode, nan, diff))
            for k in range(4):
                assert same(u_front[k], b_front[k]), (name, uMode, k)
                assert same(u_abi[k], b_abi[k]) and same(u_abi[k], u_front[k]), (name, uMode, k)
            assert (host(u_front[1]) == 2).all()
        assert nan > 0 or all(Q.periodic_axes(g))


_HORIZONS = {}


def horizon_case(name):
    """(grid, data (time first, flipped), tau, 64+ states, system parameters, scheme, uMode, dMode) of the whole-horizon tests of
    tests/test_gpu_rollout.py (integrator, dubins) and tests/test_gpu_hiquery.py (pair6d): their stacks, their states."""
    if name not in _HORIZONS:
        if name == "pair6d":
            import test_gpu_hiquery as TH
            H = TH.horizon()
            _HORIZONS[name] = (H["g"], H["data"], H["tau"], H["xs"], XC.HORIZON_PAR, "ENO2", 'max', 'min')
        else:
            import test_gpu_rollout as TR
            if name == "integrator":
                g, og, data, tau, xs = TR.integrator_case()
                _HORIZONS[name] = (g, data, tau, xs, (1.0,), "ENO3", 'min', 'min')
            else:
                g, og, data, tau, xs = TR.dubins_case()
                _HORIZONS[name] = (g, data, tau, xs, (1.0, 1.0, 1.0), "ENO2", 'max', 'min')
    return _HORIZONS[name]


@pytest.mark.parametrize("name", ["integrator", "dubins", "pair6d"])
def test_a_builtin_plant_registered_again_whole_horizon(name):
    g, data, tau, xs, par, scheme, uMode, dMode = horizon_case(name)
    fn, sid = SCHEMES[scheme]
    reg = PC.register_builtin(name)
    builtin = PC.builtin_system(name, g, par)
    mine = PC.wrapped(reg, builtin, par)
    data_t, xs_t = dev(data), dev(xs)
    bd = _rffi.plant_descriptor(PC.BUILTIN_ID[name], MODE_ID[uMode], MODE_ID[dMode], list(par))
    ud = _pffi.plant_descriptor(reg.plant_id, MODE_ID[uMode], MODE_ID[dMode], list(par))
    b_front, b_abi = both_ways(g, data_t, tau, xs_t, fn, sid, 4, builtin, bd, uMode, dMode)
    u_front, u_abi = both_ways(g, data_t, tau, xs_t, fn, sid, 4, mine, ud, uMode, dMode)
    assert "rollout_kernel<double, %d, %d>" % (sid, PC.BUILTIN_ID[name]) in b_front[4]
    assert u_front[4] == _pffi.kernel_name("float64", sid, reg.name)
    lens = host(b_front[1])
    print("%s: lengths %s, status counts %s, %d elements differ from the built-in kernel's" % (
        name, sorted(set(lens.tolist())), np.bincount(host(b_front[3]), minlength=3).tolist(), int(((host(u_front[0]) != host(b_front[0]))
                                                                                                         & ~np.isnan(host(b_front[0]))).sum())))
    assert len(set(lens.tolist())) >= 2 and (host(b_front[3]) == R.LEFT_GRID).any()
    for k in range(4):
        assert same(u_front[k], b_front[k]), (name, k)
        assert same(u_abi[k], b_abi[k]) and same(u_abi[k], u_front[k]), (name, k)
    # NumPy in, NumPy out, the default return
    out = computeOptTrajs(g, data, tau, mine, xs[:9], L.Bundle(dict(uMode=uMode, dMode=dMode, derivFunc=fn)))
    assert len(out) == 3 and isinstance(out[0], np.ndarray) and same(out[0], host(b_front[0])[:9]) and same(out[1], host(b_front[1])[:9])
    # compare: the kernel against the host loop with the built-in system's own methods
    worst, nlen, nstat = reg.compare(mine, g, data_t, tau, xs[:6], L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=4, derivFunc=fn)))
    print("%s compare on 6 states: max deviation %.3e, %d lengths, %d statuses differ" % (name, worst, nlen, nstat))
    assert worst <= TOL and nlen == 0 and nstat == 0
    assert (worst == 0.0) or name != "integrator"


# ------------------------------------------------------------------------------------------ b. the quadrotor
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_quadrotor_one_control_step(scheme, dtype):
    """Within 1e-12 of the restatement (the project's bound for states that pass through the device's sin / cos: +-2 ulp in each moves
    a state by about 2e-16, a wrong thrust by about 1e-1); lengths, statuses, tEarliest and NaN patterns equal."""
    fn, sid = SCHEMES[scheme]
    reg = PC.register_quad()
    (g, og, base, xs), = step_cases("quad")
    base = base.astype(ND[dtype])
    data = np.stack([base, base + ND[dtype](1)])
    tau = np.array([0.0, 0.1])
    q = PC.quadrotor(g)
    for uMode in ('min', 'max'):
        rtraj, rlen, rte, rstat, fragile = R.rollout_ref(og, data, tau, "quad", PC.QUAD_PAR, xs, uMode, 'min', 2, scheme)
        args = L.Bundle(dict(uMode=uMode, subSamples=2, derivFunc=fn, tEarliest=True))
        trajs, lengths, _, outs = computeOptTrajs(g, dev(data, dtype), tau, q, dev(xs), args)
        assert outs.path == _pffi.kernel_name(dtype, sid, "planar_quad") == rollout.last_path()
        got = host(trajs)
        assert (rlen == 2).all() and same(lengths, rlen) and same(outs.tEarliest, rte) and same(outs.status, rstat)
        assert same(got[:, :, 0], xs)
        assert np.array_equal(np.isnan(got), np.isnan(rtraj)), uMode
        ok = ~np.isnan(rtraj)
        err = float(np.max(np.abs(got[ok] - rtraj[ok])))
        print("quadrotor %s %s %s: max|state - restatement| %.3e, %d fragile, %d NaN trajectories" % (
            scheme, dtype, uMode, err, int(fragile.sum()), int(np.isnan(rtraj[:, 0, 1]).sum())))
        assert err <= TOL, (uMode, err)
    assert np.isnan(rtraj[:, :, 1]).any() and (rstat == R.LEFT_GRID).any()


_QUAD = {}


def quad_horizon():
    """QUAD_N's grid, the disc target, five time stamps, solved by HJIPDE_solve with the registered Hamiltonian (ENO2, fused), flipped;
    64 states; the restatement.  One object carries both registrations."""
    if not _QUAD:
        g, og = PC.quad_grids()
        q = PC.quadrotor(g)
        sd = L.Bundle(dict(grid=g, hamFunc=q.hamiltonian, partialFunc=q.dissipation, dissFunc=L.artificialDissipationGLF, derivFunc=L.upwindFirstENO2))
        stack, tau, outs = L.HJIPDE_solve(PC.quad_target(og), PC.QUAD_TAU, sd, 'minVOverTime', L.Bundle(dict(quiet=True)))
        solved_by = hidim.last_path()
        stack = np.asarray(stack)
        assert stack.shape == (5,) + og.shape and np.array_equal(tau, PC.QUAD_TAU)
        data = np.ascontiguousarray(stack[::-1])
        xs = PC.quad_states(og)
        for a in (data, xs):
            a.setflags(write=False)
        ref = R.rollout_ref(og, data, PC.QUAD_TAU, "quad", PC.QUAD_PAR, xs, 'min', 'min', 4, "ENO2")
        _QUAD.update(g=g, og=og, q=q, data=data, xs=xs, ref=ref, tau=PC.QUAD_TAU, solved_by=solved_by)
    return _QUAD


@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_quadrotor_whole_horizon(where):
    """The kept trajectories within 1e-12 of the restatement with equal lengths, statuses, tEarliest and NaN patterns; a trajectory is set
    aside only if the restatement met a switching function with 0 < |s| < 1e-6 or a bisection value within 1e-6 of 1e-4, at most 4 of
    64.  Then every kept trajectory within 1e-12 of computeOptTraj with the object's own methods.  The same object was solved fused."""
    H = quad_horizon()
    g, q, data, xs, tau = H["g"], H["q"], H["data"], H["xs"], H["tau"]
    rtraj, rlen, rte, rstat, fragile = H["ref"]
    keep = ~fragile
    print("restatement: %d of 64 fragile, lengths %s, %d leave the grid" % (
        int(fragile.sum()), sorted(set(rlen.tolist())), int((rstat == R.LEFT_GRID).sum())))
    assert H["solved_by"] == "hidim_substep_kernel<double, HamUser:planar_quad, 0>"
    assert fragile.sum() <= 4 and (rstat == R.LEFT_GRID).any() and len(set(rlen.tolist())) >= 2
    args = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO2, tEarliest=True))
    d_in, x_in = (data, xs) if where == "numpy" else (dev(data), dev(xs))
    trajs, lengths, _, outs = computeOptTrajs(g, d_in, tau, q, x_in, args)
    assert outs.path == "user_rollout_kernel<double, 0, PlantUser:planar_quad>" == rollout.last_path() == _pffi.last_kernel()
    for a in (trajs, lengths, outs.status, outs.tEarliest):
        assert (torch.is_tensor(a) and a.is_cuda) if where == "tensor" else isinstance(a, np.ndarray)
    got = host(trajs)
    ok = ~np.isnan(rtraj[keep])
    err = float(np.max(np.abs(got[keep][ok] - rtraj[keep][ok])))
    print("%s: max|state - restatement| %.3e over %d trajectories" % (where, err, int(keep.sum())))
    assert np.array_equal(host(lengths)[keep], rlen[keep])
    assert np.array_equal(np.isnan(got[keep]), np.isnan(rtraj[keep]))
    assert np.array_equal(host(outs.status)[keep], rstat[keep]) and np.array_equal(host(outs.tEarliest)[keep], rte[keep])
    assert err <= TOL, err
    if where == "tensor":
        return
    one = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO2))
    worst = 0.0
    d_t = dev(data)
    for m in np.nonzero(keep)[0]:
        sys_m = PC.Quadrotor(g)
        sys_m.x = xs[m].copy()
        traj, t1 = computeOptTraj(g, d_t, tau, sys_m, one)
        assert traj.shape[1] == rlen[m] and np.array_equal(t1, tau[:rlen[m]]), (m, traj.shape, rlen[m])
        mine = got[m][:, :rlen[m]]
        assert np.array_equal(np.isnan(traj), np.isnan(mine)), m
        fin = ~np.isnan(mine)
        worst = max(worst, float(np.max(np.abs(traj[fin] - mine[fin]))) if fin.any() else 0.0)
    print("max|computeOptTraj - kernel| %.3e" % worst)
    assert worst <= TOL, worst
    # compare() says the same of 16 states, and has no threshold of its own
    w16, nlen, nstat = q._hj_plant.reg.compare(q, g, d_t, tau, xs[np.nonzero(keep)[0][:16]], one)
    print("compare on 16 states: %.3e, %d, %d" % (w16, nlen, nstat))
    assert w16 <= worst and nlen == 0 and nstat == 0
    assert q.x is None


# ------------------------------------------------------------------------------------------ c. three controls, two disturbances
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_control_vector_of_three_and_two(scheme, dtype):
    """No trigonometry: every operation of the kernel is one the restatement states, the costates enter only through their signs --
    equality, on (8, 7, 8, 7) with every periodic set, both mode pairs."""
    fn, sid = SCHEMES[scheme]
    reg = PC.register_lin()
    tau = np.array([0.0, 0.1])
    sys_ = reg(PC.LIN_PAR)
    for g, og, base, xs in step_cases("lin"):
        base = base.astype(ND[dtype])
        data = np.stack([base, base + ND[dtype](1)])
        for uMode, dMode in MODES:
            rtraj, rlen, rte, rstat, fragile = R.rollout_ref(og, data, tau, "lin", PC.LIN_PAR, xs, uMode, dMode, 2, scheme)
            args = L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=2, derivFunc=fn, tEarliest=True))
            trajs, lengths, _, outs = computeOptTrajs(g, dev(data, dtype), tau, sys_, dev(xs), args)
            assert outs.path == _pffi.kernel_name(dtype, sid, "lin_3u2d")
            bad = int((~((host(trajs) == rtraj) | (np.isnan(host(trajs)) & np.isnan(rtraj)))).sum())
            print("lin %s %s %s/%s: %d elements differ, %d fragile" % (scheme, dtype, uMode, dMode, bad, int(fragile.sum())))
            assert same(lengths, rlen) and same(outs.tEarliest, rte) and same(outs.status, rstat)
            assert same(trajs, rtraj), (uMode, dMode, bad)


# ------------------------------------------------------------------------------------------ d. launch and lifecycle
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_groups_that_do_not_fill_a_workgroup(dtype):
    """M = 0, 1, 5 and 67 on (9, 8) (4 lanes per trajectory: 64 fill a workgroup) and on (6, 5, 7, 5, 6, 8) (a wavefront each: 4 do),
    t_earliest null and given: the built-in kernel's bits for every M, and M = 0 launches nothing."""
    lib = _pffi.lib()
    for name in ("integrator", "pair6d"):
        reg = PC.register_builtin(name)
        par = PC.BUILTIN_PAR[name]
        g, og, base, xs = step_cases(name)[0]
        hi = g.dim >= 5
        base = base.astype(ND[dtype])
        data_t = dev(np.stack([base, base + ND[dtype](1)]), dtype)
        bd = _rffi.plant_descriptor(PC.BUILTIN_ID[name], 1, 0, list(par))
        ud = _pffi.plant_descriptor(reg.plant_id, 1, 0, list(par))
        desc, N = (_marshal.descriptor_hi if hi else _marshal.descriptor)(g, dtype)
        n = int(np.prod(N))
        call = lib.hjp_rollout_hi if hi else lib.hjp_rollout
        for M in (0, 1, 5, 67):
            xs_t = dev(xs[:M].reshape(M, g.dim))
            want = rollout.rollout_states(g, data_t, xs_t, 1, 2, 0.05, bd, True) if M else None
            got = rollout.rollout_states(g, data_t, xs_t, 1, 2, 0.05, ud, True)
            assert tuple(got[0].shape) == (M, g.dim, 2) and tuple(got[2].shape) == (M, 2)
            if M:
                assert all(same(a, b) for a, b in zip(got, want)), (name, M)
            # without t_earliest
            traj = torch.full((M, g.dim, 2), 5.0, dtype=torch.float64, device="cuda")
            length, status = (torch.full((M,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
            _pffi.check(call(C.byref(desc), 1, p(data_t), 2, n, p(xs_t), M, 2, 0.05, C.byref(ud), p(traj), p(length), None, p(status), _stream()))
            assert same(traj, got[0]) and same(length, got[1]) and same(status, got[3])
        _pffi.last_kernel()


def test_two_registrations_used_alternately():
    """On one grid, one after the other and again: each gives its own result (the built-in kernel's with that bound)."""
    g, og, base, xs = step_cases("integrator")[0]
    a = PC.register_builtin("integrator")
    dim, ctl, dyn, nu, nd, npar = PC.BUILTIN["integrator"]
    b = register_plant("integrator_twice", dim, ctl.replace("par[0] * sgn(p[1])", "2.0 * par[0] * sgn(p[1])"), dyn, nu, nd, npar)
    assert a.plant_id != b.plant_id
    data_t, xs_t = dev(np.stack([base, base + 1])), dev(xs)
    tau = np.array([0.0, 0.4])
    args = L.Bundle(dict(uMode='max', subSamples=2, derivFunc=L.upwindFirstENO3))
    want = [host(computeOptTrajs(g, data_t, tau, L.DoubleIntegrator(g, bound), xs_t, args)[0]) for bound in (0.8, 1.6)]
    assert not same(want[0], want[1])
    sa, sb = a([0.8]), b([0.8])
    for _ in range(2):
        ta = computeOptTrajs(g, data_t, tau, sa, xs_t, args)[0]
        assert rollout.last_path() == "user_rollout_kernel<double, 1, PlantUser:integrator_again>"
        tb = computeOptTrajs(g, data_t, tau, sb, xs_t, args)[0]
        assert rollout.last_path() == "user_rollout_kernel<double, 1, PlantUser:integrator_twice>"
        assert same(ta, want[0]) and same(tb, want[1])
    # the parameters are read at every call
    sa.params[0] = 1.6
    assert same(computeOptTrajs(g, data_t, tau, sa, xs_t, args)[0], want[1])


def test_other_objects_keep_the_host_loop():
    """A subclass that overrides a protocol method, and a derivative function without a point kernel: the host loop and its info line;
    the built-in systems keep their kernels."""
    g, og, base, xs = step_cases("integrator")[0]
    reg = PC.register_builtin("integrator")
    data_t, tau = dev(np.stack([base, base + 1])), np.array([0.0, 0.4])
    pick = dev(xs[[3, 50, 120]])

    class Lazy(L.PlantSystem):
        def get_opt_u(self, t, deriv, uMode, x):
            return 0.5 * L.PlantSystem.get_opt_u(self, t, deriv, uMode, x)
    di = L.DoubleIntegrator(g, 0.8)
    lazy = Lazy(reg, [0.8], dynamics=lambda s, t, x, u, d: di.dynamics(t, x, u, d), get_opt_u=lambda s, t, q, m, x: di.get_opt_u(t, q, m, x))
    args = L.Bundle(dict(uMode='max', subSamples=2, derivFunc=L.upwindFirstENO3, status=True))
    out = computeOptTrajs(g, data_t, tau, lazy, pick, args)
    assert out[3].path == "host loop: Lazy has no native plant" == rollout.last_path()
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    good = PC.wrapped(reg, di, [0.8])
    loop = computeOptTrajs(g, data_t, tau, good, pick, L.Bundle(dict(uMode='max', subSamples=2, derivFunc=foreign, status=True)))
    kern = computeOptTrajs(g, data_t, tau, good, pick, args)
    assert loop[3].path.startswith("host loop: derivFunc") and kern[3].path.startswith("user_rollout_kernel<double, 1,")
    assert same(host(loop[0]), host(kern[0])) and same(host(loop[1]), host(kern[1])) and same(host(loop[3].status), host(kern[3].status))
    assert computeOptTrajs(g, data_t, tau, di, pick, args)[3].path == "rollout_kernel<double, 1, 1>"


_CACHE_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["HJ_TEST_ROOT"], "tests"))
import levelsetpy_amd as L
import plant_cases as PC, hiquery_cases as XC, query_ref as Q
g, og = PC.quad_grids()
q = PC.quadrotor(g)
base = XC.smooth(g, 1)
out = L.computeOptTrajs(g, np.stack([base, base + 1]), np.array([0.0, 0.1]), q, Q.state_set(g, 67),
                        L.Bundle(dict(uMode='min', subSamples=2, derivFunc=L.upwindFirstENO3, status=True)))
print(json.dumps(dict(stats=L.plant_kernel_cache_stats(), path=out[3].path, sum=float(np.nansum(out[0])), nan=int(np.isnan(out[0]).sum()),
                      files=sorted(os.listdir(os.environ["HJ_RTC_CACHE"])))))
"""


def test_a_second_process_finds_the_kernel_in_the_disk_cache(tmp_path):
    """Each process is a fresh child of this one (nothing replaces the program of a process that has opened the GPU)."""
    cache = tmp_path / "rtc"

    def run():
        env = dict(os.environ, HJ_RTC_CACHE=str(cache), HJ_TEST_ROOT=ROOT, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        pr = subprocess.run([sys.executable, "-c", _CACHE_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr[-2000:]
        return json.loads(pr.stdout.strip().splitlines()[-1])
    first = run()
    assert first["stats"] == [1, 0] and len(first["files"]) == 1 and first["path"] == "user_rollout_kernel<double, 1, PlantUser:planar_quad>"
    second = run()
    assert second["stats"] == [0, 1] and second["files"] == first["files"]      # loaded, nothing compiled
    assert (second["sum"], second["nan"], second["path"]) == (first["sum"], first["nan"], first["path"])


# ------------------------------------------------------------------------------------------ e. bounds
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", 700 * 1000)
    return _POOLS[dtype]


def run_guarded(op, what):
    """tests/test_gpu_rollout.py's run_guarded: op(F, S, arm) carves the fp64 arrays from F and the four-byte ones (an fp32 stack; the
    int32 outputs, as views of the fp32 pool, which compares bits) from S."""
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


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernels_stay_inside_their_arrays(dtype):
    """hjp_rollout and hjp_rollout_hi on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 and with guards of NaN
    and +-1e30, an odd M and a field_stride larger than the field: guards intact, inputs unchanged, every element of every output
    written, the same bits as on fresh arrays.  A whole horizon in 2-D (4 lanes per trajectory), one step in 4-D (16) and in 6-D (64)."""
    lib = _pffi.lib()
    import test_gpu_rollout as TR
    g2, _, data2, tau2, xs2 = TR.integrator_case()
    g4, _ = Q.make_grids(Q.SHAPES[4], (3,))
    base4 = XC.smooth(g4, 2)
    g6, _ = PC.quad_grids()
    base6 = XC.smooth(g6, 2)
    ri, rl, rq = PC.register_builtin("integrator"), PC.register_lin(), PC.register_quad()
    cases = [
        ("2-D", g2, data2, xs2, 1, _pffi.plant_descriptor(ri.plant_id, 0, 0, [1.0]), 4, float((tau2[1] - tau2[0]) / 4), ri),
        ("4-D", g4, np.stack([base4, base4 + 1]), Q.state_set(g4, 131), 3, _pffi.plant_descriptor(rl.plant_id, 1, 0, list(PC.LIN_PAR)), 2, 0.05, rl),
        ("6-D", g6, np.stack([base6, base6 + 1]), Q.state_set(g6, 131), 0, _pffi.plant_descriptor(rq.plant_id, 0, 0, PC.QUAD_PAR), 2, 0.05, rq),
    ]
    for what, g, data, xs, sid, plant, sub, dt, reg in cases:
        hi = g.dim >= 5
        desc, N = (_marshal.descriptor_hi if hi else _marshal.descriptor)(g, dtype)
        call = lib.hjp_rollout_hi if hi else lib.hjp_rollout
        T, n, M, nd = data.shape[0], data[0].size, xs.shape[0], g.dim
        assert M % 2 == 1
        stride = n + 3
        buf = TR.strided(data, stride, dtype)
        x_t = dev(xs)

        def op(F, S, arm):
            a = (F if dtype == "float64" else S).inp("data", buf)
            x = F.inp("x0", x_t)
            traj = F.out("traj", (M, nd, T))
            length, te, status = S.out("length", (M,)), S.out("t_earliest", (M, T)), S.out("status", (M,))
            arm()
            _pffi.check(call(C.byref(desc), sid, a.ptr, T, stride, x.ptr, M, sub, dt, C.byref(plant), traj.ptr,
                             length.ptr, te.ptr, status.ptr, _stream()))
            return {"kernel": _pffi.last_kernel()}
        assert run_guarded(op, what)["kernel"] == _pffi.kernel_name(dtype, sid, reg.name)
        # the strided stack gives what the contiguous one gives, through the front end's call
        dense = rollout.rollout_states(g, dev(data, dtype), x_t, sid, sub, dt, plant, True)
        traj = torch.empty((M, nd, T), dtype=torch.float64, device="cuda")
        length, status = (torch.empty((M,), dtype=torch.int32, device="cuda") for _ in range(2))
        _pffi.check(call(C.byref(desc), sid, p(buf), T, stride, p(x_t), M, sub, dt, C.byref(plant), p(traj), p(length), None, p(status), _stream()))
        assert same(traj, dense[0]) and same(length, dense[1]) and same(status, dense[3])


# ------------------------------------------------------------------------------------------ f. refusals
@pytest.mark.parametrize("hi", [False, True])
def test_entry_points_refuse_bad_arguments(hi):
    """Every refusal returns its code, sets the text and leaves sentinel-filled outputs as they were."""
    lib = _pffi.lib()
    name = "pair6d" if hi else "integrator"
    reg = PC.register_builtin(name)
    other = PC.register_builtin("plane5d" if hi else "dubins")
    par = list(PC.BUILTIN_PAR[name])
    g, og, base, xs = step_cases(name)[0]
    g_other = step_cases("plane5d" if hi else "dubins")[0][0]
    desc, N = (_marshal.descriptor_hi if hi else _marshal.descriptor)(g, "float64")
    desc_other, _ = (_marshal.descriptor_hi if hi else _marshal.descriptor)(g_other, "float64")
    tiny, _ = (_marshal.descriptor_hi if hi else _marshal.descriptor)(g, "float64")
    tiny.N[0] = 2
    entry = lib.hjp_rollout_hi if hi else lib.hjp_rollout
    n, M, T, nd = int(np.prod(N)), 5, 2, g.dim
    d_t, x_t = dev(np.stack([base, base + 1])), dev(xs[:M])
    traj = torch.full((M, nd, T), 5.0, dtype=torch.float64, device="cuda")
    ints = [torch.full(s, -77, dtype=torch.int32, device="cuda") for s in ((M,), (M, T), (M,))]
    good = _pffi.plant_descriptor(reg.plant_id, 0, 0, par)

    def call(desc=desc, scheme=_ffi.ENO3, data=p(d_t), T=T, stride=n, x0=p(x_t), M=M, sub=2, dt=0.05, plant=good,
             traj=p(traj), length=p(ints[0]), te=p(ints[1]), status=p(ints[2])):
        return entry(C.byref(desc) if desc is not None else None, scheme, data, T, stride, x0, M, sub, dt,
                     C.byref(plant) if plant is not None else None, traj, length, te, status, None)
    einval = [dict(data=None), dict(x0=None), dict(traj=None), dict(length=None), dict(status=None), dict(desc=None), dict(plant=None),
              dict(T=1), dict(T=0), dict(sub=0), dict(stride=n - 1), dict(M=-1), dict(dt=float("nan")), dict(desc=tiny),
              dict(plant=_pffi.plant_descriptor(_pffi.PLANT_BASE + 99999, 0, 0, par)),              # an unknown id
              dict(plant=_pffi.plant_descriptor(_ffi.HAM_DOUBLE_INTEGRATOR, 0, 0, par)),            # a built-in plant's id is not one
              dict(plant=_pffi.plant_descriptor(_pffi.PLANT_BASE - 1, 0, 0, par)),
              dict(plant=_pffi.plant_descriptor(other.plant_id, 0, 0, list(PC.BUILTIN_PAR["plane5d" if hi else "dubins"]))),   # another dimension
              dict(desc=desc_other),
              dict(plant=_pffi.plant_descriptor(reg.plant_id, 0, 0, par + [1.0])),                  # a wrong parameter count
              dict(plant=_pffi.plant_descriptor(reg.plant_id, 2, 0, par))]
    for kw in einval:
        assert call(**kw) == -1, kw
        assert lib.hjp_last_error(), kw
    for kw in (dict(scheme=_ffi.WENO5), dict(scheme=9)):
        assert call(**kw) == -3, kw
        assert b"scheme" in lib.hjp_last_error()
    with pytest.raises(_ffi.Unsupported):
        _pffi.check(call(scheme=_ffi.WENO5))
    assert call(M=0) == 0                                             # nothing to do: fine, and launches nothing
    # the descriptor of the other width is refused by each entry point's own range
    torch.cuda.synchronize()
    assert bool((traj == 5.0).all()) and all(bool((a == -77).all()) for a in ints)          # no output was touched
    assert call() == 0 and _pffi.last_kernel() == _pffi.kernel_name("float64", 1, reg.name)
    torch.cuda.synchronize()
    assert not bool((traj == 5.0).any()) and not any(bool((a == -77).any()) for a in ints)   # a good call writes everything
    # a plant that does not compile: HJ_EINVAL at the launch, the message points into the body, nothing launched
    bad = register_plant("broken_%d" % nd, nd, "u[0] = 1.0;", "dx[0] = x[1];\ndx[1] = nope;", 1, 0, 0)
    traj.fill_(5.0)
    assert call(plant=_pffi.plant_descriptor(bad.plant_id, 0, 0, [])) == -1 and b"broken_%d:2:" % nd in lib.hjp_last_error()
    torch.cuda.synchronize()
    assert bool((traj == 5.0).all())
    # the front end
    sys_ = PC.wrapped(reg, PC.builtin_system(name, g), par)
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, np.array([0.0, 0.1]), sys_, x_t, L.Bundle(dict(uMode='up')))
    with pytest.raises(ValueError):
        computeOptTrajs(g, d_t, np.array([0.0, 0.1]), sys_, dev(np.zeros((4, nd + 1))))
