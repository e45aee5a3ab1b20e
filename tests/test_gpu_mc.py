"""Monte Carlo rollouts in one launch (levelsetpy_amd/montecarlo.py, libhj_mc.so) against the NumPy restatement tests/mc_ref.py,
against computeOptTrajs at zero noise, the generator on the device against the restatement's integer Philox, generated against
supplied normals, chunk independence, the moments of a discrete linear SDE, guarded-buffer runs, the host loop and bad arguments.

UNPINNED throughout: the reference has no counterpart.  The value functions are test_gpu_rollout.py's cases, solved on the CPU by
oracle/hj_oracle.py, so their inputs do not depend on the device.

Tolerances.  With supplied normals the double integrator has no transcendental function: every operation of the kernel is one the
restatement states -- exact equality.  Dubins and pendulum states pass through the device's sin / cos, generated normals through its
log / cos / sin: 1e-12 absolute, the project's rule wherever libm enters (a normal is below 8.6 in magnitude and +-2 ulp in log, cos
and sin move it by about 1e-15).  The Philox words are integers: exact.

Kernel -> test that launches it (test_one_noisy_step_on_every_plant_and_scheme asserts every name through hjn_last_kernel, and
test_census_of_the_mc_library checks the table against `nm -D libhj_mc.so`):
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
from levelsetpy_amd import computeStochTrajs, reachProbability  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _marshal, _nffi, _rffi, montecarlo  # noqa: E402

import mc_ref as MC  # noqa: E402
import query_ref as Q  # noqa: E402
import rollout_ref as R  # noqa: E402
from test_gpu_rollout import (integrator_case, dubins_case, smooth, plant_of, dev, host, same, run_guarded, strided, _stream,  # noqa: E402
                              SCHEMES, PLANT_ID, PLANT_ND, CT, ND, TD)
from test_mc_ref import moments_case, check_moments  # noqa: E402

gpu = pytest.mark.gpu
TOL = 1e-12
NAMES = ("final", "length", "status", "value_end", "value_min", "traj", "t_earliest")
FIELDS = dict(final="final", length="length", status="status", value_end="valueEnd", value_min="valueMin", traj="trajs",
              t_earliest="tEarliest")
# the grids of the one-step census: odd sizes, no two axes alike
STEP_SHAPES = {2: (9, 8), 3: (13, 11, 9), 4: (8, 7, 8, 7)}
G_FULL = {2: np.array([[0.03, -0.02], [0.01, 0.25]]),
          3: np.array([[0.05, 0.01, 0.0], [-0.02, 0.04, 0.01], [0.0, 0.03, 0.2]]),
          4: np.array([[0.02, 0.0, 0.01, 0.0], [0.05, 0.3, 0.0, -0.04], [0.0, 0.01, 0.02, 0.0], [0.03, 0.0, -0.05, 0.3]])}
G_DI = np.array([[0.02, 0.0], [0.01, 0.25]])           # the whole-horizon diffusion: chosen with the restatement (test 3's conditions)
SQRT2 = np.sqrt(2.0)


def sigma_of(G):
    """What the caller passes for a diffusion G: the front end forms sqrt(2) sigma, and front_G is that product."""
    return G / SQRT2


def front_G(G):
    return SQRT2 * sigma_of(G)


SIGMA_DI = sigma_of(G_DI)

CENSUS = dict(("noisy_rollout_kernel<%s, %d, %d>" % (ct, sid, pid), "test_one_noisy_step_on_every_plant_and_scheme")
              for ct in ("double", "float") for sid in (0, 1, 3) for pid in (0, 1, 2))
CENSUS["normals_kernel"] = "test_device_generator_equals_the_restatement"
__doc__ += "\n".join("  %-40s %s" % kv for kv in sorted(CENSUS.items())) + "\n"


def launched(kernel, test):
    assert _nffi.last_kernel() == kernel, (_nffi.last_kernel(), kernel)
    assert CENSUS[kernel] == test


def outputs(outs):
    """The Bundle's arrays under the restatement's names."""
    return {k: getattr(outs, FIELDS[k]) for k in NAMES}


def all_same(a, b, names=NAMES):
    bad = [k for k in names if not same(a[k], b[k])]
    return bad == [], bad


def device_normals(seed, first, count, step0, nsteps, nd, words=False):
    z = torch.empty((count, nsteps, nd), dtype=torch.float64, device="cuda")
    w = torch.empty((count, nsteps, (nd + 1) // 2, 4), dtype=torch.int32, device="cuda") if words else None
    _nffi.check(_nffi.lib().hjn_normals(seed, first, count, step0, nsteps, nd, C.c_void_p(w.data_ptr()) if words else None,
                                        C.c_void_p(z.data_ptr()), _stream()))
    return (z, w.cpu().numpy().view(np.uint32)) if words else z


_REFS = {}


def di_args(**kw):
    d = dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO3, keepTrajs=True)
    d.update(kw)
    return L.Bundle(d)


def di_normals():
    if "xi" not in _REFS:
        xi = np.random.default_rng(11).standard_normal((67, 3, 80, 2))
        xi.setflags(write=False)
        _REFS["xi"] = xi
    return _REFS["xi"]


def di_ref(policy, dtype):
    if (policy, dtype) not in _REFS:
        g, og, data, tau, xs = integrator_case()
        _REFS[policy, dtype] = MC.mc_ref(og, data.astype(ND[dtype]), tau, "integrator", (1.0,), xs, front_G(G_DI), 3,
                                         xi=di_normals(), policy=policy, subSamples=4, scheme="ENO3")
    return _REFS[policy, dtype]


# ------------------------------------------------------------------------------------------ 1. the generator
@gpu
@pytest.mark.parametrize("nd", [2, 3, 4])
@pytest.mark.parametrize("first", [0, 2 ** 32 - 3, 2 ** 40])
def test_device_generator_equals_the_restatement(first, nd):
    seed = 0x299f31d0a4093822
    z, w = device_normals(seed, first, 300, 5, 7, nd, words=True)          # 300 x 7 x pairs threads: more than one block
    launched("normals_kernel", "test_device_generator_equals_the_restatement")
    rw = MC.words(seed, first, 300, 5, 7, nd)
    assert np.array_equal(w, rw)
    err = float(np.max(np.abs(host(z) - MC.normals_of(rw, nd))))
    print("first %d nd %d: max|device normal - restatement| %.3e" % (first, nd, err))
    assert err <= TOL
    zh = _nffi.normals_host(seed, first, 300, 5, 7, nd)
    print("              max|device normal - host library| %.3e" % float(np.max(np.abs(host(z) - zh))))
    assert float(np.max(np.abs(host(z) - zh))) <= TOL
    only = device_normals(seed, first, 300, 5, 7, nd)                       # words are optional
    assert same(only, z)


# ------------------------------------------------------------------------------------------ 2. zero noise
@gpu
def test_zero_G_equals_computeOptTrajs():
    g, og, data, tau, xs = integrator_case()
    plant = L.DoubleIntegrator(g, 1)
    trajs, lengths, _, o = L.computeOptTrajs(g, dev(data), tau, plant, dev(xs),
                                             L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO3, tEarliest=True)))
    outs = computeStochTrajs(g, dev(data), tau, plant, dev(xs), np.zeros((2, 2)), di_args(realisations=3, seed=12345))
    assert outs.path == "noisy_rollout_kernel<double, 1, 1>" == montecarlo.last_path() and outs.seed == 12345
    assert tuple(outs.trajs.shape) == (67, 3, 2, 21) and np.array_equal(outs.tau, tau)
    for k in range(3):
        assert same(outs.trajs[:, k], trajs) and same(outs.length[:, k], lengths) and same(outs.status[:, k], o.status)
        assert same(outs.tEarliest[:, k], o.tEarliest)


# ------------------------------------------------------------------------------------------ 3. whole horizon, supplied normals
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("where", ["numpy", "tensor"])
@pytest.mark.parametrize("policy", ["earliest", "clock"])
def test_supplied_normals_whole_horizon_bitwise(policy, where, dtype):
    g, og, data, tau, xs = integrator_case()
    ref = di_ref(policy, dtype)
    free = R.rollout_ref(og, data.astype(ND[dtype]), tau, "integrator", (1.0,), xs, 'min', 'min', 4, "ENO3")
    moving = (free[1] > 1) & np.isfinite(ref["traj"][:, 0, 0, 1])
    print("restatement %s %s: lengths %s, status counts %s, %d lengths differ from the noise-free ones" % (
        policy, dtype, sorted(set(ref["length"].ravel().tolist())), np.bincount(ref["status"].ravel(), minlength=3).tolist(),
        int((ref["length"] != free[1][:, None]).sum())))
    if policy == "earliest":                                     # the inputs did not degenerate
        assert moving.sum() >= 50
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert (ref["traj"][moving, a, :, 1] != ref["traj"][moving, b, :, 1]).any(axis=1).all()
        assert len(set(ref["length"].ravel().tolist())) >= 6 and (ref["length"] != free[1][:, None]).any()
        assert set(ref["status"].ravel().tolist()) == {R.REACHED, R.EXHAUSTED, R.LEFT_GRID}
    else:
        assert (ref["length"] == 21).all() and set(ref["status"].ravel().tolist()) == {R.EXHAUSTED, R.LEFT_GRID}
        assert (ref["t_earliest"] == np.r_[np.arange(20), -1]).all()
    d_in = data.astype(ND[dtype]) if where == "numpy" else dev(data, dtype)
    x_in, n_in = (xs, di_normals()) if where == "numpy" else (dev(xs), dev(di_normals()))
    plant = L.DoubleIntegrator(g, 1)
    plant.x = np.array([9.0, 9.0])
    outs = computeStochTrajs(g, d_in, tau, plant, x_in, SIGMA_DI, di_args(realisations=3, normals=n_in, policy=policy))
    assert outs.path == "noisy_rollout_kernel<%s, 1, 1>" % ("double" if where == "numpy" else CT[dtype])
    assert np.array_equal(plant.x, [9.0, 9.0])
    got = outputs(outs)
    for k, a in got.items():
        assert (torch.is_tensor(a) and a.is_cuda) if where == "tensor" else isinstance(a, np.ndarray), k
        assert str(a.dtype).endswith("int32" if k in ("length", "status", "t_earliest") else "float64"), k
    ok, bad = all_same(got, ref)
    assert ok, bad
    p, se = reachProbability(outs, 0.0, 'min')
    want = (ref["value_min"] < 0.0).mean(axis=1)
    assert np.array_equal(host(p), want) and np.allclose(host(se), np.sqrt(want * (1 - want) / 3), rtol=0, atol=1e-15)
    assert (torch.is_tensor(p) and p.is_cuda) if where == "tensor" else isinstance(p, np.ndarray)
    assert np.array_equal(host(reachProbability(outs)[0]), (ref["value_end"] < 0.0).mean(axis=1))


# ------------------------------------------------------------------------------------------ 4. one noisy step, every kernel
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("plant", sorted(PLANT_ID))
def test_one_noisy_step_on_every_plant_and_scheme(plant, scheme, dtype):
    """T = 2 with data[1] = data[0] + 1: two sub-samples of {costate, controls, RK4, noise} on smooth analytic data with a full G, for
    every periodic set, 120 states of query_ref.state_set and two realisations.  Integrator: exactly; Dubins, pendulum: 1e-12."""
    fn, sid = SCHEMES[scheme]
    nd = PLANT_ND[plant]
    kernel = "noisy_rollout_kernel<%s, %d, %d>" % (CT[dtype], sid, PLANT_ID[plant])
    tau = np.array([0.0, 0.1])
    G = G_FULL[nd]
    worst = 0.0
    for k, pd in enumerate(Q.periodic_sets(nd)):
        g, og = Q.make_grids(STEP_SHAPES[nd], pd)
        base = smooth(g, k).astype(ND[dtype])
        data = np.stack([base, base + ND[dtype](1)])
        xs = Q.state_set(g, 120)
        xi = np.random.default_rng(k).standard_normal((120, 2, 2, nd))
        system, par = plant_of(plant, g)
        uMode, dMode, policy = (('max', 'min', 'earliest'), ('min', 'max', 'clock'))[k % 2]
        ref = MC.mc_ref(og, data, tau, plant, par, xs, front_G(G), 2, xi=xi, policy=policy, uMode=uMode, dMode=dMode, subSamples=2, scheme=scheme)
        args = L.Bundle(dict(uMode=uMode, dMode=dMode, subSamples=2, derivFunc=fn, keepTrajs=True, realisations=2, normals=dev(xi),
                             policy=policy))
        outs = computeStochTrajs(g, dev(data, dtype), tau, system, dev(xs), sigma_of(G), args)
        launched(kernel, "test_one_noisy_step_on_every_plant_and_scheme")
        got = {k2: host(v) for k2, v in outputs(outs).items()}
        assert (ref["length"] == 2).all() and all_same(got, ref, ("length", "status", "t_earliest"))[0], pd
        assert np.array_equal(got["traj"][:, :, :, 0], np.repeat(xs[:, None], 2, axis=1))
        for name in ("final", "traj", "value_end", "value_min"):
            assert np.array_equal(np.isnan(got[name]), np.isnan(ref[name])), (name, pd)
            ok = ~np.isnan(ref[name])
            if plant == "integrator":
                assert np.array_equal(got[name][ok], ref[name][ok]), (name, pd)
            else:
                worst = max(worst, float(np.max(np.abs(got[name][ok] - ref[name][ok]))))
        assert np.array_equal(got["final"], got["traj"][:, :, :, 1], equal_nan=True)
        if not all(Q.periodic_axes(g)):
            assert np.isnan(ref["final"]).any() and (ref["status"] == R.LEFT_GRID).any()
    print("%s %s %s: max|output - restatement| %.3e" % (plant, scheme, dtype, worst))
    assert worst <= TOL


# ------------------------------------------------------------------------------------------ 5. generated against supplied
@gpu
@pytest.mark.parametrize("case", ["integrator", "dubins"])
def test_generated_normals_equal_supplied_ones(case):
    """A call with a seed equals the same call fed hjn_normals' output for that seed, in every output, bit for bit; a repeated call
    gives the same bits; another seed gives other paths.  Dubins: an odd number of normals a step."""
    if case == "integrator":
        g, og, data, tau, xs = integrator_case()
        system, sigma, base = L.DoubleIntegrator(g, 1), SIGMA_DI, dict(uMode='min', derivFunc=L.upwindFirstENO3)
    else:
        g, og, data, tau, xs = dubins_case()
        system, sigma, base = L.DubinsVehicleRel(g, 1, 1), sigma_of(G_FULL[3]), dict(uMode='max', dMode='min', derivFunc=L.upwindFirstENO2)
    M, T, nd, Rn, seed, first = xs.shape[0], len(tau), g.dim, 3, 2 ** 63 + 77, 2 ** 32 - 40
    nsteps = (T - 1) * 4
    base.update(subSamples=4, keepTrajs=True, realisations=Rn, firstRealisation=first)
    z = device_normals(seed, first, M * Rn, 0, nsteps, nd).reshape(M, Rn, nsteps, nd)
    for policy in ("earliest", "clock"):
        a = outputs(computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma, L.Bundle(dict(base, seed=seed, policy=policy))))
        b = outputs(computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma, L.Bundle(dict(base, normals=z, policy=policy))))
        ok, bad = all_same(a, b)
        assert ok, (policy, bad)
        again = outputs(computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma, L.Bundle(dict(base, seed=seed, policy=policy))))
        assert all_same(a, again)[0]
        other = outputs(computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma, L.Bundle(dict(base, seed=seed + 1, policy=policy))))
        assert not same(a["final"], other["final"])
    # NumPy normals from the host library drive the same paths up to the two sides' log / cos / sin
    if case == "integrator":
        zh = _nffi.normals_host(seed, first, M * Rn, 0, nsteps, nd).reshape(M, Rn, nsteps, nd)
        assert float(np.max(np.abs(zh - host(z)))) <= TOL


# ------------------------------------------------------------------------------------------ 6. chunk independence
@gpu
def test_results_do_not_depend_on_the_chunking(monkeypatch):
    g, og, data, tau, xs = integrator_case()
    plant = L.DoubleIntegrator(g, 1)
    d_t, x_t = dev(data), dev(xs)
    full = outputs(computeStochTrajs(g, d_t, tau, plant, x_t, SIGMA_DI, di_args(realisations=5, seed=7, firstRealisation=1000)))
    # states [a:b] with firstRealisation = first + a R are the slice of the full call
    for a, b in ((0, 9), (9, 40), (40, 67)):
        part = outputs(computeStochTrajs(g, d_t, tau, plant, x_t[a:b], SIGMA_DI,
                                         di_args(realisations=5, seed=7, firstRealisation=1000 + a * 5)))
        assert all(same(part[k], full[k][a:b]) for k in NAMES), (a, b)
    # R = 5 is R = 2 and then R = 3 with the offset (one state: its realisations are consecutive)
    for m in (3, 30, 65):
        two = outputs(computeStochTrajs(g, d_t, tau, plant, x_t[m:m + 1], SIGMA_DI, di_args(realisations=2, seed=7, firstRealisation=1000 + m * 5)))
        three = outputs(computeStochTrajs(g, d_t, tau, plant, x_t[m:m + 1], SIGMA_DI,
                                          di_args(realisations=3, seed=7, firstRealisation=1000 + m * 5 + 2)))
        assert all(same(torch.cat([two[k], three[k]], dim=1), full[k][m:m + 1]) for k in NAMES), m
    # a launch limit the call exceeds: the front end splits over states (10 states a launch here), with and without paths
    monkeypatch.setattr(montecarlo, "LAUNCH_THREADS", 4 * 5 * 10)
    split = outputs(computeStochTrajs(g, d_t, tau, plant, x_t, SIGMA_DI, di_args(realisations=5, seed=7, firstRealisation=1000)))
    assert all(same(split[k], full[k]) for k in NAMES)
    lean = outputs(computeStochTrajs(g, d_t, tau, plant, x_t, SIGMA_DI, di_args(realisations=5, seed=7, firstRealisation=1000, keepTrajs=False)))
    assert lean["traj"] is None and lean["t_earliest"] is None and all(same(lean[k], full[k]) for k in NAMES[:5])
    xi = dev(di_normals())
    a = outputs(computeStochTrajs(g, d_t, tau, plant, x_t, SIGMA_DI, di_args(realisations=3, normals=xi)))
    assert all_same(a, di_ref("earliest", "float64"))[0]                     # supplied normals are sliced with the states


# ------------------------------------------------------------------------------------------ 7. moments
@gpu
def test_moments_of_the_discrete_linear_sde_on_the_device():
    """test_mc_ref.py's case with generated normals: the same closed forms, the same 4 standard errors, the same condition."""
    og, data, tau, x0, G, want = moments_case()
    g = L.createGrid(np.array([[-2.], [-2.]]), np.array([[2.], [2.]]), np.array([[41], [41]]), None)
    args = L.Bundle(dict(uMode='min', subSamples=4, derivFunc=L.upwindFirstENO2, realisations=65536, seed=20261021, policy='clock'))
    outs = computeStochTrajs(g, dev(data), tau, L.DoubleIntegrator(g, 0), dev(x0), sigma_of(G), args)
    assert outs.path == "noisy_rollout_kernel<double, 0, 1>" and outs.trajs is None and outs.tEarliest is None
    assert tuple(outs.final.shape) == (1, 65536, 2) and bool((outs.length == 11).all())
    check_moments(host(outs.final)[0], host(outs.status)[0], want, "device")


# ------------------------------------------------------------------------------------------ 8. outputs without the paths
@gpu
def test_values_and_lean_outputs():
    """keepTrajs=False leaves the other outputs unchanged; valueEnd and valueMin are eval_u of the target function on the kept paths."""
    g, og, data, tau, xs = dubins_case()
    system = L.DubinsVehicleRel(g, 1, 1)
    base = dict(uMode='max', dMode='min', subSamples=4, derivFunc=L.upwindFirstENO2, realisations=4, seed=3)
    for policy in ("earliest", "clock"):
        kept = outputs(computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma_of(G_FULL[3]), L.Bundle(dict(base, keepTrajs=True, policy=policy))))
        lean = computeStochTrajs(g, dev(data), tau, system, dev(xs), sigma_of(G_FULL[3]), L.Bundle(dict(base, policy=policy)))
        assert lean.trajs is None and lean.tEarliest is None and all(same(outputs(lean)[k], kept[k]) for k in NAMES[:5])
        traj, length = host(kept["traj"]), host(kept["length"])
        M, Rn, nd, T = traj.shape
        states = traj.transpose(0, 1, 3, 2).reshape(-1, nd)
        finite = np.isfinite(states).all(axis=1)
        v = np.full(states.shape[0], np.nan)
        v[finite] = host(L.eval_u(g, dev(data[-1]), dev(states[finite])))
        v = v.reshape(M, Rn, T)
        recorded = np.arange(T)[None, None, :] < length[:, :, None]
        want_min = np.full((M, Rn), np.nan)
        want_end = np.empty((M, Rn))
        for m in range(M):
            for k in range(Rn):
                vals = v[m, k, :length[m, k]]
                want_end[m, k] = vals[-1]
                want_min[m, k] = np.nan if np.isnan(vals).any() else vals.min()
        assert same(kept["value_end"], want_end) and same(kept["value_min"], want_min)
        assert same(kept["final"], traj[np.arange(M)[:, None], np.arange(Rn)[None, :], :, length - 1])
        assert np.isnan(traj[~np.broadcast_to(recorded[:, :, None, :], traj.shape)]).all()
        assert (host(kept["status"]) == R.LEFT_GRID).any() and np.isnan(want_min).any()


# ------------------------------------------------------------------------------------------ 9. bounds
@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kernels_stay_inside_their_arrays(dtype):
    """hjn_rollout and hjn_normals on views carved from tests/guarded_pool.py's pools, at element offsets 0-3 and with guards of NaN
    and +-1e30, odd counts and a field_stride larger than the field: guards intact, inputs unchanged, every element of every output
    written, the same bits as on fresh arrays.  The whole horizon in 2-D and one step in 4-D, with and without the paths, supplied
    and generated normals."""
    lib = _nffi.lib()
    g2, _, data2, tau2, xs2 = integrator_case()
    g4, _ = Q.make_grids(Q.SHAPES[4], (3,))
    base4 = smooth(g4, 2)
    cases = [
        ("2-D", g2, data2, xs2[:33], 1, _rffi.plant_descriptor(1, 0, 0, [1.0]), 4, float((tau2[1] - tau2[0]) / 4), G_DI, 0,
         "noisy_rollout_kernel<%s, 1, 1>"),
        ("4-D", g4, np.stack([base4, base4 + 1]), Q.state_set(g4, 45), 3, _rffi.plant_descriptor(2, 1, 0, [1.25]), 2, 0.05, G_FULL[4], 1,
         "noisy_rollout_kernel<%s, 3, 2>"),
    ]
    for what, g, data, xs, sid, plant, sub, dt, G, policy, kernel in cases:
        desc, N = _marshal.descriptor(g, dtype)
        T, n, M, nd, Rn = data.shape[0], data[0].size, xs.shape[0], g.dim, 3
        assert (M * Rn) % 2 == 1
        stride = n + 3
        buf = strided(data, stride, dtype)
        x_t = dev(xs)
        nsteps = (T - 1) * sub
        xi_t = dev(np.random.default_rng(5).standard_normal((M, Rn, nsteps, nd)))
        Gm = np.ascontiguousarray(G)
        for paths in (True, False):
            for supplied in (True, False):
                def op(F, S, arm):
                    a = (F if dtype == "float64" else S).inp("data", buf)
                    x = F.inp("x0", x_t)
                    z = F.inp("normals", xi_t) if supplied else None
                    final, vend, vmin = F.out("final", (M, Rn, nd)), F.out("value_end", (M, Rn)), F.out("value_min", (M, Rn))
                    length, status = S.out("length", (M, Rn)), S.out("status", (M, Rn))
                    traj = F.out("traj", (M, Rn, nd, T)) if paths else None
                    te = S.out("t_earliest", (M, Rn, T)) if paths else None
                    arm()
                    _nffi.check(lib.hjn_rollout(C.byref(desc), sid, a.ptr, T, stride, x.ptr, M, Rn, 2 ** 32 - 20, 99, z.ptr if supplied else None,
                                                Gm.ctypes.data, float(np.sqrt(dt)), policy, sub, dt, C.byref(plant), final.ptr, length.ptr,
                                                status.ptr, vend.ptr, vmin.ptr, traj.ptr if paths else None, te.ptr if paths else None,
                                                _stream()))
                    return {"kernel": _nffi.last_kernel()}
                assert run_guarded(op, "%s paths=%s supplied=%s" % (what, paths, supplied))["kernel"] == kernel % CT[dtype]

    if dtype == "float64":
        for nd in (1, 3, 4):
            def op(F, S, arm):
                z, w = F.out("normals", (37, 5, nd)), S.out("words", (37, 5, (nd + 1) // 2, 4))
                arm()
                _nffi.check(lib.hjn_normals(5, 2 ** 32 - 9, 37, 3, 5, nd, w.ptr, z.ptr, _stream()))
                return {"kernel": _nffi.last_kernel()}
            assert run_guarded(op, "normals nd=%d" % nd)["kernel"] == "normals_kernel"


# ------------------------------------------------------------------------------------------ 10. the host loop
class _Own(L.DoubleIntegrator):
    """A subclass that overrides a protocol method (with the same result): not the kernel's plant any more."""

    def get_opt_u(self, t, deriv, uMode, x):
        return L.DoubleIntegrator.get_opt_u(self, t, deriv, uMode, x)


@gpu
@pytest.mark.parametrize("where", ["numpy", "tensor"])
def test_foreign_systems_take_the_host_loop(where):
    import plant_cases as PC
    g, og, data, tau, xs = integrator_case()
    idx = [3, 27, 50, 64, 65, 66]
    pick, xi = xs[idx], di_normals()[idx][:, :2]
    d_in, x_in, n_in = (data, pick, xi) if where == "numpy" else (dev(data), dev(pick), dev(xi))
    registered = PC.wrapped(PC.register_builtin("integrator"), L.DoubleIntegrator(g, 1), (1.0,))
    for policy in ("earliest", "clock"):
        args = di_args(realisations=2, normals=n_in, policy=policy)
        native = computeStochTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in, SIGMA_DI, args)
        assert native.path == "noisy_rollout_kernel<double, 1, 1>"
        for system, word in ((_Own(g, 1), "_Own"), (registered, "registered plant")):
            system.x = np.array([7.0, 7.0])
            outs = computeStochTrajs(g, d_in, tau, system, x_in, SIGMA_DI, args)
            assert outs.path.startswith("host loop: ") and word in outs.path and montecarlo.last_path() == outs.path
            assert np.array_equal(system.x, [7.0, 7.0])
            for k, a in outputs(outs).items():
                assert (torch.is_tensor(a) and a.is_cuda) if where == "tensor" else isinstance(a, np.ndarray), k
            ok, bad = all_same(outputs(outs), outputs(native))
            assert ok, (policy, word, bad)
    # generated normals: the host loop draws hjn_normals_host's stream
    a = computeStochTrajs(g, d_in, tau, _Own(g, 1), x_in[:3], SIGMA_DI, di_args(realisations=2, seed=4, firstRealisation=6, policy='clock'))
    zh = _nffi.normals_host(4, 6, 6, 0, 80, 2).reshape(3, 2, 80, 2)
    b = computeStochTrajs(g, d_in, tau, _Own(g, 1), x_in[:3], SIGMA_DI, di_args(realisations=2, normals=zh if where == "numpy" else dev(zh), policy='clock'))
    assert all_same(outputs(a), outputs(b))[0] and not same(a.final[:, 0], a.final[:, 1])
    lean = computeStochTrajs(g, d_in, tau, _Own(g, 1), x_in[:2], SIGMA_DI, di_args(realisations=2, seed=4, keepTrajs=False))
    assert lean.trajs is None and lean.tEarliest is None
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    c = computeStochTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in[:2], SIGMA_DI, di_args(realisations=2, normals=n_in[:2], derivFunc=foreign))
    assert c.path.startswith("host loop: derivFunc")
    d = computeStochTrajs(g, d_in, tau, L.DoubleIntegrator(g, 1), x_in[:2], SIGMA_DI, di_args(realisations=2, normals=n_in[:2]))
    assert all_same(outputs(c), outputs(d))[0]


# ------------------------------------------------------------------------------------------ 11. bad arguments, census
@gpu
def test_front_end_refuses_bad_arguments_by_name():
    g, og, data, tau, xs = integrator_case()
    d_t, x_t, plant = dev(data), dev(xs[:5]), L.DoubleIntegrator(g, 1)
    ok = computeStochTrajs(g, d_t, tau, plant, x_t, 0.1 * np.eye(2), di_args(realisations=2))
    assert tuple(ok.final.shape) == (5, 2, 2)
    for sigma, kw, word in (
            (np.array([0.1, 0.2]), {}, "vector"),
            ([[0.1, np.zeros((41, 41))], [0.0, 0.1]], {}, "cell matrix"),
            (lambda t, x: np.eye(2), {}, "callable"),
            (np.eye(3), {}, "2 x 2"),
            (np.array([[0.1, np.nan], [0.0, 0.1]]), {}, "not finite"),
            (np.eye(2), dict(seed=-1), "seed"),
            (np.eye(2), dict(seed=2 ** 64), "seed"),
            (np.eye(2), dict(seed=1.5), "seed"),
            (np.eye(2), dict(firstRealisation=-3), "firstRealisation"),
            (np.eye(2), dict(realisations=0), "realisations"),
            (np.eye(2), dict(normals=np.zeros((5, 2, 80, 3)), realisations=2), "normals"),
            (np.eye(2), dict(normals=np.zeros((5, 3, 80, 2)), realisations=2), "normals"),
            (np.eye(2), dict(policy='latest'), "policy"),
            (np.eye(2), dict(uMode='up'), "uMode"),
            (np.eye(2), dict(subSamples=0), "subSamples")):
        with pytest.raises(ValueError) as info:
            computeStochTrajs(g, d_t, tau, plant, x_t, sigma, di_args(**kw))
        assert word in str(info.value), (word, str(info.value))
    with pytest.raises(ValueError):
        computeStochTrajs(g, d_t, tau[:-1], plant, x_t, np.eye(2))
    with pytest.raises(ValueError):
        reachProbability(ok, 0.0, 'sometimes')
    assert computeStochTrajs(g, d_t, tau, plant, x_t, np.eye(2), di_args(seed=2 ** 64 - 1)).seed == 2 ** 64 - 1


@gpu
def test_census_of_the_mc_library():
    out = subprocess.check_output(["nm", "-D", "-C", _nffi.LIB_PATH]).decode()
    stubs = set(re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", out))
    assert len(stubs) == 19 and stubs == set(CENSUS), (sorted(stubs - set(CENSUS)), sorted(set(CENSUS) - stubs))
    src = open(os.path.abspath(__file__)).read()
    for kernel, test in CENSUS.items():
        assert callable(globals().get(test)), test
        body = src[src.index("def %s(" % test):]
        body = body[:body.index("\n\n\n")]
        assert 'launched(' in body and '"%s"' % test in body, test
