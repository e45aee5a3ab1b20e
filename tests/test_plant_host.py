"""register_plant (levelsetpy_amd/plant.py, libhj_plant.so) without a GPU: what is refused, ids, compile checks of every kernel
(hipRTC cross-compiles for gfx950), the generated source, the identity rule that routes a dynSys to the kernel, the library's symbols,
and the conditions the GPU tests of tests/test_gpu_plant.py rest on, checked with the oracle's solve of the same problem.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import register_plant, PlantRegistration, plant_kernel_cache_stats  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd import _ffi, _hffi, _pffi, rollout  # noqa: E402
from levelsetpy_amd.dynamics import native_of, native_plant, native_plant_hi  # noqa: E402
from levelsetpy_amd.plant import plant_of  # noqa: E402

import hidim_user_cases as UC  # noqa: E402
import plant_cases as PC  # noqa: E402
import query_ref as Q  # noqa: E402
import rollout_ref as R  # noqa: E402

CTL, DYN = "u[0] = par[0] * sgn(p[1]);", "dx[0] = x[1];\ndx[1] = u[0];"


def test_what_registration_refuses():
    for dim in (1, 7, 0):
        with pytest.raises(ValueError, match="dim must be 2..6"):
            register_plant("p", dim, CTL, DYN, 1, 0, 1)
    with pytest.raises(ValueError, match="at most 16 parameters"):
        register_plant("p", 2, CTL, DYN, 1, 0, 17)
    with pytest.raises(ValueError, match="controls and disturbances together"):
        register_plant("p", 2, CTL, DYN, 5, 4, 1)
    with pytest.raises(ValueError, match="controls and disturbances together"):
        register_plant("p", 2, CTL, DYN, 0, 0, 1)
    for name in ('a"b', "a'b"):
        with pytest.raises(ValueError, match="must not contain quotes"):
            register_plant(name, 2, CTL, DYN, 1, 0, 1)
    # the library says the same to a caller of the C ABI
    lib = _pffi.lib()
    import ctypes as C
    pid = C.c_int(-5)
    inc = os.path.join(os.path.dirname(L.__file__), "csrc").encode()
    for args in ((b"p", 1, 1, 0, 1), (b"p", 7, 1, 0, 1), (b"p", 2, 1, 0, 17), (b"p", 2, 5, 4, 1), (b"p", 2, 0, 0, 1), (b'a"b', 2, 1, 0, 1), (b"p", 2, -1, 2, 1)):
        rc = lib.hjp_plant_register(args[0], args[1], args[2], args[3], args[4], CTL.encode(), DYN.encode(), inc, None, C.byref(pid))
        assert rc in (-1, -3) and lib.hjp_last_error() and pid.value == -5, args
    assert lib.hjp_plant_register(None, 2, 1, 0, 1, CTL.encode(), DYN.encode(), inc, None, C.byref(pid)) == -1
    # a wrong parameter count: at __call__ and at attach
    reg = register_plant("p_two", 2, CTL, DYN, 1, 0, 2)
    with pytest.raises(ValueError, match="takes 2 parameters, got 1"):
        reg([1.0])
    g, _ = Q.make_grids(Q.SHAPES[2], ())
    with pytest.raises(ValueError, match="takes 2 parameters, got 3"):
        reg.attach(L.DoubleIntegrator(g, 1), params=[1.0, 2.0, 3.0])
    assert isinstance(reg, PlantRegistration) and reg([1.0, 2.0]).params == [1.0, 2.0]


def test_the_same_text_gives_the_same_id():
    a = register_plant("same", 2, CTL, DYN, 1, 0, 1)
    b = register_plant("same", 2, CTL, DYN, 1, 0, 1)
    c = register_plant("same", 2, CTL + " ", DYN, 1, 0, 1)
    d = register_plant("same", 2, CTL, DYN, 1, 0, 2)
    assert a.plant_id == b.plant_id and len({a.plant_id, c.plant_id, d.plant_id}) == 3
    # a base of its own: no built-in or registered Hamiltonian id is a plant id
    assert a.plant_id >= _pffi.PLANT_BASE > max(_hffi.HAM_USER_BASE, _ffi.HAM_USER_BASE) + 10000
    import ctypes as C
    nd, nu, ndst, npar, built = (C.c_int() for _ in range(5))
    _pffi.check(_pffi.lib().hjp_plant_info(d.plant_id, C.byref(nd), C.byref(nu), C.byref(ndst), C.byref(npar), C.byref(built)))
    assert (nd.value, nu.value, ndst.value, npar.value, built.value) == (2, 1, 0, 2, 0)
    assert _pffi.lib().hjp_plant_info(_pffi.PLANT_BASE - 1, None, None, None, None, None) == -1
    assert _pffi.lib().hjp_plant_info(_pffi.PLANT_BASE + 100000, None, None, None, None, None) == -1
    compiled, loaded = plant_kernel_cache_stats()                   # registering and compile checks load nothing
    assert compiled >= 0 and loaded >= 0 and built.value == 0


@pytest.mark.parametrize("which", ["dubins 3-D", "quadrotor 6-D"])
def test_check_compiles_all_six_kernels(which):
    reg = PC.register_builtin("dubins") if which.startswith("dubins") else PC.register_quad()
    assert reg.dim == int(which[-3])
    for scheme in ("ENO2", "ENO3", "WENO5_ASSHIPPED"):
        for dtype in ("float64", "float32"):
            assert reg.check(scheme, dtype) is reg
    with pytest.raises(_ffi.Unsupported):
        reg.check("WENO5", "float64")


def test_every_case_of_the_gpu_tests_compiles():
    for name in sorted(PC.BUILTIN):
        PC.register_builtin(name).check("ENO3", "float64")
    PC.register_lin().check("WENO5_ASSHIPPED", "float32")


def test_a_mistake_is_reported_as_name_and_line_into_its_body():
    bad = register_plant("wobbly", 3, "u[0] = par[0];", "dx[0] = x[1];\n\ndx[1] = u[0] +;\ndx[2] = 0.0;", 1, 0, 1)
    with pytest.raises(ValueError) as e:
        bad.check("ENO2", "float64")
    assert "plant 'wobbly' does not compile" in str(e.value) and re.search(r"\bwobbly:3:\d+: error", str(e.value)), str(e.value)
    bad = register_plant("wobbly", 3, "\nu[0] = par[0]\n", "dx[0] = x[1];", 1, 0, 1)
    with pytest.raises(ValueError) as e:
        bad.check("ENO2", "float64")
    assert re.search(r"\bwobbly:2:\d+: error", str(e.value)), str(e.value)
    # a name the bodies do not have: t, the value
    for body in ("dx[0] = t;", "dx[0] = data[0];"):
        with pytest.raises(ValueError, match="undeclared identifier"):
            register_plant("wobbly", 3, "u[0] = 1.0;", body, 1, 0, 0).check("ENO2", "float64")


def test_source_contains_both_bodies():
    reg = PC.register_quad()
    src = reg.source()
    assert PC.QUAD_CONTROLS in src and PC.QUAD_DYNAMICS in src
    assert "#define HJ_QUERY_MAXD 6" in src and "#define HJ_QUERY_MIND 5" in src and src.count('#line 1 "planar_quad"') == 2
    for header in ("hj_query_dev.h", "hj_rollout_dev.h"):
        assert '#include "%s"' % header in src
    assert "struct PlantUser" in src and "user_rollout_kernel" in src and "static constexpr int ND = 6, NU = 2, NDST = 0" in src
    low = PC.register_builtin("dubins").source()
    assert "#define HJ_QUERY_MAXD 4" in low and "HJ_QUERY_MIND" not in low


class _Lazy(L.PlantSystem):
    """A subclass that overrides a protocol method: not the kernel's plant any more."""

    def get_opt_u(self, t, deriv, uMode, x):
        return 0.5 * L.PlantSystem.get_opt_u(self, t, deriv, uMode, x)


class _Own(object):
    """A foreign class with the dynSys protocol."""
    x = None

    def dynamics(self, t, x, u, d=None):
        return np.array([x[1], u])

    def get_opt_u(self, t, deriv, uMode, x):
        return 1.0

    def update_state(self, u, dt, x, d=None):
        self.x = x
        return x


def test_the_identity_rule():
    g2, _ = Q.make_grids(Q.SHAPES[2], ())
    g3, _ = Q.make_grids(Q.SHAPES[3], ())
    reg = PC.register_builtin("integrator")
    fn = L.upwindFirstENO3
    sys_ = reg([0.8])
    nat, why = rollout._why_host(sys_, fn, g2)
    assert why is None and nat[0] is reg and nat[1] == [0.8]
    sys_.params[0] = 0.5                                            # the parameters are re-read at every call
    assert rollout._why_host(sys_, fn, g2)[0][1] == [0.5]
    # an existing object of a foreign class
    own = _Own()
    assert rollout._why_host(own, fn, g2) == (None, "_Own has no native plant")
    assert reg.attach(own, params=[0.3]) is own and plant_of(own) == (reg, [0.3])
    assert rollout._why_host(own, fn, g2)[1] is None
    # another grid dimension, a derivative function without a point kernel: the host loop and its line
    assert rollout._why_host(own, fn, g3) == (None, "_Own has no native plant on a 3-D grid")
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    assert rollout._why_host(own, foreign, g2)[1].startswith("derivFunc")
    # a subclass overriding get_opt_u does not qualify
    lazy = _Lazy(reg, [0.8])
    assert plant_of(lazy) is None and rollout._why_host(lazy, fn, g2) == (None, "_Lazy has no native plant")
    # an instance attribute shadowing dynamics does not
    sh = reg([0.8])
    sh.dynamics = lambda t, x, u, d=None: np.zeros(2)
    assert plant_of(sh) is None and rollout._why_host(sh, fn, g2)[1] == "PlantSystem has no native plant"
    with pytest.raises(ValueError, match="shadows dynamics"):
        reg.attach(sh, params=[0.8])
    # a method replaced in the class after attach does not
    class Later(_Own):
        pass
    late = reg.attach(Later(), params=[0.3])
    assert plant_of(late) is not None
    Later.update_state = lambda self, u, dt, x, d=None: x
    assert plant_of(late) is None
    # a class without the protocol is refused at attach
    with pytest.raises(ValueError, match="no dynamics"):
        reg.attach(object.__new__(type("Bare", (), {})), params=[0.3])
    # the built-in systems keep their kernels: their rule comes first, whatever is attached
    di = L.DoubleIntegrator(g2, 0.8)
    reg.attach(di, params=[0.8])
    assert rollout._why_host(di, fn, g2)[0] == native_plant(di) == di.native()


def test_attach_leaves_the_hamiltonian_registration_alone():
    g, _ = PC.quad_grids()
    q = PC.Quadrotor(g)
    PC.register_quad_hamiltonian().attach(q, params=lambda o: o.params, tables=UC.quad_tables(g.vs))
    before = native_of(q.hamiltonian, q.dissipation)
    marker = q._hj_native
    assert before is not None and before[0] is q and before[1] >= _hffi.HAM_USER_BASE
    assert plant_of(q) is None and native_plant(q) is None and native_plant_hi(q) is None
    reg = PC.register_quad()
    reg.attach(q, params=lambda o: o.params)
    after = native_of(q.hamiltonian, q.dissipation)
    assert q._hj_native is marker and after[0] is before[0] and after[1:] == before[1:]
    nat, why = rollout._why_host(q, L.upwindFirstENO2, g)
    assert why is None and nat[0] is reg and nat[1] == PC.QUAD_PAR
    assert PC.quadrotor(g)._hj_plant.reg.plant_id == reg.plant_id


def test_census_of_the_plant_library():
    """Only hjp_* are exported, and the library holds no kernel: every one is compiled at run time."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", _pffi.LIB_PATH]).decode()
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    code = [n for n in names if not n.startswith("__hip") and not n.startswith("_")]
    assert sorted(code) == sorted(_pffi.SIGNATURES), (sorted(code), sorted(_pffi.SIGNATURES))
    assert not any("__device_stub__" in n or "rollout_kernel" in n for n in names), names
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hj_plant.h")).read()
    assert set(re.findall(r"\b(hjp_[a-z_]+)\(", header)) == set(_pffi.SIGNATURES)
    assert "HJP_PAR_SLOTS 16" in header and _pffi.PAR_SLOTS == 16 and "HJP_PLANT_BASE = %d" % _pffi.PLANT_BASE in header
    # the other libraries got no new entry point and nothing links this one
    mk = open(os.path.join(os.path.dirname(L.__file__), "csrc", "Makefile")).read()
    assert re.search(r"^libs: all libhj_hiquery.so libhj_plant.so$", mk, re.M)
    assert re.search(r"^libhj_plant.so:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -shared -o \$@ hj_plant.hip$", mk, re.M)


def test_the_restatements_agree_with_the_python_systems():
    """The quadrotor's NumPy restatement is the gradient of quad_ham's Hamiltonian in p, and its controls attain quad_ham's optimum."""
    rng = np.random.default_rng(4)
    X, P = rng.standard_normal((50, 6)), rng.standard_normal((50, 6))
    par = PC.QUAD_PAR
    m, I, l, Cv, Cphi, g_, Tmax, s = par
    for uMode in ('min', 'max'):
        u, d, sw = PC.quad_controls(par, P, X, uMode, None)
        assert d == () and set(np.unique(np.concatenate(u))) <= {0.0, Tmax}
        f = PC.quad_f(par, X, u, d)
        pf = (P * f).sum(axis=1)
        kp, km = sw
        opt = (np.minimum if uMode == 'min' else np.maximum)
        H = (P[:, 0] * X[:, 1] - P[:, 1] * (Cv / m) * X[:, 1] + P[:, 2] * X[:, 3] - P[:, 3] * ((Cv / m) * X[:, 3] + g_) + P[:, 4] * X[:, 5]
             - P[:, 5] * (Cphi / I) * X[:, 5] + Tmax * opt(kp, 0) + Tmax * opt(km, 0))
        assert np.max(np.abs(pf - H)) <= 1e-12 * max(1.0, np.max(np.abs(H)))
    Pn = P.copy()
    Pn[0, 5] = np.nan
    u, _, _ = PC.quad_controls(par, Pn, X, 'min', None)
    assert np.isnan(u[0][0]) and np.isnan(u[1][0]) and not np.isnan(u[0][1:]).any()
    g, _ = PC.quad_grids()
    q = PC.Quadrotor(g)
    uu = q.get_opt_u(0.0, P[3].tolist(), 'min', X[3])
    c, _, _ = PC.quad_controls(par, P[3:4], X[3:4], 'min', None)
    assert uu == (c[0][0], c[1][0]) and np.array_equal(q.dynamics(0.0, X[3], uu), PC.quad_f(par, X[3:4], (c[0], c[1]), ())[0])
    new = q.update_state(uu, 0.01, X[3])
    want = R.rk4(lambda Z: PC.quad_f(par, Z, (c[0], c[1]), ()), X[3:4], 0.01)[0]
    assert new is q.x and np.array_equal(new, want)
    # the five-value control vector against its formulas
    u, d, sw = PC.lin_controls(PC.LIN_PAR, P[:, :4], X[:, :4], 'max', 'min')
    assert len(u) == 3 and len(d) == 2 and len(sw) == 5 and np.array_equal(u[2], PC.LIN_PAR[2] * R.sgn(P[:, 3]))
    assert np.array_equal(d[1], -PC.LIN_PAR[4] * R.sgn(P[:, 0] + P[:, 3]))
    assert PC.lin_f(PC.LIN_PAR, X[:, :4], u, d).shape == (50, 4)


_QUAD = {}


def quad_horizon_ref():
    """The quadrotor's horizon case from the oracle's solve (ENO2, RK3 single steps at factorCFL 0.8, minVOverTime): what
    tests/test_gpu_plant.py solves on the device with the registered Hamiltonian."""
    if not _QUAD:
        og = UC.quad_oracle_grid()
        stack = R.solve_min_over_time(og, UC.QuadOracle(og), PC.quad_target(og), PC.QUAD_TAU, "ENO2")
        data = np.ascontiguousarray(stack[::-1])
        _QUAD["ref"] = R.rollout_ref(og, data, PC.QUAD_TAU, "quad", PC.QUAD_PAR, PC.quad_states(og), 'min', 'min', 4, "ENO2")
    return _QUAD["ref"]


def test_the_chosen_states_meet_the_conditions_of_the_gpu_tests():
    """At most 4 of 64 trajectories fragile, at least two distinct lengths, at least one trajectory leaving the grid -- for the
    quadrotor's horizon, and for the stacks of the built-in plants that the whole-horizon comparisons reuse no condition is needed
    (kernel against kernel, every trajectory)."""
    rtraj, rlen, rte, rstat, fragile = quad_horizon_ref()
    print("quadrotor: %d of 64 fragile, lengths %s, status counts %s" % (int(fragile.sum()), sorted(set(rlen.tolist())),
                                                                        np.bincount(rstat, minlength=3).tolist()))
    assert rtraj.shape == (64, 6, 5)
    assert fragile.sum() <= 4 and len(set(rlen.tolist())) >= 2 and (rstat == R.LEFT_GRID).sum() >= 1
    assert (rstat == R.REACHED).any() and (rstat == R.EXHAUSTED).any()
