"""CPU-only: extraArgs.plantKernel without a device -- libhj_plant.so's kernel kinds and six new entry points (include/hj_plant.h), the
routing of montecarlo.py / safety.py, and the package's own Plane5D / DubinsPair6D texts (levelsetpy_amd/plant_builtin.py).

  * compile_kind compiles the three new kinds for lin (4-D) and the quadrotor (6-D), ENO2, fp64 and fp32 (hipRTC cross-compiles for gfx950);
    a body with an error reports name:line for each kind; a plant without controls has no filter kernel;
  * every native refusal of the six entry points returns its code with its text and leaves sentinel-filled outputs untouched: every check
    comes before the first HIP call, so host arrays stand in for the device's (tests/plant_hooks_cases.py);
  * only hjp_* is exported, and no device stub;
  * the _why_host functions with and without the flag; plantKernel='yes' is refused;
  * the package's texts are tests/plant_cases.py's, statement for statement.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _pffi, montecarlo, safety, register_plant  # noqa: E402
from levelsetpy_amd import plant_builtin  # noqa: E402  (the feature: missing before it)
from levelsetpy_amd.dynamics import native_plant  # noqa: E402

import hiquery_cases as XC  # noqa: E402
import plant_cases as PC  # noqa: E402
import plant_hooks_cases as HC  # noqa: E402
import query_ref as Q  # noqa: E402

KINDS = ("noisy", "filtered", "decide")


@pytest.mark.parametrize("which", ["lin 4-D", "quadrotor 6-D"])
def test_compile_kind_compiles_the_three_new_kinds(which):
    reg = PC.register_lin() if which.startswith("lin") else PC.register_quad()
    for kind in KINDS:
        for dtype in ("float64", "float32"):
            assert reg.check("ENO2", dtype, kind) is reg
    with pytest.raises(_ffi.Unsupported):
        reg.check("WENO5", "float64", "noisy")
    with pytest.raises(ValueError, match="kind must be"):
        reg.check("ENO2", "float64", "smoothed")
    lib = _pffi.lib()
    assert lib.hjp_plant_compile_kind(reg.plant_id, 4, 0, 0) == -1 and b"kernel kind" in lib.hjp_last_error()
    assert lib.hjp_plant_compile_kind(_pffi.PLANT_BASE - 1, 1, 0, 0) == -1
    assert (_pffi.KERNEL_ROLLOUT, _pffi.KERNEL_NOISY, _pffi.KERNEL_FILTERED, _pffi.KERNEL_DECIDE) == (0, 1, 2, 3)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hj_plant.h")).read()
    assert "HJP_KERNEL_ROLLOUT = 0, HJP_KERNEL_NOISY = 1, HJP_KERNEL_FILTERED = 2, HJP_KERNEL_DECIDE = 3" in header


def test_a_mistake_is_reported_as_name_and_line_for_each_kind():
    bad = register_plant("wobbly_hooks", 3, "u[0] = par[0];", "dx[0] = x[1];\n\ndx[1] = u[0] +;\ndx[2] = 0.0;", 1, 0, 1)
    for kind in KINDS:
        with pytest.raises(ValueError) as e:
            bad.check("ENO2", "float64", kind)
        assert "plant 'wobbly_hooks' does not compile" in str(e.value) and re.search(r"\bwobbly_hooks:3:\d+: error", str(e.value)), (kind, str(e.value))
    # nothing to filter: a plant of disturbances alone
    none = register_plant("drift_only", 2, "dst[0] = par[0] * sgn(p[1]);", "dx[0] = x[1];\ndx[1] = dst[0];", 0, 1, 1)
    assert none.check("ENO2", "float64", "noisy") is none
    for kind in ("filtered", "decide"):
        with pytest.raises(ValueError, match="plant 'drift_only' has no controls: there is nothing to filter"):
            none.check("ENO2", "float64", kind)


@pytest.mark.parametrize("hi", [False, True])
def test_every_refusal_returns_its_code_and_touches_nothing(hi):
    c = HC.Case(hi)
    lib = _pffi.lib()
    before = {k: v.copy() for k, v in c.ins.items()}
    for call, rows in ((c.noisy, c.noisy_rows()), (c.filtered, c.filtered_rows()), (c.decide, c.decide_rows())):
        for kw, code, word in rows:
            rc = call(**kw)
            assert rc == code, (call.__name__, kw, rc, lib.hjp_last_error())
            assert word.encode() in lib.hjp_last_error(), (call.__name__, kw, lib.hjp_last_error())
            assert c.untouched(), (call.__name__, kw)
    # a plant without controls is refused by name where there is nothing to filter
    nd = c.nd
    none = register_plant("drift_only_%d" % nd, nd, "dst[0] = 1.0;", "dx[0] = dst[0];", 0, 1, 0)
    for call in (c.filtered, c.decide):
        assert call(plant=_pffi.plant_descriptor(none.plant_id, 0, 0, [])) == -1
        assert b"has no controls: there is nothing to filter" in lib.hjp_last_error() and c.untouched()
    # a plant of another dimension, by name
    other = PC.register_builtin("integrator")
    assert c.filtered(plant=_pffi.plant_descriptor(other.plant_id, 0, 0, [1.0])) == -1 and b"has 2 states, the grid" in lib.hjp_last_error()
    # nothing to do: fine whatever the optional arrays, and launches nothing
    assert c.noisy(M=0) == 0 and c.filtered(M=0, traj=None, active=None, applied=None) == 0 and c.decide(M=0, costate=None) == 0
    assert _pffi.last_kernel() == "" and c.untouched()
    assert all(np.array_equal(before[k], c.ins[k]) for k in c.ins)
    with pytest.raises(_ffi.Unsupported):
        _pffi.check(c.filtered(scheme=_ffi.WENO5))


def test_census_and_one_source_of_the_checks():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _pffi.LIB_PATH]).decode()
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    code = [n for n in names if not n.startswith("__hip") and not n.startswith("_")]
    assert sorted(code) == sorted(_pffi.SIGNATURES) and all(n.startswith("hjp_") for n in code)
    for new in ("hjp_plant_compile_kind", "hjp_noisy_rollout", "hjp_noisy_rollout_hi", "hjp_filtered_rollout", "hjp_filtered_rollout_hi", "hjp_decide",
                "hjp_decide_hi"):
        assert new in code
    assert not any("__device_stub__" in n or "rollout_kernel" in n or "points_kernel" in n for n in names), names
    csrc = os.path.join(os.path.dirname(L.__file__), "csrc")
    src = lambda n: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, n)).read())      # noqa: E731
    plant = src("hj_plant.hip")
    for text in ("split over states", "must not be NaN", "level must be finite", "is neither HJF_DSTB_WORST", "nreal must be at least 1", "sq must be finite"):
        assert text not in plant, text                                  # the filter's and the noise's checks are not restated
    assert src("hj_mc.hip").count("check_noise(") == 1 and src("hj_mc_dev.h").count("static int check_noise(") == 1
    assert "__global__" not in plant.split("static std::string plant_source")[0] and plant.count("#include \"hj_filter.hip\"") == 1
    # the width trap: the noise's argument block is templated on the unit's width, and the cache key covers it and every header
    dev = src("hj_plant_dev.h")
    assert "template <typename T, int MD> struct NoisyArgs" in dev and "double G[MD * MD];" in dev
    for word in ("sizeof(NoisyArgs<double, HJH_MAX_DIM>)", "sizeof(FilterArgs<float, HJ_MAX_DIM>)", '"/hj_filter_dev.h"', '"/hj_mc_dev.h"',
                 '"/hj_plants_dev.h"', '"/../../include/hj_filter.h"', '"/../../include/hj_mc.h"'):
        assert word in plant, word
    reg = PC.register_quad()
    text = reg.source()
    for k in _pffi.KERNELS:
        assert "void %s(" % k in text


class _Own(object):
    x = None

    def dynamics(self, t, x, u, d=None):
        return np.array([x[1], u])

    def get_opt_u(self, t, deriv, uMode, x):
        return 1.0

    def update_state(self, u, dt, x, d=None):
        self.x = x
        return x


@pytest.mark.parametrize("mod,noun", [(safety, "filter"), (montecarlo, "noisy rollout")])
def test_the_routing_with_and_without_the_flag(mod, noun):
    g2, _ = Q.make_grids(Q.SHAPES[2], ())
    g3, _ = Q.make_grids(Q.SHAPES[3], ())
    fn = L.upwindFirstENO3
    reg = PC.register_builtin("integrator")
    # the built-in rule comes first, whatever is attached and whatever the flag
    di = L.DoubleIntegrator(g2, 0.8)
    reg.attach(di, params=[0.8])
    for flag in (False, True):
        assert mod._why_host(di, fn, g2, flag) == (native_plant(di), None)
    # a registered plant: the host loop without the flag, the kernel with it
    own = reg.attach(_Own(), params=[0.3])
    assert mod._why_host(own, fn, g2) == (None, "_Own is a registered plant: it has no %s kernel" % noun)
    nat, why = mod._why_host(own, fn, g2, True)
    assert why is None and nat[0] is reg and nat[1] == [0.3]
    # wrong dimension, foreign derivFunc: the host loop and why
    assert mod._why_host(own, fn, g3, True) == (None, "_Own has no native plant on a 3-D grid")
    foreign = lambda grid, a, dim, generateAll=False: L.upwindFirstENO3(grid, a, dim)        # noqa: E731
    assert mod._why_host(own, foreign, g2, True)[1].startswith("derivFunc")
    # a shadowed method is no registered plant any more
    sh = reg([0.8])
    sh.dynamics = lambda t, x, u, d=None: np.zeros(2)
    assert mod._why_host(sh, fn, g2, True) == mod._why_host(sh, fn, g2) == (None, "PlantSystem has no native plant")
    # Plane5D / DubinsPair6D: the package's own registration, once per process
    for name in ("plane5d", "pair6d"):
        g, _ = XC.grids(name)
        s = XC.system(name, g)
        if mod is safety:
            assert mod._why_host(s, fn, g)[1] == "%s has no filter kernel on a %d-D grid" % (type(s).__name__, g.dim)
        else:
            assert mod._why_host(s, fn, g)[1] == "%s has no noisy rollout kernel (5-D / 6-D systems are out of its scope)" % type(s).__name__
        nat, why = mod._why_host(s, fn, g, True)
        assert why is None and nat[0] is plant_builtin.registration_hi(PC.BUILTIN_ID[name]) and nat[0].name == type(s).__name__
        assert nat[1] == list(XC.PLANT_PAR[name]) and nat[0].dim == g.dim
        assert mod._why_host(s, fn, g, True)[0][0] is nat[0]
    for bad in ('yes', 1, None.__class__):
        with pytest.raises(ValueError, match="extraArgs.plantKernel must be True or False"):
            plant_builtin.flag(L.Bundle(dict(plantKernel=bad)))
    assert plant_builtin.flag(None) is False and plant_builtin.flag(L.Bundle(dict(plantKernel=True))) is True


def test_the_flag_is_refused_before_a_device_is_asked_for(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    for m in (safety, montecarlo):
        for name in ("require_gpu", "_device_data", "_device_states"):
            monkeypatch.setattr(m, name, no_device)
    g, _ = Q.make_grids(Q.SHAPES[2], ())
    di = L.DoubleIntegrator(g, 1)
    data, tau, xs = np.zeros((4,) + tuple(g.shape)), np.linspace(0, 0.3, 4), np.zeros((5, 2))
    with pytest.raises(ValueError, match="plantKernel"):
        L.computeSafeTrajs(g, data, tau, di, xs, np.zeros((5, 3, 1)), L.Bundle(dict(plantKernel='yes')))
    with pytest.raises(ValueError, match="plantKernel"):
        L.safeControls(g, data[0], di, xs, np.zeros((5, 1)), L.Bundle(dict(plantKernel='yes')))
    with pytest.raises(ValueError, match="plantKernel"):
        L.computeStochTrajs(g, data, tau, di, xs, np.zeros((2, 2)), L.Bundle(dict(plantKernel=0)))
    # a table of another width than the registration's controls, by name
    lin = PC.register_lin()(PC.LIN_PAR)
    g4, _ = Q.make_grids(Q.SHAPES[4], ())
    with pytest.raises(ValueError, match="nominal holds 2 controls per column, PlantSystem has 3"):
        L.computeSafeTrajs(g4, np.zeros((4,) + tuple(g4.shape)), tau, lin, np.zeros((5, 4)), np.zeros((5, 3, 2)), L.Bundle(dict(plantKernel=True, derivFunc=L.upwindFirstENO2)))
    with pytest.raises(ValueError, match="uNom holds 1 controls per state, PlantSystem has 3"):
        L.safeControls(g4, np.zeros(tuple(g4.shape)), lin, np.zeros((5, 4)), np.zeros((5, 1)), L.Bundle(dict(plantKernel=True, derivFunc=L.upwindFirstENO2)))


def test_the_packages_texts_are_plant_cases_statement_for_statement():
    norm = lambda t: [" ".join(st.split()) for st in t.split(";") if st.strip()]      # noqa: E731
    for name in ("plane5d", "pair6d"):
        mine = plant_builtin.TEXTS[PC.BUILTIN_ID[name]]
        dim, ctl, dyn, nu, nd, npar = PC.BUILTIN[name]
        assert (mine[1], mine[4], mine[5], mine[6]) == (dim, nu, nd, npar)
        assert norm(mine[2]) == norm(ctl) and norm(mine[3]) == norm(dyn)
        assert mine[0] == {"plane5d": "Plane5D", "pair6d": "DubinsPair6D"}[name]


@pytest.mark.parametrize("first", [0, 2 ** 32 - 3, 2 ** 40])
def test_the_restated_generator_is_the_host_librarys(first):
    """tests/mc_ref.py's Philox4x32-10 and Box-Muller against hjn_normals_host wherever that one reaches (four normals a step): the words bit
    for bit, the normals within 1e-12 (the two libms).  The GPU tests supply the restatement's stream where the library's stops: at five
    and six normals a step, whose third pair is counter word j = 2 of the same function."""
    import mc_ref as MC
    from levelsetpy_amd import _nffi
    seed = 0x299f31d0a4093822
    for nd in (1, 2, 3, 4):
        z, w = _nffi.normals_host(seed, first, 40, 5, 7, nd, words=True)
        assert np.array_equal(w, MC.words(seed, first, 40, 5, 7, nd))
        assert float(np.max(np.abs(z - MC.normals(seed, first, 40, 5, 7, nd)))) <= 1e-12
    # pairs 0 and 1 of a six-normal step are the four-normal step's: the counter's last word alone tells the pairs apart
    w6, w4 = MC.words(seed, first, 9, 0, 3, 6), MC.words(seed, first, 9, 0, 3, 4)
    assert w6.shape == (9, 3, 3, 4) and np.array_equal(w6[:, :, :2], w4) and not np.array_equal(w6[:, :, 2], w6[:, :, 1])
    z6 = MC.normals(seed, first, 9, 0, 3, 6)
    assert np.array_equal(z6[..., :4], MC.normals(seed, first, 9, 0, 3, 4)) and np.isfinite(z6).all()
