"""CPU-only: tests/plant_hooks_ref.py, the restatement the GPU tests of extraArgs.plantKernel compare with
(tests/test_gpu_plant_hooks.py), and the conditions those tests rest on -- evaluated with the restatement alone.

  * for the three built-in 2-D .. 4-D plants written in u / d form the restatement gives tests/filter_ref.py's filter_ref / decide_ref
    bit for bit: the double integrator's whole horizon of tests/filter_inputs.py (table and value nominal), one step each for Dubins and
    the pendulum (both disturbance rules);
  * in the lin and quadrotor horizons of tests/plant_hooks_inputs.py acting and idle sub-steps both occur, at least four trajectories
    switch twice or more, both statuses SAFE and VIOLATED occur and at most 1/8 of the states are fragile (filter_ref's rule, 1e-6).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_inputs as FI  # noqa: E402
import filter_ref as F  # noqa: E402
import hiquery_cases as XC  # noqa: E402
import plant_hooks_inputs as HI  # noqa: E402
import plant_hooks_ref as PH  # noqa: E402  (the feature's restatement: missing before it)
import query_ref as Q  # noqa: E402


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def all_same(got, want):
    assert sorted(got) == sorted(want)
    return [k for k in want if not same(got[k], want[k])]


@pytest.mark.parametrize("kind", ["table", "value"])
def test_the_integrators_horizon_is_filter_refs(kind):
    g, og, data, tau, xs, table = FI.di_case()
    want = FI.di_ref("float64", kind)
    nominal = table if kind == "table" else dict(data=FI.di_nominal_value(), uMode='min')
    got = PH.filter_ref(og, data, tau, "integrator_ud", (1.0,), xs, nominal, uMode='min', dMode='min', subSamples=FI.DI_SUB,
                        scheme=FI.DI_SCHEME, margin=FI.DI_MARGIN, level=FI.DI_LEVEL)
    assert got["applied"].shape[2] == 2 and all_same(got, want) == []
    assert want["active"].any() and not want["active"].all()


@pytest.mark.parametrize("name,par", [("dubins", (0.75, 0.75, 1.5)), ("pendulum", (1.25,))])
def test_one_step_of_dubins_and_the_pendulum_is_filter_refs(name, par):
    nd = 3 if name == "dubins" else 4
    g, og = Q.make_grids(Q.SHAPES[nd], (nd - 1,))
    base = XC.smooth(g, 1)
    data, tau, xs = np.stack([base, base + 1]), np.array([0.0, 0.1]), Q.state_set(g, 67)
    nu = F.NU[name]
    table = 0.3 * np.cos(np.arange(67 * nu).reshape(67, 1, nu))
    for dstb in ("worst", "zero"):
        for nominal in (table, dict(data=XC.smooth(g, 4), uMode='min')):
            kw = dict(uMode='max', dMode='min', subSamples=2, scheme="ENO3", margin=0.2, level=0.7, dstb=dstb)
            want = F.filter_ref(og, data, tau, name, par, xs, nominal, **kw)
            got = PH.filter_ref(og, data, tau, name + "_ud", par, xs, nominal, **kw)
            assert all_same(got, want) == [], (name, dstb)
            assert want["active"].any() and not want["active"].all()
        kw = dict(uMode='max', dMode='min', scheme="ENO3", margin=0.2, level=0.7, dstb=dstb)
        assert all_same(PH.decide_ref(og, base, name + "_ud", par, xs, table[:, 0], **kw), F.decide_ref(og, base, name, par, xs, table[:, 0], **kw)) == []


@pytest.mark.parametrize("name", ["lin", "quad"])
def test_the_horizons_meet_the_conditions_of_the_gpu_tests(name):
    for kind in ("table", "value"):
        r = HI.ref(name, "float64", kind)
        act = r["active"]
        ok = r["status"] != PH.LEFT_GRID
        switches = (act[:, 1:] != act[:, :-1]).sum(axis=1)
        print("%s %s: %d acting / %d idle sub-steps, %d trajectories switch twice or more, status counts %s, %d of %d fragile"
              % (name, kind, int(act[ok].sum()), int((~act[ok]).sum()), int((switches[ok] >= 2).sum()),
                 np.bincount(r["status"], minlength=3).tolist(), int(r["fragile"].sum()), len(ok)))
        assert act[ok].any() and (~act[ok]).any()
        assert (r["status"] == PH.SAFE).any() and (r["status"] == PH.VIOLATED).any()
        assert r["fragile"].sum() * 8 <= len(ok)
        if kind == "table":
            assert (switches[ok] >= 2).sum() >= 4
    W = PH.width(*HI.SPEC[name][2:4])
    assert HI.ref(name)["applied"].shape == (HI.M, (HI.NT - 1) * HI.SUB, W)
    if name == "lin":           # the disturbance rule shows: columns 3 and 4 are the disturbances
        z = HI.ref(name, "float64", "zero")["applied"]
        assert (z[:, :, 3:] == 0.0).all() and (HI.ref(name)["applied"][:, 0, 3:] != 0.0).any()
