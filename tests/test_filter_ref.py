"""CPU-only: the NumPy restatement of computeSafeTrajs (tests/filter_ref.py) is what include/hj_filter.h states, and the inputs of
tests/test_gpu_filter.py (tests/filter_inputs.py) meet the conditions those tests rest on.

  * margin = +inf acts at every sub-step: mc_ref's trajectory at G = 0 under the clock policy, exactly;
  * margin = -inf never acts: with a constant table on the double integrator the trajectory is the closed-form parabola
    x1 + x2 t + u t^2 / 2, x2 + u t, on which RK4 is exact -- within 16 eps scale (scale: the largest |x1| + |x2| t + |u| t^2 / 2 met),
    the accumulated rounding of T - 1 = 5 columns of 3 sub-steps with a handful of operations each;
  * a value nominal equal to the filtered value function with the same mode gives the always-acting trajectory for any margin, bit
    for bit;
  * decide_ref is the first sub-step of filter_ref;
  * the conditions on the whole-horizon inputs, the Dubins margin and the air3D start states.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_inputs as FI  # noqa: E402
import filter_ref as F  # noqa: E402
import mc_ref as MC  # noqa: E402
import rollout_ref as R  # noqa: E402
from levelsetpy_amd import computeSafeTrajs  # noqa: E402,F401  (the feature: missing before it)
from test_mc_ref import small_case  # noqa: E402

EPS = np.finfo(np.float64).eps


def test_infinite_margin_is_the_clock_rollout():
    og, data, tau, x0 = small_case()
    want = MC.mc_ref(og, data, tau, "integrator", (1.0,), x0, np.zeros((2, 2)), 1, xi=np.ones((12, 1, 15, 2)), policy='clock', subSamples=3,
                     scheme="ENO2")
    table = np.full((5, 1), 0.25)
    for level in (0.0, 0.2):
        got = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, table, 'min', 'min', 3, "ENO2", margin=np.inf, level=level)
        assert np.array_equal(got["traj"], want["traj"][:, 0], equal_nan=True)
        assert np.array_equal(got["final"], want["final"][:, 0], equal_nan=True)
        assert np.array_equal(got["value_end"], want["value_end"][:, 0], equal_nan=True)
        assert got["active"].all() and (got["interventions"] == 15).all() and (got["first"] == 0).all() and (got["length"] == 6).all()
        assert np.array_equal(got["status"] == F.LEFT_GRID, want["status"][:, 0] == R.LEFT_GRID)
        inside = got["status"] != F.LEFT_GRID
        assert np.isnan(got["gap_min"][~inside]).all() and (~inside).sum() == 2
        # the gap's minimum, from the recorded columns it cannot exceed
        v = np.stack([R._eval(og, data[c], got["traj"][:, :, c]) for c in range(6)])
        assert (got["gap_min"][inside] <= (level - v).min(axis=0)[inside]).all()
        assert np.array_equal(got["status"][inside] == F.VIOLATED, ~(got["gap_min"][inside] > 0))


def test_a_filter_that_never_acts_follows_the_parabola():
    og, data, tau, x0 = small_case()
    x0 = x0[[0, 2, 4, 6, 8, 11]]                    # states that stay on the grid
    for u in (0.3, -0.7):
        got = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, np.full((5, 1), u), 'min', 'min', 3, "ENO2", margin=-np.inf)
        assert not got["active"].any() and (got["interventions"] == 0).all() and (got["first"] == -1).all()
        assert (got["status"] != F.LEFT_GRID).all() and np.array_equal(got["applied"][:, :, 0], np.full((6, 15), u))
        assert (got["applied"][:, :, 1] == 0.0).all()
        t = tau[None, :] - tau[0]
        x1 = x0[:, 0:1] + x0[:, 1:2] * t + 0.5 * u * t * t
        x2 = x0[:, 1:2] + u * t
        scale = float(np.max(np.abs(x0[:, 0:1]) + np.abs(x0[:, 1:2]) * t + 0.5 * abs(u) * t * t))
        err = max(float(np.max(np.abs(got["traj"][:, 0] - x1))), float(np.max(np.abs(got["traj"][:, 1] - x2))))
        print("u %+.1f: max|state - parabola| %.3e = %.2f eps scale" % (u, err, err / (EPS * scale)))
        assert err <= 16 * EPS * scale


def test_a_value_nominal_equal_to_the_value_function_always_acts():
    og, data, tau, x0 = small_case()
    table = np.full((5, 1), 0.25)
    always = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, table, 'min', 'min', 3, "ENO2", margin=np.inf)
    for margin in (-np.inf, -0.1, 0.0, 0.2):
        got = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, dict(data=data, uMode='min'), 'min', 'min', 3, "ENO2", margin=margin)
        for k in ("traj", "final", "gap_min", "value_end", "applied", "status"):
            assert np.array_equal(got[k], always[k], equal_nan=True), (margin, k)
    assert not F.filter_ref(og, data, tau, "integrator", (1.0,), x0, dict(data=data, uMode='min'), 'min', 'min', 3, "ENO2",
                            margin=-np.inf)["active"][:9].any()
    # the other mode is another controller
    other = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, dict(data=data, uMode='max'), 'min', 'min', 3, "ENO2", margin=-np.inf)
    assert not np.array_equal(other["final"][:9], always["final"][:9])
    # the static policy on one field is the static policy on that slice of the stack, and 'zero' touches no control of this plant
    a = F.filter_ref(og, data, tau, "integrator", (1.0,), x0, table, 'min', 'min', 3, "ENO2", margin=0.1, policy='static', slice=2)
    b = F.filter_ref(og, data[2], tau, "integrator", (1.0,), x0, table, 'min', 'min', 3, "ENO2", margin=0.1, policy='static', dstb='zero')
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_decide_is_the_first_substep():
    g, og, data, tau, xs, table = FI.di_case()
    ref = FI.di_ref("float64", "table")
    dec = F.decide_ref(og, data[0], "integrator", (1.0,), xs, table[:, 0], 'min', 'min', FI.DI_SCHEME, FI.DI_MARGIN, FI.DI_LEVEL)
    assert np.array_equal(dec["applied"], ref["applied"][:, 0], equal_nan=True) and np.array_equal(dec["active"], ref["active"][:, 0])
    assert 0 < dec["active"][:64].sum() < 64


def test_the_whole_horizon_inputs_switch_inside_a_wavefront():
    """What test_gpu_filter's double-integrator tests rest on: a sub-step at which trajectories 0..15 (one wavefront of 4-lane groups)
    are neither all acting nor all idle, and at least 8 trajectories that switch at least twice; for every kind of run."""
    for dtype in ("float64", "float32"):
        for kind in ("table", "value", "static", "single"):
            out = FI.di_ref(dtype, kind)
            act = out["active"]
            mixed = [s for s in range(act.shape[1]) if 0 < act[:16, s].sum() < 16]
            twice = int(((np.diff(act.astype(int), axis=1) != 0).sum(axis=1) >= 2).sum())
            print("%s %s: %d mixed sub-steps in wavefront 0, %d trajectories switch twice or more, status counts %s" % (
                dtype, kind, len(mixed), twice, np.bincount(out["status"], minlength=3).tolist()))
            assert mixed and twice >= 8
            assert set(out["status"].tolist()) == {F.SAFE, F.VIOLATED, F.LEFT_GRID}
            assert (out["status"][64:66] == F.LEFT_GRID).all() and np.isnan(out["gap_min"][64:66]).all()
        assert all(np.array_equal(FI.di_ref(dtype, "static")[k], FI.di_ref(dtype, "single")[k], equal_nan=True)
                   for k in FI.di_ref(dtype, "static"))
        never = FI.di_ref(dtype, "never")
        on_grid = never["status"] != F.LEFT_GRID
        assert FI.di_ref(dtype, "always")["active"].all() and on_grid.sum() >= 32
        assert not never["active"][on_grid].any() and (never["interventions"][on_grid] == 0).all()
        assert never["active"][64].all() and never["first"][64] == 0               # a NaN gap acts: a state off the grid


def test_the_dubins_margin_sets_few_trajectories_aside():
    out = FI.dubins_ref()
    print("dubins: %d of 64 fragile, status counts %s" % (int(out["fragile"].sum()), np.bincount(out["status"], minlength=3).tolist()))
    assert out["fragile"].sum() <= 4
    keep = ~out["fragile"]
    assert set(out["status"][keep].tolist()) == {F.SAFE, F.VIOLATED, F.LEFT_GRID}
    assert len(set(out["interventions"][keep].tolist())) >= 8 and (out["interventions"][keep] == 40).any()
    assert ((np.diff(out["active"][keep].astype(int), axis=1) != 0).sum(axis=1) >= 2).sum() >= 8


def test_the_filter_does_its_job_in_the_restatement():
    """Start states with V[0](x0) - margin above one grid spacing: flying straight, at least a quarter collide; filtered, none."""
    for k in (0.25, 0.5, 0.75, 1.0):
        un, fi = FI.job_ref(False, k), FI.job_ref(True, k)
        print("margin %.2f spacings: %d states, unfiltered %s, filtered %s, smallest filtered gap %+.4f, %d + %d fragile" % (
            k, len(un["status"]), np.bincount(un["status"], minlength=3).tolist(), np.bincount(fi["status"], minlength=3).tolist(),
            float(np.nanmin(fi["gap_min"])), int(un["fragile"].sum()), int(fi["fragile"].sum())))
    un, fi = FI.job_ref(False), FI.job_ref(True)
    assert len(un["status"]) == 64
    assert (un["status"] == F.VIOLATED).sum() >= 16 and (un["interventions"] == 0).all()
    assert (fi["status"] == F.SAFE).all() and (fi["interventions"] > 0).sum() >= 16
    assert not un["fragile"].any() and not fi["fragile"].any()
