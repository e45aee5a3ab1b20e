"""The NumPy restatement of the time-to-reach recurrence (tests/ttr_ref.py) on closed forms and the golden pin of the
initialisation branch (tests/golden/ttr.npz, generated from the reference's postTimeStepTTR by
tests/golden/make_golden_ttr.py).  No GPU: tests/test_gpu_ttr.py holds the kernels to this restatement bit for bit.

Bound of (a): phi is linear in t, so the interpolated crossing time is psi / 0.8 exactly; the formula
t_last - ((t - t_last) * a) / (b - a) rounds four times (product, difference, quotient, difference; a and b carry the rounding
of the data itself), each by at most half an ulp of a quantity no larger than tau[-1]: 4 eps tau[-1].
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ttr_ref as R  # noqa: E402

EPS = 2.0 ** -52
GOLDEN = os.path.join(HERE, "golden", "ttr.npz")


# ------------------------------------------------------------------------------------------ (a) expanding disc
@pytest.mark.parametrize("T", [2, 3, 5, 9, 11])
def test_expanding_disc_interpolates_to_the_closed_form(T):
    data, tau, psi = R.expanding_disc(T)
    inside_some = (data <= 0).any(axis=0)
    assert psi.size == 957 and int(inside_some.sum()) == 602
    for crossing in ('first', 'last'):
        ttr = R.TD2TTR(data, tau, 0.0, crossing, True)
        assert np.array_equal(np.isfinite(ttr), inside_some)            # finite exactly at the nodes inside some slice
        assert not np.isnan(ttr).any()
        exact = np.where(psi > 0, psi / 0.8, 0.0)
        err = np.abs(ttr - exact)[inside_some].max()
        assert err <= 4 * EPS * tau[-1], err / EPS
        stamped = R.TD2TTR(data, tau, 0.0, crossing, False)
        assert np.array_equal(np.isfinite(stamped), inside_some)
        assert np.isin(stamped[inside_some], tau).all()                 # without interpolation every finite value is a tau
        assert (stamped[inside_some] >= ttr[inside_some] - 4 * EPS).all()


# ------------------------------------------------------------------------------------------ (b) oscillating set
def test_oscillating_set_first_and_last_crossings():
    data, tau, psi = R.oscillating_set()
    for interpolate in (True, False):
        first = R.TD2TTR(data, tau, 0.0, 'first', interpolate)
        last = R.TD2TTR(data, tau, 0.0, 'last', interpolate)
        reached = np.isfinite(first)
        assert np.array_equal(reached, np.isfinite(last))
        assert np.array_equal(reached, (data <= 0).any(axis=0))
        assert (first[reached] <= last[reached]).all()
        # every reached node is swept over more than once: the set grows and shrinks twice, and even the nodes inside at tau[0]
        # (psi >= -0.25 > -0.5) are left and entered again
        assert int(reached.sum()) == 310
        assert (first[reached] < last[reached]).all()
        assert (first[reached & (data[0] <= 0)] == tau[0]).all()


# ------------------------------------------------------------------------------------------ (c) special values
@pytest.mark.parametrize("level", [0.0, 0.1])
def test_special_values_never_raise_and_never_yield_nan(level):
    base, tau, _ = R.oscillating_set()
    data, held = R.sprinkle(base, level, seed=3, inf_transitions=False)
    with np.errstate(all='raise'):                     # the restatement silences what it provokes itself
        for crossing in ('first', 'last'):
            for interpolate in (True, False):
                ttr = R.TD2TTR(data, tau, level, crossing, interpolate)
                assert not np.isnan(ttr).any()
                assert (ttr.reshape(-1)[held] == tau[0]).all()          # held at the level from the start: inside at tau[0]
                flat = data.reshape(len(tau), -1)
                always_nan = np.isnan(flat).all(axis=0)
                always_inf = (flat == np.inf).all(axis=0)
                assert always_nan.any() and always_inf.any()
                assert (ttr.reshape(-1)[always_nan | always_inf] == np.inf).all()


# ------------------------------------------------------------------------------------------ (d) fold equivalence
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_td2ttr_equals_its_own_step_by_step_fold(dtype):
    cases = [R.expanding_disc(T)[:2] for T in (1, 2, 3, 5, 9)] + [R.oscillating_set()[:2]]
    for base, tau in cases:
        for level in (0.0, 0.1):
            data = R.sprinkle(base, level, seed=len(tau))[0].astype(dtype)
            for crossing in ('first', 'last'):
                for interpolate in (True, False):
                    a = R.TD2TTR(data, tau, level, crossing, interpolate)
                    b = R.fold(data, tau, level, R.mode_bits(crossing, interpolate))
                    assert a.dtype == b.dtype == np.float64
                    assert np.array_equal(a, b, equal_nan=True), (len(tau), level, crossing, interpolate)


# ------------------------------------------------------------------------------------------ (f) golden pin
def test_init_branch_equals_the_reference():
    z = np.load(GOLDEN)
    raised = json.loads(str(z["raised_json"]))
    assert set(raised) == {"vec", "col", "arr"} and all(raised.values())      # the reference's update branch raised: unpinned
    for name in raised:
        y, t = z[name + "_y"], float(z[name + "_t"])
        ttr, last = R.init(y, t, 0.0)
        assert np.array_equal(ttr, z[name + "_ttr"]) and ttr.shape == y.shape
        assert np.array_equal(last, z[name + "_lastY"]) and float(z[name + "_lastT"]) == t
        assert (ttr[y == 0] == t).all() and (y == 0).any()
