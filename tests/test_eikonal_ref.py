"""CPU-only: the NumPy restatement tests/eikonal_ref.py of include/hj_eikonal.h, proved on closed forms before the device
is held to it (tests/test_gpu_eikonal.py).

Bounds.  The scheme is first order with a logarithmic factor; the asserted bound on the distorted sphere, the mask and the
periodic source is 1.25 * max(dx) at the sizes used here (measured: 0.62 on (41, 41), 0.79 on (33, 27, 29), 0.44 for the
mask, 0.75 on the periodic axis).  The axis-aligned plane is exact up to rounding: 4 ulp of the largest distance.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eikonal_ref as R  # noqa: E402

EPS = np.finfo(np.float64).eps


def axes(shape, lo=-1.0, hi=1.0, periodic=()):
    """Node coordinates per axis and dx: a periodic axis leaves out its last node, as createGrid's callers do."""
    vs, dx = [], []
    for d, n in enumerate(shape):
        if d in periodic:
            h = (hi - lo) / n
            vs.append(lo + h * np.arange(n))
        else:
            h = (hi - lo) / (n - 1)
            vs.append(np.linspace(lo, hi, n))
        dx.append(h)
    return np.meshgrid(*vs, indexing='ij'), dx


def tolerance(shape, u):
    """16 eps (sum_d N_d) max finite |u|: the map is non-expansive, an update adds a bounded number of roundings and a value
    depends on a chain of at most sum_d N_d updates."""
    finite = np.abs(u[np.isfinite(u)])
    return 16 * EPS * sum(shape) * (finite.max() if finite.size else 0.0)


def test_axis_aligned_plane_is_exact():
    shape = (31, 26)
    X, dx = axes(shape)
    out = R.signed_distance(3.0 * (X[0] - 0.13), dx)
    exact = X[0] - 0.13
    err = np.abs(out - exact).max()
    print("plane: max error %.3g" % err)
    assert err <= 4 * EPS * np.abs(exact).max()


@pytest.mark.parametrize("shape", [(41, 41), (33, 27, 29)], ids=str)
def test_distorted_sphere_first_order(shape):
    X, dx = axes(shape)
    r = np.sqrt(sum(x * x for x in X))
    out = R.signed_distance((r - 0.5) * (1.0 + 0.5 * X[0]), dx)
    err = np.abs(out - (r - 0.5)).max() / max(dx)
    print("distorted sphere %r: max error %.3f max(dx)" % (shape, err))
    assert err <= 1.25
    assert np.array_equal(np.sign(out), np.sign(r - 0.5))


def test_mask_of_a_disc():
    shape = (31, 26)
    X, dx = axes(shape)
    r = np.sqrt(X[0] ** 2 + X[1] ** 2)
    mask = np.where(r - 0.5 <= 0.0, -1.0, 1.0)
    out = R.signed_distance(mask, dx)
    err = np.abs(out - (r - 0.5)).max() / max(dx)
    print("mask: max error %.3f max(dx)" % err)
    assert err <= 1.25


def test_periodic_axis_wraps():
    shape = (30, 26)
    X, dx = axes(shape, periodic=(0,))
    away = np.abs(X[0] + 0.9)
    data = np.sqrt(away ** 2 + X[1] ** 2) - 0.15
    wrapped = np.sqrt(np.minimum(away, 2.0 - away) ** 2 + X[1] ** 2) - 0.15
    out = R.signed_distance(data, dx, periodic=[True, False])
    err = np.abs(out - wrapped).max() / max(dx)
    print("periodic: max error %.3f max(dx)" % err)
    assert err <= 1.25
    plain = R.signed_distance(data, dx, periodic=[False, False])
    assert np.abs(plain - out).max() > 1.0


def wall_case(shape=(31, 26)):
    X, dx = axes(shape)
    data = np.sqrt((X[0] + 0.5) ** 2 + X[1] ** 2) - 0.2
    walled = data.copy()
    walled[shape[0] // 2, :] = np.nan
    walled[shape[0] // 2, 2:5] = data[shape[0] // 2, 2:5]           # the gap
    return data, walled, dx


def test_walls_give_geodesic_distances():
    data, walled, dx = wall_case()
    free = R.signed_distance(data, dx)
    out = R.signed_distance(walled, dx)
    wall = np.isnan(walled)
    assert np.isnan(out[wall]).all() and not np.isnan(out[~wall]).any()
    assert (out[~wall] >= free[~wall]).all()
    behind = (25, 20)                                                # far side of the wall, away from the gap
    print("walls: %.3f behind the wall, %.3f without it" % (out[behind], free[behind]))
    assert out[behind] > free[behind] + 0.5
    assert np.array_equal(out[:15], free[:15])                       # the source's side never saw the wall


def test_single_sign_is_infinite_after_one_pass():
    X, dx = axes((9, 8))
    for sign in (1.0, -1.0):
        out, passes = R.signed_distance(sign * (2.0 + X[0]), dx, return_passes=True)
        assert passes == 1 and np.array_equal(out, np.full((9, 8), sign * np.inf))
    out = R.signed_distance(2.0 + X[0], dx, band=0.3)
    assert np.array_equal(out, np.full((9, 8), 0.3))


@pytest.mark.parametrize("shape", [(41, 41), (33, 27, 29)], ids=str)
def test_the_fixed_point_does_not_depend_on_the_schedule(shape):
    X, dx = axes(shape)
    r = np.sqrt(sum(x * x for x in X))
    data = (r - 0.5) * (1.0 + 0.5 * X[0])
    sync = R.signed_distance(data, dx)
    half = R.signed_distance(data, dx, schedule=np.random.default_rng(7))
    diff = np.abs(sync - half).max()
    print("schedules %r: max difference %.3g, array_equal %s" % (shape, diff, np.array_equal(sync, half)))
    assert diff <= tolerance(shape, sync)


def test_band_clamps_and_leaves_the_rest():
    shape = (41, 41)
    X, dx = axes(shape)
    r = np.sqrt(X[0] ** 2 + X[1] ** 2)
    full = R.signed_distance(r - 0.5, dx)
    band = 4 * dx[0]
    out = R.signed_distance(r - 0.5, dx, band=band)
    inside = np.abs(full) <= band
    assert np.array_equal(out[inside], full[inside])
    assert np.array_equal(out[~inside], np.sign(full[~inside]) * band)


def test_speed_scales_arrival_times():
    shape = (21, 17)
    X, dx = axes(shape)
    data = X[0] + 0.25
    one = R.signed_distance(data, dx)
    two = R.signed_distance(data, dx, speed=2.0)
    assert np.abs(two - one / 2.0).max() <= tolerance(shape, one)
    speed = np.ones(shape)
    speed[15, 3:12] = 0.0                                            # a zero-speed wall
    out = R.signed_distance(data, dx, speed=speed)
    assert np.isnan(out[15, 3:12]).all() and np.isfinite(out[speed > 0]).all()
    assert out[16, 7] > one[16, 7]
