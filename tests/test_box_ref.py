"""CPU: the box reference (tests/box_ref.py) against the full-grid oracle, and proof that a box comparison bites.

ENO2 / ENO3 on a box equal the full-grid oracle bit for bit (same elementwise expressions on the same numbers); the WENO5 variants differ by
NumPy's own shape dependence (measured <= 2e-15), far inside the standing 1e-11 rule of tests/test_gpu_parity.close."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from levelsetpy_amd import _ffi  # noqa: E402
from oracle import hj_oracle as O  # noqa: E402

import box_ref as B  # noqa: E402
from test_gpu_parity import close  # noqa: E402  (the rule only: importing that module starts nothing on a GPU)

SCHEMES = ["ENO2", "ENO3", "WENO5_ASSHIPPED", "WENO5"]
STAGES = [_ffi.STAGE_YDOT, _ffi.STAGE_EULER, _ffi.STAGE_RK3_HALF, _ffi.STAGE_RK3_FULL]


def _dubins(rng):
    n = [int(v) for v in rng.integers(14, 26, 3)]
    G = O.Grid([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / n[2])], n, [2])
    return G, (lambda g: O.DubinsRel(g, 1, 1)), O.shape_cylinder(G, 2, None, .5)


def _integrator(rng):
    n = [int(v) for v in rng.integers(20, 40, 2)]
    G = O.Grid([-1., -1.5], [1., 1.5], n, None)
    return G, (lambda g: O.DoubleIntegrator(g, 1.25)), O.shape_sphere(G, None, .45)


def _pendulum(rng):
    n = [int(v) for v in rng.integers(8, 12, 4)]
    gmax = [np.pi, 8., np.pi, 8.]
    gmin = [-np.pi, -8., -np.pi, -8.]
    G = O.Grid(gmin, [gmax[d] - (gmax[d] - gmin[d]) / n[d] for d in range(4)], n, [0, 1, 2, 3])
    return G, (lambda g: O.DoublePendulum4D(g, 1.0)), O.shape_sphere(G, None, 2.0)


SYSTEMS = {"dubins": _dubins, "integrator": _integrator, "pendulum": _pendulum}


def _boxes(G, rng, m):
    """(lo, hi) pairs: the two opposite corners, a box across the wrap of every periodic axis (= touching both ends of an extrapolated one
    is the corner case), a box that is the whole of one axis, and a random interior one."""
    N = list(G.shape)
    D = G.dim
    out = [([0] * D, [min(4, n) for n in N]), ([max(0, n - 4) for n in N], N)]
    lo = [int(rng.integers(0, n - 3)) for n in N]
    out.append((lo, [l + 3 for l in lo]))
    for d in range(D):
        lo = [int(rng.integers(0, n - 3)) for n in N]
        hi = [l + 3 for l in lo]
        lo[d], hi[d] = 0, N[d]                                  # the whole of axis d
        out.append((lo, hi))
        lo = [int(rng.integers(0, n - 3)) for n in N]
        hi = [l + 3 for l in lo]
        lo[d], hi[d] = N[d] - 2, N[d]                           # its last two cells: the box reaches across the wrap / the boundary
        out.append((lo, hi))
    return out


def _compare(scheme, got, ref, what=""):
    if scheme.startswith("ENO"):
        assert np.array_equal(got, ref), what
    else:
        close(got, ref, 1e-11, what)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("system", sorted(SYSTEMS))
def test_box_equals_full_grid_oracle(system, seed):
    rng = np.random.default_rng(100 * seed + len(system))
    G, make_sys, smooth = SYSTEMS[system](rng)
    y = smooth + 0.05 * rng.uniform(-1, 1, G.shape)
    y0 = smooth + 0.05 * rng.uniform(-1, 1, G.shape)
    sys_full = make_sys(G)
    dt = 0.4 * O.term_lax_friedrichs(G, sys_full, "ENO2", 0., y.reshape(-1))[1]
    wrapped = corner = whole = 0
    for scheme in SCHEMES:
        eps = [O.max_d1_squared(G, y, d) for d in range(G.dim)] if scheme == "WENO5" else None
        yd = O.term_lax_friedrichs(G, sys_full, scheme, 0., y.reshape(-1), None, eps)[0].reshape(G.shape)
        for lo, hi in _boxes(G, rng, B.M_SUBSTEP):
            idx, cmp = B.box(G, lo, hi, B.M_SUBSTEP)
            wrapped += any(np.any(np.diff(i) != 1) for i in idx)
            corner += all(l == 0 for l in lo)
            whole += any(h - l == n for l, h, n in zip(lo, hi, G.shape))
            sl = np.ix_(*[np.arange(l, h) for l, h in zip(lo, hi)])
            yb, y0b = B.take(y, idx), B.take(y0, idx)
            for st in STAGES:
                got = B.stage(G, make_sys, scheme, idx, st, dt, yb, y0b, eps)[cmp]
                ref = B.stage_expr(st, dt, y, y0, yd)[sl]
                _compare(scheme, got, ref, "%s %s stage %d box %s..%s" % (system, scheme, st, lo, hi))
    assert corner and whole and (wrapped or 'periodic' not in G.bc)


@pytest.mark.parametrize("system,scheme", [("dubins", "ENO2"), ("dubins", "ENO3"), ("dubins", "WENO5_ASSHIPPED"),
                                           ("integrator", "ENO3"), ("pendulum", "WENO5_ASSHIPPED")])
def test_box_rk3_step_equals_full_grid_step(system, scheme):
    rng = np.random.default_rng(7)
    G, make_sys, smooth = SYSTEMS[system](rng)
    y = smooth + 0.05 * rng.uniform(-1, 1, G.shape)
    sys_full = make_sys(G)
    sb = O.term_lax_friedrichs(G, sys_full, scheme, 0., y.reshape(-1))[1]
    tf = 0.5 * 0.8 * sb                                          # below the CFL step: deltaT = tf
    t_full, y_full = O.ode_cfl_3(lambda tt, v: O.term_lax_friedrichs(G, sys_full, scheme, tt, v), [0., tf], y.reshape(-1), 0.8,
                                 single_step=True)
    y_full = y_full.reshape(G.shape)
    for lo, hi in _boxes(G, rng, B.M_RK3)[:5]:
        idx, cmp = B.box(G, lo, hi, B.M_RK3)
        t_box, y_box = B.rk3_step(G, make_sys, scheme, idx, B.take(y, idx), tf)
        assert t_box == t_full
        _compare(scheme, y_box[cmp], y_full[np.ix_(*[np.arange(l, h) for l, h in zip(lo, hi)])], "%s %s..%s" % (system, lo, hi))


def test_light_grid_is_the_oracle_grid_without_xs():
    G = O.Grid([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / 9)], [7, 8, 9], [2])
    Lg = B.light_grid([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / 9)], [7, 8, 9], [2])
    assert Lg.shape == G.shape and Lg.bc == G.bc and np.array_equal(Lg.dx, G.dx)
    assert all(np.array_equal(a, b) for a, b in zip(Lg.vs, G.vs))
    idx, _ = B.box(Lg, [0, 2, 7], [3, 5, 9], 3)
    a, b = B.box_grid(Lg, idx), B.box_grid(G, idx)
    assert all(np.array_equal(u, v) for u, v in zip(a.xs, b.xs)) and a.bc == ['extrapolate'] * 3


def test_gather_is_take():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    G = O.Grid([-.75, -1.25, -np.pi], [3.25, 1.25, np.pi * (1 - 2 / 9)], [11, 12, 9], [0, 2])
    a = rng.standard_normal(G.shape).astype(np.float32)
    for lo, hi in _boxes(G, rng, 3):
        idx, _ = B.box(G, lo, hi, 3)
        got = B.gather(torch.from_numpy(a), idx)
        assert got.dtype == np.float64 and np.array_equal(got, B.take(a, idx).astype(np.float64))


# ------------------------------------------------------------------ the comparison bites
def _damages(r, rng):
    swapped = r.copy()
    a = tuple(int(rng.integers(4, n - 4)) for n in r.shape)
    b = tuple(v + 1 if d == len(a) - 1 else v for d, v in enumerate(a))
    swapped[a], swapped[b] = r[b], r[a]
    return {"shifted by one plane": np.roll(r, 1, axis=0), "shifted by one row": np.roll(r, 1, axis=1), "two cells swapped": swapped}


@pytest.mark.parametrize("scheme", ["ENO2", "WENO5_ASSHIPPED"])
def test_damaged_result_fails_on_every_box_that_holds_a_damaged_cell(scheme):
    rng = np.random.default_rng(11)
    G, make_sys, smooth = _dubins(rng)
    y = smooth + 0.05 * rng.uniform(-1, 1, G.shape)
    good = O.term_lax_friedrichs(G, make_sys(G), scheme, 0., y.reshape(-1))[0].reshape(G.shape)
    boxes = _boxes(G, rng, 3)
    for _ in range(12):
        lo = [int(rng.integers(0, n - 4)) for n in G.shape]
        boxes.append((lo, [l + 4 for l in lo]))
    for what, bad in _damages(good, rng).items():
        hit = clean = 0
        for lo, hi in boxes:
            idx, cmp = B.box(G, lo, hi, 3)
            sl = np.ix_(*[np.arange(l, h) for l, h in zip(lo, hi)])
            ref = B.ydot(G, make_sys, scheme, idx, B.take(y, idx))[cmp]
            _compare(scheme, good[sl], ref)                      # the undamaged result passes on every box
            if np.array_equal(bad[sl], good[sl]):
                _compare(scheme, bad[sl], ref)
                clean += 1
                continue
            hit += 1
            with pytest.raises(AssertionError):
                _compare(scheme, bad[sl], ref, what)
        assert hit, what
        if what == "two cells swapped":                          # a local damage: boxes away from it stay clean, boxes over it fail
            assert clean
    # make sure the swap is seen: a box placed right on the swapped pair
    bad = _damages(good, np.random.default_rng(11))["two cells swapped"]
    where = np.argwhere(bad != good)
    assert len(where) == 2
    lo = [int(max(0, min(v - 1, n - 4))) for v, n in zip(where[0], G.shape)]
    idx, cmp = B.box(G, lo, [l + 4 for l in lo], 3)
    sl = np.ix_(*[np.arange(l, l + 4) for l in lo])
    with pytest.raises(AssertionError):
        _compare(scheme, bad[sl], B.ydot(G, make_sys, scheme, idx, B.take(y, idx))[cmp])
