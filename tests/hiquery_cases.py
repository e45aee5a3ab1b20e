"""What tests/test_hiquery_host.py and tests/test_gpu_hiquery.py share -- TEST INFRASTRUCTURE, NOT PRODUCT: the 5-D / 6-D grids
of tests/hidim_cases.py as package grid and oracle grid, their data, and the two plants of hjx_rollout (include/hj_hiquery.h)
restated for tests/rollout_ref.py, whose PLANTS table is extended here, at import.

The plants are dynamics.py's Plane5D / DubinsPair6D dynSys methods, one fp64 operation per element and statement:
    plane5d  par (a_max, alpha_max)       f = (x3 cos x2, x3 sin x2, x4, a, al);  a = a_max sgn(p3), al = alpha_max sgn(p4) for
                                          uMode 'max', both negated for 'min'; no disturbance
    pair6d   par (v_e, v_p, w_e, w_p)     f = (v_e cos x2, v_e sin x2, u, v_p cos x5, v_p sin x5, d);  u = w_e sgn(p2) for uMode
                                          'max', negated for 'min';  d = w_p sgn(p5) for dMode 'max', negated for 'min'
"""
import numpy as np

import hidim_cases as HC
import rollout_ref as R


def plane5d_controls(par, P, X, uMode, dMode):
    a = par[0] * R.sgn(P[:, 3])
    al = par[1] * R.sgn(P[:, 4])
    if uMode == 'min':
        a, al = -a, -al
    return a, al, [P[:, 3], P[:, 4]]


def plane5d_f(par, X, a, al):
    c = np.cos(X[:, 2])
    s = np.sin(X[:, 2])
    return np.stack([X[:, 3] * c, X[:, 3] * s, X[:, 4], a, al], axis=1)


def pair6d_controls(par, P, X, uMode, dMode):
    u = par[2] * R.sgn(P[:, 2])
    if uMode == 'min':
        u = -u
    d = par[3] * R.sgn(P[:, 5])
    if dMode == 'min':
        d = -d
    return u, d, [P[:, 2], P[:, 5]]


def pair6d_f(par, X, u, d):
    ve, vp = par[0], par[1]
    c2, s2, c5, s5 = np.cos(X[:, 2]), np.sin(X[:, 2]), np.cos(X[:, 5]), np.sin(X[:, 5])
    return np.stack([ve * c2, ve * s2, u, vp * c5, vp * s5, d], axis=1)


R.PLANTS.update({"plane5d": (plane5d_controls, plane5d_f, 5), "pair6d": (pair6d_controls, pair6d_f, 6)})

PLANT_OF = {5: "plane5d", 6: "pair6d"}
PLANT_ID = {"plane5d": 50, "pair6d": 51}
PLANT_PAR = {"plane5d": (0.8, 1.3), "pair6d": (1.5, 1.1, 0.9, 1.4)}

_GRIDS = {}


def grids(name):
    """(package grid Bundle, oracle Grid) of a case of tests/hidim_cases.py: 'plane5d' (7, 6, 8, 5, 9), 'pair6d'
    (6, 5, 7, 5, 6, 8), 'plane5d_long' (5, 5, 6, 5, 70)."""
    if name not in _GRIDS:
        import levelsetpy_amd as L
        gmin, gmax, N, pd = HC.limits(name)
        col = lambda v, t: np.asarray(v, dtype=t).reshape(-1, 1)      # noqa: E731
        _GRIDS[name] = (L.createGrid(col(gmin, np.float64), col(gmax, np.float64), col(N, np.int64), pd), HC.oracle_grid(name))
    return _GRIDS[name]


def noisy(name, seed=7):
    """hidim_cases.data: no ENO choice ties."""
    return HC.data(grids(name)[1], seed)


def smooth(g, seed=0):
    """tests/test_gpu_rollout.py's analytic data at any number of axes: bent, asymmetric, distance-like and above -0.9, so
    data[1] = data[0] + 1 holds no state."""
    xs = np.meshgrid(*[np.asarray(v).ravel() for v in g.vs], indexing='ij')
    r = np.sqrt(sum((x - 0.1 * (d + 1)) ** 2 for d, x in enumerate(xs)))
    return r + 0.2 * np.sin(2 * xs[0] + 0.3 * seed) * np.cos(xs[-1]) + 0.05 * np.sin(3.1 * xs[1] + 0.3) - 0.5


def system(name, g):
    import levelsetpy_amd as L
    par = PLANT_PAR[name]
    return L.Plane5D(g, par[0], par[1]) if name == "plane5d" else L.DubinsPair6D(g, *par)


# ---- the whole-horizon case: the pursuit game on the 6-D grid
HORIZON_TAU = np.linspace(0.0, 0.24, 5)
HORIZON_PAR = (1.0, 1.0, 1.0, 1.0)


def horizon_target(og):
    """The collision set of the two vehicles, radius 0.9, with hidim_cases' noise so that no ENO choice ties."""
    x = og.xs
    rng = np.random.default_rng(11)
    return np.sqrt((x[0] - x[3]) ** 2 + (x[1] - x[4]) ** 2 + 0.01) - 0.9 + 0.02 * rng.standard_normal(og.shape)


def horizon_states(og, M=64):
    """M joint states from a fixed seed: the evader anywhere in the inner part of its box, the pursuer up to 1.6 away, some
    of them next to the boundary of the position axes (those leave the grid)."""
    rng = np.random.default_rng(5)
    lo = np.array([float(np.asarray(v).ravel()[0]) for v in og.vs])
    hi = np.array([float(np.asarray(v).ravel()[-1]) for v in og.vs])
    xs = lo + rng.random((M, 6)) * (hi - lo)
    xs[:, 3:5] = np.clip(xs[:, 0:2] + 1.6 * (rng.random((M, 2)) - 0.5) * 2, lo[3:5] + 0.02, hi[3:5] - 0.02)
    xs[:8, 0] = hi[0] - 0.01 * (1 + np.arange(8))            # the evader next to the edge it may drive over
    xs[:8, 2] = 0.05 * np.arange(8)
    return xs
