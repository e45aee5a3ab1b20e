"""NumPy restatement of computeOptTrajs (levelsetpy_amd/rollout.py, csrc/hj_rollout.hip) -- TEST INFRASTRUCTURE, NOT PRODUCT
(the package never imports it).

Built on tests/query_ref.py: V at a state is eval_u_ref, the costate eval_u_ref over the oracle's (reference-pinned) upwind
derivatives of the slice (costate_ref, one derivative table per visited slice).  All M trajectories advance together; every
array operation below is ONE fp64 operation per element, in the order include/hj_rollout.h states, so for a plant without
trigonometry the result equals the kernel's bit for bit (the costates enter only through their signs).

    for it = 0 .. T-2:
        tE = bisection over [tE, T-1]: mid = (upper + lower + 1) // 2; V[mid](x) < 1e-4 ? lower = mid : upper = mid - 1
        stop if tE == T-1
        subSamples times: p = grad V[tE](x); controls from sgn() of the switching functions; one RK4 step of dt_small
        column it+1 = x

sgn(s) = +1 for s >= 0, -1 for s < 0, NaN for NaN.  A state outside an extrapolated axis or not finite has NaN values and
costates, hence NaN controls and NaN states from then on.

rollout_ref also reports, per trajectory, whether a decision along it was FRAGILE: a switching function with
0 < |s| < 1e-6, or a bisection value within 1e-6 of the threshold 1e-4 -- a last-place difference in sin / cos could
legitimately flip such a decision.  Exact zeros are not fragile: sgn(0) = +1 is deterministic.
"""
import numpy as np

import query_ref as Q

REACHED, EXHAUSTED, LEFT_GRID = 0, 1, 2
SMALL = 1e-4
FRAGILE = 1e-6


def sgn(s):
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(s >= 0, 1.0, np.where(s < 0, -1.0, np.nan))


# ------------------------------------------------------------------------------------------ the plants
# controls(par, P, X, uMode, dMode) -> (c0, c1, [switching functions]);  f(par, X, c0, c1) -> Xdot.  X, P are (M, dim).
def dubins_controls(par, P, X, uMode, dMode):
    ve, vp, w = par
    s1 = P[:, 0] * X[:, 1]
    s2 = P[:, 1] * X[:, 0]
    s = s1 - s2
    s = s - P[:, 2]
    a = w * sgn(s)
    if uMode == 'min':
        a = -a
    b = w * sgn(P[:, 2])
    if dMode == 'min':
        b = -b
    return a, b, [s, P[:, 2]]


def dubins_f(par, X, a, b):
    ve, vp, w = par
    vc = vp * np.cos(X[:, 2])
    drift = -ve + vc
    ax2 = a * X[:, 1]
    f1 = drift + ax2
    vs = vp * np.sin(X[:, 2])
    ax1 = a * X[:, 0]
    f2 = vs - ax1
    f3 = b - a
    return np.stack([f1, f2, f3], axis=1)


def integrator_controls(par, P, X, uMode, dMode):
    u = par[0] * sgn(P[:, 1])
    if uMode == 'min':
        u = -u
    return u, np.zeros_like(u), [P[:, 1]]


def integrator_f(par, X, u, _):
    return np.stack([X[:, 1], u], axis=1)


def pendulum_controls(par, P, X, uMode, dMode):
    u1 = par[0] * sgn(P[:, 1])
    u2 = par[0] * sgn(P[:, 3])
    if uMode == 'min':
        u1, u2 = -u1, -u2
    return u1, u2, [P[:, 1], P[:, 3]]


def pendulum_f(par, X, u1, u2):
    G, L1, L2, M1, M2 = 9.8, 1.0, 1.0, 1.0, 1.0
    th1, w1, th2, w2 = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    s1, c1, s2, c2 = np.sin(th1), np.cos(th1), np.sin(th2), np.cos(th2)
    sd, cd = s2 * c1 - c2 * s1, c2 * c1 + s2 * s1
    den1 = (M1 + M2) * L1 - M2 * L1 * cd * cd
    f1 = (M2 * L1 * w1 * w1 * sd * cd + M2 * G * s2 * cd + M2 * L2 * w2 * w2 * sd - (M1 + M2) * G * s1) / den1
    den2 = (L2 / L1) * den1
    f3 = (-M2 * L2 * w2 * w2 * sd * cd + (M1 + M2) * G * s1 * cd - (M1 + M2) * L1 * w1 * w1 * sd - (M1 + M2) * G * s2) / den2
    return np.stack([w1, f1 + u1, w2, f3 + u2], axis=1)


PLANTS = {"dubins": (dubins_controls, dubins_f, 3), "integrator": (integrator_controls, integrator_f, 2),
          "pendulum": (pendulum_controls, pendulum_f, 4)}


def rk4(f, X, dt):
    h = .5 * dt
    k1 = f(X)
    k2 = f(X + h * k1)
    k3 = f(X + h * k2)
    k4 = f(X + dt * k3)
    return X + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


# ------------------------------------------------------------------------------------------ queries
def outside(grid, X):
    """Rows of X outside an extrapolated axis or not finite."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.dim)
    bad = ~np.isfinite(X).all(axis=1)
    per = Q.periodic_axes(grid)
    with np.errstate(invalid='ignore'):
        for d in range(grid.dim):
            if not per[d]:
                v = np.asarray(grid.vs[d], dtype=np.float64).ravel()
                bad |= (X[:, d] < v[0]) | (X[:, d] > v[-1])
    return bad


def _eval(grid, arr, X):
    """eval_u_ref with NaN for states that are not finite (eval_u_ref itself only knows states outside an axis)."""
    bad = ~np.isfinite(X).all(axis=1)
    first = np.array([float(np.asarray(v).ravel()[0]) for v in grid.vs])
    v = Q.eval_u_ref(grid, arr, np.where(bad[:, None], first[None, :], X))
    v[bad] = np.nan
    return v


class Stack(object):
    """V and grad V of the slices of a time-first stack at states, one derivative table per slice, made when first used."""

    def __init__(self, ogrid, data, scheme):
        self.g, self.data, self.scheme = ogrid, np.asarray(data), scheme
        self.tables = {}

    def values(self, idx, X):
        out = np.empty(len(idx))
        for k in np.unique(idx):
            sel = idx == k
            out[sel] = _eval(self.g, self.data[k], X[sel])
        return out

    def costates(self, idx, X):
        from oracle import hj_oracle as O
        out = np.empty((len(idx), self.g.dim))
        for k in np.unique(idx):
            if k not in self.tables:
                self.tables[k] = O.compute_gradients(self.g, np.asarray(self.data[k], dtype=np.float64), self.scheme)
            sel = idx == k
            for d in range(self.g.dim):
                out[sel, d] = _eval(self.g, self.tables[k][d], X[sel])
        return out


def rollout_ref(ogrid, data, tau, plant, par, x0s, uMode='min', dMode='min', subSamples=4, scheme='WENO5_ASSHIPPED'):
    """-> trajs (M, dim, T) with NaN past the length, lengths (M,) int32, tEarliest (M, T) int32 (-1 where no bisection ran),
    status (M,) int32, fragile (M,) bool.  `data` fp64 or fp32 (widened exactly); `par` the plant's parameters:
    dubins (v_e, v_p, w), integrator (u_bound,), pendulum (u_max,)."""
    controls, f, nd = PLANTS[plant]
    assert nd == ogrid.dim
    tau = np.asarray(tau, dtype=np.float64).ravel()
    T = len(tau)
    dt = (tau[1] - tau[0]) / subSamples
    S = Stack(ogrid, data, scheme)
    X = np.array(x0s, dtype=np.float64).reshape(-1, nd)
    M = X.shape[0]
    trajs = np.full((M, nd, T), np.nan)
    trajs[:, :, 0] = X
    lengths = np.ones(M, dtype=np.int32)
    te = np.full((M, T), -1, dtype=np.int32)
    tE = np.zeros(M, dtype=np.int64)
    done, reached, fragile = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    left = outside(ogrid, X)
    with np.errstate(invalid='ignore', over='ignore'):
        for it in range(T - 1):
            act = ~done
            lower = tE.copy()
            upper = np.where(act, T - 1, tE)
            while True:
                op = np.nonzero(upper > lower)[0]
                if op.size == 0:
                    break
                mid = (upper[op] + lower[op] + 1) // 2
                v = S.values(mid, X[op])
                fragile[op] |= np.abs(v - SMALL) < FRAGILE
                yes = v < SMALL
                lower[op[yes]] = mid[yes]
                upper[op[~yes]] = mid[~yes] - 1
            tE[act] = upper[act]
            te[act, it] = tE[act]
            new = act & (tE == T - 1)
            done |= new
            reached |= new
            run = np.nonzero(~done)[0]
            if run.size:
                Xr = X[run]
                for _ in range(subSamples):
                    P = S.costates(tE[run], Xr)
                    c0, c1, sw = controls(par, P, Xr, uMode, dMode)
                    for s in sw:
                        fragile[run] |= (np.abs(s) > 0) & (np.abs(s) < FRAGILE)
                    Xr = rk4(lambda Z: f(par, Z, c0, c1), Xr, dt)
                X[run] = Xr
                lengths[run] = it + 2
                left[run] |= outside(ogrid, Xr)
                trajs[run, :, it + 1] = Xr
    status = np.where(left, LEFT_GRID, np.where(reached, REACHED, EXHAUSTED)).astype(np.int32)
    return trajs, lengths, te, status, fragile


def solve_min_over_time(ogrid, system, data0, tau, scheme, factor_cfl=0.8):
    """The stack HJIPDE_solve(..., 'minVOverTime') stores, from the oracle: RK3 single steps at factor_cfl up to every time
    stamp, each followed by the minimum with the state before it; time first, NOT flipped."""
    from oracle import hj_oracle as O
    term = lambda t, y: O.term_lax_friedrichs(ogrid, system, scheme, t, y)      # noqa: E731
    tau = np.asarray(tau, dtype=np.float64).ravel()
    y = np.asarray(data0, dtype=np.float64).reshape(-1, 1)
    out = [y.reshape(ogrid.shape).copy()]
    t = float(tau[0])
    for k in range(1, len(tau)):
        while t < tau[k] - 1e-4:
            last = y
            t, y = O.ode_cfl_3(term, [t, tau[k]], y, factor_cfl, single_step=True)
            y = np.minimum(y.reshape(-1, 1), last)
        out.append(y.reshape(ogrid.shape).copy())
    return np.stack(out)
