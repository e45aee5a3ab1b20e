"""NumPy restatement of HJIPDE_solve with extraArgs.addGaussianNoiseStandardDeviation -- TEST INFRASTRUCTURE, NOT PRODUCT (the
package never imports it).

The reference's wiring (ValueFuncs/hji_solver.py:449-471): termSum of the deterministic term and termTraceHessian with
L = sigma^T, R = sigma, hessianFunc = hessianSecond.  Composed here, in termSum's order (term_sum.py:87-110), from
  * oracle.hj_oracle.term_lax_friedrichs (and term_restrict_update for minWithZero / zero),
  * trace_hess_ref.term_trace_hessian / step_bound,
  * oracle.hj_oracle.ode_cfl_1/2/3,
with HJIPDE_solve's interval loop (`while tNow < tau[i] - 1e-4`, one singleStep odeCFL3 call per pass, factorCFL 0.8) and its
post-step operators (hji_solver.py:566-599, 641-644).  `og` is an oracle Grid, `osys` an oracle system.
"""
import numpy as np

from oracle import hj_oracle as O
import trace_hess_ref as TH

SMALL = 1e-4
FACTOR_CFL = 0.8
ODE = {1: O.ode_cfl_1, 2: O.ode_cfl_2, 3: O.ode_cfl_3}


def matrices(sigma, n):
    """(L, R) = (sigma^T, sigma) as cell matrices of numbers."""
    s = np.asarray(sigma, dtype=np.float64)
    assert s.shape == (n, n)
    return [[float(s[j, i]) for j in range(n)] for i in range(n)], [[float(s[i, j]) for j in range(n)] for i in range(n)]


def step_bounds(og, osys, scheme, sigma, y):
    """(sb, sb_LF, sb_TH): termSum's bound of the two terms and the terms' own."""
    _, sb_lf = O.term_lax_friedrichs(og, osys, scheme, 0.0, np.asarray(y, dtype=np.float64).reshape(-1, 1))
    L, R = matrices(sigma, og.dim)
    sb_th = TH.step_bound(og, L, R)
    inv = 0.0
    inv += 1 / sb_lf
    inv += 1 / sb_th
    return (float('inf') if inv == 0 else 1 / inv), float(sb_lf), float(sb_th)


def term(og, osys, scheme, sigma, restrict_sign=0, parts=None):
    """term(t, y) -> (ydot, stepBound) of termSum([LF or restricted LF, trace term]); y an (N, 1) column.  sigma None: the
    deterministic term alone.  `parts`, a dict, receives the last call's 'lf' and 'trace' columns."""
    L, R = matrices(sigma, og.dim) if sigma is not None else (None, None)

    def f(t, y):
        ylf, sb_lf = O.term_lax_friedrichs(og, osys, scheme, t, y)
        if restrict_sign:
            ylf = np.maximum(ylf, 0) if restrict_sign > 0 else np.minimum(ylf, 0)
        if sigma is None:
            return ylf, sb_lf
        ytr, sb_th = TH.term_trace_hessian(og, y.reshape(og.shape), L, R)
        ytr = ytr.reshape(y.shape)
        if parts is not None:
            parts['lf'], parts['trace'] = ylf, ytr
        ydot = ylf + ytr                                               # term_sum.py:97
        inv = 0.0
        inv += 1 / sb_lf                                               # :98
        inv += 1 / sb_th
        return ydot, (float('inf') if inv == 0 else 1 / inv)
    return f


def stage(og, osys, scheme, sigma, name, y, y0=None, dt=0.0, restrict_sign=0, parts=None):
    """One stage expression of odeCFLn on grid-shaped arrays: 'YDOT', 'EULER', 'RK2_FULL', 'RK3_HALF', 'RK3_FULL'."""
    col = np.asarray(y, dtype=np.float64).reshape(-1, 1)
    ydot, _ = term(og, osys, scheme, sigma, restrict_sign, parts)(0.0, col)
    if name == 'YDOT':
        return ydot.reshape(og.shape)
    e = col + dt * ydot
    if name == 'EULER':
        out = e
    else:
        x0 = np.asarray(y0, dtype=np.float64).reshape(-1, 1)
        if name == 'RK2_FULL':
            out = 0.5 * (x0 + e)                                       # ode_cfl_2.py:201
        elif name == 'RK3_HALF':
            out = 0.25 * (3 * x0 + e)                                  # ode_cfl_3.py:193
        else:
            out = (1 / 3) * (x0 + 2 * e)                               # :241
    return out.reshape(og.shape)


def post_step(y, y_last, y_init, compMethod, target, obstacle):
    if compMethod == 'minVOverTime':
        y = np.minimum(y, y_last)
    elif compMethod == 'maxVOverTime':
        y = np.maximum(y, y_last)
    elif compMethod == 'minVWithV0':
        y = np.minimum(y, y_init)
    elif compMethod == 'maxVWithV0':
        y = np.maximum(y, y_init)
    elif compMethod in ('minVWithL', 'minVwithL', 'minVWithTarget'):
        y = np.minimum(y, target)
    elif compMethod in ('maxVWithL', 'maxVwithL', 'maxVWithTarget'):
        y = np.maximum(y, target)
    else:
        assert compMethod in (None, 'none', 'set', 'zero', 'minWithZero'), compMethod
    if obstacle is not None:
        y = np.maximum(y, -obstacle)
    return y


def interval(og, osys, scheme, sigma, y, t0, tf, order=3, restrict_sign=0, compMethod=None, y_init=None, target=None,
             obstacle=None, stop_tol=SMALL):
    """HJIPDE_solve's loop over one interval on an (N, 1) column: (t, y, steps)."""
    f = term(og, osys, scheme, sigma, restrict_sign)
    t, steps = t0, 0
    col = lambda a: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1, 1)   # noqa: E731
    y_init, target, obstacle = col(y_init), col(target), col(obstacle)
    while t < tf - stop_tol:
        y_last = y
        t, y = ODE[order](f, [t, tf], y, FACTOR_CFL, single_step=True)
        y = post_step(y, y_last, y_init, compMethod, target, obstacle)
        steps += 1
    return t, y, steps


def solve(og, osys, scheme, sigma, data0, tau, compMethod=None, targets=None, obstacles=None):
    """(data (len(tau),) + shape, times reached, steps per interval) of HJIPDE_solve in store-all mode."""
    data0 = np.asarray(data0, dtype=np.float64)
    nd = og.dim
    y = data0.reshape(-1, 1).copy()
    y_init = y.copy()
    rs = -1 if compMethod in ('zero', 'minWithZero') else 0
    out, times, steps = [data0.copy()], [], []
    for i in range(1, len(tau)):
        tg = None if targets is None else (targets[i] if np.ndim(targets) == nd + 1 else targets)
        ob = None if obstacles is None else (obstacles[i] if np.ndim(obstacles) == nd + 1 else obstacles)
        t, y, n = interval(og, osys, scheme, sigma, y, tau[i - 1], tau[i], 3, rs, compMethod, y_init, tg, ob)
        out.append(y.reshape(og.shape).copy())
        times.append(t)
        steps.append(n)
    return np.stack(out), np.asarray(times), np.asarray(steps)
