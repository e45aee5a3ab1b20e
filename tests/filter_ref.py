"""NumPy restatement of computeSafeTrajs and safeControls (levelsetpy_amd/safety.py, csrc/hj_filter.hip, include/hj_filter.h) --
TEST INFRASTRUCTURE, NOT PRODUCT (the package never imports it).

Built on tests/rollout_ref.py: its plants, rk4, Stack (V and grad V at states) and outside, and on tests/mc_ref.py's nmin.  All M
trajectories advance together; every array operation is ONE fp64 operation per element in the order include/hj_filter.h states, so
for a plant without trigonometry the result equals the kernel's bit for bit.

    column 0 = x
    for it = 0 .. T-2:
        sl = clock ? it : slice
        subSamples times: v = V[sl](x); p = grad V[sl](x); gap = uMode max ? v - level : level - v; gap_min = nmin(gap_min, gap)
                          (c0, c1) = the plant's controls for p;  act = !(gap > margin)
                          where !act, every CONTROL among (c0, c1): the table's u_nom[m][it][j], or the plant's controls for
                          grad Vn[nom has one field ? 0 : it](x) with the nominal's uMode
                          'zero': every DISTURBANCE among (c0, c1) = 0.0
                          one RK4 step of dt_small
        column it+1 = x
    v = V[clock ? T-1 : slice](x); gap; gap_min = nmin(gap_min, gap); value_end = v

decide_ref is one sub-step's decision without the step.  Both report which rows are FRAGILE: a switching function the decision read
with 0 < |s| < 1e-6 (rollout_ref's rule), or a gap within 1e-6 of the margin -- a last-place difference in sin / cos could
legitimately flip such a decision.
"""
import numpy as np

import mc_ref as MC
import rollout_ref as R

SAFE, VIOLATED, LEFT_GRID = 0, 1, 2
FRAGILE = R.FRAGILE
# which of the two held values is a control ('c'), a disturbance ('d') or neither ('-'): include/hj_filter.h's table
HELD = {"dubins": "cd", "integrator": "c-", "pendulum": "cc"}
NU = dict((k, v.count("c")) for k, v in HELD.items())


class _Field(object):
    """A Stack that may hold ONE field serving every slice index (the stride-0 stack of the static policy)."""

    def __init__(self, ogrid, data, scheme):
        data = np.asarray(data)
        self.single = data.ndim == ogrid.dim
        self.S = R.Stack(ogrid, data[None] if self.single else data, scheme)

    def _idx(self, idx):
        return np.zeros_like(idx) if self.single else idx

    def values(self, idx, X):
        return self.S.values(self._idx(idx), X)

    def costates(self, idx, X):
        return self.S.costates(self._idx(idx), X)


def _gap(v, level, uMode):
    return v - level if uMode == 'max' else level - v


def _decide(plant, par, V, Vn, sl, sn, X, u_rows, uMode, dMode, nomMode, level, margin, dstb):
    """One sub-step's decision for every row -> v, p, gap, act, c0, c1, fragile."""
    controls = R.PLANTS[plant][0]
    v = V.values(sl, X)
    P = V.costates(sl, X)
    gap = _gap(v, level, uMode)
    c0, c1, sw = controls(par, P, X, uMode, dMode)
    c = [np.array(c0, dtype=np.float64), np.array(c1, dtype=np.float64)]
    act = ~(gap > margin)
    fragile = np.abs(gap - margin) < FRAGILE
    for s in sw:
        fragile |= (np.abs(s) > 0) & (np.abs(s) < FRAGILE)
    idle = np.nonzero(~act)[0]
    if idle.size:
        if Vn is None:
            j = 0
            for h in range(2):
                if HELD[plant][h] == 'c':
                    c[h][idle] = u_rows[idle, j]
                    j += 1
        else:
            Qn = Vn.costates(sn[idle], X[idle])
            n0, n1, swn = controls(par, Qn, X[idle], nomMode, dMode)
            for s in swn:
                fragile[idle] |= (np.abs(s) > 0) & (np.abs(s) < FRAGILE)
            for h, n in enumerate((n0, n1)):
                if HELD[plant][h] == 'c':
                    c[h][idle] = n
    if dstb == 'zero':
        for h in range(2):
            if HELD[plant][h] == 'd':
                c[h][:] = 0.0
    return v, P, gap, act, c[0], c[1], fragile


def filter_ref(ogrid, data, tau, plant, par, x0s, nominal, uMode='max', dMode='min', subSamples=4, scheme='WENO5_ASSHIPPED',
               margin=0.0, level=0.0, policy='clock', slice=0, dstb='worst', nomMode=None):
    """`data`: a (T,) + shape stack, or one field (policy 'static').  `nominal`: an (M, T-1, NU) or (T-1, NU) table, or a dict
    (data=..., uMode=...) of a second value function (a stack or one field).
    -> dict(traj (M, dim, T), final (M, dim), gap_min, value_end (M,), interventions, first, length, status (M,) int32,
            active (M, nsteps) bool, applied (M, nsteps, 2), fragile (M,) bool)."""
    f, nd = R.PLANTS[plant][1], R.PLANTS[plant][2]
    assert nd == ogrid.dim and policy in ('clock', 'static') and dstb in ('worst', 'zero')
    tau = np.asarray(tau, dtype=np.float64).ravel()
    T = len(tau)
    dt = (tau[1] - tau[0]) / subSamples
    V = _Field(ogrid, data, scheme)
    assert not (V.single and policy == 'clock')
    X = np.array(x0s, dtype=np.float64).reshape(-1, nd)
    M = X.shape[0]
    Vn, table = None, None
    if isinstance(nominal, dict):
        Vn = _Field(ogrid, nominal["data"], scheme)
        nomMode = nominal.get("uMode", nomMode or uMode)
    else:
        table = np.broadcast_to(np.asarray(nominal, dtype=np.float64), (M, T - 1, NU[plant]))
    nsteps = (T - 1) * subSamples
    traj = np.empty((M, nd, T))
    traj[:, :, 0] = X
    active = np.zeros((M, nsteps), dtype=bool)
    applied = np.empty((M, nsteps, 2))
    count, first = np.zeros(M, dtype=np.int32), np.full(M, -1, dtype=np.int32)
    fragile = np.zeros(M, dtype=bool)
    left = R.outside(ogrid, X)
    gmin = None
    with np.errstate(invalid='ignore', over='ignore'):
        for it in range(T - 1):
            sl = np.full(M, it if policy == 'clock' else slice, dtype=np.int64)
            sn = np.full(M, 0 if (Vn is not None and Vn.single) else it, dtype=np.int64)
            for s in range(subSamples):
                v, _, gap, act, c0, c1, fr = _decide(plant, par, V, Vn, sl, sn, X, table[:, it] if table is not None else None, uMode,
                                                     dMode, nomMode, level, margin, dstb)
                gmin = gap if gmin is None else MC.nmin(gmin, gap)
                fragile |= fr
                step = it * subSamples + s
                first[act & (count == 0)] = step
                count[act] += 1
                active[:, step] = act
                applied[:, step, 0], applied[:, step, 1] = c0, c1
                X = R.rk4(lambda Z: f(par, Z, c0, c1), X, dt)
            left |= R.outside(ogrid, X)
            traj[:, :, it + 1] = X
        vend = V.values(np.full(M, T - 1 if policy == 'clock' else slice, dtype=np.int64), X)
        gap = _gap(vend, level, uMode)
        fragile |= np.abs(gap) < FRAGILE
        gmin = MC.nmin(gmin, gap)
        status = np.where(left, LEFT_GRID, np.where(~(gmin > 0), VIOLATED, SAFE)).astype(np.int32)
    return dict(traj=traj, final=X, gap_min=gmin, value_end=vend, interventions=count, first=first,
                length=np.full(M, T, dtype=np.int32), status=status, active=active, applied=applied, fragile=fragile)


def decide_ref(ogrid, field, plant, par, xs, u_nom, uMode='max', dMode='min', scheme='WENO5_ASSHIPPED', margin=0.0, level=0.0,
               dstb='worst'):
    """-> dict(applied (M, 2), active (M,) bool, value, gap (M,), costate (M, dim), fragile (M,) bool)."""
    nd = R.PLANTS[plant][2]
    X = np.array(xs, dtype=np.float64).reshape(-1, nd)
    M = X.shape[0]
    z = np.zeros(M, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        v, P, gap, act, c0, c1, fr = _decide(plant, par, _Field(ogrid, field, scheme), None, z, z, X,
                                             np.broadcast_to(np.asarray(u_nom, dtype=np.float64), (M, NU[plant])), uMode, dMode, None,
                                             level, margin, dstb)
    return dict(applied=np.stack([c0, c1], axis=1), active=act, value=v, gap=gap, costate=P, fragile=fr)
