"""NumPy restatement of computeSafeTrajs and safeControls for a plant whose held values are a tuple of controls u and a tuple of
disturbances d (extraArgs.plantKernel: libhj_plant.so's user_filtered_rollout_kernel / user_decide_points_kernel) -- TEST
INFRASTRUCTURE, NOT PRODUCT (the package never imports it).

The plants are rollout_ref.PLANTS' in the convention of 'lin' and 'quad' (tests/plant_cases.py): controls(par, P, X, uMode, dMode) ->
(u tuple, d tuple, switching functions), f(par, X, u, d).  UD gives the three built-in 2-D .. 4-D plants in that form, from their own
restatements, so that this file can be held against tests/filter_ref.py bit for bit.  Built on filter_ref._Field, rollout_ref.rk4 /
outside and mc_ref.nmin; the trajectory is filter_ref's statement for statement with

    where !act:  u = the table's row (NU values), or the u of the plant's controls for grad Vn with the nominal's uMode
    'zero':      every d[j] = 0.0
    applied[m][step] = (u, d, 0.0 ...) W = max(2, NU + NDST) wide

The noisy trajectory needs no restatement of its own: mc_ref.mc_ref takes 'quad', 'lin', 'plane5d' and 'pair6d' by name.
"""
import numpy as np

import filter_ref as F
import hiquery_cases as XC      # noqa: F401  (adds plane5d / pair6d to rollout_ref.PLANTS)
import mc_ref as MC
import rollout_ref as R

SAFE, VIOLATED, LEFT_GRID = F.SAFE, F.VIOLATED, F.LEFT_GRID
FRAGILE = 1e-6


# filter_ref.HELD for the two 5-D / 6-D systems: Plane5D's acceleration and turn rate are controls, DubinsPair6D holds the evader's turn
# rate and the pursuer's (include/hj_hiquery.h's table)
HELD = dict(F.HELD, plane5d="cc", pair6d="cd")


def _ud(name):
    """A built-in plant of HELD in u / d form."""
    controls, f, nd = R.PLANTS[name]
    held = HELD[name]

    def ud_controls(par, P, X, uMode, dMode):
        c0, c1, sw = controls(par, P, X, uMode, dMode)
        c = (c0, c1)
        return tuple(c[h] for h in range(2) if held[h] == 'c'), tuple(c[h] for h in range(2) if held[h] == 'd'), sw

    def ud_f(par, X, u, d):
        vals, iu, idd = [], 0, 0
        for h in range(2):
            if held[h] == 'c':
                vals.append(u[iu])
                iu += 1
            elif held[h] == 'd':
                vals.append(d[idd])
                idd += 1
            else:
                vals.append(0.0)
        return f(par, X, vals[0], vals[1])
    return ud_controls, ud_f, nd


UD = dict((name + "_ud", _ud(name)) for name in HELD)


def plant_of(name):
    return UD[name] if name in UD else R.PLANTS[name]


def _cols(t, M):
    return [np.broadcast_to(np.asarray(v, dtype=np.float64), (M,)).copy() for v in t]


def _decide(plant, par, V, Vn, sl, sn, X, u_rows, uMode, dMode, nomMode, level, margin, dstb):
    """One sub-step's decision for every row -> v, p, gap, act, u (list of columns), d (list), fragile."""
    controls = plant_of(plant)[0]
    M = X.shape[0]
    v = V.values(sl, X)
    P = V.costates(sl, X)
    gap = v - level if uMode == 'max' else level - v
    u, d, sw = controls(par, P, X, uMode, dMode)
    u, d = _cols(u, M), _cols(d, M)
    act = ~(gap > margin)
    fragile = np.abs(gap - margin) < FRAGILE
    for s in sw:
        fragile |= (np.abs(s) > 0) & (np.abs(s) < FRAGILE)
    idle = np.nonzero(~act)[0]
    if idle.size:
        if Vn is None:
            for j in range(len(u)):
                u[j][idle] = u_rows[idle, j]
        else:
            Qn = Vn.costates(sn[idle], X[idle])
            un, _, swn = controls(par, Qn, X[idle], nomMode, dMode)
            for s in swn:
                fragile[idle] |= (np.abs(s) > 0) & (np.abs(s) < FRAGILE)
            for j in range(len(u)):
                u[j][idle] = un[j]
    if dstb == 'zero':
        for j in range(len(d)):
            d[j][:] = 0.0
    return v, P, gap, act, u, d, fragile


def width(nu, ndst):
    return max(2, nu + ndst)


def _row(u, d, M):
    W = width(len(u), len(d))
    out = np.zeros((M, W))
    for k, c in enumerate(list(u) + list(d)):
        out[:, k] = c
    return out


def filter_ref(ogrid, data, tau, plant, par, x0s, nominal, uMode='max', dMode='min', subSamples=4, scheme='WENO5_ASSHIPPED',
               margin=0.0, level=0.0, policy='clock', slice=0, dstb='worst', nomMode=None):
    """filter_ref.filter_ref's arguments and result; `nominal` a table (M, T-1, NU) or (T-1, NU) or a dict(data=, uMode=); applied is
    (M, nsteps, W)."""
    f, nd = plant_of(plant)[1], plant_of(plant)[2]
    assert nd == ogrid.dim and policy in ('clock', 'static') and dstb in ('worst', 'zero')
    tau = np.asarray(tau, dtype=np.float64).ravel()
    T = len(tau)
    dt = (tau[1] - tau[0]) / subSamples
    V = F._Field(ogrid, data, scheme)
    assert not (V.single and policy == 'clock')
    X = np.array(x0s, dtype=np.float64).reshape(-1, nd)
    M = X.shape[0]
    Vn, table = None, None
    if isinstance(nominal, dict):
        Vn = F._Field(ogrid, nominal["data"], scheme)
        nomMode = nominal.get("uMode", nomMode or uMode)
    else:
        table = np.asarray(nominal, dtype=np.float64)
        table = np.broadcast_to(table, (M,) + table.shape[-2:])
    nsteps = (T - 1) * subSamples
    traj = np.empty((M, nd, T))
    traj[:, :, 0] = X
    active = np.zeros((M, nsteps), dtype=bool)
    applied = None
    count, first = np.zeros(M, dtype=np.int32), np.full(M, -1, dtype=np.int32)
    fragile = np.zeros(M, dtype=bool)
    left = R.outside(ogrid, X)
    gmin = None
    with np.errstate(invalid='ignore', over='ignore'):
        for it in range(T - 1):
            sl = np.full(M, it if policy == 'clock' else slice, dtype=np.int64)
            sn = np.full(M, 0 if (Vn is not None and Vn.single) else it, dtype=np.int64)
            for s in range(subSamples):
                v, _, gap, act, u, d, fr = _decide(plant, par, V, Vn, sl, sn, X, table[:, it] if table is not None else None, uMode,
                                                   dMode, nomMode, level, margin, dstb)
                gmin = gap if gmin is None else MC.nmin(gmin, gap)
                fragile |= fr
                step = it * subSamples + s
                first[act & (count == 0)] = step
                count[act] += 1
                active[:, step] = act
                row = _row(u, d, M)
                if applied is None:
                    applied = np.empty((M, nsteps, row.shape[1]))
                applied[:, step] = row
                ut, dt_ = tuple(u), tuple(d)
                X = R.rk4(lambda Z: f(par, Z, ut, dt_), X, dt)
            left |= R.outside(ogrid, X)
            traj[:, :, it + 1] = X
        vend = V.values(np.full(M, T - 1 if policy == 'clock' else slice, dtype=np.int64), X)
        gap = vend - level if uMode == 'max' else level - vend
        fragile |= np.abs(gap) < FRAGILE
        gmin = MC.nmin(gmin, gap)
        status = np.where(left, LEFT_GRID, np.where(~(gmin > 0), VIOLATED, SAFE)).astype(np.int32)
    return dict(traj=traj, final=X, gap_min=gmin, value_end=vend, interventions=count, first=first,
                length=np.full(M, T, dtype=np.int32), status=status, active=active, applied=applied, fragile=fragile)


def decide_ref(ogrid, field, plant, par, xs, u_nom, uMode='max', dMode='min', scheme='WENO5_ASSHIPPED', margin=0.0, level=0.0,
               dstb='worst'):
    """-> dict(applied (M, W), active (M,) bool, value, gap (M,), costate (M, dim), fragile (M,) bool)."""
    nd = plant_of(plant)[2]
    X = np.array(xs, dtype=np.float64).reshape(-1, nd)
    M = X.shape[0]
    z = np.zeros(M, dtype=np.int64)
    rows = np.asarray(u_nom, dtype=np.float64)
    rows = np.broadcast_to(rows, (M, rows.shape[-1]))
    with np.errstate(invalid='ignore', over='ignore'):
        v, P, gap, act, u, d, fr = _decide(plant, par, F._Field(ogrid, field, scheme), None, z, z, X, rows, uMode, dMode, None, level,
                                           margin, dstb)
    return dict(applied=_row(u, d, M), active=act, value=v, gap=gap, costate=P, fragile=fr)
