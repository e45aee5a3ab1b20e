"""NumPy restatement of computeStochTrajs (levelsetpy_amd/montecarlo.py, csrc/hj_mc.hip, include/hj_mc.h) -- TEST
INFRASTRUCTURE, NOT PRODUCT (the package never imports it).

Built on tests/rollout_ref.py: its plants, rk4, Stack (V and grad V at states) and _eval.  All Q = M R realisations advance
together, realisation q = m R + k with the global index first + q; every array operation is ONE fp64 operation per element in
the order include/hj_mc.h states, so for a plant without trigonometry and supplied normals the result equals the kernel's bit
for bit.  Philox4x32-10 runs in integer arithmetic (uint64 products, masked to 32 bits).

    column 0 = x; v = V[T-1](x); value_end = value_min = v
    for it = 0 .. T-2:
        earliest: tE = rollout_ref's bisection, stop if tE == T-1;   clock: tE = it
        subSamples times: p = grad V[tE](x); controls; one RK4 step of dt_small;
                          n_i = ((G_i0 xi_0) + (G_i1 xi_1)) + ...; x_i = x_i + sq n_i
        column it+1 = x; v = V[T-1](x); value_end = v; value_min = nmin(value_min, v)
"""
import numpy as np

import rollout_ref as R

REACHED, EXHAUSTED, LEFT_GRID = R.REACHED, R.EXHAUSTED, R.LEFT_GRID
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586


def philox4x32_10(ctr, key):
    """ctr: four broadcastable integer arrays (each below 2^32), key: two integers -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    k0, k1 = int(key[0]), int(key[1])
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0 = np.uint64(M0) * c0                     # below 2^64: exact
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed, first, count, step0, nsteps, nd):
    """(count, nsteps, (nd+1)//2, 4) uint32: the words of pair j of (realisation first + i, step step0 + s)."""
    seed, first = int(seed), int(first)
    r = [(first + i) % 2 ** 64 for i in range(count)]
    r_lo = np.array([v & 0xFFFFFFFF for v in r], dtype=np.uint64).reshape(-1, 1, 1)
    r_hi = np.array([v >> 32 for v in r], dtype=np.uint64).reshape(-1, 1, 1)
    step = (np.arange(nsteps, dtype=np.uint64) + np.uint64(step0)).reshape(1, -1, 1)
    j = np.arange((nd + 1) // 2, dtype=np.uint64).reshape(1, 1, -1)
    w = philox4x32_10((r_lo, r_hi, step, j), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=-1)


def normals_of(w, nd):
    """Box-Muller on the words (..., npairs, 4) -> (..., nd) float64."""
    w = w.astype(np.uint64)
    k1 = ((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6))
    k2 = ((w[..., 2] >> np.uint64(5)) << np.uint64(26)) + (w[..., 3] >> np.uint64(6))
    u1 = (k1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = k2.astype(np.float64) * 2.0 ** -53
    rad = np.sqrt(-2.0 * np.log(u1))
    a = TWO_PI * u2
    z = np.stack([rad * np.cos(a), rad * np.sin(a)], axis=-1)          # (..., npairs, 2)
    return z.reshape(z.shape[:-2] + (-1,))[..., :nd]


def normals(seed, first, count, step0, nsteps, nd):
    return normals_of(words(seed, first, count, step0, nsteps, nd), nd)


def nmin(a, b):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(b < a, b, a))


def mc_ref(ogrid, data, tau, plant, par, x0s, G, nreal, xi=None, seed=0, first=0, policy='earliest', uMode='min', dMode='min',
           subSamples=4, scheme='WENO5_ASSHIPPED'):
    """-> dict(final (M, R, dim), length, status (M, R) int32, value_end, value_min (M, R), traj (M, R, dim, T) with NaN past the
    length, t_earliest (M, R, T) int32).  `xi`: (M, R, (T-1) subSamples, dim) supplied normals, or None for the generator's."""
    controls, f, nd = R.PLANTS[plant]
    assert nd == ogrid.dim and policy in ('earliest', 'clock')
    tau = np.asarray(tau, dtype=np.float64).ravel()
    T = len(tau)
    dt = (tau[1] - tau[0]) / subSamples
    sq = np.sqrt(np.float64(dt))
    G = np.asarray(G, dtype=np.float64).reshape(nd, nd)
    S = R.Stack(ogrid, data, scheme)
    x0s = np.array(x0s, dtype=np.float64).reshape(-1, nd)
    M = x0s.shape[0]
    Q = M * nreal
    nsteps = (T - 1) * subSamples
    X = np.repeat(x0s, nreal, axis=0)
    if xi is not None:
        xi = np.asarray(xi, dtype=np.float64).reshape(Q, nsteps, nd)
    trajs = np.full((Q, nd, T), np.nan)
    trajs[:, :, 0] = X
    lengths = np.ones(Q, dtype=np.int32)
    te = np.full((Q, T), -1, dtype=np.int32)
    tE = np.zeros(Q, dtype=np.int64)
    done, reached = np.zeros(Q, dtype=bool), np.zeros(Q, dtype=bool)
    left = R.outside(ogrid, X)
    last = np.full(Q, T - 1, dtype=np.int64)
    vend = S.values(last, X)
    vmin = vend.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        for it in range(T - 1):
            act = ~done
            if policy == 'clock':
                tE[:] = it
            else:
                lower = tE.copy()
                upper = np.where(act, T - 1, tE)
                while True:
                    op = np.nonzero(upper > lower)[0]
                    if op.size == 0:
                        break
                    mid = (upper[op] + lower[op] + 1) // 2
                    yes = S.values(mid, X[op]) < R.SMALL
                    lower[op[yes]] = mid[yes]
                    upper[op[~yes]] = mid[~yes] - 1
                tE[act] = upper[act]
                new = act & (tE == T - 1)
                done |= new
                reached |= new
            te[act, it] = tE[act]
            run = np.nonzero(~done)[0]
            if run.size:
                Xr = X[run]
                for s in range(subSamples):
                    P = S.costates(tE[run], Xr)
                    c0, c1, _ = controls(par, P, Xr, uMode, dMode)
                    Xr = R.rk4(lambda Z: f(par, Z, c0, c1), Xr, dt)
                    step = it * subSamples + s
                    z = xi[run, step] if xi is not None else _gen(seed, first, run, step, nd)
                    shift = np.empty_like(Xr)
                    for i in range(nd):
                        n = G[i, 0] * z[:, 0]
                        for j in range(1, nd):
                            n = n + G[i, j] * z[:, j]
                        shift[:, i] = sq * n
                    Xr = Xr + shift
                X[run] = Xr
                lengths[run] = it + 2
                left[run] |= R.outside(ogrid, Xr)
                trajs[run, :, it + 1] = Xr
                v = S.values(last[run], Xr)
                vend[run] = v
                vmin[run] = nmin(vmin[run], v)
    status = np.where(left, LEFT_GRID, np.where(reached, REACHED, EXHAUSTED)).astype(np.int32)
    sh = (M, nreal)
    return dict(final=X.reshape(sh + (nd,)), length=lengths.reshape(sh), status=status.reshape(sh), value_end=vend.reshape(sh),
                value_min=vmin.reshape(sh), traj=trajs.reshape(sh + (nd, T)), t_earliest=te.reshape(sh + (T,)))


def _gen(seed, first, run, step, nd):
    """The generator's normals of one step for the realisations first + run (vectorised over them)."""
    r = [(int(first) + int(q)) % 2 ** 64 for q in run]
    r_lo = np.array([v & 0xFFFFFFFF for v in r], dtype=np.uint64).reshape(-1, 1)
    r_hi = np.array([v >> 32 for v in r], dtype=np.uint64).reshape(-1, 1)
    j = np.arange((nd + 1) // 2, dtype=np.uint64).reshape(1, -1)
    w = philox4x32_10((r_lo, r_hi, np.uint64(step), j), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    return normals_of(np.stack(w, axis=-1), nd)
