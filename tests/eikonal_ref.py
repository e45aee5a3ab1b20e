"""NumPy restatement of include/hj_eikonal.h, rules 1-3, for the tests of signedDistance (test infrastructure).

Synchronous passes over the whole grid (every node is updated from the values of the previous pass) until a pass changes
nothing.  The arithmetic is the header's, operation by operation: every product, sum, quotient and square root is a NumPy
operation of its own in fp64, in the header's order.  `schedule` swaps the synchronous pass for one that updates a random
half of the nodes; the fixed point must not depend on it.
"""
import numpy as np

INF = np.inf


def shift(a, d, side, periodic, fill):
    """The neighbour's value along axis d: side 0 the lower neighbour (index - 1), side 1 the upper; `fill` outside a
    non-periodic axis."""
    r = np.roll(a, 1 if side == 0 else -1, axis=d)
    if not periodic:
        edge = [slice(None)] * a.ndim
        edge[d] = 0 if side == 0 else -1
        r[tuple(edge)] = fill
    return r


def speed_array(shape, speed):
    if speed is None:
        return np.ones(shape)
    return np.broadcast_to(np.asarray(speed, dtype=np.float64), shape).copy()


def init(data, level, dx, periodic, speed=None):
    """Rule 1 -> (u: frozen values at near nodes, +inf elsewhere, NaN at walls; near; wall; s = 1 / speed; phi)."""
    phi = np.asarray(data).astype(np.float64) - float(level)
    sp = speed_array(phi.shape, speed)
    wall = np.isnan(phi) | ~(sp > 0.0)
    pos = phi > 0.0
    S = np.zeros(phi.shape)
    crossing = np.zeros(phi.shape, dtype=bool)
    with np.errstate(all='ignore'):
        for d in range(phi.ndim):
            td = np.full(phi.shape, INF)
            for side in (0, 1):
                pj = shift(phi, d, side, periodic[d], np.nan)
                wj = shift(wall, d, side, periodic[d], True)
                cross = ~wall & ~wj & (pos != (pj > 0.0))
                num = dx[d] * np.abs(phi)
                den = np.abs(phi - pj)
                t = num / den
                t = np.where(np.isinf(phi) | np.isinf(pj), dx[d] / 2.0, t)
                td = np.where(cross & (t < td), t, td)
            has = td < INF
            q = td * td
            r = 1.0 / q
            S = np.where(has, np.where(crossing, S + r, r), S)
            crossing = crossing | has
        s = 1.0 / sp
        u = s / np.sqrt(S)
    u[phi == 0.0] = 0.0
    near = ~wall & ((phi == 0.0) | crossing)
    u = np.where(wall, np.nan, np.where(near, u, INF))
    return u, near, wall, s, phi


def candidates(u, dx, periodic, s, band=INF):
    """Rule 2's new value at EVERY node from the neighbours in u (walls NaN); the caller keeps it where a node is live."""
    D = u.ndim
    v = np.where(np.isnan(u), INF, u)
    a = np.stack([np.minimum(shift(v, d, 0, periodic[d], INF), shift(v, d, 1, periodic[d], INF)) for d in range(D)])
    h = np.stack([np.full(u.shape, float(dx[d])) for d in range(D)])
    order = np.argsort(a, axis=0, kind='stable')
    a = np.take_along_axis(a, order, axis=0)
    h = np.take_along_axis(h, order, axis=0)
    hh = h * h
    w = 1.0 / hh
    with np.errstate(all='ignore'):
        step = h[0] * s
        cand = a[0] + step
        done = np.ones(u.shape, dtype=bool) if D == 1 else cand <= a[1]
        A, B, Q = w[0].copy(), np.zeros(u.shape), np.zeros(u.shape)
        ss = s * s
        for k in range(1, D):
            b = a[k] - a[0]
            p = w[k] * b
            A = A + w[k]
            B = B + p
            pb = p * b
            Q = Q + pb
            C = Q - ss
            BB = B * B
            AC = A * C
            disc = BB - AC
            root = np.sqrt(disc)
            num = B + root
            quot = num / A
            c = a[0] + quot
            cand = np.where(done, cand, c)
            done = done | (np.ones(u.shape, dtype=bool) if k == D - 1 else c <= a[k + 1])
        take = (a[0] < INF) & (cand <= band) & (cand < v)
    return np.where(take, cand, v)


def sweep(u, near, wall, dx, periodic, s, band=INF, mask=None):
    live = ~near & ~wall
    if mask is not None:
        live = live & mask
    new = candidates(u, dx, periodic, s, band)
    return np.where(live, new, u)


def fixed_point(u, near, wall, dx, periodic, s, band=INF, schedule=None, limit=100000):
    """-> (u at the fixed point, passes up to and including the first that changed nothing).  schedule: None for
    synchronous passes, or a numpy Generator: every pass updates a random half of the nodes, and the end is a synchronous
    pass that changes nothing."""
    for n in range(1, limit + 1):
        if schedule is None:
            new = sweep(u, near, wall, dx, periodic, s, band)
            if np.array_equal(new, u, equal_nan=True):
                return u, n
        else:
            new = sweep(u, near, wall, dx, periodic, s, band, schedule.random(u.shape) < 0.5)
            if np.array_equal(new, u, equal_nan=True) and np.array_equal(sweep(u, near, wall, dx, periodic, s, band), u, equal_nan=True):
                return u, n
        u = new
    raise RuntimeError("no fixed point after %d passes" % limit)


def finish(u, phi, wall, band=INF, dtype=np.float64):
    """Rule 3."""
    v = np.minimum(u, band)
    out = np.where(phi > 0.0, v, np.where(phi < 0.0, -v, 0.0))
    out = np.where(wall, np.nan, out)
    return out.astype(dtype)


def signed_distance(data, dx, periodic=None, level=0.0, band=INF, speed=None, dtype=None, schedule=None, return_passes=False):
    """The restatement of signedDistance for one member: data of the grid's shape -> array of `dtype` (default: the data's
    when it is fp32, else fp64)."""
    data = np.asarray(data)
    periodic = [False] * data.ndim if periodic is None else list(periodic)
    dx = [float(v) for v in np.asarray(dx).ravel()]
    if dtype is None:
        dtype = np.float32 if data.dtype == np.float32 else np.float64
    u, near, wall, s, phi = init(data, level, dx, periodic, speed)
    u, passes = fixed_point(u, near, wall, dx, periodic, s, band, schedule)
    out = finish(u, phi, wall, band, dtype)
    return (out, passes) if return_passes else out
