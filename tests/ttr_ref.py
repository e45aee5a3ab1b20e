"""NumPy restatement of the time-to-reach recurrence (levelsetpy_amd/ttr.py, include/hj_ttr.h) -- a helper module, not
collected.  It restates the toolbox semantics that the docstring of the reference's postTimeStepTTR describes (its
update branch itself cannot run); tests/test_ttr_ref.py proves it on closed forms, tests/test_gpu_ttr.py holds the
kernels to it bit for bit.

    init(y, t, level)                                   -> ttr, last_y
    update(y, t, t_last, ttr, last_y, level, mode)      -> ttr, last_y      (new arrays)
    fold(data, tau, level, mode)                        the two above, slice by slice
    TD2TTR(data, tau, level, crossing, interpolate)     the same result from whole-stack array expressions

All arithmetic is fp64 (fp32 data widened first), one rounding per operation, in the order of the header.
"""
import numpy as np

FIRST, NO_INTERP = 1, 2


def mode_bits(crossing, interpolate):
    assert crossing in ('first', 'last')
    return (FIRST if crossing == 'first' else 0) | (0 if interpolate else NO_INTERP)


def init(y, t, level=0.0):
    y = np.asarray(y)
    return np.where(y.astype(np.float64) <= level, np.float64(t), np.inf), y.copy()


def update(y, t, t_last, ttr, last_y, level=0.0, mode=0):
    y = np.asarray(y)
    yd, ld = y.astype(np.float64), np.asarray(last_y).astype(np.float64)
    t, t_last = np.float64(t), np.float64(t_last)
    with np.errstate(all='ignore'):
        a = ld - level
        b = yd - level
        changed = (yd <= level) & (ld > level)
        if mode & FIRST:
            changed = changed & (ttr == np.inf)
        if mode & NO_INTERP:
            tc = np.full(yd.shape, t)
        else:
            tc = t_last - ((t - t_last) * a) / (b - a)
    return np.where(changed, tc, ttr), y.copy()


def fold(data, tau, level=0.0, mode=0):
    tau = np.asarray(tau, dtype=np.float64)
    ttr, last = init(data[0], tau[0], level)
    for k in range(1, len(tau)):
        ttr, last = update(data[k], tau[k], tau[k - 1], ttr, last, level, mode)
    return ttr


def TD2TTR(data, tau, level=0.0, crossing='first', interpolate=False):
    """The fold, from array expressions over the whole stack: the crossing that counts is picked by argmax."""
    d = np.asarray(data).astype(np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    assert d.shape[0] == tau.size and np.all(np.diff(tau) >= 0)
    start = np.where(d[0] <= level, tau[0], np.inf)
    if tau.size == 1:
        return start
    col = (-1,) + (1,) * (d.ndim - 1)
    cross = (d[1:] <= level) & (d[:-1] > level)
    with np.errstate(all='ignore'):
        a = d[:-1] - level
        b = d[1:] - level
        if interpolate:
            tc = tau[:-1].reshape(col) - ((tau[1:] - tau[:-1]).reshape(col) * a) / (b - a)
        else:
            tc = np.broadcast_to(tau[1:].reshape(col), cross.shape)
    some = cross.any(axis=0)
    if crossing == 'first':
        k = np.argmax(cross, axis=0)
        some = some & (start == np.inf)         # a node inside at tau[0] keeps tau[0]
    else:
        k = cross.shape[0] - 1 - np.argmax(cross[::-1], axis=0)
    pick = np.take_along_axis(tc, k[None], axis=0)[0]
    return np.where(some, pick, start)


# ---------------------------------------------------------------------------------------------- the closed-form cases
def disc_psi():
    """psi = hypot(x, y) - 0.25 on the 33 x 29 grid of the tests."""
    x, y = np.meshgrid(np.linspace(-1.3, 1.1, 33), np.linspace(-0.9, 1.2, 29), indexing='ij')
    return np.hypot(x, y) - 0.25


def expanding_disc(T):
    """phi_k = psi - 0.8 tau_k, tau = linspace(0, 1, T): linear in t, the interpolated TTR is psi / 0.8."""
    tau = np.linspace(0.0, 1.0, T)
    psi = disc_psi()
    return np.stack([psi - 0.8 * t for t in tau]), tau, psi


def oscillating_set():
    """phi_k = psi - 0.5 sin(2 pi tau_k), tau = linspace(0, 2, 17): the set grows and shrinks twice."""
    tau = np.linspace(0.0, 2.0, 17)
    psi = disc_psi()
    return np.stack([psi - 0.5 * np.sin(2 * np.pi * t) for t in tau]), tau, psi


def sprinkle(data, level=0.0, seed=0, inf_transitions=True):
    """A copy of the stack with special nodes: NaN and +inf held for the whole time, NaN / +inf / -inf in single slices, a
    node held exactly at the level, nodes at the level in single slices.  Returns (stack, index of the node held at the level).
    inf_transitions=False leaves the single-slice +inf out: a node that comes from +inf interpolates to inf / inf = NaN, which is
    what the formula says and what the bit-for-bit comparisons cover, but not what the no-NaN property is about."""
    d = np.array(data, dtype=np.float64)
    T = d.shape[0]
    flat = d.reshape(T, -1)
    n = flat.shape[1]
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)[:min(n, 24)]
    groups = np.array_split(idx, 8) if n >= 8 else [idx[:1]] + [idx[:0]] * 7
    held_level = groups[0]
    flat[:, groups[0]] = level
    flat[:, groups[1]] = np.nan
    flat[:, groups[2]] = np.inf
    for grp, val in ((groups[3], np.nan), (groups[4], np.inf if inf_transitions else -np.inf), (groups[5], -np.inf), (groups[6], level)):
        for j in grp:
            flat[rng.integers(0, T), j] = val
    return flat.reshape(d.shape), held_level
