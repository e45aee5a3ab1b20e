"""NumPy / Python-integer restatement of include/hj_measure.h (levelsetpy_amd/measure.py): the volume of { phi <= level } for the
piecewise-linear interpolant on the Kuhn subdivision, as exact integer sums of per-simplex fractions q (2^52 the whole simplex).
UNPINNED -- the reference has no such function; tests/test_measure_ref.py proves this restatement on closed forms (half-spaces in a
box, balls, integer identities, the enclosed volume of the extracted mesh), tests/test_measure_host.py holds the library's host run
of the per-simplex function to it, and tests/test_gpu_measure.py the kernels, every integer with ==.

Definition.  Cells: N[d] - 1 per axis, N[d] on a periodic axis (the last one wraps to node 0).  f = float64(data) - level.  Corner b
of a cell: bit d selects the upper node of axis d.  Simplex s: the s-th permutation p of (0..D-1) in lexicographic order, vertices
v0 = 0, v_k = v_{k-1} | 1 << p[k-1].  A cell with a non-finite corner is invalid, without a positive corner full, without a negative
one empty, otherwise cut.  The arithmetic of simplex_q is Python's float: IEEE fp64, one rounding per operation.
"""
import itertools
import math

import numpy as np

Q_ONE = 1 << 52
SETS = ("A", "B", "union", "intersection")


def chains(D):
    """The corner numbers v0..vD of every simplex, in lexicographic order of the permutation."""
    out = []
    for p in itertools.permutations(range(D)):
        c = [0]
        for a in p:
            c.append(c[-1] | (1 << a))
        out.append(c)
    return out


def simplex_q(f):
    """q of the simplex with vertex values f (path order)."""
    f = [float(v) for v in f]
    a = [v for v in f if v < 0.0]
    b = [v for v in f if v > 0.0]
    k, m = len(a), len(b)
    if m == 0:
        return Q_ONE
    if k == 0:
        return 0
    F = [[0.0] * (m + 1) for _ in range(k + 1)]
    for i in range(k):
        F[i][m] = 1.0
    for i in range(k - 1, -1, -1):
        for j in range(m - 1, -1, -1):
            theta = (-a[i]) / (b[j] - a[i])
            F[i][j] = (theta * F[i][j + 1]) + ((1.0 - theta) * F[i + 1][j])
    return min(Q_ONE, int(round(F[0][0] * 4503599627370496.0)))        # round(): half to even, as rint


def cell_count(N, periodic=()):
    n = 1
    for d, v in enumerate(N):
        n *= int(v) - (0 if d in periodic else 1)
    return n


def cell_volume(dx):
    """The left-to-right fp64 product of dx."""
    v = float(dx[0])
    for s in dx[1:]:
        v = v * float(s)
    return v


def corner_values(f, periodic=()):
    """[2^D arrays over the cells]: f at corner b of every cell."""
    N = f.shape
    D = len(N)
    cells = tuple(slice(0, n if d in periodic else n - 1) for d, n in enumerate(N))
    out = []
    for b in range(1 << D):
        g = f
        for d in range(D):
            if (b >> d) & 1:
                g = np.roll(g, -1, axis=d)
        out.append(g[cells])
    return out


def record_of_f(f, periodic=()):
    """The record of one field from its f = data - level (fp64, the grid's shape)."""
    N = f.shape
    D = len(N)
    periodic = tuple(periodic)
    cv = corner_values(f, periodic)
    stack = np.stack([c.reshape(-1) for c in cv])                  # (2^D, cells)
    bad = ~np.isfinite(stack).all(axis=0)
    with np.errstate(invalid="ignore"):
        pos = (stack > 0).any(axis=0)
        neg = (stack < 0).any(axis=0)
        inside = f <= 0
    full = ~bad & ~pos
    cut = ~bad & pos & neg
    ch = chains(D)
    q = 0
    for c in np.flatnonzero(cut):
        vals = stack[:, c]
        for chain in ch:
            q += simplex_q([vals[v] for v in chain])
    lo, hi = [], []
    for d in range(D):
        along = np.flatnonzero(inside.any(axis=tuple(e for e in range(D) if e != d)))
        lo.append(int(along[0]) if len(along) else int(N[d]))
        hi.append(int(along[-1]) if len(along) else -1)
    return dict(cells=cell_count(N, periodic), full=int(full.sum()), cut=int(cut.sum()), invalid=int(bad.sum()), Q_cut=q,
                Q=int(full.sum()) * math.factorial(D) * Q_ONE + q, inside=int(inside.sum()), nan=int(np.isnan(f).sum()), lo=lo, hi=hi)


def widen(data):
    return np.asarray(data).astype(np.float64)


def measure_ref(data, level=0.0, periodic=()):
    """The record of one field `data` (fp64 or fp32, the grid's shape)."""
    return record_of_f(widen(data) - float(level), periodic)


def compare_ref(a, b, level=0.0, periodic=()):
    """{set: record} of the fields a and b: np.minimum / np.maximum of the widened values, then the level."""
    a, b = widen(a), widen(b)
    level = float(level)
    with np.errstate(invalid="ignore"):
        return {"A": record_of_f(a - level, periodic), "B": record_of_f(b - level, periodic),
                "union": record_of_f(np.minimum(a, b) - level, periodic), "intersection": record_of_f(np.maximum(a, b) - level, periodic)}


def volume_of(Q, D, cellvol):
    """(Q / (D! 2^52)) cellvol: a Python integer true division, then one multiplication."""
    return (Q / (math.factorial(D) * Q_ONE)) * cellvol


def compare_values(recs, D, cellvol):
    """(volA, volB, union, intersection, symdiff, iou) of compare_ref's records."""
    QU, QI = recs["union"]["Q"], recs["intersection"]["Q"]
    vol = [volume_of(recs[s]["Q"], D, cellvol) for s in SETS]
    return tuple(vol) + (volume_of(max(0, QU - QI), D, cellvol), QI / QU if QU else float("nan"))


# ------------------------------------------------------------------------------------------ bounds and truncation
def bounds_ref(N, vs, dx, periodic, lo, hi, pad=1):
    """setBounds from a record's lo / hi: padded, clipped, periodic axes whole; None for an empty set."""
    if any(h < 0 for h in hi):
        return None
    D = len(N)
    lo2 = [0 if d in periodic else max(0, lo[d] - pad) for d in range(D)]
    hi2 = [N[d] - 1 if d in periodic else min(N[d] - 1, hi[d] + pad) for d in range(D)]
    xmin = np.array([vs[d][lo2[d]] - dx[d] / 2 for d in range(D)])
    xmax = np.array([vs[d][hi2[d]] + dx[d] / 2 for d in range(D)])
    return lo2, hi2, xmin, xmax


def truncate_ref(vs, data, xmin, xmax, lead=0):
    """(kept node indices per axis, the data cut to them): strict inequalities, as Grids/truncate.py.  lead: time axes in front."""
    keep = [np.flatnonzero((np.asarray(v).ravel() > xmin[d]) & (np.asarray(v).ravel() < xmax[d])) for d, v in enumerate(vs)]
    out = None
    if data is not None:
        out = np.asarray(data)
        for d, k in enumerate(keep):
            out = np.take(out, k, axis=lead + d)
    return keep, out


# ------------------------------------------------------------------------------------------ closed forms
def halfspace_volume(a, c, lo, hi):
    """vol { x in the box [lo, hi] : a . x <= c } by inclusion-exclusion over the box's corners (all a[d] != 0):
    (1 / (D! prod a)) sum over corners v of (-1)^(number of upper coordinates of v) max(0, c - a . v)^D, for a > 0 after reflecting."""
    a, lo, hi = [float(v) for v in a], [float(v) for v in lo], [float(v) for v in hi]
    D = len(a)
    # reflect the axes with a negative coefficient: x -> lo + hi - x
    c = float(c)
    for d in range(D):
        if a[d] < 0:
            c -= a[d] * (lo[d] + hi[d])
            a[d] = -a[d]
    total = 0.0
    for bits in range(1 << D):
        v = [hi[d] if (bits >> d) & 1 else lo[d] for d in range(D)]
        r = c - sum(a[d] * v[d] for d in range(D))
        if r > 0:
            total += (-1) ** bin(bits).count("1") * r ** D
    return total / (math.factorial(D) * math.prod(a))


def ball_volume(D, r):
    return math.pi ** (D / 2) / math.gamma(D / 2 + 1) * r ** D


# ------------------------------------------------------------------------------------------ the GPU test's cases
GRIDS = [((37,), ()), ((19, 17), (1,)), ((9, 8, 7), (2,)), ((6, 5, 4, 5), ()), ((5, 3, 4, 3, 3), (2,)), ((5, 3, 3, 2, 3, 3), (5,)),
         ((2,) * 6, ())]
SEED = 20261020


def grid_vectors(N, periodic=()):
    """Coordinate vectors on [-1, 1]^D as createGrid makes them (np.linspace), a periodic axis shrunk by its last node; and dx."""
    vs, dx, mins, maxs = [], [], [], []
    for d, n in enumerate(N):
        hi = 1.0 - 2.0 / n if d in periodic else 1.0
        vs.append(np.linspace(-1.0, hi, n))
        dx.append((hi - (-1.0)) / (n - 1))
        mins.append(-1.0)
        maxs.append(hi)
    return vs, dx, mins, maxs


def field(N, periodic=(), seed=SEED, stack=None):
    """x0 + 0.15 sum x_d - 0.07 + 0.02 noise on the grid's nodes; stack: that many fields with noise of their own, shifted apart."""
    vs, _, _, _ = grid_vectors(N, periodic)
    X = np.meshgrid(*vs, indexing="ij")
    base = X[0] + 0.15 * sum(X) - 0.07
    rng = np.random.default_rng(seed)
    if stack is None:
        return base + 0.02 * rng.standard_normal(base.shape)
    return np.stack([base + 0.11 * k + 0.02 * rng.standard_normal(base.shape) for k in range(stack)])


def field_b(N, periodic=(), seed=77):
    """A second set that overlaps field()'s only partly: the plane tilted against the last axis, x0 - 0.4 x_last + 0.15 sum x_d - 0.02."""
    vs, _, _, _ = grid_vectors(N, periodic)
    X = np.meshgrid(*vs, indexing="ij")
    return X[0] - 0.4 * X[-1] + 0.15 * sum(X) - 0.02 + 0.02 * np.random.default_rng(seed).standard_normal(X[0].shape)
