"""NumPy restatement of libhj_hishapes.so (include/hj_hishapes.h, levelsetpy_amd/shapes.py): tests/shapes_ref.py, whose leaves
loop over g.dim and work at any dimension, with the one leaf more and an interpreter that knows it.

  * ball_of: the sphere in J linear images of the coordinates, as the header defines it -- every image all dim products, summed
    left to right from the first, the squares summed from the first image on;
  * run_program: an interpreter of a program compiled by levelsetpy_amd.shapes.compile_program_hi.

Every operation is one NumPy ufunc call on fp64 arrays: each is rounded on its own, as the kernel's.  Pinned to the reference
on a 5-D and a 6-D grid by tests/golden/hishapes.npz (tests/test_hishapes_ref.py).
"""
import numpy as np

from shapes_ref import (SPHERE, CYLINDER, RECT, HALFSPACE, ARRAY, UNION, INTERSECT, DIFFERENCE, COMPLEMENT, NEG, POS, ZERO,  # noqa: F401
                        coords, ball, rect, halfspace, flags, nested_scene)

SPHERE_OF = 10


def ball_of(xs, rows, center, radius):
    """rows: (J, dim); center: (J,)."""
    data = None
    for j in range(len(rows)):
        e = np.multiply(rows[j][0], xs[0])
        for i in range(1, len(xs)):
            q = np.multiply(rows[j][i], xs[i])
            e = np.add(e, q)
        e = np.subtract(e, center[j])
        q = np.multiply(e, e)
        data = q if data is None else np.add(data, q)
    return np.subtract(np.sqrt(data), radius)


def sphere_of(g, rows, center=None, radius=1):
    rows = np.asarray(rows, dtype=np.float64)
    center = np.zeros(len(rows)) if center is None else np.asarray(center, dtype=np.float64) * np.ones(len(rows))
    return ball_of(coords(g), rows, center, radius)


def run_program(g, comp, arrays=None):
    """A program compiled by compile_program_hi on grid g -> fp64 array (members,) + g.shape.  `arrays`: the array leaves as
    NumPy arrays in slot order (default: comp.arrays' own data through np.asarray), fp32 widened."""
    xs = coords(g)
    dim = len(xs)
    if arrays is None:
        arrays = [np.asarray(a) for a, _ in comp.arrays]
    out = []
    for k in range(comp.members):
        row = comp.params[k]
        stack = []
        for code, arg, off in comp.ops:
            if code in (SPHERE, CYLINDER):
                ignore = [d for d in range(dim) if (arg >> d) & 1] if code == CYLINDER else []
                stack.append(ball(xs, row[off:off + dim], row[off + dim], ignore))
            elif code == RECT:
                stack.append(rect(xs, row[off:off + dim], row[off + dim:off + 2 * dim]))
            elif code == HALFSPACE:
                stack.append(halfspace(xs, row[off:off + dim], row[off + dim:off + 2 * dim]))
            elif code == SPHERE_OF:
                J = arg
                stack.append(ball_of(xs, row[off:off + J * dim].reshape(J, dim), row[off + J * dim:off + J * dim + J], row[off + J * dim + J]))
            elif code == ARRAY:
                a = arrays[arg]
                stack.append(np.asarray(a[k] if comp.arrays[arg][1] else a, dtype=np.float64))
            elif code == COMPLEMENT:
                stack.append(-stack.pop())
            else:
                b = stack.pop()
                a = stack.pop()
                stack.append(np.minimum(a, b) if code == UNION else np.maximum(a, b) if code == INTERSECT else np.maximum(a, -b))
            assert len(stack) <= 8
        assert len(stack) == 1
        out.append(stack[0])
    return np.stack(out)


class PlainGrid(object):
    """dim, N, vs and shape from coordinate vectors alone: all the restatement and the compiler read of a grid."""

    def __init__(self, vs):
        self.vs = [np.asarray(v, dtype=np.float64).ravel() for v in vs]
        self.dim = len(self.vs)
        self.N = np.array([len(v) for v in self.vs], dtype=np.int64).reshape(-1, 1)
        self.shape = tuple(len(v) for v in self.vs)


def box(shape, seed=0):
    """A PlainGrid of the given shape around the origin, unevenly spaced limits per axis so that no two axes share coordinates."""
    return PlainGrid([np.linspace(-1.0 - 0.1 * d, 1.0 + 0.05 * d, n) if n > 1 else np.array([0.05 * (d + 1)]) for d, n in enumerate(shape)])
