"""NumPy restatement of libhj_shapes.so (include/hj_shapes.h, levelsetpy_amd/shapes.py).

Two things, both over np.meshgrid(*g.vs):

  * the shape functions, written as the reference writes those of its functions that run (InitialConditions/
    rect_corners.py, rect_center.py, shape_ops.py, sphere.py, cylinder.py) and, for the two hyperplane shapes that do not run
    there, as the header defines them;
  * run_program: an interpreter of a COMPILED program (levelsetpy_amd.shapes.compile_program), so that the compiler is under
    test too: a tree evaluated directly must equal its program run here.

Every operation is one NumPy ufunc call on fp64 arrays: each is rounded on its own, as the kernel's.  Pinned to the
reference by tests/golden/shapes.npz (tests/test_shapes_ref.py).
"""
import numpy as np

SPHERE, CYLINDER, RECT, HALFSPACE, ARRAY, UNION, INTERSECT, DIFFERENCE, COMPLEMENT = range(1, 10)
NEG, POS, ZERO = 1, 2, 4


def coords(g):
    """Dense coordinates from the grid's coordinate vectors (plain coordinates on periodic axes too)."""
    return np.meshgrid(*[np.asarray(v, dtype=np.float64).ravel() for v in g.vs], indexing='ij')


def _vec(v, dim, default):
    if v is None or not np.any(v):
        return default * np.ones(dim)
    v = np.asarray(v, dtype=np.float64)
    return v.item() * np.ones(dim) if v.size == 1 else v.ravel()


# ------------------------------------------------------------------------------------------ leaves on dense coordinates
def ball(xs, center, radius, ignore=()):
    data = np.zeros(xs[0].shape)
    for i in range(len(xs)):
        if i not in ignore:
            e = xs[i] - center[i]
            data = data + e * e
    return np.sqrt(data) - radius


def rect(xs, lower, upper):
    data = np.maximum(xs[0] - upper[0], lower[0] - xs[0])
    for i in range(1, len(xs)):
        data = np.maximum(data, xs[i] - upper[i])
        data = np.maximum(data, lower[i] - xs[i])
    return data


def halfspace(xs, normal, point):
    data = normal[0] * (xs[0] - point[0])
    for i in range(1, len(xs)):
        data = data + normal[i] * (xs[i] - point[i])
    return data


# ------------------------------------------------------------------------------------------ the package's functions
def sphere(g, center=None, radius=1):
    return ball(coords(g), _vec(center, g.dim, 0.0), radius)


def cylinder(g, axis_align, center=None, radius=1):
    ignore = list(axis_align) if isinstance(axis_align, (list, tuple)) else [axis_align]
    return ball(coords(g), _vec(center, g.dim, 0.0), radius, ignore)


def rectangle_by_corners(g, lower=None, upper=None):
    return rect(coords(g), _vec(lower, g.dim, 0.0), _vec(upper, g.dim, 1.0))


def rectangle_by_center(g, center=None, widths=None):
    c, w = _vec(center, g.dim, 0.0), _vec(widths, g.dim, 1.0)
    return rect(coords(g), c - 0.5 * w, c + 0.5 * w)


def hyperplane(g, normal, point=None):
    n = np.asarray(normal, dtype=np.float64).ravel()
    return halfspace(coords(g), n / np.linalg.norm(n), _vec(point, g.dim, 0.0))


def hyperplane_normal(points, positivePoint):
    """Unit normal of the hyperplane through the rows of `points`, pointing to the side of positivePoint."""
    pts = np.asarray(points, dtype=np.float64)
    dim = pts.shape[0]
    n = np.ones(1) if dim == 1 else np.linalg.svd(pts[1:] - pts[0])[2][-1]
    n = n / np.linalg.norm(n)
    return -n if np.dot(n, np.asarray(positivePoint, dtype=np.float64).ravel() - pts[0]) < 0 else n


def hyperplane_by_points(g, points, positivePoint):
    return halfspace(coords(g), hyperplane_normal(points, positivePoint), np.asarray(points, dtype=np.float64)[0])


def union(*shapes):
    return np.minimum.reduce(shapes)


def intersection(*shapes):
    return np.maximum.reduce(shapes)


def difference(a, b):
    return np.maximum(a, -b)


def complement(a):
    return -a


# ------------------------------------------------------------------------------------------ the interpreter
def run_program(g, comp, arrays=None):
    """A compiled program on grid g -> fp64 array (members,) + g.shape.  `arrays`: the array leaves as NumPy arrays in slot
    order (default: comp.arrays' own data through np.asarray), fp32 widened."""
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


# ------------------------------------------------------------------------------------------ a scene at the limits
def nested_scene(S, dim, K=None):
    """8 leaves at depth 8 from the node constructors of module S (levelsetpy_amd.shapes): a right-nested tree with every
    leaf kind that has parameters and every operator in it; K: every parameter batched over K members.
    -> (node, leaves, operators from the innermost outwards)."""
    rng = np.random.default_rng(11 * dim)
    c = lambda: rng.uniform(-0.4, 0.4, (K, dim) if K else dim)                   # noqa: E731
    r = lambda: rng.uniform(0.3, 0.7, K) if K else float(rng.uniform(0.3, 0.7))    # noqa: E731
    leaves = [S.sphere(c(), r()), S.cylinder([dim - 1], c(), r()), S.rectangle_by_corners(c() - 0.5, c() + 0.5),
              S.rectangle_by_center(c(), 0.8), S.hyperplane(np.ones(dim), c()), S.sphere(c(), r()),
              S.cylinder([0], c(), r()), S.rectangle_by_corners(-np.inf, c() + 0.6)]
    ops = [S.union, S.intersection, S.difference, S.union, S.intersection, S.difference, S.union]
    node = leaves[-1]
    for leaf, op in zip(leaves[-2::-1], ops):
        node = op(leaf, -node if op is S.union else node)
    return node, leaves, ops


def flags(data):
    """The sign flags of one member's stored values."""
    data = np.asarray(data)
    return (NEG if np.any(data < 0) else 0) | (POS if np.any(data > 0) else 0) | (ZERO if np.any((data == 0) | np.isnan(data)) else 0)
