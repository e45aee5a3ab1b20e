"""Shapes on the device: targets, obstacles and their set algebra, built where the solve reads them.

A shape is a tree of nodes -- sphere, cylinder, rectangle_by_corners, rectangle_by_center, hyperplane,
hyperplane_by_points and array leaves under union, intersection, difference and complement (`|`, `&`, `-`, unary `-`).
evaluate_shape(g, node) compiles the tree into a postfix program and runs it in libhj_shapes.so (include/hj_shapes.h):
`scene_kernel` evaluates the whole tree per node in one pass and stores the result once, reading only the grid's
coordinate vectors g.vs -- no dense g.xs (a low_mem grid has none), no intermediate arrays, no host pass and no copy.

Batches.  Any numeric parameter may carry a leading axis K -- a centre of shape (K, dim), a radius of shape (K,) -- and an
array leaf may be a stack (K,) + g.shape.  (The reference's "not any -> default" rule holds for batched vectors too: an
all-zero (K, dim) array means the default for each of its K members.)  All of them must agree on K; the result is then the stack (K,) + g.shape of K
members from ONE launch: a sweep over capture radii for HJIPDE_solve_batch, an obstacle that moves along tau for
HJIPDE_solve.

Arithmetic (the header has the definitions): fp64 throughout, every operation rounded on its own and in the reference's
order, min / max as np.minimum / np.maximum (a NaN on either side gives NaN), plain coordinates on periodic axes; an
fp32 result is the fp64 one rounded once.  What is prepared on the host, in NumPy: the corners of rectangle_by_center
(center -+ 0.5 widths), the unit normal of hyperplane (np.linalg.norm), the normal of hyperplane_by_points.

The only thing that crosses back to the host is one int32 of sign flags per member, which drives the reference's "single
sign on grid" warning; last_info() returns them with the program and the kernel's name.

Grids of 5 and 6 dimensions, and the leaf sphere_of (a sphere in J linear images of the coordinates; sphere_between builds
the capture set of two vehicles from it), run in libhj_hishapes.so (include/hj_hishapes.h): `hi_scene_kernel`, the same
interpreter and the same leaves over an index decode that divides by nothing.  evaluate_shape takes that library when
g.dim > 4 or the tree holds a sphere_of, and scene_kernel otherwise, exactly as before.  series(g, node) is a time-varying
target or obstacle WITHOUT its stack: a ShapeSeries evaluates member i alone when it is indexed, which is how
HJIPDE_solve on a 5-D / 6-D grid reads it, one member per interval.

Parity.  PINNED to the reference (tests/golden/shapes.npz): shapeRectangleByCorners, shapeRectangleByCenter, shapeUnion of
three shapes, shapeIntersection, shapeDifference, shapeComplement.  HELD to the NumPy restatement tests/shapes_ref.py:
both hyperplane shapes (the reference's hyperplane.py and hyper_pts.py do not run), shapeUnion of two shapes (the
reference raises IndexError), batching, array leaves and fp32.
"""
import numpy as np

from . import _ffi, _gffi, _hffi, _kffi
from .context import is_tensor, require_gpu
from .utilities import error, warn, eps
from ._marshal import (unlazy as _unlazy, wants_tensor as _wants_tensor, device_data as _device_data, stream as _stream,
                       ptr as _ptr, descriptor as _descriptor)
from . import _qffi

__all__ = ["sphere", "cylinder", "rectangle_by_corners", "rectangle_by_center", "hyperplane", "hyperplane_by_points",
           "array", "union", "intersection", "difference", "complement", "compile_program", "evaluate_shape", "last_info",
           "sphere_of", "sphere_between", "compile_program_hi", "series", "ShapeSeries",
           "shapeRectangleByCorners", "shapeRectangleByCenter", "shapeHyperplane", "shapeHyperplaneByPoints",
           "shapeUnion", "shapeIntersection", "shapeDifference", "shapeComplement"]

MAX_OPS, MAX_DEPTH, MAX_ARRAYS = _gffi.MAX_OPS, _gffi.MAX_DEPTH, _gffi.MAX_ARRAYS
HINT = "evaluate a subtree first (evaluate_shape) and pass the result as an array leaf"
SINGLE_SIGN = 'Implicit surface not visible because function has single sign on grid'


# ------------------------------------------------------------------------------------------ nodes
class Node(object):
    """A shape: a leaf or an operator over shapes.  Immutable; evaluate_shape(g, node) gives its values on a grid."""

    def __or__(self, other):
        return union(self, other)

    def __and__(self, other):
        return intersection(self, other)

    def __sub__(self, other):
        return difference(self, other)

    def __neg__(self):
        return complement(self)


class Leaf(Node):
    def __init__(self, code, vectors=(), scalars=(), axes=None, data=None):
        self.code, self.vectors, self.scalars, self.axes, self.data = code, tuple(vectors), tuple(scalars), axes, data


class Operator(Node):
    def __init__(self, code, children):
        for c in children:
            if not isinstance(c, Node):
                error('the operands of a shape operator are shapes (got %s): wrap a grid array in array(...)' % type(c).__name__)
        self.code, self.children = code, tuple(children)


def sphere(center=None, radius=1):
    """sqrt(sum_i (x_i - c_i)^2) - r.  center: a vector, a scalar (times ones) or None / all zero (the origin)."""
    return Leaf(_gffi.SPHERE, [(center, 0.0)], [radius])


def cylinder(axis_align, center=None, radius=1):
    """The sphere's formula over the axes NOT in axis_align (an axis or a list of axes the cylinder runs along)."""
    axes = list(axis_align) if isinstance(axis_align, (list, tuple, np.ndarray)) else [axis_align]
    return Leaf(_gffi.CYLINDER, [(center, 0.0)], [radius], axes=[int(a) for a in axes])


class _Rows(object):
    """The (J, dim) coefficient rows of sphere_of, or (K, J, dim) for K members."""

    def __init__(self, rows):
        self.rows = rows


def sphere_of(rows, center=None, radius=1):
    """A sphere in J linear images of the coordinates: sqrt(sum_j (rows[j] . x - center[j])^2) - radius, 1 <= J <= 6.
    rows: (J, dim), or (K, J, dim) for K members; center: (J,), a scalar (times ones) or None (zeros), or (K, J); radius: a scalar
    or (K,).  Every image takes all dim products, left to right, zero coefficients included (include/hj_hishapes.h)."""
    if rows is None:
        error('sphere_of needs its rows')
    return Leaf(_kffi.SPHERE_OF, [(_Rows(rows), None), (center, 0.0)], [radius])


def sphere_between(axes_a, axes_b, radius=1, offset=None):
    """The sphere in the differences x[axes_a[j]] - x[axes_b[j]]: sphere_between((0, 1), (3, 4), r) is the capture set
    sqrt((x0 - x3)^2 + (x1 - x4)^2) - r of two vehicles.  offset: the centre of the differences (default zeros).  The rows end
    at the last axis named; the compiler gives them zero coefficients for the grid's further axes."""
    a = [int(v) for v in (axes_a if isinstance(axes_a, (list, tuple, np.ndarray)) else [axes_a])]
    b = [int(v) for v in (axes_b if isinstance(axes_b, (list, tuple, np.ndarray)) else [axes_b])]
    if len(a) != len(b) or not a:
        error('sphere_between pairs axes: axes_a and axes_b have the same length, at least 1 (got %d and %d)' % (len(a), len(b)))
    if min(a + b) < 0:
        error('sphere_between: axes are counted from 0')
    if any(i == j for i, j in zip(a, b)):
        error('sphere_between: the difference of an axis with itself is zero')
    rows = np.zeros((len(a), max(a + b) + 1))
    for j, (i, k) in enumerate(zip(a, b)):
        rows[j, i], rows[j, k] = 1.0, -1.0
    leaf = sphere_of(rows, offset, radius)
    leaf.pad = True                             # rows shorter than the grid's dimension get zero coefficients for the further axes
    return leaf


def rectangle_by_corners(lower=None, upper=None):
    """max_i max(x_i - upper_i, lower_i - x_i).  Defaults 0 and 1; components may be +-inf (slabs, intervals)."""
    return Leaf(_gffi.RECT, [(lower, 0.0), (upper, 1.0)])


class _Halves(object):
    """center -+ 0.5 widths, formed once the grid's dimension is known."""

    def __init__(self, center, widths, sign):
        self.center, self.widths, self.sign = center, widths, sign


def rectangle_by_center(center=None, widths=None):
    """The rectangle with corners center -+ 0.5 widths (formed on the host).  Defaults 0 and 1."""
    return Leaf(_gffi.RECT, [(_Halves(center, widths, -1.0), None), (_Halves(center, widths, 1.0), None)])


class _Unit(object):
    """normal / np.linalg.norm(normal), per member."""

    def __init__(self, normal):
        self.normal = normal


def hyperplane(normal, point=None):
    """n^T (x - point) with n = normal / |normal| (normalised on the host).  point defaults to the origin."""
    if normal is None:
        error('hyperplane needs a normal')
    return Leaf(_gffi.HALFSPACE, [(_Unit(normal), None), (point, 0.0)])


def hyperplane_by_points(points, positivePoint):
    """The hyperplane through the dim rows of the square matrix `points`, positive on the side of positivePoint.  The normal
    is the null vector of the differences points[1:] - points[0]; it must be unique (the points affinely independent).
    A null vector has no sign of its own, so positivePoint is required and must not lie on the hyperplane."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[0] != pts.shape[1]:
        error('points must be a square matrix, one point per row (got shape %s)' % (pts.shape,))
    if positivePoint is None:
        error('positivePoint is required: the null vector of the point differences has no sign of its own')
    dim = pts.shape[0]
    pos = np.asarray(positivePoint, dtype=np.float64).ravel()
    if pos.size != dim:
        error('positivePoint must have %d components (got %d)' % (dim, pos.size))
    if not (np.all(np.isfinite(pts)) and np.all(np.isfinite(pos))):
        error('points and positivePoint must be finite')
    if dim == 1:
        normal = np.ones(1)
    else:
        A = pts[1:] - pts[0]
        _, s, vt = np.linalg.svd(A)
        if s[-1] <= dim * eps * max(s[0], np.finfo(np.float64).tiny):
            error('the points do not define a unique hyperplane (they are affinely dependent)')
        normal = vt[-1]
    normal = normal / np.linalg.norm(normal)
    side = float(np.dot(normal, pos - pts[0]))
    if abs(side) < 1e3 * eps:
        error('positivePoint lies on the hyperplane')
    if side < 0:
        normal = -normal
    return Leaf(_gffi.HALFSPACE, [(normal, None), (pts[0].copy(), None)])


def array(data):
    """An existing grid array as a leaf: g.shape, or a stack (K,) + g.shape with one slice per member.  fp32 and fp64
    arrays are read as they are (fp32 widened); NumPy arrays, tensors and HostViews all do."""
    if isinstance(data, Node):
        return data
    return Leaf(_gffi.ARRAY, data=data)


def _operands(nodes):
    if len(nodes) == 1 and isinstance(nodes[0], (list, tuple)):
        nodes = tuple(nodes[0])
    if not nodes:
        error('an operator needs at least one shape')
    return nodes


def union(*nodes):
    """Pointwise minimum, folded left to right as np.minimum.reduce."""
    nodes = _operands(nodes)
    return nodes[0] if len(nodes) == 1 and isinstance(nodes[0], Node) else Operator(_gffi.UNION, nodes)


def intersection(*nodes):
    """Pointwise maximum, folded left to right."""
    nodes = _operands(nodes)
    return nodes[0] if len(nodes) == 1 and isinstance(nodes[0], Node) else Operator(_gffi.INTERSECT, nodes)


def difference(a, b):
    """max(a, -b)."""
    return Operator(_gffi.DIFFERENCE, (a, b))


def complement(a):
    """-a."""
    return Operator(_gffi.COMPLEMENT, (a,))


# ------------------------------------------------------------------------------------------ the compiler
class Compiled(object):
    """What compile_program returns.

      ops      [(code, arg, off)]: the postfix program
      params   (K or 1, P) fp64: one row of leaf parameters per member
      arrays   [(data, per_member)]: the array leaves in slot order, as the caller gave them
      K        number of members, None for an unbatched scene (one member, result of g.shape)
      depth    the deepest the evaluation stack gets
    """

    def __init__(self, ops, params, arrays, K, depth):
        self.ops, self.params, self.arrays, self.K, self.depth = ops, params, arrays, K, depth

    @property
    def members(self):
        return 1 if self.K is None else self.K


def _numeric(v, what):
    v = _unlazy(v)
    if is_tensor(v):
        v = v.detach().cpu().numpy()
    try:
        return np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        error('%s must be numeric' % what)


def _vector(value, default, dim, what):
    """-> (dim,) or (K, dim) fp64.  None or all zero: the default (the reference's "not any" rule; an all-zero (K, dim) array
    gives the default for each of its K members and stays batched); one element: scalar times ones; (dim,) or a (dim, 1)
    column: the vector; (K, dim): one vector per member."""
    if isinstance(value, _Halves):
        c = _vector(value.center, 0.0, dim, 'center')
        w = _vector(value.widths, 1.0, dim, 'widths')
        return c + value.sign * (0.5 * w)
    if isinstance(value, _Unit):
        n = _vector(value.normal, None, dim, 'normal')
        length = np.linalg.norm(n, axis=-1, keepdims=True)
        if not np.all(length > 0) or not np.all(np.isfinite(length)):
            error('the normal of a hyperplane must be finite and not zero')
        return n / length
    if value is None or (default is not None and not np.any(_numeric(value, what))):
        if default is None:
            error('%s is required' % what)
        shape = () if value is None else _numeric(value, what).shape
        if len(shape) == 2 and shape[1] == dim and shape[0] * dim > 1 and not (shape == (dim, 1) and dim > 1):
            return default * np.ones(shape)             # all zero AND batched: the default for each of the K members
        return default * np.ones(dim)
    a = _numeric(value, what)
    if np.any(np.isnan(a)):
        error('%s holds NaN' % what)
    if a.size == 1:
        return a.item() * np.ones(dim)
    if a.ndim == 1 and a.size == dim and dim > 1:
        return a.copy()
    if a.ndim == 2 and a.shape == (dim, 1) and dim > 1:
        return a[:, 0].copy()
    if a.ndim == 2 and a.shape[1] == dim and a.shape[0] >= 1:
        return a.copy()
    error('%s of shape %s fits no grid of %d dimensions: a scalar, %d values, or (K, %d) for K members' % (what, a.shape, dim, dim, dim))


def _scalar(value, what):
    """-> () or (K,) fp64."""
    a = _numeric(value, what)
    if np.any(np.isnan(a)):
        error('%s holds NaN' % what)
    if a.size == 1:
        return a.reshape(())
    if a.ndim == 1:
        return a.copy()
    error('%s of shape %s: a scalar, or (K,) for K members' % (what, a.shape))


def _rows(value, dim, pad):
    """-> (J, dim) or (K, J, dim) fp64, 1 <= J <= 6."""
    a = _numeric(value, 'rows')
    if np.any(np.isnan(a)):
        error('rows holds NaN')
    if a.ndim not in (2, 3):
        error('rows of shape %s: (J, %d), or (K, J, %d) for K members' % (a.shape, dim, dim))
    if pad and a.shape[-1] < dim:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (dim - a.shape[-1],))], axis=-1)
    if a.shape[-1] != dim:
        error('rows of length %d fit no grid of %d dimensions: every row has %d coefficients' % (a.shape[-1], dim, dim))
    J = a.shape[-2]
    if J < 1 or J > _kffi.MAX_DIM:
        error('sphere_of takes J = 1 .. %d rows (got %d)' % (_kffi.MAX_DIM, J))
    if a.ndim == 3 and a.shape[0] < 1:
        error('rows of shape %s: K is at least 1' % (a.shape,))
    return a.copy()


def _images(value, J):
    """The centre of sphere_of -> (J,) or (K, J) fp64: None: zeros; one element: times ones; (J,); (K, J)."""
    if value is None:
        return np.zeros(J)
    a = _numeric(value, 'center')
    if np.any(np.isnan(a)):
        error('center holds NaN')
    if a.size == 1 and a.ndim < 2:
        return a.item() * np.ones(J)
    if a.ndim == 1 and a.size == J:
        return a.copy()
    if a.ndim == 2 and a.shape[1] == J and a.shape[0] >= 1:
        return a.copy()
    error('center of shape %s fits no sphere_of with %d rows: a scalar, %d values, or (K, %d) for K members' % (a.shape, J, J, J))


def compile_program(node, dim):
    """The tree `node` as a postfix program for a grid of `dim` dimensions -> Compiled.  Pure Python: no GPU is touched.
    An n-ary union / intersection is folded left to right (a b op c op ...), so its own depth is that of its deepest
    operand plus one.  Raises ValueError for a tree beyond the limits, for parameters that fit no such grid and for
    batched parameters that disagree on K."""
    return _compile(node, dim, False)


def compile_program_hi(node, dim):
    """compile_program for libhj_hishapes.so: grids of 1 .. 6 dimensions, and the leaf sphere_of."""
    return _compile(node, dim, True)


def _compile(node, dim, hi):
    dim = int(dim)
    if not isinstance(node, Node):
        error('evaluate a shape node (got %s): wrap a grid array in array(...)' % type(node).__name__)
    limit = _kffi.MAX_DIM if hi else _qffi.MAX_DIM
    if dim < 1:
        error('grids have 1 .. %d dimensions (got %d)' % (limit, dim))
    if dim > limit:
        error('grids of more than %d dimensions have no device implementation' % limit)
    ops, columns, arrays, slots, ks = [], [], [], {}, []
    state = dict(off=0, depth=0, deepest=0)

    def member_axis(k, what):
        ks.append((int(k), what))

    def push():
        state['depth'] += 1
        state['deepest'] = max(state['deepest'], state['depth'])
        if state['depth'] > MAX_DEPTH:
            error('the shape needs an evaluation stack more than %d deep, the kernel\'s limit: %s' % (MAX_DEPTH, HINT))

    def leaf(n):
        if n.code == _gffi.ARRAY:
            data = _unlazy(n.data)
            shape = tuple(int(s) for s in (data.shape if hasattr(data, 'shape') else np.shape(data)))
            if len(shape) == dim + 1:
                member_axis(shape[0], 'an array leaf')
            elif len(shape) != dim:
                error('an array leaf of shape %s fits no grid of %d dimensions' % (shape, dim))
            if id(n.data) not in slots:
                slots[id(n.data)] = len(arrays)
                arrays.append((n.data, len(shape) == dim + 1))
            ops.append((n.code, slots[id(n.data)], 0))
            return
        if n.code == _kffi.SPHERE_OF:
            if not hi:
                error('sphere_of runs in libhj_hishapes.so: compile it with compile_program_hi (evaluate_shape does)')
            rows = _rows(n.vectors[0][0].rows, dim, getattr(n, 'pad', False))
            J = rows.shape[-2]
            center = _images(n.vectors[1][0], J)
            radius = _scalar(n.scalars[0], 'radius')
            ops.append((n.code, J, state['off']))
            for v, batched, what in ((rows.reshape(rows.shape[:-2] + (J * dim,)), rows.ndim == 3, 'rows'),
                                     (center, center.ndim == 2, 'center'), (radius[..., None], radius.ndim == 1, 'radius')):
                if batched:
                    member_axis(v.shape[0], what)
                columns.append(v)
                state['off'] += v.shape[-1]
            return
        arg = 0
        if n.code == _gffi.CYLINDER:
            for a in n.axes:
                if a < 0 or a >= dim:
                    error('cylinder: axis %d is outside the %d of the grid' % (a, dim))
                arg |= 1 << a
        ops.append((n.code, arg, state['off']))
        names = {_gffi.SPHERE: ('center',), _gffi.CYLINDER: ('center',), _gffi.RECT: ('lower', 'upper'),
                 _gffi.HALFSPACE: ('normal', 'point')}[n.code]
        for (value, default), what in zip(n.vectors, names):
            v = _vector(value, default, dim, what)
            if v.ndim == 2:
                member_axis(v.shape[0], what)
            columns.append(v)
            state['off'] += dim
        for value in n.scalars:
            s = _scalar(value, 'radius')
            if s.ndim == 1:
                member_axis(s.shape[0], 'radius')
            columns.append(s[..., None])
            state['off'] += 1

    def walk(n):
        if isinstance(n, Leaf):
            push()
            leaf(n)
        elif n.code == _gffi.COMPLEMENT:
            walk(n.children[0])
            ops.append((n.code, 0, 0))
        else:
            walk(n.children[0])
            for c in n.children[1:]:
                walk(c)
                ops.append((n.code, 0, 0))
                state['depth'] -= 1

    # the length first, without recursion: a tree within it is at most MAX_OPS levels deep, so the walk below cannot exhaust
    # Python's stack and every tree beyond a limit is refused with the same ValueError
    count, pending = 0, [node]
    while pending and count <= MAX_OPS:
        n = pending.pop()
        if isinstance(n, Operator):
            count += max(1, len(n.children) - 1)
            pending.extend(n.children)
        else:
            count += 1
    if count > MAX_OPS:
        error('the shape compiles to more than %d instructions, a program\'s limit: %s' % (MAX_OPS, HINT))
    walk(node)
    if len(arrays) > MAX_ARRAYS:
        error('the shape has %d array leaves, a program holds %d: %s' % (len(arrays), MAX_ARRAYS, HINT))
    K = None
    for k, what in ks:
        if K is None:
            K = k
        elif k != K:
            error('batched parameters disagree on K: %s has %d members, %s has %d' % (ks[0][1], K, what, k))
    rows = 1 if K is None else K
    params = np.empty((rows, state['off']), dtype=np.float64)
    at = 0
    for c in columns:
        params[:, at:at + c.shape[-1]] = c
        at += c.shape[-1]
    return Compiled(ops, params, arrays, K, state['deepest'])


# ------------------------------------------------------------------------------------------ the launch
_LAST = [None]


def last_info():
    """Of the calling process's last evaluation: dict(flags = int32 per member (bits NEG 1, POS 2, ZERO-or-NaN 4), program =
    [(code, arg, off)], kernel = the kernel's name, K = members, P = parameters per member)."""
    return _LAST[0]


def _coord_tables(g, torch, device):
    cache = g.__dict__.get("_hj_shape_tables")
    if cache is None:
        cache = {}
        object.__setattr__(g, "_hj_shape_tables", cache)
    key = (device.type, device.index)
    if key not in cache:
        cache[key] = [torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()).copy()).to(device) for v in g.vs]
    return cache[key]


def _leaf_tensor(data):
    """An array leaf on the device as it is: fp32 stays fp32 (NumPy's too), anything but fp32 / fp64 becomes fp64."""
    data = _unlazy(data)
    if isinstance(data, np.ndarray) and data.dtype == np.float32:
        a = np.ascontiguousarray(data)
        return require_gpu().from_numpy(a if a.flags.writeable else a.copy()).to("cuda")
    return _device_data(data)


def _run(desc, N, coords, comp, dtype, device, member_note=True, hi=False):
    """Launch a compiled scene on a described grid -> tensor (members,) + N.  Sets last_info() and warns.  hi: the program and the
    descriptor are libhj_hishapes.so's (hjk_evaluate, hi_scene_kernel), otherwise libhj_shapes.so's (hjg_evaluate, scene_kernel)."""
    torch = require_gpu()
    if dtype not in ('float64', 'float32'):
        error('dtype must be \'float64\' or \'float32\' (got %r)' % (dtype,))
    K = comp.members
    keep, arrs = [], []
    for data, per_member in comp.arrays:
        t = _leaf_tensor(data)
        if t.device != device:
            t = t.to(device)
        if tuple(t.shape) != ((K,) + N if per_member else N):
            error('data parameter does not agree in array size with grid')
        keep.append(t)
        arrs.append((t.data_ptr(), _ffi.F32 if t.dtype == torch.float32 else _ffi.F64, per_member))
    ffi = _kffi if hi else _gffi
    evaluate = ffi.lib().hjk_evaluate if hi else ffi.lib().hjg_evaluate
    prog = ffi.program(comp.ops, arrs, [c.data_ptr() for c in coords])
    P = comp.params.shape[1]
    params = torch.from_numpy(comp.params).to(device) if P else None
    out = torch.empty((K,) + N, dtype=torch.float64 if dtype == 'float64' else torch.float32, device=device)
    flags = torch.zeros(K, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        ffi.check(evaluate(desc, prog, _ptr(params), K, P, _ptr(out), _ffi.F64 if dtype == 'float64' else _ffi.F32,
                           _ptr(flags), _stream(torch, device)))
    seen = flags.cpu().numpy()
    _LAST[0] = dict(flags=seen, program=list(comp.ops), kernel=ffi.last_kernel(), K=K, P=P)
    for k in np.nonzero((seen == _gffi.NEG) | (seen == _gffi.POS))[0]:
        warn(SINGLE_SIGN + (' (member %d)' % k if comp.K is not None and member_note else ''))
    return out


def _takes_hi(g, node):
    """Whether the tree runs in libhj_hishapes.so: a grid of more than 4 dimensions, or a sphere_of anywhere in the tree."""
    if int(g.dim) > _qffi.MAX_DIM:
        return True
    pending = [node]
    while pending:
        n = pending.pop()
        if isinstance(n, Operator):
            pending.extend(n.children)
        elif isinstance(n, Leaf) and n.code == _kffi.SPHERE_OF:
            return True
    return False


def _hi_descriptor(g, dtype_name):
    """(hjh_grid of a grid of 1 .. 6 dimensions, its shape): _hffi.grid_descriptor directly, descriptor_hi keeps to 5-D / 6-D."""
    N = [int(v) for v in np.asarray(g.N).ravel()]
    return _kffi.grid_descriptor(N, dtype_name), tuple(N)


def _launch(g, comp, dtype, hi, member_note=True):
    torch = require_gpu()
    device = torch.device('cuda', torch.cuda.current_device())
    name = dtype if dtype in ('float64', 'float32') else 'float64'
    desc, N = _hi_descriptor(g, name) if hi else _descriptor(g, name)
    return _run(desc, N, _coord_tables(g, torch, device), comp, dtype, device, member_note, hi)


def evaluate_shape(g, node, dtype='float64', output='tensor'):
    """The shape `node` on grid g, computed on the device in one launch.  Returns a device tensor of g.shape -- or of
    (K,) + g.shape when a parameter or an array leaf carries K members -- of `dtype` ('float64' | 'float32': the fp64 result
    rounded once); output='numpy' copies it to the host.  Warns once per member whose values have a single sign."""
    if output not in ('tensor', 'numpy'):
        error('output must be \'tensor\' or \'numpy\' (got %r)' % (output,))
    hi = _takes_hi(g, node)
    comp = _compile(node, g.dim, hi)
    out = _launch(g, comp, dtype, hi)
    if comp.K is None:
        out = out[0]
    return out if output == 'tensor' else out.cpu().numpy()


# ------------------------------------------------------------------------------------------ a moving set without its stack
class ShapeSeries(object):
    """The K members of a batched shape on grid g, evaluated one at a time: series[i] is ONE launch with K = 1 -- parameter
    row i, per-member array leaves sliced to member i, shared ones as they are -- and returns a fresh device tensor of g.shape.
    It looks like the stack (K,) + g.shape to what asks for its shape (ndim, shape, dtype, len), so HJIPDE_solve on a 5-D / 6-D
    grid takes it as a time-varying targetFunction / obstacleFunction and reads one member per interval; the stack itself
    never exists.  materialize() is the whole stack from one launch, equal to evaluate_shape's.  `evaluated` lists the
    members evaluated so far, in order."""

    def __init__(self, g, node, dtype='float64'):
        if dtype not in ('float64', 'float32'):
            error('dtype must be \'float64\' or \'float32\' (got %r)' % (dtype,))
        self.grid, self.node, self.dtype = g, node, dtype
        self._hi = _takes_hi(g, node)
        self._comp = _compile(node, g.dim, self._hi)
        if self._comp.K is None:
            error('a series needs a shape with K members: give a parameter or an array leaf a leading axis')
        self.evaluated = []

    @property
    def shape(self):
        return (self._comp.K,) + tuple(int(v) for v in np.asarray(self.grid.N).ravel())

    @property
    def ndim(self):
        return int(self.grid.dim) + 1

    def __len__(self):
        return self._comp.K

    def __getitem__(self, i):
        if isinstance(i, slice) or not isinstance(i, (int, np.integer)):
            raise TypeError('a ShapeSeries is indexed by one member at a time (got %s): materialize() gives the stack' % type(i).__name__)
        K = self._comp.K
        if not -K <= i < K:
            raise IndexError('member %d of a series of %d' % (i, K))
        i = int(i) % K
        c = self._comp
        arrays = [(_unlazy(data)[i], False) if per_member else (data, False) for data, per_member in c.arrays]
        one = Compiled(c.ops, np.ascontiguousarray(c.params[i:i + 1]), arrays, None, c.depth)
        out = _launch(self.grid, one, self.dtype, self._hi)[0]
        self.evaluated.append(i)
        return out

    def materialize(self):
        """The stack (K,) + g.shape as a device tensor, from one launch."""
        return evaluate_shape(self.grid, self.node, self.dtype)


def series(g, node, dtype='float64'):
    """The batched shape `node` on grid g as a ShapeSeries: its K members on demand, one launch each, never the stack."""
    return ShapeSeries(g, node, dtype)


# ------------------------------------------------------------------------------------------ the reference's names
def _grid_shape(g, node, output):
    if output not in ('numpy', 'tensor'):
        error('output must be \'numpy\' or \'tensor\' (got %r)' % (output,))
    return evaluate_shape(g, node, 'float64', output)


def shapeRectangleByCorners(grid, lower=None, upper=None, output='numpy'):
    """rect_corners.py:14: the (hyper)rectangle with the given corners (defaults 0 and 1; +-inf components give slabs),
    computed on the device.  Returns NumPy like shapeCylinder / shapeSphere; output='tensor' leaves it on the device."""
    return _grid_shape(grid, rectangle_by_corners(lower, upper), output)


def shapeRectangleByCenter(grid, center=None, widths=None, output='numpy'):
    """rect_center.py:8: the (hyper)rectangle with the given centre and full widths (defaults 0 and 1)."""
    return _grid_shape(grid, rectangle_by_center(center, widths), output)


def shapeHyperplane(grid, normal, point=None, output='numpy'):
    """hyperplane.py:8 (which does not run in the reference): n^T (x - point), n the normalised outward normal."""
    return _grid_shape(grid, hyperplane(normal, point), output)


def shapeHyperplaneByPoints(grid, points, positivePoint=None, output='numpy'):
    """shapeHyperplaneByPoints of the toolbox (the reference's hyper_pts.py is not Python): the hyperplane through the rows of
    `points`, positive at positivePoint -- which is required here, see hyperplane_by_points."""
    return _grid_shape(grid, hyperplane_by_points(points, positivePoint), output)


def _array_shapes(code, shapes):
    """A set operation on grid arrays alone: no grid is needed, the arrays' own shape stands in for one."""
    torch = require_gpu()
    tensors = [_leaf_tensor(s) for s in shapes]
    shape = tuple(tensors[0].shape)
    for t in tensors[1:]:
        if tuple(t.shape) != shape:
            error('the shapes do not agree in array size')
    N = shape if 1 <= len(shape) <= _qffi.MAX_DIM else (int(np.prod(shape[:-1], dtype=np.int64)), int(shape[-1])) if shape else (1,)
    device = tensors[0].device
    tensors = [t.reshape(N) for t in tensors]
    node = array(tensors[0])
    if code == _gffi.COMPLEMENT:
        node = complement(node)
    elif len(tensors) > 1:
        node = Operator(code, [array(t) for t in tensors])
    dtype = 'float32' if all(t.dtype == torch.float32 for t in tensors) else 'float64'
    desc = _qffi.grid_descriptor(len(N), N, [0.0] * len(N), [0.0] * len(N), [1.0] * len(N), [0] * len(N), [0] * len(N), dtype)
    zeros = torch.zeros(max(max(N), 1), dtype=torch.float64, device=device)       # no leaf reads a coordinate
    out = _run(desc, N, [zeros] * len(N), compile_program(node, len(N)), dtype, device)[0].reshape(shape)
    if any(_wants_tensor(s) for s in shapes):
        first = next(_unlazy(s) for s in shapes if _wants_tensor(s))
        return out if (not is_tensor(first) or first.is_cuda) else out.to(first.device)
    return out.cpu().numpy()


def shapeUnion(shapes):
    """shape_ops.py:12: the pointwise minimum of a list of shapes, as np.minimum.reduce.  A union of TWO shapes works here;
    the reference indexes shapes[2] in that case and raises IndexError.  NumPy in -> NumPy out, tensors or HostViews in
    -> a tensor out."""
    shapes = list(shapes)
    if not shapes:
        error('shapeUnion needs at least one shape')
    return _array_shapes(_gffi.UNION, shapes)


def shapeIntersection(shape1, shape2):
    """shape_ops.py:49: the pointwise maximum."""
    return _array_shapes(_gffi.INTERSECT, [shape1, shape2])


def shapeDifference(shape1, shape2):
    """shape_ops.py:88: max(shape1, -shape2)."""
    return _array_shapes(_gffi.DIFFERENCE, [shape1, shape2])


def shapeComplement(shape):
    """shape_ops.py:128: -shape."""
    return _array_shapes(_gffi.COMPLEMENT, [shape])
