"""libhj_hishapes.so on the GPU against the NumPy restatement tests/hishapes_ref.py and the golden pin tests/golden/hishapes.npz:
every comparison is array_equal (NaN equal to NaN where an array leaf holds one); fp32 = the fp64 reference rounded once.

Grids, the smallest at which hi_scene_kernel can still go wrong: (7, 6, 8, 5, 9) -- 5-D, 15120 nodes, no multiple of 64 --,
(6, 5, 7, 5, 6, 8) -- 6-D --, (5, 5, 6, 5, 70) -- a last axis of 64 nodes or more: a wave lies in at most two rows --,
(2, 2, 2, 2, 2) -- 32 nodes, less than a wavefront --, (3, 1, 4, 1, 5, 1) -- extents of 1 --, and (37,), (9, 8), (13, 11, 9),
(8, 7, 8, 7), where the SAME programs also run through libhj_shapes.so and the two kernels must agree in every bit and flag.

  * every leaf and operator, sphere_of included, in one scene per grid; members K = 3 and K = 65537; array leaves shared
    and per member with NaN and +-inf; a view at an odd element offset; the sign flags and the warning;
  * the reference's names on the 5-D / 6-D goldens; the package's host shapeSphere / shapeCylinder at 5-D; a low_mem grid;
  * ShapeSeries: members on demand, and HJIPDE_solve on a 5-D grid fed a series against the same solve fed its stack;
  * guarded-buffer runs (tests/guarded_pool.py) in 2-D, 5-D and 6-D.
"""
import logging
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import _ffi, _gffi, _kffi, _marshal, hidim, shapes as S  # noqa: E402
import hishapes_ref as H  # noqa: E402
import shapes_ref as R  # noqa: E402
import hidim_cases as HC  # noqa: E402
from guarded_pool import GuardedPool, run_case  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "hishapes.npz"))
HI = [(7, 6, 8, 5, 9), (6, 5, 7, 5, 6, 8), (5, 5, 6, 5, 70), (2, 2, 2, 2, 2), (3, 1, 4, 1, 5, 1)]
LO = [(37,), (9, 8), (13, 11, 9), (8, 7, 8, 7)]
DTYPES = ["float64", "float32"]
NP = {"float64": np.float64, "float32": np.float32}
TD = {"float64": torch.float64, "float32": torch.float32}
CASE_OF = {(7, 6, 8, 5, 9): "plane5d", (6, 5, 7, 5, 6, 8): "pair6d", (5, 5, 6, 5, 70): "plane5d_long"}
_GRIDS, _REF = {}, {}
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def col(v, t=np.float64):
    return np.asarray(v, dtype=t).reshape(-1, 1)


def grid(shape, low_mem=False):
    """The three solver grids are tests/hidim_cases.py's (periodic axes and all); (13, 11, 9) is the air3D grid; an extent of 1
    has no spacing, so those grids are coordinate vectors alone (hishapes_ref.box) -- all evaluate_shape reads of a grid."""
    key = (shape, low_mem)
    if key not in _GRIDS:
        nd = len(shape)
        if shape in CASE_OF:
            gmin, gmax, N, pd = HC.limits(CASE_OF[shape])
            _GRIDS[key] = L.createGrid(col(gmin), col(gmax), col(N, np.int64), pd, low_mem=low_mem)
        elif min(shape) == 1 or nd > 4:
            _GRIDS[key] = H.box(shape)
        elif nd == 3:
            _GRIDS[key] = L.createGrid(col([-.75, -1.25, -np.pi]), col([3.25, 1.25, np.pi * (1 - 2 / shape[2])]), col(shape, np.int64), 2)
        else:
            _GRIDS[key] = L.createGrid(col([-1.0 - 0.1 * d for d in range(nd)]), col([1.0 + 0.05 * d for d in range(nd)]), col(shape, np.int64), None)
    return _GRIDS[key]


def field(shape, seed, dtype=np.float64, K=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, ((K,) if K else ()) + tuple(shape)).astype(dtype)


def centre(g):
    """A point well inside the grid, off its nodes."""
    return np.array([0.5 * (v[0] + v[-1]) + 0.013 * (d + 1) for d, v in enumerate(np.asarray(x, dtype=np.float64).ravel() for x in g.vs)])


def scene(shape, K=None):
    """Every leaf and every operator in one tree: sphere_of (rotated rows, and the selecting rows of sphere_between), sphere,
    cylinder, both rectangles, both hyperplanes, two array leaves, union, intersection, difference, complement."""
    g, dim = grid(shape), len(shape)
    rng = np.random.default_rng(31 * dim + len(shape))
    c = centre(g)
    b = lambda v: (v + rng.uniform(-0.05, 0.05, (K,) + np.shape(v))) if K else v     # noqa: E731
    J = min(3, dim)
    rows = rng.uniform(-1.0, 1.0, (J, dim))
    images = rows @ c
    pts = np.eye(dim) * 0.5 + 0.1 * np.arange(dim)[:, None] + c
    parts = [S.sphere_of(b(rows), b(images), 0.9), S.sphere(b(c), 0.8), S.cylinder([dim - 1], c, b(np.float64(0.7))),
             S.rectangle_by_corners(b(c - 0.6), c + 0.7), S.rectangle_by_center(c, 1.1), S.hyperplane(np.arange(1.0, dim + 1), b(c)),
             S.hyperplane_by_points(pts, c + 2.0), S.array(field(shape, 1)), S.array(field(shape, 2, np.float32, K=K))]
    if dim >= 2:
        parts.append(S.sphere_between(0, dim - 1, 0.6, c[0] - c[dim - 1]))
    a, bb, cy, rc, rz, hp, hq, ar, af = parts[:9]
    node = ((a | bb) & -(cy - rc)) | ((rz & hp) - (hq | ar)) & -af
    return (node | parts[9]) if dim >= 2 else node


def reference(shape):
    if shape not in _REF:
        comp = S.compile_program_hi(scene(shape), len(shape))
        assert set(o[0] for o in comp.ops) == set(range(1, 11)) or len(shape) == 1
        ref = H.run_program(grid(shape), comp)[0]
        ref.setflags(write=False)
        _REF[shape] = ref
    return _REF[shape]


def raw(g, comp, dtype, out, hi=True, arrays=None, flags=None):
    """hjk_evaluate / hjg_evaluate through the C ABI into `out` (a tensor or view of K x total elements) -> (flags, kernel)."""
    K = comp.members
    N = [int(v) for v in np.asarray(g.N).ravel()]
    coords = S._coord_tables(g, torch, out.device)
    did = _ffi.F64 if dtype == "float64" else _ffi.F32
    arrs = arrays if arrays is not None else []
    params = torch.from_numpy(comp.params).cuda()
    flags = torch.zeros(K, dtype=torch.int32, device="cuda") if flags is None else flags
    if hi:
        desc, prog = _kffi.grid_descriptor(N, dtype), _kffi.program(comp.ops, arrs, [c.data_ptr() for c in coords])
        _kffi.check(_kffi.lib().hjk_evaluate(desc, prog, params.data_ptr(), K, comp.params.shape[1], out.data_ptr(), did, flags.data_ptr(), None))
        name = _kffi.last_kernel()
    else:
        desc, _ = _marshal.descriptor(g, dtype)
        prog = _gffi.program(comp.ops, arrs, [c.data_ptr() for c in coords])
        _gffi.check(_gffi.lib().hjg_evaluate(desc, prog, params.data_ptr(), K, comp.params.shape[1], out.data_ptr(), did, flags.data_ptr(), None))
        name = _gffi.last_kernel()
    torch.cuda.synchronize()
    return tuple(int(f) for f in flags.cpu()), name


# ------------------------------------------------------------------------------------------ leaves and operators
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", HI + LO, ids=ids)
def test_every_leaf_and_operator(shape, dtype):
    g = grid(shape)
    got = S.evaluate_shape(g, scene(shape), dtype)
    assert got.is_cuda and got.dtype == TD[dtype] and tuple(got.shape) == tuple(shape)
    want = reference(shape).astype(NP[dtype])
    assert np.any(want < 0) and np.any(want > 0)
    assert np.array_equal(got.cpu().numpy(), want)
    info = S.last_info()
    assert info["kernel"] == _kffi.kernel_name(dtype) and info["K"] == 1 and info["flags"][0] == R.flags(want)
    assert np.array_equal(S.evaluate_shape(g, scene(shape), dtype, output="numpy"), want)


@pytest.mark.parametrize("shape", HI[:3], ids=ids)
def test_sphere_of_alone_and_the_capture_set(shape):
    g, dim = grid(shape), len(shape)
    c = centre(g)
    assert np.array_equal(S.evaluate_shape(g, S.sphere_of(np.eye(dim), c, 0.9), output="numpy"), R.sphere(g, c, 0.9))
    xs = R.coords(g)
    e0, e1 = xs[0] - xs[3], xs[1] - xs[4]
    want = np.sqrt(e0 * e0 + e1 * e1) - 0.75
    assert np.any(want < 0) and np.any(want > 0)
    assert np.array_equal(S.evaluate_shape(g, S.sphere_between((0, 1), (3, 4), 0.75), output="numpy"), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", LO, ids=ids)
def test_old_programs_give_the_old_kernels_bits_and_flags(shape, dtype):
    """The SAME programs of the old leaves through hjk_evaluate and hjg_evaluate on one grid: one source for the leaves."""
    g, dim = grid(shape), len(shape)
    total = int(np.prod(shape))
    nested = R.nested_scene(S, dim, K=2)[0]
    c = centre(g)
    programs = {"nested": nested, "sphere": S.sphere(c, 0.6), "cylinder": S.cylinder([dim - 1], c, [0.45, 5.0, 1e-3]),
                "corners-inf": S.rectangle_by_corners(-np.inf, c + 0.5), "hyperplane": S.hyperplane(np.arange(1.0, dim + 1), c),
                "array": -S.array(field(shape, 5, np.float32, K=2)) | S.array(field(shape, 6))}
    for name, node in programs.items():
        lo, hi = S.compile_program(node, dim), S.compile_program_hi(node, dim)
        assert lo.ops == hi.ops and np.array_equal(lo.params, hi.params), name
        K = lo.members
        keep = [S._leaf_tensor(d) for d, _ in lo.arrays]
        arrs = [(t.data_ptr(), _ffi.F32 if t.dtype == torch.float32 else _ffi.F64, pm) for t, (_, pm) in zip(keep, lo.arrays)]
        a = torch.empty(K * total, dtype=TD[dtype], device="cuda")
        b = torch.empty(K * total, dtype=TD[dtype], device="cuda")
        fa, ka = raw(g, lo, dtype, a, hi=False, arrays=arrs)
        fb, kb = raw(g, hi, dtype, b, hi=True, arrays=arrs)
        assert ka == _gffi.kernel_name(dtype) and kb == _kffi.kernel_name(dtype), name
        assert torch.equal(a.view(torch.int64 if dtype == "float64" else torch.int32), b.view(torch.int64 if dtype == "float64" else torch.int32)), name
        assert fa == fb and all(f != 0 for f in fa), (name, fa, fb)
        want = R.run_program(g, lo, [t.cpu().numpy() for t in keep]).astype(NP[dtype])
        assert np.array_equal(b.cpu().numpy().reshape((K,) + shape), want), name
    # the routing is as it was: a tree of old leaves on a grid of at most 4 dimensions runs scene_kernel
    S.evaluate_shape(g, programs["sphere"], dtype)
    assert S.last_info()["kernel"] == _gffi.kernel_name(dtype)


# ------------------------------------------------------------------------------------------ the reference's names
def golden_grid(name, low_mem=False):
    pd = int(GOLDEN[name + "_pd"][0])
    return L.createGrid(GOLDEN[name + "_min"], GOLDEN[name + "_max"], GOLDEN[name + "_N"].reshape(-1, 1), None if pd < 0 else pd, low_mem=low_mem)


def garg(name, case, j):
    key = "%s_%s_arg%d" % (name, case, j)
    if key not in GOLDEN.files:
        return None
    return GOLDEN[key].item() if GOLDEN[key].ndim == 0 else GOLDEN[key]


@pytest.mark.parametrize("name", ["g5", "g6"])
def test_pinned_cases_on_the_device(name):
    g = golden_grid(name)
    for case in ("corners_vec", "corners_scalar", "corners_default", "corners_inf"):
        got = L.shapeRectangleByCorners(g, garg(name, case, 0), garg(name, case, 1))
        assert isinstance(got, np.ndarray) and np.array_equal(got, GOLDEN["%s_%s" % (name, case)]), case
        assert S.last_info()["kernel"] == "hi_scene_kernel<double>"
    for case in ("center_vec", "center_scalar"):
        assert np.array_equal(L.shapeRectangleByCenter(g, garg(name, case, 0), garg(name, case, 1)), GOLDEN["%s_%s" % (name, case)]), case
    a, b, c = (GOLDEN["%s_%s" % (name, k)] for k in ("corners_vec", "center_vec", "corners_inf"))
    A, B, Cc = S.array(a), S.array(b), S.array(c)
    for key, node in (("union3", S.union(A, B, Cc)), ("intersection", A & B), ("difference", B - A), ("complement", -A)):
        assert np.array_equal(S.evaluate_shape(g, node, output="numpy"), GOLDEN["%s_%s" % (name, key)]), key


def test_reference_named_functions_follow_the_marshalling_rule_in_6d():
    g = grid((6, 5, 7, 5, 6, 8))
    c = centre(g)
    want = R.rectangle_by_corners(g, c - 0.9, c + 1.1)
    got = L.shapeRectangleByCorners(g, c - 0.9, c + 1.1)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want) and np.any(want < 0) and np.any(want > 0)
    t = L.shapeRectangleByCorners(g, c - 0.9, c + 1.1, output="tensor")
    assert torch.is_tensor(t) and t.is_cuda and np.array_equal(t.cpu().numpy(), want)
    assert np.array_equal(L.shapeRectangleByCenter(g, c, 1.7), R.rectangle_by_center(g, c, 1.7))
    n = np.arange(1.0, 7.0)
    assert np.array_equal(L.shapeHyperplane(g, n, c), R.hyperplane(g, n, c))
    pts = np.eye(6) * 0.5 + 0.1 * np.arange(6)[:, None] + c
    assert np.array_equal(L.shapeHyperplaneByPoints(g, pts, c + 2.0), R.hyperplane_by_points(g, pts, c + 2.0))


def test_device_shapes_equal_the_host_shapes_of_the_package_in_5d():
    g = grid((7, 6, 8, 5, 9))
    c = centre(g).reshape(-1, 1)
    assert np.array_equal(S.evaluate_shape(g, S.sphere(c, 1.6), output="numpy"), L.shapeSphere(g, c, 1.6))
    assert np.array_equal(S.evaluate_shape(g, S.sphere(0.25, 1.5), output="numpy"), L.shapeSphere(g, 0.25, 1.5))
    for ignore in ([4], [0, 4], 2):
        assert np.array_equal(S.evaluate_shape(g, S.cylinder(ignore, c, 1.45), output="numpy"), L.shapeCylinder(g, ignore, c, 1.45)), ignore


def test_low_mem_6d_grid_has_no_dense_coordinates_and_needs_none():
    shape = (6, 5, 7, 5, 6, 8)
    g = grid(shape, low_mem=True)
    assert g.xs[0].size == 6
    assert np.array_equal(S.evaluate_shape(g, scene(shape), output="numpy"), reference(shape))


# ------------------------------------------------------------------------------------------ members
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_members_on_the_odd_grid(dtype):
    shape = (7, 6, 8, 5, 9)
    g = grid(shape)
    node = scene(shape, K=3)
    comp = S.compile_program_hi(node, 5)
    assert comp.K == 3 and int(np.prod(shape)) % 64 != 0
    want = H.run_program(g, comp).astype(NP[dtype])
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    got = S.evaluate_shape(g, node, dtype)
    assert tuple(got.shape) == (3,) + shape and np.array_equal(got.cpu().numpy(), want)
    assert list(S.last_info()["flags"]) == [R.flags(w) for w in want]


def test_more_members_than_one_launch_holds():
    K, shape = 65537, (2, 1, 2, 1, 2)
    g = grid(shape)
    rng = np.random.default_rng(65537)
    rows = rng.uniform(-1.0, 1.0, (K, 2, 5))
    radii = rng.uniform(0.5, 0.9, K)
    xs = R.coords(g)
    e = []
    for j in range(2):
        s = rows[:, j, 0, None, None, None, None, None] * xs[0][None]
        for d in range(1, 5):
            s = s + rows[:, j, d, None, None, None, None, None] * xs[d][None]
        e.append(s - 0.1)
    want = np.sqrt(e[0] * e[0] + e[1] * e[1]) - radii[:, None, None, None, None, None]
    got = S.evaluate_shape(g, S.sphere_of(rows, 0.1, radii))
    assert tuple(got.shape) == (K,) + shape and np.array_equal(got.cpu().numpy(), want)
    seen = S.last_info()["flags"]
    assert seen.shape == (K,) and np.array_equal(seen, [R.flags(w) for w in want])
    assert np.array_equal(seen[[0, 65534, 65535, 65536]] != 0, [True] * 4)
    assert _kffi.plan(shape, K).member_launches == 2


# ------------------------------------------------------------------------------------------ array leaves
@pytest.mark.parametrize("dtype", DTYPES)
def test_array_leaves_shared_and_per_member_with_nan_and_inf(dtype):
    shape, K = (7, 6, 8, 5, 9), 3
    g = grid(shape)
    a64, b32 = field(shape, 11), field(shape, 12, np.float32, K=K)
    c64, d32 = field(shape, 13, K=K), field(shape, 14, np.float32)
    a64[0, 0, 0, 0, 0], a64[6, 5, 7, 4, 8], a64[3, 3, 3, 3, 3] = np.nan, np.inf, -np.inf
    b32[1, 3, 3, 3, 3, 3], b32[2, 6, 5, 7, 4, 8], b32[0, 0, 0, 0, 0, 1] = np.nan, -np.inf, np.inf
    c64[2, 5, 4, 6, 2, 6], c64[0, 1, 1, 1, 1, 1], d32[4, 4, 4, 4, 4] = np.nan, -np.inf, -np.inf
    node = ((S.array(a64) | S.array(torch.as_tensor(b32, device="cuda"))) & -S.array(L.lazy.HostView(torch.as_tensor(c64, device="cuda")))) - S.array(d32)
    comp = S.compile_program_hi(node, 5)
    assert [p for _, p in comp.arrays] == [False, True, True, False]
    want = H.run_program(g, comp, [a64, b32, c64, d32]).astype(NP[dtype])
    assert np.isnan(want).sum() >= 3 and np.isinf(want).sum() >= 3
    got = S.evaluate_shape(g, node, dtype).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))
    with pytest.raises(ValueError, match="array size"):
        S.evaluate_shape(g, S.array(np.zeros((7, 6, 8, 5, 8))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [1, 3])
def test_a_view_at_an_odd_element_offset(dtype, offset):
    shape = (7, 6, 8, 5, 9)
    g, total = grid(shape), int(np.prod(shape))
    comp = S.compile_program_hi(S.sphere_between((0, 1), (3, 4), 0.75) | S.sphere(centre(g), 0.8), 5)
    buf = torch.full((total + 8,), -7.0, dtype=TD[dtype], device="cuda")
    flags, name = raw(g, comp, dtype, buf[offset:offset + total])
    want = H.run_program(g, comp)[0].astype(NP[dtype])
    host = buf.cpu().numpy()
    assert buf[offset:].data_ptr() % 16 != 0 and name == _kffi.kernel_name(dtype)
    assert np.array_equal(host[offset:offset + total].reshape(shape), want) and flags == (R.flags(want),)
    assert np.all(host[:offset] == -7.0) and np.all(host[offset + total:] == -7.0)


# ------------------------------------------------------------------------------------------ flags and the warning
@pytest.mark.parametrize("dtype", DTYPES)
def test_sign_flags_and_the_warning(dtype, caplog):
    shape = (7, 6, 8, 5, 9)
    g = grid(shape)
    stack = np.ones((6,) + shape)
    stack[0] = -1.0                              # all negative
    stack[2, 3:] = -2.0                          # mixed
    stack[3, 4, 4, 4, 4, 4] = np.nan             # positive and a NaN
    stack[4] = -1.0
    stack[4, 6, 5, 7, 4, 8] = 0.0                # negative and a zero: the very last node
    stack[5, :2] = -3.0
    stack[5, 0, 0, 0, 0, 0] = 0.0                # all three: the very first node
    with caplog.at_level(logging.WARNING, logger="levelsetpy_amd"):
        S.evaluate_shape(g, S.array(stack), dtype)
    seen = list(S.last_info()["flags"])
    N_, P_, Z_ = _gffi.NEG, _gffi.POS, _gffi.ZERO
    assert seen == [N_, P_, N_ | P_, P_ | Z_, N_ | Z_, N_ | P_ | Z_] and len(set(seen)) == 6      # every member another sign class
    told = [r.getMessage() for r in caplog.records if "single sign" in r.getMessage()]
    assert len(told) == 2 and "member 0" in told[0] and "member 1" in told[1]
    caplog.clear()
    radii = np.array([100.0, 1e-4, 0.8])         # the grid inside the sphere, the sphere between the nodes, a sphere that shows
    with caplog.at_level(logging.WARNING, logger="levelsetpy_amd"):
        got = S.evaluate_shape(g, S.sphere_of(np.eye(5), centre(g), radii), dtype).cpu().numpy()
    assert list(S.last_info()["flags"]) == [R.flags(w) for w in got] == [N_, P_, N_ | P_]
    assert len([r for r in caplog.records if "single sign" in r.getMessage()]) == 2
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="levelsetpy_amd"):
        L.shapeRectangleByCorners(g, 50.0, 60.0)                     # off the grid: the reference's warning, no member named
    told = [r.getMessage() for r in caplog.records if "single sign" in r.getMessage()]
    assert len(told) == 1 and "member" not in told[0]


# ------------------------------------------------------------------------------------------ series
def moving(g, K):
    """K centres along the grid's diagonal."""
    return centre(g)[None] + np.linspace(-0.3, 0.3, K)[:, None] * np.ones(g.dim)[None]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(7, 6, 8, 5, 9), (6, 5, 7, 5, 6, 8), (9, 8), (37,)], ids=ids)
def test_series_members_one_at_a_time(shape, dtype):
    g, dim, K = grid(shape), len(shape), 4
    per, shared = field(shape, 41, np.float32, K=K), field(shape, 42)
    node = (S.cylinder([dim - 1], moving(g, K), 0.7) | S.array(per)) & -S.array(shared)
    if dim >= 2:
        node = node | S.sphere_between(0, dim - 1, np.linspace(0.3, 0.6, K))
    s = S.series(g, node, dtype)
    assert s.ndim == dim + 1 and s.shape == (K,) + shape and len(s) == K and s.dtype == dtype and np.ndim(s) == dim + 1
    whole = s.materialize()
    assert tuple(whole.shape) == (K,) + shape and whole.dtype == TD[dtype] and S.last_info()["K"] == K
    assert torch.equal(whole, S.evaluate_shape(g, node, dtype))
    comp = S.compile_program_hi(node, dim)
    assert np.array_equal(whole.cpu().numpy(), H.run_program(g, comp, [per, shared]).astype(NP[dtype]))
    assert s.evaluated == []
    for i in (2, 0, 3, 1, -1, -K):
        one = s[i]
        info = S.last_info()
        assert info["K"] == 1 and info["kernel"] == (_kffi if dim >= 2 else _gffi).kernel_name(dtype)
        assert one.is_cuda and tuple(one.shape) == shape and one.dtype == TD[dtype] and torch.equal(one, whole[i]), i
    assert s.evaluated == [2, 0, 3, 1, K - 1, 0]
    first, again = s[1], s[1]
    assert first.data_ptr() != again.data_ptr() and torch.equal(first, again)  # a fresh tensor per access
    with pytest.raises(TypeError):
        s[0:2]


def plane5d(g):
    sys5 = L.Plane5D(g, **HC.PARAMS["plane5d"])
    return L.Bundle(dict(grid=g, hamFunc=sys5.hamiltonian, partialFunc=sys5.dissipation, dissFunc=L.artificialDissipationGLF,
                         derivFunc=L.upwindFirstENO2))


def as_numpy(a):
    a = _marshal.unlazy(a)
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def test_solve_reads_a_series_one_member_per_interval():
    shape = (7, 6, 8, 5, 9)
    g = grid(shape)
    tau = np.array([0.0, 0.02, 0.04])
    c = centre(g)
    rows = np.zeros((2, 5))
    rows[0, 0], rows[1, 1] = 1.0, 1.2                                           # an ellipse in the plane of the first two axes
    target = S.sphere_of(rows, [c[0], 1.2 * c[1]], 1.0)
    data0 = S.evaluate_shape(g, target)
    assert S.last_info()["flags"][0] == _gffi.NEG | _gffi.POS
    centers = c[None] + np.array([0.9, 1.0, 1.1])[:, None] * np.array([1.0, 0.5, 0.0, 0.0, 0.0])[None]     # the obstacle translates over tau
    obstacle = S.rectangle_by_center(centers, [0.9, 0.9, np.inf, np.inf, np.inf])
    series = S.series(g, obstacle)
    stack = series.materialize()
    assert tuple(stack.shape) == (3,) + shape and not torch.equal(stack[1], stack[2])
    out = []
    for obs in (series, stack):
        args = L.Bundle(dict(quiet=True, obstacleFunction=obs, targetFunction=data0))
        data, tout, extra = L.HJIPDE_solve(data0, tau, plane5d(g), 'minVOverTime', args)
        out.append((as_numpy(data), np.asarray(tout)))
        assert "HamPlane5D" in hidim.last_path() and extra.path == hidim.last_path()
    assert series.evaluated == [1, 2]
    assert out[0][0].shape == (3,) + shape and np.all(np.isfinite(out[0][0])) and not np.array_equal(out[0][0][2], out[0][0][0])
    assert np.array_equal(out[0][0], out[1][0]) and np.all(out[0][1] == out[1][1]) and np.all(out[0][1] == tau)
    # the obstacle bites: without it the result differs
    free, _, _ = L.HJIPDE_solve(data0, tau, plane5d(g), 'minVOverTime', L.Bundle(dict(quiet=True)))
    assert not np.array_equal(as_numpy(free)[2], out[0][0][2])


def test_the_four_axis_solver_refuses_a_series_by_name():
    g = grid((13, 11, 9))
    s = L.DubinsVehicleRel(g, 1, 1)
    sd = L.Bundle(dict(grid=g, hamFunc=s.hamiltonian, partialFunc=s.dissipation, derivFunc=L.upwindFirstENO2))
    series = S.series(g, S.rectangle_by_center(np.array([[1.5, 0.5, 0.0], [1.6, 0.4, 0.0]]), [0.6, 0.6, np.inf]))
    data0 = S.evaluate_shape(g, S.cylinder(2, None, 0.5))
    for name in ("obstacleFunction", "targetFunction"):
        with pytest.raises(ValueError, match=r"%s is a ShapeSeries.*materialize\(\)" % name):
            L.HJIPDE_solve(data0, np.array([0.0, 0.05]), sd, 'minVOverTime', L.Bundle({"quiet": True, "keepLast": True, name: series}))
    assert series.evaluated == []


# ------------------------------------------------------------------------------------------ guarded buffers
POOL_ELEMS = 400 * 1000
_POOLS = {}


def pool(dtype):
    if dtype not in _POOLS:
        _POOLS[dtype] = GuardedPool(TD[dtype], "cuda", POOL_ELEMS)
    return _POOLS[dtype]


@pytest.mark.parametrize("shape", [(9, 8), (4, 3, 5, 3, 4), (3, 4, 3, 3, 2, 4)], ids=ids)
def test_guarded_buffers(shape):
    """Through the C ABI, fp32: the output (K, ...) and both array leaves are views of one arena with sentinel guards around each;
    at element offsets 0 .. 3 and with NaN / +-1e30 guards, the guards and the inputs stay intact, every output element is
    written, and the results are those of a run on fresh unguarded arrays.  720 and 864 nodes: more than one workgroup, the
    last one partly filled."""
    dtype, K, dim = "float32", 2, len(shape)
    g = H.box(shape)
    shared, each = field(shape, 21, np.float32), field(shape, 22, np.float32, K=K)
    rng = np.random.default_rng(23)
    centers = rng.uniform(-0.3, 0.3, (K, dim))
    keep = {}

    def op(alloc):
        a = alloc.inp("shared", torch.as_tensor(shared, device="cuda"))
        b = alloc.inp("each", torch.as_tensor(each, device="cuda"))
        out = alloc.out("out", (K,) + shape)
        node = (S.sphere_of(np.eye(dim)[:2] * 1.5, centers[:, :2], 0.5) | S.array(a.view)) & -(S.array(b.view) - S.rectangle_by_center(centers, 0.7))
        comp = S.compile_program_hi(node, dim)
        alloc.arm()
        flags, name = raw(g, comp, dtype, out.view, arrays=[(a.view.data_ptr(), _ffi.F32, False), (b.view.data_ptr(), _ffi.F32, True)])
        keep["comp"] = comp
        return {"flags": flags, "kernel": name}

    ref, arrays = run_case(op, pool(dtype), what="hi scene %s" % (shape,))
    want = H.run_program(g, keep["comp"], [shared, each]).astype(np.float32)
    assert np.array_equal(arrays["out"].cpu().numpy().reshape((K,) + shape), want)
    assert ref["kernel"] == _kffi.kernel_name(dtype) and list(ref["flags"]) == [R.flags(w) for w in want]
