"""CPU-only: the NumPy restatement tests/decomp_ref.py on closed forms, so that the GPU tests compare the kernels with
something that is itself known to be right.  The shapes are those of the package (shapeCylinder, shapeSphere) and of
tests/shapes_ref.py (rectangle_by_corners, the restatement of shapeRectangleByCorners that the goldens pin); the grids are
cut by the package's own sepGrid, which builds grids on the host.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import levelsetpy_amd as L  # noqa: E402
from levelsetpy_amd import decomp  # noqa: E402
import decomp_ref as D  # noqa: E402
import shapes_ref as R  # noqa: E402

SHAPE = (7, 6, 5, 4)


def grid(shape, lo=-1.0, hi=1.0, pd=None):
    nd = len(shape)
    return L.createGrid(lo * np.ones((nd, 1)) - 0.1 * np.arange(nd).reshape(-1, 1), hi * np.ones((nd, 1)),
                        np.array(shape, dtype=np.int64).reshape(-1, 1), pd)


def test_sepgrid_builds_the_subsystem_grids_on_the_host():
    g = grid(SHAPE)
    gs, ds = decomp.sepGrid(g, [[0, 2], [3, 1], [2]])
    assert ds == [None, None, None]
    assert [tuple(int(v) for v in s.N.ravel()) for s in gs] == [(7, 5), (6, 4), (5,)]
    for s, axes in zip(gs, ([0, 2], [1, 3], [2])):                 # ascending, as proj keeps them
        for k, a in enumerate(axes):
            assert np.array_equal(np.ravel(s.vs[k]), np.ravel(g.vs[a])) and s.bdry[k] is g.bdry[a]
    assert decomp.sepGrid(g, [[0, 1, 2, 3]])[0][0] is g


def test_box_is_the_intersection_of_its_back_projected_faces():
    g = grid(SHAPE)
    lower, upper = np.array([-0.5, -0.3, -0.6, -0.2]), np.array([0.4, 0.6, 0.1, 0.7])
    box = R.rectangle_by_corners(g, lower, upper)
    dims = [[0, 2], [1, 3]]
    gs, _ = decomp.sepGrid(g, dims)
    faces = [R.rectangle_by_corners(s, lower[a], upper[a]) for s, a in zip(gs, dims)]
    got, active = D.back_project(SHAPE, gs, faces, dims, 'intersection', return_active=True)
    assert np.array_equal(got, box)            # a max over the same numbers in any grouping is the same number
    assert set(np.unique(active)) == {0, 1}
    assert np.array_equal(np.where(active == 0, np.broadcast_to(faces[0][:, None, :, None], SHAPE),
                                   np.broadcast_to(faces[1][None, :, None, :], SHAPE)), box)
    assert np.all(active[np.broadcast_to(faces[0][:, None, :, None], SHAPE) == np.broadcast_to(faces[1][None, :, None, :], SHAPE)] == 0)


def test_union_of_back_projected_cylinders():
    g = grid((7, 6, 5))
    gs, _ = decomp.sepGrid(g, [[0, 1], [1, 2]])
    a = L.shapeSphere(gs[0], np.array([[0.1], [-0.2]]), 0.5)
    b = L.shapeSphere(gs[1], np.array([[0.2], [0.3]]), 0.4)
    want = np.minimum(L.shapeCylinder(g, 2, np.array([[0.1], [-0.2], [0.0]]), 0.5), L.shapeCylinder(g, 0, np.array([[0.0], [0.2], [0.3]]), 0.4))
    assert np.array_equal(D.back_project((7, 6, 5), gs, [a, b], [[0, 1], [1, 2]], 'union'), want)
    f32 = D.back_project((7, 6, 5), gs, [a.astype(np.float32), b], [[0, 1], [1, 2]], 'union', dtype=np.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, np.minimum(a.astype(np.float32).astype(np.float64)[:, :, None], b[None]).astype(np.float32))


def test_permuted_axes_are_a_transposition():
    g = grid((7, 6, 5))
    gs, _ = decomp.sepGrid(g, [[0, 2], [1]])
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((7, 5)), rng.standard_normal((6, 1))
    g20 = grid((5, 7))
    g20.vs = [gs[0].vs[1], gs[0].vs[0]]
    straight = D.back_project((7, 6, 5), gs, [a, b], [[0, 2], [1]])
    assert np.array_equal(D.back_project((7, 6, 5), [g20, gs[1]], [a.T.copy(), b], [[2, 0], [1]]), straight)
    assert np.array_equal(straight, np.maximum(a[:, None, :], b.reshape(1, 6, 1)))


def test_an_uncovered_axis_gives_identical_hyperplanes():
    g = grid((7, 6, 5))
    gs, _ = decomp.sepGrid(g, [[2, 0]])
    a = np.random.default_rng(1).standard_normal((3, 7, 5))
    got, active = D.back_project((7, 6, 5), gs, [a], [[0, 2]], return_active=True)
    assert got.shape == (3, 7, 6, 5) and np.all(active == 0)
    for j in range(6):
        assert np.array_equal(got[:, :, j, :], a)


def test_nan_and_the_active_index():
    g = grid((4, 3))
    gs, _ = decomp.sepGrid(g, [[0], [1], [1]])
    a, b, c = np.array([0.0, 1.0, np.nan, -np.inf]), np.array([0.5, np.inf, -1.0]), np.array([0.5, 2.0, np.nan])
    got, active = D.back_project((4, 3), gs, [a, b, c], [[0], [1], [1]], 'intersection', return_active=True)
    assert np.array_equal(got, np.maximum(np.maximum(a[:, None], b[None, :]), c[None, :]), equal_nan=True)
    assert np.array_equal(active, [[1, 1, -1], [0, 1, -1], [-1, -1, -1], [1, 1, -1]])          # ties go to the lowest subsystem
    low, act = D.back_project((4, 3), gs, [a, b, c], [[0], [1], [1]], 'union', return_active=True)
    assert np.array_equal(act, [[0, 0, -1], [1, 0, -1], [-1, -1, -1], [0, 0, -1]]) and low[3, 1] == -np.inf


def test_sepgrid_then_intersection_returns_a_box_and_bounds_a_sphere():
    g = grid(SHAPE)
    dims = [[0, 2], [1, 3]]
    gs, _ = decomp.sepGrid(g, dims)
    box = R.rectangle_by_corners(g, -0.5, 0.45)
    assert np.array_equal(D.back_project(SHAPE, gs, D.sep_grid(g, dims, box), dims), box)
    centre = np.array([float(np.ravel(g.vs[d])[n // 2]) for d, n in enumerate(SHAPE)])      # on a node of every axis
    ball = L.shapeSphere(g, centre.reshape(-1, 1), 0.6)
    got = D.back_project(SHAPE, gs, D.sep_grid(g, dims, ball), dims)
    # sqrt(a + b) - r against max(sqrt(a), sqrt(b)) - r: the 'min' projections (sepGrid's default) bound the sphere's VALUES
    # from below -- the set they describe, two crossed cylinders, contains the ball -- and the 'max' projections from above
    assert np.all(got <= ball) and not np.array_equal(got, ball)
    assert np.all(D.back_project(SHAPE, gs, D.sep_grid(g, dims, ball, 'max'), dims) >= ball)
    mid = [n // 2 for n in SHAPE]
    assert np.array_equal(got[:, mid[1], :, mid[3]], ball[:, mid[1], :, mid[3]])             # the subsystem planes through the centre
    assert np.array_equal(got[mid[0], :, mid[2], :], ball[mid[0], :, mid[2], :])


def test_interpolating_variants_on_the_subsystems_own_nodes_give_the_gather():
    g = grid((7, 6, 5), pd=2)
    dims = [[0, 2], [1, 2]]
    gs, _ = decomp.sepGrid(g, dims)
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((2, 7, 5)), rng.standard_normal((6, 5))
    exact = D.back_project((7, 6, 5), gs, [a, b], dims, 'union')
    coords = [np.ravel(v) for v in g.vs]
    # a node's coordinate need not land on weight exactly 0 or 1 ((x - x0) / dx is rounded): close, not equal
    assert np.allclose(D.back_project_coords(coords, gs, [a, b], dims, 'union'), exact, rtol=0, atol=1e-12)
    xs = D.node_states(coords)[::7]
    vals, active = D.points(gs, [a, b], dims, xs, 'union', return_active=True)
    assert np.allclose(vals, exact.reshape(2, -1)[:, ::7], rtol=0, atol=1e-12) and vals.shape == (2, xs.shape[0]) and active.dtype == np.int32
    xs[0, 0] = 5.0                                                 # outside an extrapolated axis of subsystem 0
    xs[1, 2] += 3 * 5 * float(np.ravel(g.dx)[2])                             # three periods away: the same value
    again, act = D.points(gs, [a, b], dims, xs, 'union', return_active=True)
    assert np.all(np.isnan(again[:, 0])) and np.all(act[:, 0] == -1) and np.allclose(again[:, 1], vals[:, 1], rtol=0, atol=1e-12)
