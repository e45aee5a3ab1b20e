"""tests/surface_ref.py, the NumPy restatement that the level-set kernels are held to (tests/test_gpu_surface.py), proved on
closed-form surfaces: manifoldness, orientation, Euler characteristic, second-order convergence of the enclosed volume,
contourpy's vertices in 2-D, and the orientation bit rules against geometry.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import surface_ref as S  # noqa: E402


def closed_and_oriented(verts, faces):
    """Closed 2-manifold, consistently oriented: every undirected edge in exactly 2 faces, every directed edge once."""
    und, ucount, dmax = S.edge_census(faces)
    assert len(faces) > 0 and np.all(ucount == 2), np.unique(ucount, return_counts=True)
    assert dmax == 1
    assert set(np.unique(faces)) == set(range(len(verts)))          # all-finite data: every vertex is used


@pytest.mark.parametrize("n", [9, 17])
def test_sphere_is_a_closed_oriented_sphere(n):
    verts, faces = S.extract(S.sphere(n))
    closed_and_oriented(verts, faces)
    assert S.euler_characteristic(len(verts), faces) == 2
    r = np.linalg.norm(verts - np.array([0.03, -0.02, 0.01]), axis=1)
    assert np.max(np.abs(r - 0.6)) < (2.0 / (n - 1)) ** 2             # vertices: linear interpolation of a distance function
    assert S.measure(verts, faces)[1] > 0                              # normals outward: toward increasing phi


def test_sphere_volume_converges_at_second_order():
    exact = 4.0 / 3.0 * np.pi * 0.6 ** 3
    err = {}
    for n in (9, 17):
        verts, faces = S.extract(S.sphere(n))
        vol = S.measure(verts, faces)[1]
        err[n] = (exact - vol) / exact
        print("sphere n=%d: volume %.6f, exact %.6f, below by %.3f %%" % (n, vol, exact, 100 * err[n]))
    assert 0 < err[17] < 0.03
    assert 3.0 <= err[9] / err[17] <= 5.0, err


def test_torus_has_genus_one():
    verts, faces = S.extract(S.torus())
    closed_and_oriented(verts, faces)
    assert S.euler_characteristic(len(verts), faces) == 0


def test_nodes_exactly_on_the_level_keep_the_mesh_closed():
    case = S.sphere_on_nodes()
    assert int((case["phi"] == 0.0).sum()) == 6
    verts, faces = S.extract(case)
    closed_and_oriented(verts, faces)
    assert S.euler_characteristic(len(verts), faces) == 2
    # the node on the level is the t = 0 (or t = 1) end of its edges: coincident vertices, zero-area faces, all kept
    assert len(np.unique(verts, axis=0)) < len(verts)


def test_anisotropic_grid_and_nonzero_level():
    case = S.anisotropic()
    verts, faces = S.extract(case)
    closed_and_oriented(verts, faces)
    assert S.euler_characteristic(len(verts), faces) == 2
    assert np.max(np.abs(np.linalg.norm(verts, axis=1) - 0.6)) < 0.25 ** 2


def test_surface_cut_by_the_grid_face_is_open_only_there():
    case = S.cut_sphere()
    verts, faces = S.extract(case)
    und, ucount, dmax = S.edge_census(faces)
    assert ucount.max() == 2 and dmax == 1
    boundary = und[ucount == 1]
    assert len(boundary) > 0
    assert np.all(verts[boundary.ravel(), 0] == case["xmin"][0])


def test_ellipse_is_one_oriented_loop_with_the_right_area():
    case = S.ellipse()
    verts, faces = S.extract(case)
    assert np.array_equal(np.bincount(faces[:, 0], minlength=len(verts)), np.ones(len(verts), dtype=np.int64))     # out-degree 1
    assert np.array_equal(np.bincount(faces[:, 1], minlength=len(verts)), np.ones(len(verts), dtype=np.int64))     # in-degree 1
    length, area = S.measure(verts, faces)
    exact = np.pi * 0.36 / 0.8
    print("ellipse: signed area %.5f, exact %.5f" % (area, exact))
    assert area > 0 and abs(area - exact) <= 0.005 * exact
    # one loop: following the segments from vertex 0 visits every vertex
    nxt = np.empty(len(verts), dtype=np.int64)
    nxt[faces[:, 0]] = faces[:, 1]
    seen, at = 0, 0
    while True:
        at = nxt[at]
        seen += 1
        if at == 0:
            break
    assert seen == len(verts)


def test_ellipse_vertices_on_grid_edges_are_contourpy_s():
    contourpy = pytest.importorskip("contourpy")
    case = S.ellipse()
    N, xmin, dx = case["N"], case["xmin"], case["dx"]
    verts, faces = S.extract(case)
    x = np.linspace(-1, 1, N[0])
    y = np.linspace(-1.5, 1, N[1])
    gen = contourpy.contour_generator(x=x, y=y, z=case["phi"].T.copy())           # z[j, i] at (x[i], y[j])
    theirs = np.concatenate([np.asarray(l)[:-1] if np.array_equal(l[0], l[-1]) else np.asarray(l) for l in gen.lines(0.0)])
    # our vertices on axis-aligned edges: one coordinate is a node coordinate
    on_x = np.min(np.abs(verts[:, 0:1] - x[None, :]), axis=1) < 1e-13
    on_y = np.min(np.abs(verts[:, 1:2] - y[None, :]), axis=1) < 1e-13
    ours = verts[on_x | on_y]
    print("contourpy: %d vertices, ours on axis-aligned edges: %d" % (len(theirs), len(ours)))
    assert len(ours) == len(theirs)
    a = ours[np.lexsort((ours[:, 1], ours[:, 0]))]
    b = theirs[np.lexsort((np.round(theirs[:, 1], 9), np.round(theirs[:, 0], 9)))]
    a = a[np.lexsort((np.round(a[:, 1], 9), np.round(a[:, 0], 9)))]
    assert np.max(np.abs(a - b)) <= 1e-12


def test_orientation_bits_equal_the_geometry():
    """On random non-degenerate simplices with random dx: 3-D faces have (b - a) x (c - a) along grad phi of their simplex,
    2-D segments have grad phi to their right (the inside to their left)."""
    rng = np.random.default_rng(11)
    checked = {2: 0, 3: 0}
    for D, N in ((3, (7, 6, 8)), (2, (40, 37))):
        perms = S.permutations(D)
        for rep in range(4):
            dx = rng.uniform(0.2, 3.0, D)
            xmin = rng.uniform(-1, 1, D)
            phi = rng.standard_normal(N)
            verts, faces, cell, simplex = S.level_set_ref(N, xmin, dx, phi, 0.0, with_simplex=True)
            M = tuple(n - 1 for n in N)
            ci = np.unravel_index(cell, M)
            grad = np.zeros((len(faces), D))
            for s, (perm, chain, par) in enumerate(perms):
                sel = simplex == s
                for k in range(1, D + 1):
                    d = perm[k - 1]
                    hi = tuple(ci[e][sel] + ((chain[k] >> e) & 1) for e in range(D))
                    lo = tuple(ci[e][sel] + ((chain[k - 1] >> e) & 1) for e in range(D))
                    grad[sel, d] = (phi[hi] - phi[lo]) / dx[d]
            p = verts[faces.astype(np.int64)]
            if D == 3:
                nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
                dot = np.sum(nrm * grad, axis=1)
                big = np.linalg.norm(nrm, axis=1) > 1e-9
                assert np.all(dot[big] > 0)
                # and the normal is parallel to the gradient: phi is linear in the simplex
                cosine = dot[big] / (np.linalg.norm(nrm[big], axis=1) * np.linalg.norm(grad[big], axis=1))
                assert np.all(cosine > 1 - 1e-6)
            else:
                d = p[:, 1] - p[:, 0]
                right = np.stack([d[:, 1], -d[:, 0]], axis=1)
                dot = np.sum(right * grad, axis=1)
                big = np.linalg.norm(d, axis=1) > 1e-9
                assert np.all(dot[big] > 0)
            checked[D] += len(np.unique(np.stack([cell, simplex]), axis=1).T)
    assert checked[3] >= 4000 and checked[2] >= 4000, checked


def test_non_finite_nodes_cut_holes_and_keep_their_neighbours_vertices():
    case = S.sphere(9)
    phi = case["phi"].copy()
    clean_v, clean_f = S.extract(case)
    phi[4, 4, 7] = np.nan
    phi[1, 4, 4] = np.inf
    phi[4, 1, 4] = -np.inf
    verts, faces = S.level_set_ref(case["N"], case["xmin"], case["dx"], phi, 0.0)
    assert 0 < len(faces) < len(clean_f) and np.isfinite(verts).all()
    und, ucount, dmax = S.edge_census(faces)
    assert ucount.max() == 2 and dmax == 1 and (ucount == 1).any()
    # vertices that no face uses may remain next to the holes; with finite data there are none
    assert len(np.unique(faces)) <= len(verts)


def test_fp32_data_is_converted_exactly_and_empty_results_are_empty():
    case = S.sphere(9)
    phi32 = case["phi"].astype(np.float32)
    v32, f32 = S.level_set_ref(case["N"], case["xmin"], case["dx"], phi32, 0.0)
    v64, f64 = S.level_set_ref(case["N"], case["xmin"], case["dx"], phi32.astype(np.float64), 0.0)
    assert np.array_equal(v32, v64) and np.array_equal(f32, f64) and v32.dtype == np.float64 and f32.dtype == np.int32
    for fill in (1.0, -1.0):
        v, f = S.level_set_ref((4, 5, 3), [0, 0, 0], [1, 1, 1], np.full((4, 5, 3), fill), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = S.level_set_ref((4, 5), [0, 0], [1, 1], np.full((4, 5), 1.0), 0.0)
    assert v.shape == (0, 2) and f.shape == (0, 2)
