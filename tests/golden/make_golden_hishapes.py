#!/usr/bin/env python3
"""Generate tests/golden/hishapes.npz by running the UNMODIFIED reference's shape functions (InitialConditions/
rect_corners.py, rect_center.py, shape_ops.py) on a 5-D and a 6-D grid.

Build-container only, like make_golden_shapes.py (same loader: oracle/_harness/ref_loader.py).  Run as

    python tests/golden/make_golden_hishapes.py

Everything written is DATA: the grids' limits and coordinate vectors, seeded parameters and the arrays the reference
returned for them.  Grids: 4 x 3 x 5 x 3 x 4 with a periodic axis 2, and 3 x 4 x 3 x 3 x 2 x 4.  Cases, those of
make_golden_shapes.py: shapeRectangleByCorners with vector, scalar, default and +-inf corners; shapeRectangleByCenter with
vector and scalar arguments; shapeUnion of three shapes; shapeIntersection, shapeDifference (centre rectangle minus corner
rectangle), shapeComplement.

The reference's shapeRectangleByCenter truncates center -+ 0.5 widths toward zero (make_golden_shapes.py has the story), so
the centre cases have whole-number corners, where the truncation changes nothing.

Every pinned array has BOTH signs (asserted below): with so few nodes per axis a rectangle easily misses every node, and an
array of one sign pins little.  The axis limits are chosen per extent so that each axis has a node in [0, 0.45) and one
beyond 1 or below -1 somewhere on the grid.
"""
import io
import os
import sys
import contextlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_harness"))
import ref_loader  # noqa: E402

ref_loader.load()

from LevelSetPy.Grids import createGrid  # noqa: E402
from LevelSetPy.InitialConditions import (shapeRectangleByCorners, shapeRectangleByCenter, shapeUnion,  # noqa: E402
                                          shapeIntersection, shapeDifference, shapeComplement)

# limits per extent: 2 nodes -1, 0.25; 3 nodes -1, 0.1, 1.2; 4 nodes -0.8, -0.2, 0.4, 1; 5 nodes (periodic) -1, -0.6, -0.2, 0.2, 0.6
LIMITS = {2: (-1.0, 0.25), 3: (-1.0, 1.2), 4: (-0.8, 1.0), 5: (-1.0, 0.6)}
GRIDS = {"g5": ((4, 3, 5, 3, 4), 2), "g6": ((3, 4, 3, 3, 2, 4), None)}


def col(v):
    return np.asarray(v, dtype=np.float64).reshape(-1, 1).copy()


def main():
    out = {}
    rng = np.random.default_rng(20261020)
    for name, (shape, pd) in GRIDS.items():
        dim = len(shape)
        gmin, gmax = [LIMITS[n][0] for n in shape], [LIMITS[n][1] for n in shape]
        with contextlib.redirect_stdout(io.StringIO()):
            g = createGrid(col(gmin), col(gmax), np.array(shape, dtype=np.int64).reshape(-1, 1), pd)
        out[name + "_min"], out[name + "_max"], out[name + "_N"] = col(gmin), col(gmax), np.array(shape, dtype=np.int64)
        out[name + "_pd"] = np.array([-1 if pd is None else pd], dtype=np.int64)
        for d in range(dim):
            out["%s_vs%d" % (name, d)] = np.asarray(g.vs[d], dtype=np.float64).ravel()
        lo = rng.uniform(-0.9, -0.3, dim)
        hi = rng.uniform(0.45, 0.8, dim)
        lo_inf, hi_inf = lo.copy(), hi.copy()
        lo_inf[0], hi_inf[-1] = -np.inf, np.inf
        lo_whole = np.array([-1.0, 0.0] * 3)[:dim]
        hi_whole = 2.0 * np.ones(dim)
        center = (lo_whole + hi_whole) / 2                               # exact: center -+ 0.5 widths are the whole corners
        widths = hi_whole - lo_whole
        cases = {"corners_vec": (shapeRectangleByCorners, [col(lo), col(hi)]),
                 "corners_scalar": (shapeRectangleByCorners, [-0.3, 0.45]),
                 "corners_default": (shapeRectangleByCorners, [None, None]),
                 "corners_inf": (shapeRectangleByCorners, [col(lo_inf), col(hi_inf)]),
                 "center_vec": (shapeRectangleByCenter, [col(center), col(widths)]),
                 "center_scalar": (shapeRectangleByCenter, [0.0, 2.0])}
        got = {}
        for cname, (fn, args) in cases.items():
            for j, a in enumerate(args):
                if a is not None:
                    out["%s_%s_arg%d" % (name, cname, j)] = np.array(a, dtype=np.float64)
            with contextlib.redirect_stdout(io.StringIO()):
                got[cname] = np.asarray(fn(g, *[None if a is None else (a.copy() if isinstance(a, np.ndarray) else a) for a in args]),
                                        dtype=np.float64)
            assert got[cname].shape == tuple(shape)
            out["%s_%s" % (name, cname)] = got[cname]
        a, b, c = got["corners_vec"], got["center_vec"], got["corners_inf"]
        with contextlib.redirect_stdout(io.StringIO()):
            out[name + "_union3"] = np.asarray(shapeUnion([a, b, c]))
            out[name + "_intersection"] = np.asarray(shapeIntersection(a, b))
            out[name + "_difference"] = np.asarray(shapeDifference(b, a))       # b - a: a lies inside b, so a - b has one sign
            out[name + "_complement"] = np.asarray(shapeComplement(a))
        pinned = list(cases) + ["union3", "intersection", "difference", "complement"]
        for k in pinned:
            v = out["%s_%s" % (name, k)]
            assert v.shape == tuple(shape) and np.any(v < 0) and np.any(v > 0), (name, k, float(v.min()), float(v.max()))
        print("%s %s: %d rectangle cases, 4 set operations pinned, every array with both signs" % (name, shape, len(cases)))
    path = os.path.join(HERE, "hishapes.npz")
    np.savez_compressed(path, **out)
    print("wrote hishapes.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
