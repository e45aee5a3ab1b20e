#!/usr/bin/env python3
"""Generate tests/golden/shapes.npz by running the UNMODIFIED reference's shape functions (InitialConditions/
rect_corners.py, rect_center.py, shape_ops.py).

Build-container only, like make_golden_query.py (same loader: oracle/_harness/ref_loader.py).  Run as

    python tests/golden/make_golden_shapes.py

Everything written is DATA: the grids' limits and coordinate vectors, seeded parameters, the arrays the reference
returned for them, and a record of what it raised.  Grids: 7 x 6 x 5 with a periodic last axis, and 9 x 8.  Cases:
shapeRectangleByCorners with vector, scalar, default and +-inf corners; shapeRectangleByCenter with vector and scalar
arguments; shapeUnion of three shapes; shapeIntersection, shapeDifference, shapeComplement.  shapeUnion of TWO shapes is
attempted and its exception recorded (the reference indexes shapes[2]).

The reference's shapeRectangleByCenter keeps its corners in an int64 array (its zeros() is integer), so center -+ 0.5 widths
is truncated toward zero before shapeRectangleByCorners sees it.  The pinned centre cases therefore have corners that are
whole numbers, where the truncation changes nothing and the function is the toolbox's; one further case, center_frac, has
fractional corners and records what the reference returns for them (the rectangle of the truncated corners).
"""
import io
import json
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

GRIDS = {"g3": ((7, 6, 5), [-1.0, -0.8, -np.pi], [1.2, 0.9, np.pi * (1 - 2 / 5)], 2),
         "g2": ((9, 8), [-1.5, -1.0], [1.0, 1.25], None)}


def col(v):
    return np.asarray(v, dtype=np.float64).reshape(-1, 1).copy()


def main():
    out, raised = {}, {}
    rng = np.random.default_rng(20261018)
    for name, (shape, gmin, gmax, pd) in GRIDS.items():
        dim = len(shape)
        g = createGrid(col(gmin), col(gmax), np.array(shape, dtype=np.int64).reshape(-1, 1), pd)
        out[name + "_min"], out[name + "_max"], out[name + "_N"] = col(gmin), col(gmax), np.array(shape, dtype=np.int64)
        out[name + "_pd"] = np.array([-1 if pd is None else pd], dtype=np.int64)
        for d in range(dim):
            out["%s_vs%d" % (name, d)] = np.asarray(g.vs[d], dtype=np.float64).ravel()
        lo = rng.uniform(-0.9, -0.1, dim)
        hi = rng.uniform(0.1, 0.8, dim)
        lo_inf, hi_inf = lo.copy(), hi.copy()
        lo_inf[0], hi_inf[-1] = -np.inf, np.inf
        lo_whole, hi_whole = {3: ([-1.0, 0.0, -2.0], [1.0, 1.0, 2.0]), 2: ([-1.0, 0.0], [0.0, 1.0])}[dim]
        center = (np.array(lo_whole) + np.array(hi_whole)) / 2           # exact: center -+ 0.5 widths are the whole corners
        widths = np.array(hi_whole) - np.array(lo_whole)
        center_frac = rng.uniform(-0.3, 0.3, dim)
        widths_frac = rng.uniform(2.4, 3.1, dim)
        cases = {"corners_vec": (shapeRectangleByCorners, [col(lo), col(hi)]),
                 "corners_scalar": (shapeRectangleByCorners, [-0.3, 0.45]),
                 "corners_default": (shapeRectangleByCorners, [None, None]),
                 "corners_inf": (shapeRectangleByCorners, [col(lo_inf), col(hi_inf)]),
                 "center_vec": (shapeRectangleByCenter, [col(center), col(widths)]),
                 "center_scalar": (shapeRectangleByCenter, [0.5, 3.0]),
                 "center_frac": (shapeRectangleByCenter, [col(center_frac), col(widths_frac)])}
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
            out[name + "_difference"] = np.asarray(shapeDifference(a, b))
            out[name + "_complement"] = np.asarray(shapeComplement(a))
        try:
            shapeUnion([a, b])
            raised[name + "_union2"] = None
        except Exception as e:                  # noqa: BLE001  (whatever the reference raises is the record)
            raised[name + "_union2"] = "%s: %s" % (type(e).__name__, str(e)[:120])
        print("%s %s: %d rectangle cases, 4 set operations pinned; union of two %s" % (name, shape, len(cases), raised[name + "_union2"] or "ran"))
    out["raised_json"] = np.array(json.dumps(raised))
    path = os.path.join(HERE, "shapes.npz")
    np.savez_compressed(path, **out)
    print("wrote shapes.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
