#!/usr/bin/env python3
"""Generate tests/golden/truncate.npz by running the UNMODIFIED reference's truncateGrid (Grids/truncate.py) on a 2-D, a 3-D
and a 4-D grid.

Build-container only, like make_golden_hishapes.py (same loader: oracle/_harness/ref_loader.py).  Run as

    python tests/golden/make_golden_truncate.py

Everything written is DATA: the grids' limits, the bounds, and what the reference returned for them -- the new grid's N, min,
max, coordinate vectors and which axes are periodic, and the truncated data.  Cases: an interior box on each grid; on the 3-D
grid, whose axis 2 is periodic, a box that keeps the periodic axis whole (it stays periodic) and one that crops it (it becomes
extrapolated); on the 2-D grid a box that leaves ONE node on axis 1 (max += 1e-3).

The reference's file lacks an import (see below, where the name is supplied); nothing else of it is touched.

UNPINNED, because the reference cannot run them: process=True (its processGrid turns the list of coordinate vectors into one
array and fails when the axes keep different numbers of nodes; the calls below pass process=False, and what processGrid adds is
this package's own processGrid, pinned elsewhere), its 1-D branch (`if dataOld:` on an array raises), grids of more than four
dimensions (it stops with an error), time-first stacks, and its return of the grid ALONE for data that is all zeros (recorded in
levelsetpy_amd/measure.py, not followed).  The reference also rebinds gOld.bdry[i] in place; the grids here are made anew per case.
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

from LevelSetPy.Grids import createGrid, truncateGrid  # noqa: E402
from LevelSetPy.BoundaryCondition import addGhostPeriodic, addGhostExtrapolate  # noqa: E402
import LevelSetPy.Grids.truncate as _truncate  # noqa: E402

# Grids/truncate.py names addGhostExtrapolate without importing it: as shipped, every call that crops an axis ends in a NameError.
# The file is run unmodified; the name it misses is bound, in its module, to the reference's own function.
if not hasattr(_truncate, "addGhostExtrapolate"):
    _truncate.addGhostExtrapolate = addGhostExtrapolate

# name: (N, min, max, periodic axis or None, xmin, xmax)
CASES = {
    "g2_box": ((9, 7), (-1.0, -2.0), (1.0, 1.0), None, (-0.6, -1.2), (0.7, 0.8)),
    "g2_one_node": ((9, 7), (-1.0, -2.0), (1.0, 1.0), None, (-0.6, -0.7), (0.7, -0.3)),
    "g3_box": ((6, 5, 8), (-1.0, -1.0, 0.0), (1.0, 1.0, 5.25), 2, (-0.7, -0.6, 1.0), (0.5, 0.9, 4.0)),
    "g3_periodic_whole": ((6, 5, 8), (-1.0, -1.0, 0.0), (1.0, 1.0, 5.25), 2, (-0.7, -0.6, -1.0), (0.5, 0.9, 7.0)),
    "g4_box": ((5, 4, 6, 4), (-1.0, 0.0, -2.0, -1.0), (1.0, 3.0, 2.0, 1.0), None, (-0.6, 0.5, -1.3, -0.5), (0.6, 2.5, 1.3, 1.5)),
}


def col(v, t=np.float64):
    return np.asarray(v, dtype=t).reshape(-1, 1).copy()


def main():
    out = {}
    rng = np.random.default_rng(20261020)
    for name, (N, gmin, gmax, pd, xmin, xmax) in CASES.items():
        D = len(N)
        with contextlib.redirect_stdout(io.StringIO()):
            g = createGrid(col(gmin), col(gmax), col(N, np.int64), pd)
        data = rng.standard_normal(N) + 0.5                      # any(data) is true: the reference returns (gNew, dataNew)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide="ignore"):
            gNew, dataNew = truncateGrid(g, data.copy(), col(xmin), col(xmax), process=False)
        out[name + "_N"], out[name + "_min"], out[name + "_max"] = np.array(N, dtype=np.int64), col(gmin), col(gmax)
        out[name + "_pd"] = np.array([-1 if pd is None else pd], dtype=np.int64)
        out[name + "_xmin"], out[name + "_xmax"], out[name + "_data"] = col(xmin), col(xmax), data
        out[name + "_newN"] = np.asarray(gNew.N, dtype=np.int64).reshape(-1)
        out[name + "_newmin"] = np.asarray(gNew.min, dtype=np.float64).reshape(-1)
        out[name + "_newmax"] = np.asarray(gNew.max, dtype=np.float64).reshape(-1)
        out[name + "_newperiodic"] = np.array([gNew.bdry[d] is addGhostPeriodic for d in range(D)])
        for d in range(D):
            out["%s_newvs%d" % (name, d)] = np.asarray(gNew.vs[d], dtype=np.float64).ravel()
        out[name + "_newdata"] = np.asarray(dataNew, dtype=np.float64)
        assert out[name + "_newdata"].shape == tuple(out[name + "_newN"]) and out[name + "_newdata"].size < data.size
        print("%s %s -> %s, periodic %s" % (name, N, tuple(out[name + "_newN"]), list(out[name + "_newperiodic"])))
    assert out["g2_one_node_newN"][1] == 1 and not out["g3_box_newperiodic"][2] and out["g3_periodic_whole_newperiodic"][2]
    path = os.path.join(HERE, "truncate.npz")
    np.savez_compressed(path, **out)
    print("wrote truncate.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
