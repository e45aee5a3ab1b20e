#!/usr/bin/env python3
"""Generate tests/golden/query.npz by running the UNMODIFIED reference's eval_u (ValueFuncs/evaluate_u.py:15).

Build-container only, like make_golden.py (same loader: oracle/_harness/ref_loader.py).  Run as

    python tests/golden/make_golden_query.py

Everything written is DATA: seeded inputs, the values the reference returned for them, and a record of the attempted
cases on which the reference RAISED -- those are unpinned, and the tests say so.  One state per call: with several states
the reference returns the value of the first only (`v.take(0)`, :117).

Cases: 2-D 7x6, 3-D 7x6x9 and 4-D 5x6x4x7 grids; periodic sets none, {0}, {last}, {1,2} (3-D / 4-D), all; states inside
the grid (random, an exact node, the last node) and, on periodic axes, in the wrap cell beyond the last node.  The
reference's createGrid cannot mark axis 0 periodic (`if not pdDims`, create_grid.py:34), so the boundary functions are
set on the grid Bundle after it is made -- as its callers would.  Also attempted: proj with 'min', 'max' and a slice.
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
from LevelSetPy.BoundaryCondition import addGhostPeriodic  # noqa: E402
from LevelSetPy.ValueFuncs.evaluate_u import eval_u  # noqa: E402
from LevelSetPy.ValueFuncs.data_proj import proj  # noqa: E402

SHAPES = {"g2": (7, 6), "g3": (7, 6, 9), "g4": (5, 6, 4, 7)}


def periodic_sets(nd):
    sets = [(), (0,), (nd - 1,), tuple(range(nd))]
    if nd >= 3:
        sets.append((1, 2))
    return sets


def bounds(shape, pd):
    nd = len(shape)
    gmin = np.array([-1.0 - 0.25 * d for d in range(nd)])
    span = np.array([2.5 + 0.5 * d for d in range(nd)])
    gmax = gmin + span
    for d in pd:
        gmax[d] = gmin[d] + span[d] * (1.0 - 1.0 / shape[d])        # a periodic axis stops one node short of the period
    return gmin, gmax


def make_grid(shape, pd):
    gmin, gmax = bounds(shape, pd)
    g = createGrid(gmin.reshape(-1, 1), gmax.reshape(-1, 1), np.array(shape, dtype=np.int64).reshape(-1, 1), None)
    for d in pd:
        g.bdry[d] = addGhostPeriodic
    return g, gmin, gmax


def attempt(fn):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return float(np.asarray(fn()).ravel()[0]), None
    except Exception as e:                      # noqa: BLE001  (whatever the reference raises is the record)
        return np.nan, "%s: %s" % (type(e).__name__, str(e)[:120])


def main():
    out, raised = {}, {}
    rng = np.random.default_rng(20260117)
    for name, shape in SHAPES.items():
        nd = len(shape)
        data = rng.standard_normal(shape)
        out[name + "_data"] = data
        for pd in periodic_sets(nd):
            key = "%s_p%s" % (name, "".join(str(d) for d in pd) or "none")
            g, gmin, gmax = make_grid(shape, pd)
            vs = [np.asarray(v, dtype=np.float64).ravel() for v in g.vs]
            dx = np.asarray(g.dx, dtype=np.float64).ravel()
            inside = np.stack([vs[d][0] + rng.random(8) * (vs[d][-1] - vs[d][0]) for d in range(nd)], axis=1)
            node = np.array([[vs[d][2] for d in range(nd)]])
            last = np.array([[vs[d][-1] for d in range(nd)]])
            states = [inside, node, last]
            if pd:
                wrap = inside[:3].copy()
                for d in pd:
                    wrap[:, d] = vs[d][-1] + (0.2 + 0.2 * np.arange(3)) * dx[d]     # between the last node and node 0 + period
                states.append(wrap)
            xs = np.concatenate(states)
            vals, errs = np.empty(len(xs)), []
            for k, x in enumerate(xs):
                gk, _, _ = make_grid(shape, pd)              # the reference modifies the grid and the state it is given
                vals[k], err = attempt(lambda: eval_u(gk, data.copy(), x.reshape(1, -1).copy()))
                if err:
                    errs.append((k, err))
            out[key + "_min"], out[key + "_max"] = gmin, gmax
            out[key + "_pd"] = np.array(pd, dtype=np.int64)
            out[key + "_xs"], out[key + "_vals"] = xs, vals
            out[key + "_raised"] = np.isnan(vals)
            raised[key] = errs
            print("%-12s %2d states, reference raised on %2d" % (key, len(xs), len(errs)))
    # proj: every kind of projection is attempted on the non-periodic 3-D grid
    g, _, _ = make_grid(SHAPES["g3"], ())
    data = out["g3_data"]
    for what, xs in (("min", 'min'), ("max", 'max'), ("slice", np.array([0.1]))):
        g, _, _ = make_grid(SHAPES["g3"], ())
        _, err = attempt(lambda: proj(g, data.copy(), np.array([0, 0, 1]), xs)[1])
        raised["proj_" + what] = [(0, err)] if err else []
        print("proj %-6s %s" % (what, err or "ran"))
    out["raised_json"] = np.array(json.dumps(raised))
    path = os.path.join(HERE, "query.npz")
    np.savez_compressed(path, **out)
    print("wrote query.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
