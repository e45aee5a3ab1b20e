#!/usr/bin/env python3
"""How large is the set, how far apart are two, and what box holds it: setVolume, setCompare, setBounds and truncateGrid.

    python examples/set_measures.py [n] [horizon]

Four things a reachability study reports, each one launch of measure_kernel (levelsetpy_amd/measure.py) and a handful of numbers:

  1. the volume of the air3D capture tube over tau, against the node count the other examples print.  The set is the one
     extract_level_set meshes (piecewise linear on the Kuhn subdivision), measured to second order in the grid step;
  2. a sweep of 16 tubes solved in one batch, ranked by volume from ONE call on the stack;
  3. the symmetric difference, as a set, of a coarse-to-fine solve and the all-fine one: setCompare reads both once and makes no
     temporary array;
  4. setBounds -> truncateGrid -> the solve continued on the cropped grid, with the share of the nodes that were dropped.

Nothing is asserted.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import measure

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
quiet = lambda **kw: lsp.Bundle(dict(quiet=True, **kw))      # noqa: E731


def air3d(n):
    gmin, gmax = np.array([[-.75, -1.25, -np.pi]]).T, np.array([[3.25, 1.25, np.pi]]).T
    N = n * np.ones((3, 1), dtype=np.int64)
    gmax[2] *= (1 - 2 / N[2])
    g = lsp.createGrid(gmin, gmax, N, 2)
    return g, lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5)


def scheme(g, system):
    return lsp.Bundle(dict(grid=g, hamFunc=system.hamiltonian, partialFunc=system.dissipation, derivFunc=lsp.upwindFirstWENO5))


# ---- 1. the tube's volume over tau
g, target = air3d(n)
car = lsp.DubinsVehicleRel(g, 1.0, 1.0)
tau = np.linspace(0, horizon, 6)
tube = lsp.HJIPDE_solve(torch.as_tensor(target, device="cuda"), tau, scheme(g, car), 'minVOverTime', quiet())[0]
tube = tube if tuple(tube.shape[1:]) == tuple(target.shape) else tube.movedim(-1, 0)          # time first
vols, info = lsp.setVolume(g, tube, return_info=True)
cell = float(np.prod(np.asarray(g.dx)))
print("air3D tube on %d^3 [%s]" % (n, measure.last_path()))
print("   t     volume    nodes x cell   cut cells of %d" % info["cells"][0])
for t, v, k, c in zip(tau, vols, info["inside"], info["cut"]):
    print("%5.2f  %9.5f  %12.5f  %8d" % (t, v, k * cell, c))

# ---- 2. a sweep ranked by volume, one call on the stack
sweep = [(ve, w) for ve in (0.75, 1.0, 1.25, 1.5) for w in (0.6, 0.8, 1.0, 1.2)]
systems = []
for ve, w in sweep:
    s = lsp.DubinsVehicleRel(g, 1.0, w)
    s.v_e, s.v_p = ve, 1.0
    systems.append(s)
data0s = torch.as_tensor(np.broadcast_to(target, (len(sweep),) + target.shape).copy(), device="cuda")
tubes = lsp.HJIPDE_solve_batch(data0s, tau[[0, -1]], scheme(g, systems[0]), 'minVOverTime', quiet(keepLast=True, systems=systems))[0]
vols = lsp.setVolume(g, tubes)
print("\n%d tubes of one batched solve, ranked by capture volume" % len(sweep))
for rank, k in enumerate(np.argsort(-vols)):
    print("%3d   v_e %.2f  w %.2f   %9.5f" % (rank + 1, sweep[k][0], sweep[k][1], vols[k]))

# ---- 3. coarse to fine against all fine, as sets
nC = max(11, (n + 1) // 2)
gC, targetC = air3d(nC)
split = 0.75 * horizon
VC = lsp.HJIPDE_solve(torch.as_tensor(targetC, device="cuda"), np.array([0.0, split]), scheme(gC, lsp.DubinsVehicleRel(gC, 1.0, 1.0)),
                      'minVOverTime', quiet(keepLast=True))[0]
VF = lsp.HJIPDE_solve(lsp.migrateGrid(gC, VC, g), np.array([split, horizon]), scheme(g, car), 'minVOverTime', quiet(keepLast=True))[0]
Vref = tube[-1]
c = lsp.setCompare(g, VF, Vref)
print("\ncoarse (%d^3) to fine against all fine at t = %.2f: volumes %.5f and %.5f, symmetric difference %.5f (%.2f %% of the union), "
      "intersection over union %.4f" % (nC, horizon, c.volA, c.volB, c.symdiff, 100 * c.symdiff / c.union, c.iou))

# ---- 4. crop the grid to the set and go on there
b = lsp.setBounds(g, Vref, pad=4)
gT, VT = lsp.truncateGrid(g, Vref, b.xmin, b.xmax)
kept = np.prod(VT.shape) / np.prod(Vref.shape)
more = lsp.HJIPDE_solve(VT, np.array([horizon, horizon + 0.2]), scheme(gT, lsp.DubinsVehicleRel(gT, 1.0, 1.0)), 'minVOverTime',
                        quiet(keepLast=True))[0]
whole = lsp.HJIPDE_solve(Vref, np.array([horizon, horizon + 0.2]), scheme(g, car), 'minVOverTime', quiet(keepLast=True))[0]
print("\nthe tube lies in nodes %s .. %s of %s: cropped to %s (%.0f %% of the nodes; axis 2 is periodic and stays whole)"
      % ([int(v) for v in b.lo], [int(v) for v in b.hi], tuple(Vref.shape), tuple(VT.shape), 100 * kept))
print("0.2 further on the cropped grid: volume %.5f; on the whole grid %.5f (the crop's extrapolated faces are %d nodes from the set)"
      % (lsp.setVolume(gT, more), lsp.setVolume(g, whole), 4))
