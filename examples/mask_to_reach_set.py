#!/usr/bin/env python3
"""From an occupancy mask to a reach-avoid set: signedDistance and addCRadius in front of an existing solve.

    python examples/mask_to_reach_set.py [n] [intervals]

The small air3D problem (examples/air3d_brt.py): from which relative states can the pursuer force a capture?  Here the
region the pursuer must stay out of arrives as an occupancy map, a 0 / 1 image over the relative positions.  A mask is no
level-set function a solver can use: signedDistance turns it (as -1 inside, +1 outside) into the signed distance to the
occupied cells' boundary, in a few passes over the tiles near it; addCRadius then inflates the obstacle by a safety
margin, helperOC's name for `signedDistance - radius`; the result is extruded over the heading axis and handed to
HJIPDE_solve as obstacleFunction.  Everything stays on the device.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import eikonal

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
intervals = int(sys.argv[2]) if len(sys.argv) > 2 else 8
margin = 0.15

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
cell = float(np.prod(np.asarray(g.dx)))
tau = np.linspace(0, 1.0, intervals + 1)

# the occupancy map over (x, y): an L-shaped block of occupied cells
g2 = lsp.createGrid(gmin[:2], gmax[:2], N[:2])
x, y = torch.as_tensor(g2.xs[0], device="cuda"), torch.as_tensor(g2.xs[1], device="cuda")
occupied = ((x > 1.4) & (x < 2.4) & (y > -0.7) & (y < -0.3)) | ((x > 2.0) & (x < 2.4) & (y > -0.7) & (y < 0.6))
mask = torch.where(occupied, -1.0, 1.0).to(torch.float64)

distance, info = lsp.signedDistance(g2, mask, return_info=True)
print("mask %s with %d occupied cells -> signed distance in %d passes, %.0f %% of the tile launches did work (%s)" % (
    tuple(mask.shape), int(occupied.sum()), info.passes, 100 * info.active_tile_launch_fraction, eikonal.last_path()))
inflated = lsp.addCRadius(g2, mask, margin)
print("inflated by %.2f: %d cells inside the obstacle, %d before" % (margin, int((inflated <= 0).sum()), int((distance <= 0).sum())))
obstacle = inflated[:, :, None].expand(n, n, n).contiguous()         # whatever the heading

data0 = torch.as_tensor(lsp.shapeCylinder(g, 2, np.zeros((3, 1)), 0.5), device="cuda")
dubins = lsp.DubinsVehicleRel(g, 1.0, 1.0)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation, derivFunc=lsp.upwindFirstWENO5))
free, _, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))
avoid, _, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime',
                               lsp.Bundle(dict(quiet=True, keepLast=True, obstacleFunction=obstacle)))
vol = lambda v: float((v <= 0).sum()) * cell          # noqa: E731
print("capture set after %.1f: volume %.3f without the obstacle, %.3f with the inflated mask in the way (target %.3f)" % (
    tau[-1], vol(free), vol(avoid), vol(data0)))
