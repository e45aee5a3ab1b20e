#!/usr/bin/env python3
"""Reach-avoid with a moving obstacle, and a sweep over capture radii: every implicit surface built on the device.

    python examples/moving_obstacle.py [n] [intervals]

The small air3D problem (examples/air3d_brt.py): from which relative states can the pursuer force a capture?  Here a
rectangular obstacle -- a region of relative positions the pursuer must stay out of, whatever the heading -- translates across
the grid while the tube grows backwards.  HJIPDE_solve takes a time-varying obstacle as a stack (len(tau),) + g.shape; the
whole stack comes from ONE evaluate_shape call, the rectangle's centre carrying the leading axis.  The target is a cylinder
with a notch cut out (difference of two shapes), built by the same kernel.  Then the capture radius is swept: one
evaluate_shape call with a radius of shape (B,) gives the B initial conditions that HJIPDE_solve_batch advances together.
Nothing is built on the host and nothing is copied to the device.  Needs an MI355X (the package has no CPU fallback).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import levelsetpy_amd as lsp
from levelsetpy_amd import shapes as S

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41
intervals = int(sys.argv[2]) if len(sys.argv) > 2 else 8

gmin = np.array([[-.75, -1.25, -np.pi]]).T
gmax = np.array([[3.25, 1.25, np.pi]]).T
N = n * np.ones((3, 1), dtype=np.int64)
gmax[2] *= (1 - 2 / N[2])
g = lsp.createGrid(gmin, gmax, N, 2)
cell = float(np.prod(np.asarray(g.dx)))
tau = np.linspace(0, 1.0, intervals + 1)

# the target: capture within 0.5, except from a notch behind the evader
target = S.cylinder(2, None, 0.5) - S.rectangle_by_corners([-np.inf, -0.1, -np.inf], [0.0, 0.1, np.inf])
data0 = lsp.evaluate_shape(g, target)

# the obstacle: a 0.6 x 0.8 box over all headings whose centre moves from (2.4, -0.6) to (1.0, 0.6) over tau
centers = np.stack([np.linspace(2.4, 1.0, len(tau)), np.linspace(-0.6, 0.6, len(tau)), np.zeros(len(tau))], axis=1)
obstacle = lsp.evaluate_shape(g, S.rectangle_by_center(centers, [0.6, 0.8, np.inf]))
print("grid %d^3: target %s, obstacle stack %s, both device tensors; kernel %s" % (
    n, tuple(data0.shape), tuple(obstacle.shape), S.last_info()["kernel"]))

dubins = lsp.DubinsVehicleRel(g, 1.0, 1.0)
schemeData = lsp.Bundle(dict(grid=g, hamFunc=dubins.hamiltonian, partialFunc=dubins.dissipation, derivFunc=lsp.upwindFirstWENO5))
free, _, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime', lsp.Bundle(dict(quiet=True, keepLast=True)))
avoid, _, _ = lsp.HJIPDE_solve(data0, tau, schemeData, 'minVOverTime',
                               lsp.Bundle(dict(quiet=True, keepLast=True, obstacleFunction=obstacle)))
vol = lambda v: float((v <= 0).sum()) * cell          # noqa: E731
print("capture set after %.1f: volume %.3f without the obstacle, %.3f with it moving through (target %.3f)" % (
    tau[-1], vol(free), vol(avoid), vol(data0)))

# the sweep: B capture radii, one evaluate_shape call, one batched solve
radii = np.linspace(0.3, 0.8, 6)
data0s = lsp.evaluate_shape(g, S.cylinder(2, None, radii))
tubes, _, outs = lsp.HJIPDE_solve_batch(data0s, tau, schemeData, 'minVOverTime',
                                         lsp.Bundle(dict(quiet=True, keepLast=True, systems=[dubins] * len(radii))))
print("capture radius   target volume   tube volume   steps")
for r, d0, tube, k in zip(radii, data0s, tubes, outs.steps.sum(1)):
    print("   %5.2f        %9.3f      %9.3f    %5d" % (r, vol(d0), vol(torch.as_tensor(tube)), k))
